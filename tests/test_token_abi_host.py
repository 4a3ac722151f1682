"""-m "not gpu": the argument checks of the token path's C ABI (include/objcavit_hip.h), on a machine without a GPU.  Every call
below returns before a launch: it is refused (-1, ocv_last_error() naming the entry point and the reason) or has no rows
(M == 0 -> 0).  Addresses are 16-byte aligned host addresses that are never dereferenced, as in tests/test_encoders_host.py.
The layouts these checks ACCEPT are run on the device by tests/test_hip_token_abi.py."""
import ctypes
import os

import pytest

from objcavit_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from objcavit_amd.build import build
        build()
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16          # a 16-byte aligned host address: never dereferenced
    yield addr
    del buf


def refused(lib, rc, entry, *words):
    msg = lib.ocv_last_error()
    return rc == -1 and msg.startswith(entry.encode() + b":") and all(w.encode() in msg for w in words)


def test_linear_argument_checks(lib, p):
    def call(M=33, N=40, K=24, lda=24, ldw=24, ldo=40, w_kn=0, batch=1, act=0, A=p, W=p, out=p):
        return lib.ocv_linear_fwd(A, lda, 0, W, ldw, 0, w_kn, None, out, ldo, 0, batch, M, N, K, act, None)

    e = "ocv_linear_fwd"
    assert refused(lib, call(lda=23), e, "leading dimension")
    assert refused(lib, call(ldo=39), e, "leading dimension")
    assert refused(lib, call(w_kn=1, ldw=39), e, "leading dimension")                 # [K, N] weights: rows of N, and 39 >= K
    assert refused(lib, call(N=16, ldo=16, ldw=23), e, "leading dimension")           # [N, K] weights: rows of K, and 23 >= N
    assert refused(lib, call(batch=0), e, "bad sizes", "batch=0")
    assert refused(lib, call(batch=-1), e, "bad sizes")
    assert refused(lib, call(act=3), e, "unknown activation 3")
    assert refused(lib, call(act=-1), e, "unknown activation")
    assert refused(lib, call(batch=65536), e, "grid too large", "65536")              # blockIdx.z
    assert refused(lib, call(A=None), e, "null pointer")
    assert call(M=0) == 0 and call(M=0, batch=65535) == 0 and call(M=0, w_kn=1, ldw=40) == 0


def test_linear_residual_layernorm_argument_checks(lib, p):
    def call(M=33, N=128, K=24, lda=24, ldw=24, ldres=128, ldo=128):
        return lib.ocv_linear_residual_layernorm_fwd(p, lda, p, ldw, p, p, ldres, p, p, 1e-5, None, p, ldo, M, N, K, None)

    e = "ocv_linear_residual_layernorm_fwd"
    assert refused(lib, call(N=127, ldres=127, ldo=127), e, "N must be 128", "127")
    assert refused(lib, call(N=256, ldres=256, ldo=256), e, "N must be 128")
    assert refused(lib, call(ldres=127), e, "bad sizes")
    assert refused(lib, call(ldo=127), e, "bad sizes")
    assert refused(lib, call(lda=23), e, "bad sizes")
    assert refused(lib, call(ldw=23), e, "bad sizes")
    assert call(M=0) == 0


def test_split3_linear_argument_checks(lib, p):
    def plain(M=33, N=40, K=24, lda=24, ldo=40, A=p, act=0):
        return lib.ocv_linear_split3_fwd(A, lda, p, None, p, ldo, M, N, K, act, None)

    def with_ln(M=33, N=128, K=24, lda=24, ldres=128, ldo=128, A=p):
        return lib.ocv_linear_residual_layernorm_split3_fwd(A, lda, p, p, p, ldres, p, p, 1e-5, None, p, ldo, M, N, K, None)

    for call, e in ((plain, "ocv_linear_split3_fwd"), (with_ln, "ocv_linear_residual_layernorm_split3_fwd")):
        assert refused(lib, call(K=20, lda=20), e, "bad sizes")                       # K % 8
        assert refused(lib, call(K=4, lda=4), e, "bad sizes")
        assert refused(lib, call(lda=26), e, "bad sizes")                             # lda % 4
        assert refused(lib, call(lda=20), e, "bad sizes")                             # lda < K
        assert refused(lib, call(A=p + 4), e, "16-byte aligned")
        assert refused(lib, call(A=p + 8), e, "16-byte aligned")
        assert call(M=0) == 0 and call(M=0, lda=28) == 0                              # a padded lda that is a multiple of 4 passes
    assert refused(lib, plain(ldo=39), "ocv_linear_split3_fwd", "bad sizes")
    assert refused(lib, plain(act=3), "ocv_linear_split3_fwd", "unknown activation 3")
    assert refused(lib, with_ln(N=64, ldres=64, ldo=64), "ocv_linear_residual_layernorm_split3_fwd", "N must be 128")
    assert refused(lib, with_ln(ldres=127), "ocv_linear_residual_layernorm_split3_fwd", "bad sizes")


def test_packer_argument_checks(lib, p):
    for name in ("ocv_pack_split3_fwd", "ocv_pack_split_h2_fwd"):
        fn = getattr(lib, name)
        assert refused(lib, fn(p, 23, 33, 24, p, None), name, "bad sizes", "ldw=23")
        assert refused(lib, fn(p, 24, 0, 24, p, None), name, "bad sizes")
        assert refused(lib, fn(p, 27, 33, 24, p + 8, None), name, "packed must be 16-byte aligned")
        assert refused(lib, fn(p, 27, 33, 24, p + 2, None), name, "packed must be 16-byte aligned")
        assert refused(lib, fn(p, 27, 33, 24, None, None), name, "null pointer")
    assert lib.ocv_split3_packed_elems(33, 24) == 2 * 2 * 512 * 3 and lib.ocv_split_h2_packed_elems(130, 72) == 5 * 5 * 512 * 2
    assert lib.ocv_split3_packed_elems(0, 24) == 0 and lib.ocv_split_h2_packed_elems(33, 0) == 0


def test_ffn_argument_checks(lib, p):
    def call(x=p, w1=p, w2=p, M=33, E=128, FF=256):
        return lib.ocv_ffn_residual_layernorm_fwd(x, w1, p, w2, p, p, p, 1e-5, None, p, M, E, FF, None)

    e = "ocv_ffn_residual_layernorm_fwd"
    assert refused(lib, call(x=p + 4), e, "16-byte aligned")
    assert refused(lib, call(w1=p + 4), e, "16-byte aligned")
    assert refused(lib, call(w2=p + 8), e, "16-byte aligned")
    assert refused(lib, call(FF=100), e, "multiple of 128")
    assert refused(lib, call(E=64), e, "E = 128")
    assert call(M=0) == 0
