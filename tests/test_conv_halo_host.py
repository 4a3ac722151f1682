"""-m "not gpu": the host side of the halo-staged 3 x 3 kernel (conv_halo_dma_kernel, csrc/conv_dma.hip) -- the new symbols,
ocv_conv3x3_halo_supported over a grid of shapes (against the stated rule and against the library's own split-K query), the LDS bytes
its launch requests, and the dispatch setter's argument check."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB4 = 1 << 32


@pytest.fixture(scope="module")
def lib():
    from objcavit_amd import _lib
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from objcavit_amd import _lib
    header = open(os.path.join(ROOT, "include", "objcavit_hip.h")).read()
    assert re.search(r"\bint\s+ocv_conv3x3_halo_supported\s*\(", header) and re.search(r"\bint\s+ocv_conv3x3_set_dispatch\s*\(", header)
    assert re.search(r"\bsize_t\s+ocv_conv3x3_halo_lds_bytes\s*\(", header)
    for name in ("ocv_conv3x3_halo_supported", "ocv_conv3x3_set_dispatch", "ocv_conv3x3_halo_lds_bytes", "ocv_conv3x3_last_kernel"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.ocv_abi_version() == _lib.ABI_VERSION == 5                      # symbols are only added


def _expected(B, H, W, Cin, Cout):
    """Whole 8 x 32 patches; a K axis of fewer than 128 steps of 32 channels (nine taps per 32-channel chunk), the length from which
    ocv_conv_nhwc_split_x_fwd considers split-K; both operands below 4 GiB."""
    if min(B, H, W, Cin, Cout) < 1:
        return 0
    ok = H % 8 == 0 and W % 32 == 0 and 9 * -(-Cin // 32) < 128
    ok = ok and B * H * W * (Cin + 32) * 4 < GIB4 and 9 * Cout * (Cin + 32) * 2 < GIB4
    return int(ok)


def test_supported_exactly_on_whole_patches_within_the_size_limits(lib):
    seen = set()
    for B in (1, 2, 16):
        for H in (0, 1, 7, 8, 9, 12, 16, 120, 176, 240, 244):
            for W in (0, 16, 31, 32, 33, 40, 48, 64, 160, 320, 608, 624):
                for Cin in (0, 1, 24, 32, 40, 128, 256, 448, 449, 480):
                    for Cout in (0, 1, 8, 12, 128, 136, 256):
                        want = _expected(B, H, W, Cin, Cout)
                        assert lib.ocv_conv3x3_halo_supported(B, H, W, Cin, Cout) == want, (B, H, W, Cin, Cout)
                        if want:        # the library's own split-K query agrees: no supported shape is a split-K shape
                            assert lib.ocv_conv_nhwc_split_workspace_bytes(B, H, W, Cin, Cout, 3) == 0, (B, H, W, Cin, Cout)
                        seen.add(want)
    assert seen == {0, 1}
    # and the limit is not tighter than split-K needs: just past it the library does split a many-tile shape
    assert lib.ocv_conv3x3_halo_supported(16, 240, 320, 449, 128) == 0 and lib.ocv_conv_nhwc_split_workspace_bytes(16, 56, 96, 449, 128, 3) > 0
    # the benchmark's launches and KITTI's map
    for shape in ((16, 240, 320, 128, 128), (16, 120, 160, 256, 256), (4, 176, 608, 128, 128)):
        assert lib.ocv_conv3x3_halo_supported(*shape) == 1
    # the operand limits: 2^32 bytes of activations, of weights
    assert lib.ocv_conv3x3_halo_supported(16, 1024, 1024, 32, 8) == 0 and _expected(16, 1024, 1024, 32, 8) == 0
    assert lib.ocv_conv3x3_halo_supported(15, 1024, 1024, 32, 8) == 1 and _expected(15, 1024, 1024, 32, 8) == 1
    assert lib.ocv_conv3x3_halo_supported(1, 8, 32, 448, 500000) == 0 and _expected(1, 8, 32, 448, 500000) == 0
    assert lib.ocv_conv3x3_halo_supported(-1, 8, 32, 32, 8) == 0 and lib.ocv_conv3x3_halo_supported(1, -8, 32, 32, 8) == 0


def test_lds_request_fits_the_compute_unit(lib):
    """Two halo patches of (8 + 2) x 40 pixels x (hi, lo) x 64 B and the weights' ring of three 16 KiB slots; the parked-accumulator
    epilogue (4 x 128 rows x 68 floats) must fit in it too."""
    n = lib.ocv_conv3x3_halo_lds_bytes()
    assert n == 2 * (2 * 10 * 40 * 64) + 3 * 16384 == 151552
    assert 4 * 128 * 68 * 4 <= n <= 160 * 1024


def test_setter_rejects_unknown_modes(lib):
    """(The forced-mode refusal on an unsupported shape is checked with real buffers: tests/test_hip_conv_halo.py.)"""
    try:
        assert lib.ocv_conv3x3_set_dispatch(3) == -1 and b"ocv_conv3x3_set_dispatch" in lib.ocv_last_error()
        assert lib.ocv_conv3x3_set_dispatch(-1) == -1
        for mode in (1, 2, 0):
            assert lib.ocv_conv3x3_set_dispatch(mode) == 0
        assert lib.ocv_conv3x3_last_kernel() in (0, 1, 2)
    finally:
        assert lib.ocv_conv3x3_set_dispatch(0) == 0
