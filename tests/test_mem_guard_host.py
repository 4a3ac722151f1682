"""The guarded-allocation harness (tests/mem_guard.py) on CPU tensors: no GPU, no project kernel.  The overruns here are made
with ``torch.as_strided`` views of the harness's own payloads."""
import struct

import pytest
import torch

import mem_guard
from mem_guard import Breach, guarded
from objcavit_amd import _lib, hip_ops

CPU = torch.device("cpu")
G = 1024                                              # guard bytes here: small, so the CPU fills and compares stay instant


def _saved():
    return {n: getattr(torch, n) for n in mem_guard.ALLOCATORS}


def test_pattern_is_the_point_cloud_tests_nan():
    assert mem_guard.PATTERN == 0x7FC0DEAD
    as_f32 = struct.unpack("<f", struct.pack("<I", mem_guard.PATTERN))[0]
    assert as_f32 != as_f32                           # NaN as fp32
    halves = torch.tensor([mem_guard._PATTERN_I32], dtype=torch.int32)
    assert torch.isnan(halves.view(torch.bfloat16).float()).any() and torch.isnan(halves.view(torch.float16).float()).any()
    assert float(halves.view(torch.bfloat16).float().abs().nan_to_num(0).max()) > 1e18
    assert mem_guard.DEFAULT_GUARD_BYTES == 1 << 20 and mem_guard.DEFAULT_GUARD_BYTES >= 2 * 256 * 512 * 4


def test_guard_bytes_must_keep_torch_alignment():
    with pytest.raises(ValueError):
        guarded(CPU, guard_bytes=1000)


def test_clean_run_reports_nothing_and_idioms_fill():
    before = _saved()
    with guarded(CPU, guard_bytes=G) as g:
        e = torch.empty(3, 5, dtype=torch.float32, device=CPU)
        z = torch.zeros((2, 7), dtype=torch.int32)
        o = torch.ones(4, dtype=torch.float16)
        f = torch.full((3,), 2.5)
        fi = torch.full((3,), 7, dtype=torch.int64, device="cpu")
        zl = torch.zeros_like(e)
        ol = torch.ones_like(e, dtype=torch.float64)
        fl = torch.full_like(z, 9)
        el = torch.empty_like(o)
        m = torch.zeros(5, dtype=torch.bool)
        t = torch.tensor([1.0, 2.0, 3.0])
        ar = torch.arange(6)
        assert len(g.arenas) == 12
        assert torch.isnan(e).all() and g.never_written(e) == 15
        assert torch.isnan(el.float()).any() and g.never_written(el) == 2
        assert z.dtype == torch.int32 and not z.any() and o.dtype == torch.float16 and bool((o == 1).all())
        assert f.dtype == torch.float32 and bool((f == 2.5).all()) and fi.dtype == torch.int64 and bool((fi == 7).all())
        assert not zl.any() and ol.dtype == torch.float64 and bool((ol == 1).all()) and bool((fl == 9).all()) and fl.dtype == torch.int32
        assert m.dtype == torch.bool and not m.any()
        assert t.tolist() == [1.0, 2.0, 3.0] and ar.tolist() == list(range(6)) and ar.dtype == torch.int64
        for x in (e, z, o, f, fi, zl, ol, fl, el, m, t, ar):
            a = g._arena_of(x.data_ptr())
            assert a is not None and a.start == x.data_ptr() and a.nbytes == x.numel() * x.element_size()
            assert (x.data_ptr() - a.raw.data_ptr()) == G
        e.fill_(1.0)
        assert g.never_written(e) == 0
        g.check()
    assert _saved() == before


@pytest.mark.parametrize("dtype,numel", [(torch.float32, 15), (torch.bfloat16, 7), (torch.uint8, 13), (torch.int64, 3)])
def test_one_element_behind_the_payload_is_reported(dtype, numel):
    item = torch.empty((), dtype=dtype).element_size()
    with pytest.raises(Breach) as ei:
        with guarded(CPU, guard_bytes=G) as g:
            other = torch.zeros(8)
            t = torch.empty(numel, dtype=dtype)
            t.zero_()
            torch.as_strided(t, (1,), (1,), t.storage_offset() + numel).fill_(1)          # element [numel]: the first one of the trailing guard
            assert other is not None
    msg = str(ei.value)
    assert msg.count("guard of") == 1 and "trailing guard" in msg and f"({numel},)" in msg and str(dtype) in msg
    assert "test_mem_guard_host.py" in msg and "test_one_element_behind_the_payload_is_reported" in msg
    # fill_(1) changes the bytes of one element that differ from the pattern's; all lie in [nbytes, nbytes + item)
    first = int(msg.split("first at payload offset ")[1].split(",")[0])
    last = int(msg.split("last at ")[1].split(" ")[0])
    assert numel * item <= first <= last < numel * item + item


def test_one_element_in_front_of_the_payload_is_reported():
    with guarded(CPU, guard_bytes=G) as g:
        a = torch.zeros(4, 6)
        b = torch.empty(5, dtype=torch.float32)
        b.zero_()
        g.check()
        base = b.data_ptr() - G
        raw = g._arena_of(b.data_ptr()).raw
        assert raw.data_ptr() == base
        torch.as_strided(raw.view(torch.float32), (1,), (1,), G // 4 - 1).fill_(0.0)     # the word in front of b[0]
        with pytest.raises(Breach) as ei:
            g.check()
        msg = str(ei.value)
        assert "leading guard" in msg and "(5,)" in msg and "(4, 6)" not in msg
        assert "first at payload offset -4," in msg and "last at -1 " in msg
        raw.view(torch.int32)[G // 4 - 1] = mem_guard._PATTERN_I32                        # mended: the exit check passes
        assert a is not None


def test_never_written_counts_words_of_two_byte_payloads():
    with guarded(CPU, guard_bytes=G) as g:
        h = torch.empty(2, 3, 64, dtype=torch.bfloat16)
        assert g.never_written(h) == 2 * 3 * 32
        h[0].zero_()
        assert g.never_written(h) == 3 * 32 and g.never_written(h[0]) == 0 and g.never_written(h[1]) == 3 * 32
        h.zero_()
        assert g.never_written(h) == 0
        with pytest.raises(ValueError):
            g.never_written(torch.zeros(3).clone())


def test_strides_are_preserved():
    with guarded(CPU, guard_bytes=G) as g:
        y = torch.empty(2, 5, 3, 4, dtype=torch.float32, device=CPU, memory_format=torch.channels_last)
        assert y.shape == (2, 5, 3, 4) and y.stride() == (60, 1, 20, 5) and y.is_contiguous(memory_format=torch.channels_last)
        like = torch.empty_like(y)
        assert like.stride() == y.stride()
        perm = torch.zeros(4, 6).t()
        assert perm.shape == (6, 4) and torch.empty_like(perm).stride() == perm.stride() == (1, 6)
        assert torch.zeros_like(y, memory_format=torch.contiguous_format).stride() == (60, 12, 4, 1)
        assert torch.empty_like(y[:, :2]).stride() == (24, 1, 8, 2)  # (not dense: torch keeps the order and packs it, so do we)
        c = g.copy(torch.arange(120.0).view(2, 5, 3, 4).contiguous(memory_format=torch.channels_last))
        assert c.stride() == (60, 1, 20, 5) and c.flatten().tolist() == torch.arange(120.0).tolist()
        c2 = g.copy(torch.arange(12.0).view(3, 4)[:, ::2])
        assert c2.is_contiguous() and c2.tolist() == [[0.0, 2.0], [4.0, 6.0], [8.0, 10.0]]
        for t in (y, like, c, c2):
            a = g._arena_of(t.data_ptr())
            assert a.nbytes == t.numel() * 4


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 1023])
def test_byte_sizes_that_are_no_multiple_of_four(n):
    with guarded(CPU, guard_bytes=G) as g:
        t = torch.empty(n, dtype=torch.uint8)
        a = g._arena_of(t.data_ptr())
        assert a.nbytes == n and a.raw.numel() % 4 == 0 and a.raw.numel() >= 2 * G + n
        assert g.never_written(t) == n // 4
        t.zero_()                                                   # a full write of the payload breaches nothing ...
        g.check()
        assert g.never_written(t) == 0
        torch.as_strided(t, (1,), (1,), t.storage_offset() + n).fill_(0)                 # ... and the very next byte does
        with pytest.raises(Breach) as ei:
            g.check()
        assert f"first at payload offset {n}, last at {n} " in str(ei.value)
        a.raw[G + n] = mem_guard._PATTERN_BYTES[(G + n) % 4]


def test_zero_sized_allocations():
    with guarded(CPU, guard_bytes=G) as g:
        t = torch.empty(0, 4)
        assert t.shape == (0, 4) and g.never_written(t) == 0
        assert g.copy(torch.zeros(3, 0)).shape == (3, 0)


def test_patched_names_are_restored_after_an_exception():
    before = _saved()
    load = _lib.load
    depth = len(hip_ops._core._ws_stack())
    with pytest.raises(RuntimeError, match="boom"):
        with guarded(CPU, guard_bytes=G) as g:
            assert _saved() != before
            assert len(hip_ops._core._ws_stack()) == depth + 1
            raise RuntimeError("boom")
    assert _saved() == before and _lib.load is load and len(hip_ops._core._ws_stack()) == depth
    assert torch.empty(3).shape == (3,)


def test_other_devices_and_unhandled_calls_pass_through():
    with guarded(CPU, guard_bytes=G) as g:
        m = torch.empty(4, 4, device="meta")
        zm = torch.zeros_like(m)
        c = torch.zeros(3, dtype=torch.complex64)                   # a dtype the harness does not handle
        buf = torch.empty(3)
        n = len(g.arenas)
        o = torch.zeros(3, out=buf)                                 # out=: torch's business
        assert m.device.type == "meta" and zm.device.type == "meta" and c.dtype == torch.complex64 and o is buf
        assert len(g.arenas) == n == 1
    with guarded("meta", guard_bytes=G) as g:                       # a harness for another device leaves CPU tensors alone
        t = torch.zeros(5)
        assert g._arena_of(t.data_ptr()) is None and not g.arenas


def test_workspaces_are_exact_size_and_never_shared(monkeypatch):
    class _Stream:
        cuda_stream = 0
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    with guarded(CPU, guard_bytes=G) as g:
        big = hip_ops.workspace(4096, CPU, "t")
        small = hip_ops.workspace(100, CPU, "t")
        zeroed = hip_ops.workspace(37, CPU, "t", zero=True)
        empty = hip_ops.workspace(0, CPU, "t")
        assert big.numel() == 4096 and small.numel() == 100 and zeroed.numel() == 37 and empty.numel() == 1
        ptrs = {t.data_ptr() for t in (big, small, zeroed, empty)}
        assert len(ptrs) == 4
        for t in (big, small, zeroed, empty):
            a = g._arena_of(t.data_ptr())
            assert a.start == t.data_ptr() and a.nbytes == t.numel() and "workspace" in a.site
        assert g.never_written(big) == 1024 and g.never_written(small) == 25 and not zeroed.any()
        torch.as_strided(small, (1,), (1,), small.storage_offset() + 100).fill_(0)            # one byte behind a 100-byte request
        with pytest.raises(Breach, match="first at payload offset 100, last at 100 "):
            g.check()
        torch.as_strided(small, (1,), (1,), small.storage_offset() + 100).fill_(mem_guard._PATTERN_BYTES[(G + 100) % 4])
    assert hip_ops._core._ws_stack()[-1] is not g.store


def test_call_recorder_names_calls_and_unguarded_pointers(monkeypatch):
    import ctypes as C

    class FakeLib:
        def __init__(self):
            self.seen = []

        def ocv_layernorm_residual_fwd(self, *a):
            self.seen.append(a)
            return 0

        def ocv_abi_version(self):
            return _lib.ABI_VERSION

    fake = FakeLib()
    real_load = _lib.load
    monkeypatch.setattr(_lib, "load", lambda path=None: fake)
    patched = _lib.load
    outside = torch.zeros(8)
    with guarded(CPU, guard_bytes=G) as g:
        g.record_calls()
        x = torch.zeros(4, 8)
        y = torch.empty(4, 8)
        lib = _lib.load()
        # (x, residual, gamma, beta, eps, y, M, D, stream): gamma outside every payload, beta one byte behind x's payload
        rc = lib.ocv_layernorm_residual_fwd(x.data_ptr(), None, outside.data_ptr(), x.data_ptr() + x.numel() * 4, 1e-5,
                                            y.data_ptr() + 4, 4, 8, 12345)
        assert rc == 0
        assert g.calls == ["ocv_layernorm_residual_fwd"] and len(fake.seen) == 1
        assert [(n, i) for n, i, _ in g.stray] == [("ocv_layernorm_residual_fwd", 2), ("ocv_layernorm_residual_fwd", 3)]
    assert _lib.load is patched
    monkeypatch.undo()
    assert _lib.load is real_load
    assert C.c_void_p is _lib.PROTOTYPES["ocv_layernorm_residual_fwd"][1][0]
