"""Guarded allocations for the tests: every tensor the Python layer allocates sits between two poisoned guards.

``with guarded(device) as g:`` replaces the allocation idioms of ``objcavit_amd`` (``ALLOCATORS``) until exit.  A tensor asked
for on ``device`` becomes the payload of one flat uint8 ARENA,

    [ guard_bytes | payload, exactly numel * itemsize bytes | guard_bytes (+ 0..3 bytes up to a whole word) ]

filled with the 32-bit pattern 0x7FC0DEAD (a quiet NaN with a payload as fp32 -- the one tests/test_hip_point_cloud.py poisons
with; its halves are NaN (0x7FC0) and -6.1e18 (0xDEAD) as bf16, NaN and -375.25 as fp16; as int32 it is 2143346349) before the
payload is zeroed / set to one / filled where the idiom says so.  The payload starts ``guard_bytes`` (a multiple of 512) behind
the arena's start, so it is aligned as torch's own allocation would be, and it ends byte-exactly where the trailing guard
begins.  Arenas live until the scope ends: no address is handed out twice inside one scope, so a launch that writes through a
stale pointer hits a guard or a dead payload, never a live neighbour.

Workspaces: the scope opens ``hip_ops.workspace_scope`` on a store that never hands a buffer out twice, so every
``workspace(nbytes)`` request is an arena of exactly ``nbytes`` bytes, guarded and poisoned (zeroed for ``zero=True``): a
``*_workspace_bytes`` formula that is short, or a kernel that reads scratch it never wrote, shows.

``g.copy(t)`` guards an input or a weight, ``g.record_calls()`` records every ``ocv_*`` call and every device pointer argument
that lies in no guarded payload, ``g.check()`` (also run at exit) compares every guard with the pattern and raises ``Breach``,
``g.never_written(t)`` counts the 32-bit words of an output that still hold the pattern.

guard_bytes.  The default, 1 MiB, is twice the largest store one mis-masked tile of the dense kernels can make in the table of
tests/test_hip_memory_bounds.py: the convolutions' tile (csrc/conv_tile.hpp CBM) is 256 output rows, a row of at most 512 fp32 channels is 2 KiB,
256 x 512 x 4 B = 512 KiB (an hl32 row costs the same 4 B per channel: 2 x 2 B x ceil32(C)).  A table row whose output is wider
passes a larger figure (the dense split-K row writes 1032 channels: 8 MiB).  A stray store that flies further than the guard
lands in another arena's guard or in memory nobody owns; the first is reported against that arena, the second is not seen.

Everything patched is restored on exit, also when the body raises.  Test-side only: nothing here is imported by the package.
"""
from __future__ import annotations

import bisect
import ctypes as C
import struct
import sys
from typing import List, Optional

import torch

PATTERN = 0x7FC0DEAD
_PATTERN_I32 = struct.unpack("<i", struct.pack("<I", PATTERN))[0]
_PATTERN_BYTES = tuple(struct.pack("<I", PATTERN))
DEFAULT_GUARD_BYTES = 1 << 20

# grep of objcavit_amd/ for torch.<factory>(: the issue's six, plus ones_like / full_like (modules/ObjCAViT.py) and the two
# factories that carry data, torch.tensor / torch.arange (frames.py, conv.py, ObjCAViT.py, predict.py), guarded as copies
ALLOCATORS = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like", "tensor", "arange")

_HANDLED = (torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16, torch.uint16, torch.int32,
            torch.int64, torch.bool)
_THIS_FILE = __file__[:-1] if __file__.endswith(".pyc") else __file__
_PASS = object()


class Breach(AssertionError):
    pass


class Arena:
    __slots__ = ("raw", "nbytes", "shape", "dtype", "site", "start", "note")

    def __init__(self, raw, nbytes, shape, dtype, site, start, note):
        self.raw, self.nbytes, self.shape, self.dtype, self.site, self.start, self.note = raw, nbytes, shape, dtype, site, start, note

    def describe(self) -> str:
        return f"{self.note} {tuple(self.shape)} {self.dtype} ({self.nbytes} bytes) allocated at {self.site}"


def _call_site() -> str:
    f = sys._getframe(1)
    out = []
    while f is not None and len(out) < 2:
        name = f.f_code.co_filename
        if name != _THIS_FILE and "/torch/" not in name:
            out.append(f"{name}:{f.f_lineno} in {f.f_code.co_name}")
        f = f.f_back
    return " <- ".join(out) if out else "?"


def _sizes(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


def _dense(shape, strides) -> bool:
    """Non-overlapping and dense: some permutation of the dimensions is contiguous."""
    want = 1
    for size, stride in sorted(((n, s) for n, s in zip(shape, strides) if n != 1), key=lambda p: p[1]):
        if stride != want:
            return False
        want *= size
    return True


def _make_store():
    """A hip_ops.WorkspaceStore that forgets: ``workspace()`` finds no buffer, allocates one of exactly the requested size
    through the patched ``torch.empty`` / ``torch.zeros`` -- an arena -- and stores it; the next request, smaller, larger or
    equal, gets a new one."""
    from objcavit_amd import hip_ops

    class ExactStore(hip_ops.WorkspaceStore):
        def get(self, key, default=None):
            return default

    return ExactStore()


class guarded:
    def __init__(self, device, guard_bytes: int = DEFAULT_GUARD_BYTES, workspaces: bool = True):
        self.device = torch.device(device)
        if guard_bytes <= 0 or guard_bytes % 512:
            raise ValueError("guard_bytes must be a positive multiple of 512")
        self.guard_bytes = int(guard_bytes)
        self.workspaces = workspaces
        self.arenas: List[Arena] = []
        self._starts: List[int] = []              # payload start addresses, sorted, and the arena at each
        self._at = {}
        self.calls: List[str] = []                # every ocv_* call, in order (record_calls)
        self.stray: List[tuple] = []              # (name, argument index, pointer) of pointers in no guarded payload
        self._saved = {}
        self._scope = None
        self._load = None
        self._expect = None
        self._open = False

    # ------------------------------------------------------------------ scope
    def __enter__(self):
        for name in ALLOCATORS:
            self._saved[name] = getattr(torch, name)
        try:
            for name in ALLOCATORS:
                setattr(torch, name, self._wrap(name, self._saved[name]))
            if self.workspaces:
                from objcavit_amd import hip_ops
                self.store = _make_store()
                self._scope = hip_ops.workspace_scope(self.store)
                self._scope.__enter__()
        except BaseException:
            self._restore()
            raise
        self._open = True
        return self

    def __exit__(self, et, ev, tb):
        self._restore()
        if et is None:
            self.check()
        return False

    def _restore(self):
        self._open = False
        for name, fn in self._saved.items():
            setattr(torch, name, fn)
        self._saved = {}
        if self._scope is not None:
            self._scope.__exit__(None, None, None)
            self._scope = None
        if self._load is not None:
            from objcavit_amd import _lib
            _lib.load = self._load
            self._load = None

    # ------------------------------------------------------------------ allocation
    def _mine(self, device) -> bool:
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
        d = torch.device(device)
        if d.type != self.device.type:
            return False
        if d.type == "cpu":
            return True
        if torch.cuda.is_current_stream_capturing():
            return False
        cur = torch.cuda.current_device()
        return (cur if d.index is None else d.index) == (cur if self.device.index is None else self.device.index)

    def _real(self, name):
        return self._saved.get(name) or getattr(torch, name)

    def _arena(self, shape, dtype, strides=None, note="tensor") -> torch.Tensor:
        """A new arena; -> its payload, still holding the pattern."""
        numel = 1
        for s in shape:
            numel *= s
        item = self._real("empty")((), dtype=dtype, device="meta").element_size()
        nbytes = numel * item
        g = self.guard_bytes
        total = (2 * g + nbytes + 3) // 4 * 4
        raw = self._real("empty")(total, dtype=torch.uint8, device=self.device)
        raw.view(torch.int32).fill_(_PATTERN_I32)
        body = raw[g:g + nbytes]
        flat = body.view(dtype)
        if strides is None:
            t = flat.view(shape)
        else:
            t = flat.as_strided(shape, strides)
        a = Arena(raw, nbytes, tuple(shape), dtype, _call_site(), raw.data_ptr() + g, note)
        self.arenas.append(a)
        bisect.insort(self._starts, a.start)
        self._at[a.start] = a
        return t

    def _strides(self, shape, dtype, memory_format):
        if memory_format in (None, torch.contiguous_format):
            return None
        return self._real("empty")(shape, dtype=dtype, device="meta", memory_format=memory_format).stride()

    def _like_strides(self, t, dtype, memory_format):
        meta = torch.empty_strided(tuple(t.shape), tuple(t.stride()), dtype=t.dtype, device="meta")
        kw = {} if memory_format is None else {"memory_format": memory_format}
        return self._real("empty_like")(meta, dtype=dtype, **kw).stride()

    def _factory(self, name, args, kw):
        """-> payload (pattern inside) and the fill value (None: leave the pattern), or _PASS."""
        kw = dict(kw)
        if kw.pop("out", None) is not None or kw.pop("pin_memory", False) or kw.pop("layout", torch.strided) != torch.strided:
            return _PASS, None
        kw.pop("names", None)
        like = name.endswith("_like")
        fill = {"zeros": 0, "ones": 1, "zeros_like": 0, "ones_like": 1}.get(name)
        args = list(args)
        if like:
            src = args.pop(0) if args else kw.pop("input")
            if not isinstance(src, torch.Tensor) or src.layout != torch.strided:
                return _PASS, None
            if name == "full_like":
                fill = args.pop(0) if args else kw.pop("fill_value")
            device = kw.pop("device", None) or src.device
            dtype = kw.pop("dtype", None) or src.dtype
            mf = kw.pop("memory_format", None)
            shape = tuple(src.shape)
        else:
            if name == "full":
                size = args.pop(0) if args else kw.pop("size")
                fill = args.pop(0) if args else kw.pop("fill_value")
                shape = _sizes((size,))
            else:
                shape = _sizes(args) if args else _sizes((kw.pop("size"),))
            device = kw.pop("device", None)
            dtype = kw.pop("dtype", None)
            mf = kw.pop("memory_format", None)
            if dtype is None:
                if name == "full" and not isinstance(fill, torch.Tensor):
                    dtype = (torch.bool if isinstance(fill, bool) else torch.int64 if isinstance(fill, int)
                             else torch.get_default_dtype() if isinstance(fill, float) else None)
                else:
                    dtype = torch.get_default_dtype()
        requires_grad = kw.pop("requires_grad", False)
        if kw or dtype not in _HANDLED or not self._mine(device) or isinstance(fill, torch.Tensor):
            return _PASS, None
        if dtype == torch.bool and fill is None:           # pattern bytes are no booleans
            return _PASS, None
        strides = self._like_strides(src, dtype, mf) if like else self._strides(shape, dtype, mf)
        t = self._arena(shape, dtype, strides, note=f"torch.{name}")
        if requires_grad:
            t.requires_grad_(True)
        return t, fill

    def _wrap(self, name, real):
        if name in ("tensor", "arange"):
            def data_factory(*args, **kw):
                t = real(*args, **kw)
                if (isinstance(t, torch.Tensor) and t.layout == torch.strided and t.dtype in _HANDLED and not t.requires_grad
                        and kw.get("out") is None and self._open and self._mine(t.device)):
                    return self.copy(t, note=f"torch.{name}")
                return t
            data_factory.__wrapped__ = real
            return data_factory

        def factory(*args, **kw):
            if not self._open:
                return real(*args, **kw)
            t, fill = self._factory(name, args, kw)
            if t is _PASS:
                return real(*args, **kw)
            if fill is not None:
                with torch.no_grad():
                    t.fill_(fill)
            return t
        factory.__wrapped__ = real
        return factory

    def copy(self, t: torch.Tensor, note: str = "copy") -> torch.Tensor:
        """A guarded copy of ``t`` on the guarded device: same shape, dtype and (for a dense tensor) strides."""
        if t.dtype not in _HANDLED:
            raise TypeError(f"mem_guard.copy: {t.dtype} is not handled")
        dense = t.numel() > 0 and _dense(t.shape, t.stride())
        out = self._arena(tuple(t.shape), t.dtype, tuple(t.stride()) if dense and not t.is_contiguous() else None, note=note)
        with torch.no_grad():
            out.copy_(t.detach())
        return out

    # ------------------------------------------------------------------ checks
    def _expected(self, phase: int, n: int) -> torch.Tensor:
        need = self.guard_bytes + 8
        if self._expect is None:
            pat = self._real("tensor")(_PATTERN_BYTES, dtype=torch.uint8, device=self.device)
            self._expect = pat.repeat((need + 3) // 4)
        return self._expect[phase:phase + n]

    def _arena_of(self, ptr: int) -> Optional[Arena]:
        i = bisect.bisect_right(self._starts, ptr) - 1
        if i < 0:
            return None
        a = self._at[self._starts[i]]
        return a if (ptr < a.start + a.nbytes or (a.nbytes == 0 and ptr == a.start)) else None

    def check(self) -> None:
        """Compare both guards of every arena with the pattern; raise ``Breach`` naming every breached allocation."""
        if not self.arenas:
            return
        g = self.guard_bytes
        flags = []
        for a in self.arenas:
            lead = a.raw[:g]
            tail = a.raw[g + a.nbytes:]
            flags.append((lead != self._expected(0, g)).any())
            flags.append((tail != self._expected((g + a.nbytes) % 4, tail.numel())).any())
        bad = torch.stack(flags).cpu().view(-1, 2)
        msgs = []
        for a, (bl, bt) in zip(self.arenas, bad.tolist()):
            for which, hit in (("leading", bl), ("trailing", bt)):
                if not hit:
                    continue
                lo = 0 if which == "leading" else g + a.nbytes
                region = a.raw[:g] if which == "leading" else a.raw[g + a.nbytes:]
                idx = (region != self._expected(lo % 4, region.numel())).nonzero().flatten()
                first, last = int(idx[0]) + lo - g, int(idx[-1]) + lo - g
                msgs.append(f"{which} guard of {a.describe()}: {idx.numel()} byte(s) changed, first at payload offset {first}, "
                            f"last at {last} (payload is bytes 0..{a.nbytes - 1})")
        if msgs:
            raise Breach("memory written outside an operand:\n  " + "\n  ".join(msgs))

    def never_written(self, t: torch.Tensor) -> int:
        """How many whole 32-bit words of ``t``'s memory still hold the pattern exactly.  ``t`` is a dense payload (or a dense
        view of one); a strided view is judged on its own elements where they are 4 or 8 bytes wide."""
        if t.numel() == 0:
            return 0
        dense = _dense(t.shape, t.stride())
        if not dense:
            if t.element_size() not in (4, 8):
                raise ValueError("never_written: a strided view of 1- or 2-byte elements has no 32-bit words of its own")
            return int((t.contiguous().view(-1).view(torch.int32) == _PATTERN_I32).sum())
        a = self._arena_of(t.data_ptr())
        if a is None:
            raise ValueError("never_written: the tensor is not inside a guarded payload")
        g = self.guard_bytes
        lo = g + (t.data_ptr() - a.start)
        hi = lo + t.numel() * t.element_size()
        w0, w1 = (lo + 3) // 4, hi // 4                    # whole words of the arena inside [lo, hi): the pattern's own phase
        if w1 <= w0:
            return 0
        return int((a.raw.view(torch.int32)[w0:w1] == _PATTERN_I32).sum())

    # ------------------------------------------------------------------ call recorder
    def record_calls(self):
        """Swap ``objcavit_amd._lib.load`` for a proxy over the loaded library until the scope ends."""
        from objcavit_amd import _lib
        if self._load is not None:
            return self
        real_load = _lib.load
        lib = real_load()
        guard = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                proto = _lib.PROTOTYPES.get(name)
                if not name.startswith("ocv_") or proto is None:
                    return fn
                argtypes = proto[1]

                def call(*args):
                    guard.calls.append(name)
                    last = len(argtypes) - 1
                    for i, (ty, v) in enumerate(zip(argtypes, args)):
                        if ty is not C.c_void_p or not isinstance(v, int) or v == 0:
                            continue                       # (ctypes.POINTER types are host structs / host arrays: exempt)
                        if i == last and name.endswith("_fwd"):
                            continue                       # the stream
                        if guard._arena_of(v) is None:
                            guard.stray.append((name, i, v))
                    return fn(*args)
                return call

        proxy = Proxy()
        self._load = real_load
        _lib.load = lambda path=None: proxy if path is None else real_load(path)
        return self
