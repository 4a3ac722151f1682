"""Statement P of the pixel formats on ingest (csrc/pixel_fetch.hpp, objcavit_amd/pixel_formats.py), in numpy integers on the host.

Formats: rgb24 / bgr24 [B, Hs, Ws, 3]; rgba32 / bgra32 [B, Hs, Ws, 4] (alpha ignored); nv12 = (Y [B, Hs, Ws], CbCr [B, Hc, Wc, 2]);
i420 = (Y, Cb [B, Hc, Wc], Cr [B, Hc, Wc]) with Hc = ceil(Hs / 2), Wc = ceil(Ws / 2).  Pixel (x, y) takes chroma sample (x >> 1, y >> 1).

    Kr, Kb: bt601 0.299, 0.114; bt709 0.2126, 0.0722; Kg = 1 - Kr - Kb.   y0, sy, sc: limited 16, 255 / 219, 255 / 224; full 0, 1, 1.
    T0[v] = rint(2^16 sy (v - y0)) + 2^15                       T1[v] = rint(2^16 sc 2 (1 - Kr) (v - 128))
    T2[v] = rint(2^16 sc (-2 Kb (1 - Kb) / Kg) (v - 128))       T3[v] = rint(2^16 sc (-2 Kr (1 - Kr) / Kg) (v - 128))
    T4[v] = rint(2^16 sc 2 (1 - Kb) (v - 128))
    R = clamp((T0[Y] + T1[Cr]) >> 16)   G = clamp((T0[Y] + T2[Cb] + T3[Cr]) >> 16)   B = clamp((T0[Y] + T4[Cb]) >> 16)

``>>`` is the arithmetic shift (numpy's on signed integers), clamp is to 0 .. 255.  Nothing here imports the package.
"""
import numpy as np

K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGE = {"limited": (16, 255 / 219, 255 / 224), "full": (0, 1.0, 1.0)}
PACKED = {"rgb24": (0, 1, 2), "bgr24": (2, 1, 0), "rgba32": (0, 1, 2), "bgra32": (2, 1, 0)}     # where R, G, B sit in a pixel


def coefficients(matrix, range_):
    """(y0, sy, [Cr -> R, Cb -> G, Cr -> G, Cb -> B] already times sc) in float64."""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    y0, sy, sc = RANGE[range_]
    return y0, sy, [sc * 2 * (1 - kr), sc * (-2 * kb * (1 - kb) / kg), sc * (-2 * kr * (1 - kr) / kg), sc * 2 * (1 - kb)]


def tables(matrix, range_):
    """int64 [5, 256]: every entry on its own, from Python floats (float64), rounded once with round() (ties to even, as rint)."""
    y0, sy, c = coefficients(matrix, range_)
    t = np.zeros((5, 256), dtype=np.int64)
    for v in range(256):
        t[0, v] = round(65536 * sy * (v - y0)) + 32768
        for i in range(4):
            t[1 + i, v] = round(65536 * c[i] * (v - 128))
    return t


def ycbcr_to_rgb(y, cb, cr, matrix, range_):
    """Arrays of Y, Cb, Cr of one shape -> uint8 [..., 3] by Statement P."""
    t = tables(matrix, range_)
    y, cb, cr = (np.asarray(a).astype(np.int64) for a in (y, cb, cr))
    r = (t[0][y] + t[1][cr]) >> 16
    g = (t[0][y] + t[2][cb] + t[3][cr]) >> 16
    b = (t[0][y] + t[4][cb]) >> 16
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def real_rgb(y, cb, cr, matrix, range_):
    """The float64 real-coefficient formula rounded half up: clamp(floor(x + 0.5)) -> int64 [..., 3]."""
    y0, sy, c = coefficients(matrix, range_)
    y, cb, cr = (np.asarray(a).astype(np.float64) for a in (y, cb, cr))
    l = sy * (y - y0)
    r = l + c[0] * (cr - 128)
    g = l + c[1] * (cb - 128) + c[2] * (cr - 128)
    b = l + c[3] * (cb - 128)
    return np.clip(np.floor(np.stack([r, g, b], -1) + 0.5), 0, 255).astype(np.int64)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def rgb_of(frames, fmt, top, left, Hw, Ww):
    """The Hw x Ww window at (top, left) of ``frames`` as uint8 [B, Hw, Ww, 3].  ``fmt``: (name, matrix, range), or an object with
    those attributes; ``frames``: one array / tensor for the packed formats, a sequence of planes for nv12 / i420."""
    name, matrix, range_ = fmt if isinstance(fmt, tuple) else (fmt.name, fmt.matrix, fmt.range)
    if name in PACKED:
        f = _np(frames)
        assert f.ndim == 4 and f.shape[3] == (4 if name.endswith("32") else 3)
        return np.ascontiguousarray(f[:, top:top + Hw, left:left + Ww][..., list(PACKED[name])])
    planes = [_np(p) for p in frames]
    y = planes[0]
    B, Hs, Ws = y.shape
    rows = (np.arange(top, top + Hw) >> 1)[:, None]
    cols = (np.arange(left, left + Ww) >> 1)[None, :]
    if name == "nv12":
        assert len(planes) == 2 and planes[1].shape[1] >= (Hs + 1) // 2 and planes[1].shape[2] >= (Ws + 1) // 2
        cb, cr = planes[1][:, rows, cols, 0], planes[1][:, rows, cols, 1]
    else:
        assert name == "i420" and len(planes) == 3
        cb, cr = planes[1][:, rows, cols], planes[2][:, rows, cols]
    return ycbcr_to_rgb(y[:, top:top + Hw, left:left + Ww], cb, cr, matrix, range_)
