"""Statement R of the resize on ingest (csrc/frame_resize.hip, hip_ops.resize_taps), in float64 on the host, written out tap by tap.

Per axis, ``n_in -> n_out``, all in float64:
    s = n_in / n_out,  support = max(s, 1),  inv = 1 / max(s, 1)
    output i:  c = s (i + 0.5),  lo = max(0, int(c - support + 0.5)),  hi = min(n_in, int(c + support + 0.5))   (int truncates)
               w_j = max(0, 1 - |(j - c + 0.5) inv|)  for j = lo .. hi - 1, divided by their sum
Output, (top, left, Hw, Ww) the window:
    out[b, ch, y, x] = sum_j sum_k wy[y][j] wx[x][k] table[ch][ frames[b, top + ylo[y] + j, left + xlo[x] + k, ch] ]
The mirrored half is the flip along W of that, not a resize of the flipped frame.  It is the antialiased triangle filter, separable,
half-pixel centred: tests/test_resize_host.py pins it to torch's CPU float64 ``interpolate(antialias=True)``.
"""
import torch


def taps(n_in, n_out):
    """-> [(lo, [w_lo, ..., w_hi-1])] per output index: Python floats are float64."""
    s = n_in / n_out
    support = max(s, 1.0)
    inv = 1.0 / max(s, 1.0)
    rows = []
    for i in range(n_out):
        c = s * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        w = [max(0.0, 1.0 - abs((j - c + 0.5) * inv)) for j in range(lo, hi)]
        total = sum(w)
        rows.append((lo, [v / total for v in w]))
    return rows


def matrix(n_in, n_out):
    """The dense float64 [n_out, n_in] matrix of one axis."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i, (lo, w) in enumerate(taps(n_in, n_out)):
        m[i, lo:lo + len(w)] = torch.tensor(w, dtype=torch.float64)
    return m


def max_taps(n_in, n_out):
    return max(len(w) for _, w in taps(n_in, n_out))


def resized_input(frames, table, top, left, Hw, Ww, H, W, mirror=False):
    """frames uint8 [B, Hs, Ws, 3], table [3, 256] -> float64 [B (2 B with ``mirror``), 3, H, W]."""
    win = frames[:, top:top + Hw, left:left + Ww].long()
    vals = torch.stack([table.double()[c][win[..., c]] for c in range(3)], 1)            # [B, 3, Hw, Ww]
    out = matrix(Hw, H) @ vals @ matrix(Ww, W).t()
    return torch.cat([out, out.flip(3)], 0) if mirror else out


def bar(Hw, Ww, H, W, table):
    """The derived bar of the fp32 two-pass evaluation against R: one rounding per tap and pass plus the weights' own."""
    return (max_taps(Hw, H) + max_taps(Ww, W) + 4) * 2.0 ** -24 * float(table.abs().max())
