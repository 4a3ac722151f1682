"""-m gpu: every unit of the token path -- the layer tails, the fused next projection, the attention core on the operands a
stack hands it, the two cross-attentions on stack outputs -- called through the C ABI on its own and compared with float64
on the float32 tensors it actually read (tests/token_ref.py, anchored in tests/test_token_units_host.py).

Deviation = util.rel_dev = max |y - ref| / max |ref|.  BARS ARE NOT CONSTANTS: a unit's bar is margin x max(d32, 2e-7), d32 = the
deviation of the same token_ref formula evaluated in float32 on the CPU, on the same input, in the same run; never above
TOL = 2e-5.  Margin 4 for the two-term fp16 kernels: operand rounding (<= d32, shown by the host test) + float32 accumulation in
another order (~ d32), times two; margin 2 for the three-term bf16 and exact-fp32 kernels (accumulation order, times two).

One margin had to be raised: x2 of the three-term tail, 8 (see TAIL_MARGIN).

MEASURED (MI355X): per unit the case with the largest deviation / max(d32, 2e-7), over the direct calls AND the stacks' own
intermediates, as deviation / d32 of that case / bar of that case (n = checks made):
  ocv_layer_tail_h2_fwd        x2        3.0e-7 / 2.3e-7 / 9.2e-7   (n 54)     qkv_next  1.3e-7 / 1.9e-7 / 8.0e-7   (n 29)
  ocv_layer_tail_h2_ws_fwd     x2        2.9e-7 / 2.8e-7 / 1.1e-6   (n 62)     qkv_next  1.8e-7 / 2.3e-7 / 9.2e-7   (n 35)
  ocv_layer_tail_split3_fwd    x2        6.1e-7 / 2.6e-7 / 2.1e-6   (n 70)     qkv_next  2.8e-7 / 2.2e-7 / 4.4e-7   (n 41)
  ocv_linear_split3_fwd        qkv of layer 0                3.9e-7 / 3.9e-7 / 7.8e-7   (n 12)
  ocv_attention_fwd            h2  2.6e-7 / 1.6e-7 / 8.0e-7  (n 56)            fp32  5.9e-7 / 4.3e-7 / 8.7e-7   (n 8)
  cross-attention #1, 9 live keys     h2  1.4e-7 / 3.2e-7 / 1.3e-6    split3  2.6e-7 / 3.2e-7 / 6.3e-7    fp32  2.6e-7 / 3.2e-7 / 6.3e-7
  cross-attention #2, 132 keys        h2 = split3  7.7e-7 / 6.5e-7 / 2.6e-6                               fp32  6.1e-7 / 6.5e-7 / 2.6e-6
  full object tensor: #1              h2 = split3  3.7e-7 / 4.2e-7 / 1.7e-6                               fp32  4.7e-7 / 4.2e-7 / 1.7e-6
                      #2              h2 = split3  4.8e-7 / 5.5e-7 / 2.2e-6                               fp32  5.2e-7 / 5.5e-7 / 2.2e-6
Every hand chain equalled its stack bit for bit.
"""
import copy
import ctypes as C
import functools
import math

import pytest
import torch

import gen
import token_cases as tc
import token_ref as tr
from util import rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 2e-5
FLOOR = 2e-7
SENT = 777.0                 # rows behind M hold this before a call and must hold it afterwards
H2, EXACT = 4, 2             # margins: two-term fp16 kernels / three-term bf16 and exact-fp32 kernels (module docstring)
# The three-term tail's x2 at 8, not 2: it measured up to 2.34 x d32 (6.1e-7 against d32 2.6e-7, M = 31) where the two-term fp16
# tails stay at 1.3 x.  Rounding only, by the kernel's text: mfma6 (csrc/token_tile.hpp) adds all six bf16 products of a K step into
# ONE fp32 accumulator, so the running sum is rounded six times per step -- 384 times over the feed-forward block's 1024 hidden
# units -- where the two-term kernel keeps hi.hi in an accumulator of its own (once per step) and float32 on the CPU sums in
# vector lanes; operands (24 bits) and dropped products (2^-27) are below that.  Restating that order of summation in float32 on
# the CPU gives the same picture (three-term 1.5 - 1.8 x d32, two-term 0.7 - 1.0 x).  8 = the smallest power of two with 2 x
# headroom over the measured worst.  Its qkv_next (one 128-long product: 1.3 x) keeps 2.
TAIL_MARGIN = {("h2", "x2"): H2, ("h2", "qkv_next"): H2, ("h2_ws", "x2"): H2, ("h2_ws", "qkv_next"): H2,
               ("split3", "x2"): 8, ("split3", "qkv_next"): EXACT}
PAD_VALUE = 1e-4


def bar(margin, d32):
    b = margin * max(d32, FLOOR)
    assert b <= TOL, (margin, d32)
    return b


def report(unit, dev, d32, b):
    print(f"UNIT {unit}: dev {dev:.3e} d32 {d32:.3e} bar {b:.3e}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def ops():
    from objcavit_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@functools.lru_cache(maxsize=None)
def _enc():
    return tc.encoder()


class DevLayer:
    """One layer on the device with every packed form of its weights (three-term bf16 and two-term fp16), + its CPU parameters."""

    def __init__(self, ops, module):
        assert ops.token_mode() == "h2"                     # (layer_params packs the fp16 copies only in this mode)
        self.cpu = tc.params(module)
        self.mod = copy.deepcopy(module).cuda()
        self.cache = {}
        self.st, self.keep = ops.layer_params(self.mod, self.cache)
        assert self.st.out_proj_h2 and self.st.out_proj_p3 and self.st.in_proj_h2 and self.st.in_proj_p3


_DEV = {}


def dev_layer(ops, l, FF=1024):
    if (l, FF) not in _DEV:
        _DEV[(l, FF)] = DevLayer(ops, tc.layer_module(_enc(), l, FF))
    return _DEV[(l, FF)]


def run_tail(lib, kind, st, nxt, ctx, x, M, FF, mask=None, ws=None):
    """One ocv_layer_tail_* call on ctx / x [M, 128] (device).  ``nxt``: the next layer's struct or None.  Returns (rc, out
    [M + 32, 128], qkv_next [M + 32, 384]); the 32 rows behind M, and all of qkv_next without ``nxt``, are sentinels."""
    out = torch.full((M + 32, 128), SENT, device="cuda")
    qkv = torch.full((M + 32, 384), SENT, device="cuda")
    wq = None if nxt is None else (nxt.in_proj_p3 if kind == "split3" else nxt.in_proj_h2)
    assert nxt is None or wq
    args = (ctx.data_ptr(), x.data_ptr(), C.byref(st), wq, None if nxt is None else nxt.in_proj_b, 1e-5, _ptr(mask), out.data_ptr(),
            None if nxt is None else qkv.data_ptr(), M, 128, FF)
    if kind == "split3":
        rc = lib.ocv_layer_tail_split3_fwd(*args, _stream())
    elif kind == "h2":
        rc = lib.ocv_layer_tail_h2_fwd(*args, _stream())
    else:
        rc = lib.ocv_layer_tail_h2_ws_fwd(*args, ws.data_ptr(), ws.numel(), _stream())
    return rc, out, qkv


def tail_workspace(lib, M, FF):
    return torch.zeros(max(int(lib.ocv_layer_tail_h2_workspace_bytes(M, FF)), 16), dtype=torch.uint8, device="cuda")


def tickets(lib, ws, M, FF):
    """The arrival tickets behind the partial sums of a few-token tail's workspace (empty when the form is not shared out)."""
    if int(lib.ocv_layer_tail_h2_workspace_bytes(M, FF)) == 0:
        return ws[:0]
    nblk, G = (M + 31) // 32, int(lib.ocv_layer_tail_h2_groups(M, FF))
    off = nblk * G * 32 * 128 * 4
    return ws[off:off + 4 * nblk]


def run_attention(lib, ops, packed, mask, B, S):
    """ocv_attention_fwd on a packed [B * S, 384] projection with the strides ocv_encoder_stack_fwd uses -> ctx [B * S + 32, 128]."""
    ops.attention_form_sync()
    ctx = torch.full((B * S + 32, 128), SENT, device="cuda")
    p = packed.data_ptr()
    rc = lib.ocv_attention_fwd(p, S * 384, 384, p + 128 * 4, S * 384, 384, p + 256 * 4, S * 384, 384, _ptr(mask), ctx.data_ptr(),
                               S * 128, 128, B, 4, S, S, 1.0 / math.sqrt(32.0), _stream())
    assert rc == 0
    return ctx


def check_tail_outputs(unit, kind, out, qkv, M, ctx_cpu, x_cpu, p, nxt_cpu, zero_rows=None):
    """(a): x2 against tail() on (ctx, x); qkv_next against qkv() on the kernel's OWN out."""
    x2_64 = tr.tail(ctx_cpu.double(), x_cpu.double(), p)[1]
    x2_32 = tr.tail(ctx_cpu, x_cpu, p)[1]
    if zero_rows is not None:
        x2_64, x2_32 = x2_64.masked_fill(zero_rows[:, None], 0.0), x2_32.masked_fill(zero_rows[:, None], 0.0)
    d32 = rel_dev(x2_32, x2_64)
    dev = rel_dev(out[:M], x2_64)
    margin = TAIL_MARGIN[(kind, "x2")]
    report(f"{unit} x2", dev, d32, bar(margin, d32))
    assert dev < bar(margin, d32), (unit, "x2", dev, d32)
    if nxt_cpu is not None:
        own = out[:M].cpu()
        wq, bq = nxt_cpu["self_attn.in_proj_weight"], nxt_cpu["self_attn.in_proj_bias"]
        q_64 = tr.qkv(own.double(), wq, bq)
        d32q = rel_dev(tr.qkv(own, wq, bq), q_64)
        devq = rel_dev(qkv[:M], q_64)
        margin = TAIL_MARGIN[(kind, "qkv_next")]
        report(f"{unit} qkv_next", devq, d32q, bar(margin, d32q))
        assert devq < bar(margin, d32q), (unit, "qkv_next", devq, d32q)


def check_attention(unit, margin, ctx, packed, mask_cpu, B, S):
    """(c): the attention core against attention() on the packed buffer it read."""
    pk = packed[:B * S].cpu().view(B, S, 384)
    ref = tr.attention(pk.double(), mask_cpu)
    d32 = rel_dev(tr.attention(pk, mask_cpu), ref)
    dev = rel_dev(ctx[:B * S].view(B, S, 128), ref)
    report(unit, dev, d32, bar(margin, d32))
    assert dev < bar(margin, d32), (unit, dev, d32)
    assert bool((ctx[B * S:] == SENT).all())


# ------------------------------------------------------------------ (a) the tails, one call each
GROUPS = {(1, 1024): 8, (31, 1024): 8, (32, 1024): 8, (33, 1024): 8, (768, 1024): 8, (769, 1024): 4, (1792, 1024): 4, (1793, 1024): 1,
          (33, 128): 1, (33, 256): 2, (33, 384): 1, (33, 512): 4, (33, 640): 1, (33, 768): 2,
          (769, 128): 1, (769, 256): 2, (769, 384): 1, (769, 512): 4, (769, 640): 1, (769, 768): 2}
TAIL_CASES = [(M, 1024, 0) for M in (1, 31, 32, 33, 768, 769, 1792, 1793)] + [(M, 1024, 2) for M in (33, 769, 1793)] + \
             [(M, FF, 0) for M in (33, 769) for FF in (128, 256, 384, 512, 640, 768)]


@pytest.mark.parametrize("M,FF,l", TAIL_CASES)
@pytest.mark.parametrize("kind", ["h2", "h2_ws", "split3"])
def test_layer_tail_alone(ops, lib, kind, M, FF, l):
    """ocv_layer_tail_h2_fwd (one workgroup per row block: FF / 128 = 1 .. 8 feed-forward chunks in one workgroup, every remainder
    of the period-three fragment rotation), ocv_layer_tail_h2_ws_fwd (G workgroups per row block on a zeroed workspace: both sides
    of the 24 and 56 row-block boundaries, layer_tail_h2_kernel<2> at FF = 256 / 768) and ocv_layer_tail_split3_fwd, with layer
    l's parameters, with layer l + 1's packed in-projection and without one; one row, around the 32-row tile, ragged last row
    blocks.  x2 and qkv_next against float64, rows >= M untouched, tickets left zero, a second call bit-identical, and with a
    zero_row_mask (every third row, no next projection) masked rows exactly 0 and every other row bit-identical.
    Measured worst / d32: x2 h2 3.0e-7 / 2.3e-7, h2_ws 2.9e-7 / 2.8e-7, split3 6.1e-7 / 2.6e-7 (margin 8, TAIL_MARGIN); qkv_next h2
    1.3e-7 / 1.9e-7, h2_ws 1.8e-7 / 2.3e-7, split3 2.8e-7 / 2.2e-7."""
    assert int(lib.ocv_layer_tail_h2_groups(M, FF)) == GROUPS[(M, FF)] == tc.expected_groups(M, FF)
    assert (int(lib.ocv_layer_tail_h2_workspace_bytes(M, FF)) > 0) == (GROUPS[(M, FF)] > 1)
    dl, nx = dev_layer(ops, l, FF), dev_layer(ops, l + 1)
    ctx_cpu, x_cpu = tc.tail_inputs(M, tc.tail_seed(M, FF, l))
    ctx, x = ctx_cpu.cuda(), x_cpu.cuda()
    ws = tail_workspace(lib, M, FF) if kind == "h2_ws" else None
    unit = f"tail_{kind}"
    outs = []
    for nxt in (nx, None):
        rc, out, qkv = run_tail(lib, kind, dl.st, None if nxt is None else nxt.st, ctx, x, M, FF, None, ws)
        assert rc == 0
        rc2, out2, qkv2 = run_tail(lib, kind, dl.st, None if nxt is None else nxt.st, ctx, x, M, FF, None, ws)
        torch.cuda.synchronize()
        assert rc2 == 0 and torch.equal(out, out2) and torch.equal(qkv, qkv2)
        assert bool((out[M:] == SENT).all()) and bool((qkv[M if nxt is not None else 0:] == SENT).all())
        if ws is not None:
            assert int(tickets(lib, ws, M, FF).to(torch.int32).abs().sum()) == 0
        check_tail_outputs(unit, kind, out, qkv, M, ctx_cpu, x_cpu, dl.cpu, None if nxt is None else nxt.cpu)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])                                    # the next projection does not touch x2
    mask = (torch.arange(M) % 3 == 0).to(torch.uint8).cuda()
    rc, outm, qkvm = run_tail(lib, kind, dl.st, None, ctx, x, M, FF, mask, ws)
    torch.cuda.synchronize()
    assert rc == 0 and bool((outm[M:] == SENT).all()) and bool((qkvm == SENT).all())
    z = mask.bool()
    assert float(outm[:M][z].abs().max()) == 0.0 and torch.equal(outm[:M][~z], outs[1][:M][~z])


# ------------------------------------------------------------------ (b) masked rows + next projection: rejected
@pytest.mark.parametrize("kind", ["h2", "h2_ws", "split3"])
def test_layer_tail_rejects_a_row_mask_together_with_a_next_projection(ops, lib, kind):
    """qkv_next is projected from the LN2 tile, not from the zeroed rows of ``out`` (include/objcavit_hip.h): the combination returns
    -1 before any launch, ocv_last_error() names it, nothing is written."""
    M, FF = 33, 1024
    dl, nx = dev_layer(ops, 0), dev_layer(ops, 1)
    ctx_cpu, x_cpu = tc.tail_inputs(M, 5)
    ws = tail_workspace(lib, M, FF)
    mask = (torch.arange(M) % 3 == 0).to(torch.uint8).cuda()
    rc, out, qkv = run_tail(lib, kind, dl.st, nx.st, ctx_cpu.cuda(), x_cpu.cuda(), M, FF, mask, ws)
    msg = lib.ocv_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0
    assert "zero_row_mask" in msg and "next projection" in msg and msg.startswith("ocv_layer_tail_" + ("split3" if kind == "split3" else "h2")), msg
    assert bool((out == SENT).all()) and bool((qkv == SENT).all()) and int(ws.to(torch.int32).sum()) == 0


# ------------------------------------------------------------------ (c) attention on a tail's packed projection
@pytest.mark.parametrize("B,S,counts", [(1, 1, [1]), (3, 33, [33, 7, 1]), (2, 129, [129, 128]), (2, 300, [300, 100])])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_attention_on_a_tails_packed_projection(ops, lib, monkeypatch, form, masked, B, S, counts):
    """ocv_attention_fwd on the packed [B, S, 384] rows ocv_layer_tail_h2_fwd just wrote, addressed as the stack addresses them:
    both forms, with and without a key-padding mask; one key, ragged tiles, a second 128-key chunk holding one key (live or,
    masked, dead), several chunks.  Measured worst / d32: h2 2.6e-7 / 1.6e-7, fp32 5.9e-7 / 4.3e-7."""
    monkeypatch.setenv("OCV_ATTN_FORM", form)
    M = B * S
    dl, nx = dev_layer(ops, 0), dev_layer(ops, 1)
    ctx_cpu, x_cpu = tc.tail_inputs(M, 70 + S)
    rc, out, qkv = run_tail(lib, "h2", dl.st, nx.st, ctx_cpu.cuda(), x_cpu.cuda(), M, 1024)
    assert rc == 0
    mask_cpu = tc.key_mask(counts, S) if masked else None
    ctx = run_attention(lib, ops, qkv, None if mask_cpu is None else mask_cpu.to(torch.uint8).cuda(), B, S)
    torch.cuda.synchronize()
    check_attention(f"attention_{form}", H2 if form == "h2" else EXACT, ctx, qkv, mask_cpu, B, S)


# ------------------------------------------------------------------ (d) the stack is exactly these units
@pytest.fixture(scope="module")
def dev_enc():
    return copy.deepcopy(_enc()).cuda()


@pytest.mark.parametrize("B,S,counts", [(2, 132, None), (4, 300, None), (4, 418, None), (5, 132, None), (2, 1200, None), (3, 7, [7, 3, 1])])
@pytest.mark.parametrize("mode", ["h2", "split3"])
def test_stack_is_exactly_its_units(ops, lib, dev_enc, monkeypatch, mode, B, S, counts):
    """The hand chain -- ocv_linear_split3_fwd for layer 0, then per layer ocv_attention_fwd and the tail in the form
    ocv_encoder_stack_fwd picks (workspace form only for B <= 4 and FF = 1024; the mask and no next projection for the last layer)
    -- gives HipEncoderStack's output BIT FOR BIT under OCV_TOKENS = h2 and = split3: 9 row blocks (G = 8), 38 and 53 (G = 4), B = 5
    and 75 row blocks (G = 1), and the masked object stack.  So the chain's intermediates are the stack's own, and every one of
    them is checked as in (a) and (c): every unit of a real stack on the input it actually read.  Measured: all twelve chains equal in bits; the
    units' figures are folded into the module docstring's table (layer 0's projection 3.9e-7 / 3.9e-7)."""
    from objcavit_amd.modules.layers import HipEncoderStack
    monkeypatch.setenv("OCV_TOKENS", mode)
    monkeypatch.delenv("OCV_ATTN_FORM", raising=False)
    M, FF = B * S, 1024
    x_cpu = gen.randn("x", (B, S, 128), 40 + B)
    mask_cpu = None if counts is None else tc.key_mask(counts, S)
    if mask_cpu is not None:
        x_cpu[mask_cpu] = PAD_VALUE                                           # what object_tokens_pad leaves in padded rows
    x = x_cpu.cuda()
    mask = None if mask_cpu is None else mask_cpu.to(torch.uint8).cuda()
    got = HipEncoderStack(dev_enc)(x, None if mask_cpu is None else mask_cpu.cuda())
    caches = [dict() for _ in dev_enc.layers]
    sts = [ops.layer_params(layer, caches[i]) for i, layer in enumerate(dev_enc.layers)]
    assert all(bool(st.in_proj_h2) == (mode == "h2") for st, _ in sts)
    G = int(lib.ocv_layer_tail_h2_groups(M, FF))
    kind = "split3" if mode == "split3" else ("h2_ws" if B <= 4 and G > 1 else "h2")
    assert (mode, kind) in (("split3", "split3"), ("h2", "h2_ws" if (B, S) in ((2, 132), (4, 300), (4, 418), (3, 7)) else "h2"))
    ws = tail_workspace(lib, M, FF) if kind == "h2_ws" else None
    qkv = torch.full((M + 32, 384), SENT, device="cuda")
    st0 = sts[0][0]
    assert lib.ocv_linear_split3_fwd(x.data_ptr(), 128, st0.in_proj_p3, st0.in_proj_b, qkv.data_ptr(), 384, M, 384, 128, 0, _stream()) == 0
    cur, steps = x.view(M, 128), []
    for l in range(4):
        last = l == 3
        ctx = run_attention(lib, ops, qkv, mask, B, S)
        rc, out, qkv_next = run_tail(lib, kind, sts[l][0], None if last else sts[l + 1][0], ctx[:M], cur, M, FF,
                                     mask.view(M) if (last and mask is not None) else None, ws)
        assert rc == 0
        steps.append((qkv, ctx, cur, out, qkv_next))
        cur, qkv = out[:M], qkv_next
    torch.cuda.synchronize()
    assert torch.equal(cur.view(B, S, 128), got)
    if ws is not None:
        assert int(tickets(lib, ws, M, FF).to(torch.int32).abs().sum()) == 0
    # every unit on the input it read
    p = [tc.params(layer) for layer in _enc().layers]
    q0 = steps[0][0][:M].cpu()
    q_64 = tr.qkv(x_cpu.view(M, 128).double(), p[0]["self_attn.in_proj_weight"], p[0]["self_attn.in_proj_bias"])
    d32 = rel_dev(tr.qkv(x_cpu.view(M, 128), p[0]["self_attn.in_proj_weight"], p[0]["self_attn.in_proj_bias"]), q_64)
    report("stack linear_split3 qkv_0", rel_dev(q0, q_64), d32, bar(EXACT, d32))
    assert rel_dev(q0, q_64) < bar(EXACT, d32)
    for l, (qk, ctx, xin, out, qkv_next) in enumerate(steps):
        last = l == 3
        assert bool((out[M:] == SENT).all()) and bool((qkv_next[0 if last else M:] == SENT).all())
        check_attention(f"stack_{mode} attention_h2", H2, ctx, qk, mask_cpu, B, S)
        check_tail_outputs(f"stack_{mode} tail_{kind}", kind, out, qkv_next, M, ctx[:M].cpu(), xin.cpu(), p[l],
                           None if last else p[l + 1], mask_cpu.view(M) if (last and mask_cpu is not None) else None)
    if mask_cpu is not None:
        assert float(got[mask_cpu.cuda()].abs().max()) == 0.0


# ------------------------------------------------------------------ (e) the cross-attentions on their in-model operands
@pytest.fixture(scope="module")
def saca(ops):
    """A seeded SelfAttnCrossAttn and, by hand, the steps of its forward in front of the cross-attentions: the image stack, the
    object stack (lists of 9, 4 and 1 objects), object_front_pad; + the object stack on a full B x S x E tensor (saca_2's input)."""
    from objcavit_amd.config import make_args
    from objcavit_amd.modules.ObjCAViT import SelfAttnCrossAttn
    assert ops.token_mode() == "h2"
    m = SelfAttnCrossAttn(make_args(no_obj_sa=False), 128, 4, dim_feedforward=1024)
    gen.load_into(m, 31, gen.PEAKY)
    m = m.eval().cuda()
    B, S, counts = 3, 132, [9, 4, 1]
    tok = gen.randn("tok", (B, S, 128), 31).cuda()
    objs = [gen.randn(f"obj{i}", (n, 128), 31).cuda() for i, n in enumerate(counts)]
    att_img = m._img_stack(tok)
    att_obj, mask, cnt = m.object_self_attention(objs, tok.device)
    cap = att_obj.shape[1]
    att_obj_p, kpm = ops.object_front_pad(att_obj, cnt, S, PAD_VALUE)
    full = gen.randn("objfull", (B, S, 128), 32).cuda()
    att_full, mask_full, _ = m.object_self_attention(full, tok.device)
    torch.cuda.synchronize()
    assert cap == 9 and tuple(att_obj_p.shape) == (B, S, 128) and not bool(mask_full.any())
    # rows padded at the FRONT with the constant, mask padded at the BACK
    assert bool((att_obj_p[:, :S - cap] == PAD_VALUE).all()) and torch.equal(kpm.bool().cpu(), tc.key_mask(counts, S))
    return dict(m=m, att_img=att_img, att_obj_p=att_obj_p, kpm=kpm, cap=cap, att_full=att_full, mask_full=mask_full)


def _mha_weights(ca):
    return (ca.in_proj_weight.detach(), ca.in_proj_bias.detach(), ca.out_proj.weight.detach(), ca.out_proj.bias.detach())


def _check_mha(unit, margin, got, q, k, v, w, mask):
    c = lambda t: None if t is None else t.cpu()                          # noqa: E731
    wc = [t.cpu() for t in w]
    ref = tr.mha(c(q).double(), c(k).double(), c(v).double(), *wc, None if mask is None else c(mask).bool())
    d32 = rel_dev(tr.mha(c(q), c(k), c(v), *wc, None if mask is None else c(mask).bool()), ref)
    dev = rel_dev(got, ref)
    report(unit, dev, d32, bar(margin, d32))
    assert not bool(torch.isnan(ref).any()) and dev < bar(margin, d32), (unit, dev, d32)


@pytest.mark.parametrize("mode", ["h2", "split3", "fp32"])
def test_cross_attentions_on_stack_outputs(ops, saca, monkeypatch, mode):
    """final_img = mha(att_img, att_obj_p, att_img, kpm, kv_limit = cap) -- the few-key routes: every contraction two-term fp16 (h2),
    three-term bf16 projections + exact-fp32 scores (split3), one exact-fp32 launch (fp32) -- and final_obj = mha(att_obj_p, att_img,
    att_obj_p) -- 132 keys: projections around the attention core -- on the stacks' outputs and the front-padded object rows; then
    both with a full 3 x 132 x 128 tensor in the object slot (saca_2: no padding, 132 live keys under an all-False mask).  The
    packed-weight cache keys show the route.  Margin 2 where no two-term fp16 product is involved (few keys, split3 / fp32), else 4
    (the attention core of the many-key routes is the two-term fp16 one in every token mode).  Measured worst / d32: #1 few keys
    h2 1.4e-7, split3 2.6e-7, fp32 2.6e-7 / 3.2e-7; #2 7.7e-7 / 6.5e-7; full tensor #1 4.7e-7 / 4.2e-7, #2 5.2e-7 / 5.5e-7."""
    monkeypatch.setenv("OCV_TOKENS", mode)
    monkeypatch.delenv("OCV_ATTN_FORM", raising=False)
    m, att_img, att_obj_p, kpm, cap = saca["m"], saca["att_img"], saca["att_obj_p"], saca["kpm"], saca["cap"]
    w1, w2 = _mha_weights(m.cross_attn_obj_im), _mha_weights(m.cross_attn_im_obj)
    few_keys = {"h2": {"in_proj_h2", "out_proj_h2"}, "split3": {"in_proj_p3", "out_proj_p3"}, "fp32": set()}[mode]
    many_keys = set() if mode == "fp32" else {"in_proj_p3", "out_proj_p3"}
    few_margin = H2 if mode == "h2" else EXACT
    cache = {}
    final_img = ops.mha(att_img, att_obj_p, att_img, *w1, kpm, 4, kv_limit=cap, packed=cache)
    assert set(cache) == few_keys
    _check_mha(f"cross_attn_1 few keys {mode}", few_margin, final_img, att_img, att_obj_p, att_img, w1, kpm)
    cache = {}
    final_obj = ops.mha(att_obj_p, att_img, att_obj_p, *w2, None, 4, packed=cache)
    assert set(cache) == many_keys
    _check_mha(f"cross_attn_2 {mode}", H2, final_obj, att_obj_p, att_img, att_obj_p, w2, None)
    # saca_2's operands: a full tensor in the object slot
    att_full, mask_full = saca["att_full"], saca["mask_full"]
    cache = {}
    img2 = ops.mha(att_img, att_full, att_img, *w1, mask_full, 4, kv_limit=att_full.shape[1], packed=cache)
    assert set(cache) == many_keys
    _check_mha(f"cross_attn_1 full object tensor {mode}", H2, img2, att_img, att_full, att_img, w1, mask_full)
    cache = {}
    obj2 = ops.mha(att_full, att_img, att_full, *w2, None, 4, packed=cache)
    assert set(cache) == many_keys
    _check_mha(f"cross_attn_2 full object tensor {mode}", H2, obj2, att_full, att_img, att_full, w2, None)
