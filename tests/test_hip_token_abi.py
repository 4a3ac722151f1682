"""-m gpu: the token path's C ABI as include/objcavit_hip.h promises it to a C host, called through
ctypes on raw addresses: padded leading dimensions, batch strides, [K, N] weights, bases and strides that are no multiple of 16
bytes, seq-first and packed attention operands, outputs that alias an input -- every layout the hip_ops wrappers never pass, and
with them every kernel behind ocv_linear_fwd / ocv_attention_fwd that only such a layout selects.

Reference: float64 (tests/token_ref.py, plain torch) on the float32 values of the LOGICAL operands.  Bars follow
tests/test_hip_token_units.py: bar = margin x max(d32, 2e-7) <= TOL = 2e-5, d32 = the same formula in float32 on the CPU in the same
run; margin 2 for the exact-fp32 and three-term bf16 kernels, 4 where the two-term fp16 attention core takes part.

One margin had to be raised: exact-fp32 contractions of 512 terms and more, 8 (see LONG_K).

Layout discipline of every case: every float of an input that is not a logical element -- leading-dimension slack, the gap
between batches, the floats in front of an offset base and behind the last row -- is NaN; outputs live in buffers filled with
SENT, and after the call the logical output meets its bar and is finite and EVERY other element of the buffer still is SENT.

Bit-equality (torch.equal) is asserted where the kernels' text shows the same arithmetic in the same order:
  padded vs dense operands of one variant      a leading dimension only enters the address of a load / store
  batch element z vs a call on slice z         blockIdx.z only offsets the three bases (linear.hip: A / W / out + z * stride)
  linear_kernel<.., VEC> vs <.., scalar>       VEC chooses between ld4 and four guarded loads into the SAME LDS tile
  attention_*<true> vs attention_*<false>      VEC chooses between ld4 / a float4 store and four scalar ones, nothing else
  out aliasing x / tokens vs a separate out    every workgroup reads its rows before it writes them and reads nobody else's
linear_stream_kernel walks K in another order than linear_kernel: no such relation between those two.

MEASURED (MI355X): per unit the case with the largest deviation / max(d32, 2e-7), as deviation / d32 / bar (n = checks made):
  ocv_linear_fwd   stream                5.0e-7 / 4.5e-7 / 8.9e-7   (n 20)     stream, K = 520      5.7e-7 / 2.3e-7 / 1.9e-6   (n 4)
                   <w_kn 0, VEC>         3.5e-7 / 8.1e-8 / 4.0e-7   (n 12)     <w_kn 0, scalar>     4.5e-7 / 4.5e-7 / 8.9e-7   (n 8)
                   <w_kn 1, VEC>         3.3e-7 / 3.3e-7 / 6.6e-7   (n 7)      <w_kn 1, scalar>     3.3e-7 / 3.3e-7 / 6.6e-7   (n 11)
                   (n counts the dense twins under the variant they ran as)
  ocv_linear_residual_layernorm_fwd      stream  2.7e-7 / 1.2e-7 / 4.0e-7 (n 12)   VEC  1.6e-7 / 1.6e-7 / 4.0e-7 (n 4)   scalar  2.6e-7 / 2.6e-7 / 5.3e-7 (n 14)
  ocv_linear_split3_fwd                  2.8e-7 / 2.5e-7 / 4.9e-7   (n 12)     ocv_linear_residual_layernorm_split3_fwd   1.7e-7 / 2.0e-7 / 4.0e-7   (n 12)
  ocv_attention_fwd, scalar forms        h2  2.0e-7 / 3.5e-7 / 1.4e-6   (n 24)            fp32  4.7e-7 / 5.1e-7 / 1.0e-6   (n 24)
  ocv_attention_fwd, seq-first / two buffers / padded ctx (the same figures for all three)
                                         h2  1.7e-7 / 3.6e-7 / 1.4e-6   (n 6)             fp32  1.8e-7 / 3.6e-7 / 7.2e-7   (n 6)
  ocv_mha_fwd, 7 and 1 live keys         five launches: h2 core  5.9e-7 / 7.0e-7 / 2.8e-6, fp32 core  6.4e-7 / 7.0e-7 / 1.4e-6;  fused  6.0e-7 / 7.0e-7
  ocv_encoder_layer_fwd                  FF = 100  6.9e-7 / 7.6e-7 / 3.0e-6    130  6.0e-7 / 6.9e-7 / 2.8e-6    200  9.1e-7 / 8.8e-7 / 3.5e-6   (n 2 each)
                                         FF = 1024  fp32  7.6e-7 / 7.4e-7 / 3.0e-6, split3  7.6e-7 / 6.5e-7 / 2.6e-6
                                         FF = 128   fp32  8.3e-7 / 7.1e-7 / 2.9e-6, split3  9.5e-7 / 7.1e-7 / 2.9e-6
  ocv_ffn_residual_layernorm_fwd         FF = 128  2.0e-7 / 1.6e-7 / 4.0e-7       FF = 1024  5.3e-7 / 2.0e-7 / 1.6e-6
Every bit-equality held: padded = dense, batch element = slice, VEC = scalar (both linears, both attention cores), aliased = separate;
both packers with ldw = K + 3 = the contiguous packing, and the three-term buffer = the header's formula.
"""
import contextlib
import copy
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn as nn

import gen
import token_abi_cases as tac
import token_cases as tc
import token_ref as tr
from util import rel_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 2e-5
FLOOR = 2e-7
H2, EXACT = 4, 2             # margins (module docstring)
# Exact-fp32 contractions of 512 terms and more at 8, not 2: linear_stream_kernel at K = 520 measured up to 2.46 x d32 (5.7e-7 against
# d32 2.3e-7) and ffn_fused_kernel at FF = 1024 2.7 x (5.3e-7 against 2.0e-7), every shorter contraction in this file at most 1.8 x max(d32, 2e-7).
# Rounding only, by the kernels' text: chunk_mfma (csrc/linear.hip) issues v_mfma_f32_32x32x2_f32 after v_mfma_f32_32x32x2_f32 into
# ONE fp32 accumulator per output, so a K-long sum is rounded K / 2 times in sequence -- 260 times at K = 520, 512 times in the
# feed-forward block's second contraction -- and the error of such a running sum grows like sqrt(K), where float32 matmul on
# the CPU sums in vector lanes and cache blocks (error ~ sqrt(log K): its d32 at K = 520, 1.6e-7 - 2.5e-7, is no larger than at K = 136, 4.0e-7).  Restating
# that order in float32 on the CPU (an fp32 running sum over pairs of products, K = 520, the shapes of this file) gives 5.9e-7,
# the device's own figure.  8 = the smallest power of two with 2 x headroom over the measured worst, as TAIL_MARGIN in
# tests/test_hip_token_units.py.
LONG_K = 8
NAN = float("nan")
SENT = 777.0
SLACK = 40                   # floats behind the last logical element of every buffer (NaN in inputs, SENT in outputs)
E, HEADS = 128, 4
SCALE = 1.0 / math.sqrt(32.0)


def bar(margin, d32):
    b = margin * max(d32, FLOOR)
    assert b <= TOL, (margin, d32)
    return b


def check_dev(unit, margin, got, ref64, ref32):
    """got (device, logical) against the float64 reference under the bar its float32 restatement gives; finite."""
    d32 = rel_dev(ref32, ref64)
    dev = rel_dev(got, ref64)
    b = bar(margin, d32)
    print(f"UNIT {unit}: dev {dev:.3e} d32 {d32:.3e} bar {b:.3e}")
    assert bool(torch.isfinite(got).all()), unit
    assert dev < b, (unit, dev, d32, b)


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


def lay(vals, strides, off=0, fill=NAN):
    """``vals`` (CPU float32, any rank) at the element ``strides`` behind ``off`` floats of a fresh device buffer that holds
    ``fill`` everywhere else.  Returns (buffer, strided view of the logical elements).  Allocations are 512-byte aligned, so
    the view's base is 16-byte aligned iff off % 4 == 0."""
    span = 1 + sum((n - 1) * s for n, s in zip(vals.shape, strides))
    buf = torch.full((off + span + SLACK,), fill, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 512 == 0
    view = buf.as_strided(tuple(vals.shape), tuple(strides), off)
    view.copy_(vals)
    return buf, view


def lay_out(shape, strides, off=0):
    return lay(torch.full(tuple(shape), SENT), strides, off, SENT)


def take(buf, view):
    """The logical output, after checking that nothing but it was written: with the view put back to SENT the whole buffer is SENT."""
    got = view.clone()
    view.fill_(SENT)
    assert bool((buf == SENT).all()), "a padding element of the output was written"
    return got


# ------------------------------------------------------------------ a. ocv_linear_fwd
def act_ref(y, act):
    if act == tac.ACT_RELU:
        return torch.relu(y)
    if act == tac.ACT_LEAKY:
        return torch.where(y > 0, y, 0.01 * y)
    return y


def linear_ref(A, W, bias, act, dt):
    y = A.to(dt) @ W.to(dt).transpose(-1, -2)
    if bias is not None:
        y = y + bias.to(dt)
    return act_ref(y, act)


def lay_linear(c, A, W):
    """A [1 or batch, M, K], W [1 or batch, N, K] (CPU, logical) in the layout of row ``c``."""
    Ab, Av = lay(A, (max(c.sA, 1), c.lda, 1), c.offA)
    Wb, Wv = lay(W.transpose(1, 2) if c.w_kn else W, (max(c.sW, 1), c.ldw, 1), c.offW)
    return (Ab, Av), (Wb, Wv)


def call_linear(lib, c, Av, Wv, bias, z=None):
    """One ocv_linear_fwd on laid-out operands: the whole batch, or (z given) batch = 1 on slice z of the same buffers."""
    nb = c.batch if z is None else 1
    ob, ov = lay_out((nb, c.M, c.N), (c.sO, c.ldo, 1), 1 if (c.offA or c.offW) else 0)
    pa = Av.data_ptr() + (0 if z is None else 4 * z * c.sA)
    pw = Wv.data_ptr() + (0 if z is None else 4 * z * c.sW)
    rc = lib.ocv_linear_fwd(pa, c.lda, c.sA, pw, c.ldw, c.sW, c.w_kn, _ptr(bias), ov.data_ptr(), c.ldo, c.sO, nb, c.M, c.N, c.K,
                            c.act, _stream())
    assert rc == 0, lib.ocv_last_error()
    torch.cuda.synchronize()
    return take(ob, ov), tac.variant_of(pa, c.lda, c.sA, pw, c.ldw, c.sW, c.w_kn, c.K)


@pytest.mark.parametrize("c", tac.LINEAR_CASES, ids=tac.lin_id)
def test_linear_variants(lib, c):
    """Every row of tests/token_abi_cases.py: the row selects the variant it is listed under (launch_linear restated on the
    actual addresses), meets the float64 bar with NaN in every padding float, leaves the output's padding alone, equals the
    dense call in bits where that call runs the same arithmetic, and (batch > 1) equals one call per slice in bits."""
    assert tac.case_variant(c) == c.variant
    seed = 100 + tac.LINEAR_CASES.index(c)
    A = gen.randn("A", (1 if c.sA == 0 else c.batch, c.M, c.K), seed)
    W = gen.randn("W", (1 if c.sW == 0 else c.batch, c.N, c.K), seed, 1.0 / math.sqrt(c.K))
    bias_cpu = gen.randn("bias", (c.N,), seed, 0.5) if c.bias else None
    bias = None if bias_cpu is None else bias_cpu.cuda()
    (Ab, Av), (Wb, Wv) = lay_linear(c, A, W)
    got, v = call_linear(lib, c, Av, Wv, bias)
    assert v == c.variant
    ref64, ref32 = linear_ref(A, W, bias_cpu, c.act, torch.float64), linear_ref(A, W, bias_cpu, c.act, torch.float32)
    assert tuple(ref64.shape) == (c.batch, c.M, c.N)
    margin = LONG_K if c.K >= 512 else EXACT
    check_dev(f"linear {c.variant}{' K >= 512' if c.K >= 512 else ''}", margin, got, ref64, ref32)
    t = tac.dense_twin(c)
    (tAb, tAv), (tWb, tWv) = lay_linear(t, A, W)
    got_t, v_t = call_linear(lib, t, tAv, tWv, bias)
    check_dev(f"linear {v_t}{' K >= 512' if c.K >= 512 else ''} (dense twin)", margin, got_t, ref64, ref32)
    if tac.same_arithmetic(v, v_t):
        assert torch.equal(got, got_t), (v, v_t)
    else:
        assert v_t == "stream" and v == "scalar"                          # (no relation: another order over K)
    for z in range(c.batch if c.batch > 1 else 0):
        got_z, v_z = call_linear(lib, c, Av, Wv, bias, z)
        assert tac.same_arithmetic(v, v_z), (v, v_z)
        assert torch.equal(got_z[0], got[z]), z


# ------------------------------------------------------------------ b. ocv_linear_residual_layernorm_fwd
LN_VARIANT = {8: "stream", 72: "stream", 136: "stream", 36: "vec", 35: "scalar"}


def ln_linear_ref(A, W, bias, res, gamma, beta, dt):
    return tr.layernorm(res.to(dt) + A.to(dt) @ W.to(dt).t() + bias.to(dt), gamma, beta, 1e-5)


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("K", [8, 72, 136, 36, 35])
def test_linear_residual_layernorm_layouts(lib, K, M):
    """linear_stream_kernel<EPI_RES_LN> on short and ragged chunks and the LayerNorm epilogue INSIDE linear_kernel (K = 36: VEC,
    K = 35: scalar; any K under odd leading dimensions), with lda / ldw / ldres / ldo dense, padded by 4 (the variant stays) and
    padded by 1 / 3 (scalar); with a zero_row_mask masked rows are exactly 0 and every other row keeps its bits."""
    N = 128
    seed = 300 + K + M
    A, W = gen.randn("A", (M, K), seed), gen.randn("W", (N, K), seed, 1.0 / math.sqrt(K))
    bias, res = gen.randn("bias", (N,), seed, 0.5), gen.randn("res", (M, N), seed)
    gamma, beta = 1.0 + gen.randn("gamma", (N,), seed, 0.1), gen.randn("beta", (N,), seed, 0.1)
    ref64 = ln_linear_ref(A, W, bias, res, gamma, beta, torch.float64)
    ref32 = ln_linear_ref(A, W, bias, res, gamma, beta, torch.float32)
    dev = [t.cuda() for t in (bias, gamma, beta)]
    mask_cpu = torch.arange(M) % 3 == 0
    mask = mask_cpu.to(torch.uint8).cuda()
    results = {}
    for name, (lda, ldw, ldres, ldo) in {"dense": (K, K, N, N), "pad4": (K + 4, K + 4, N + 4, N + 4), "odd": (K + 1, K + 3, N + 1, N + 3)}.items():
        (Ab, Av), (Wb, Wv), (Rb, Rv) = lay(A, (lda, 1)), lay(W, (ldw, 1)), lay(res, (ldres, 1))
        v = tac.variant_of(Av.data_ptr(), lda, 0, Wv.data_ptr(), ldw, 0, 0, K)
        assert v == ("scalar" if name == "odd" else LN_VARIANT[K])
        outs = []
        for m in (None, mask):
            ob, ov = lay_out((M, N), (ldo, 1))
            rc = lib.ocv_linear_residual_layernorm_fwd(Av.data_ptr(), lda, Wv.data_ptr(), ldw, dev[0].data_ptr(), Rv.data_ptr(), ldres,
                                                       dev[1].data_ptr(), dev[2].data_ptr(), 1e-5, _ptr(m), ov.data_ptr(), ldo, M, N, K, _stream())
            assert rc == 0, lib.ocv_last_error()
            torch.cuda.synchronize()
            outs.append(take(ob, ov))
        check_dev(f"linear_ln {v}", EXACT, outs[0], ref64, ref32)
        z = mask_cpu.cuda()
        assert float(outs[1][z].abs().max()) == 0.0 and torch.equal(outs[1][~z], outs[0][~z])
        results[name] = (v, outs[0])
    for name in ("pad4", "odd"):
        if tac.same_arithmetic(results[name][0], results["dense"][0]):
            assert torch.equal(results[name][1], results["dense"][1]), name
    assert results["pad4"][0] == results["dense"][0]


# ------------------------------------------------------------------ c. split3 linears and the packers
SENT16 = 0x7B7B


def pack(lib, kind, Wv, ldw, N, K):
    """ocv_pack_split3_fwd / ocv_pack_split_h2_fwd of the device view Wv [N, K] (row stride ldw) -> int16 bits of the packed buffer;
    the 64 elements behind it stay untouched."""
    n = int((lib.ocv_split3_packed_elems if kind == "split3" else lib.ocv_split_h2_packed_elems)(N, K))
    assert n == ((N + 31) // 32) * ((K + 15) // 16) * 512 * (3 if kind == "split3" else 2)
    buf = torch.full((n + 64,), SENT16, dtype=torch.int16, device="cuda")
    fn = lib.ocv_pack_split3_fwd if kind == "split3" else lib.ocv_pack_split_h2_fwd
    rc = fn(Wv.data_ptr(), ldw, N, K, buf.data_ptr(), _stream())
    assert rc == 0, lib.ocv_last_error()
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENT16).all())
    return buf[:n]


def split3_layout_host(W):
    """The header's formula on the host: packed[((jt * nsteps + s) * 3 + part) * 512 + lane * 8 + e] =
    part of W[32 jt + (lane & 31)][16 s + 8 (lane >> 5) + e], zero beyond N and K; h = bf16(v), m = bf16(v - h), l = bf16(v - h - m)."""
    N, K = W.shape
    nt, ns = (N + 31) // 32, (K + 15) // 16
    Wz = torch.zeros(nt * 32, ns * 16)
    Wz[:N, :K] = W
    h = Wz.to(torch.bfloat16)
    r1 = Wz - h.float()
    m = r1.to(torch.bfloat16)
    l = (r1 - m.float()).to(torch.bfloat16)
    parts = torch.stack([h, m, l]).view(torch.int16)                      # [part, n, k]
    p = parts.view(3, nt, 32, ns, 2, 8)                                   # [part, jt, lane & 31, s, lane >> 5, e]
    return p.permute(1, 3, 0, 4, 2, 5).contiguous().view(-1)              # [jt, s, part, lane >> 5, lane & 31, e]


@pytest.mark.parametrize("N,K", [(33, 24), (130, 72)])
@pytest.mark.parametrize("kind", ["split3", "h2"])
def test_packers_take_a_row_stride(lib, kind, N, K):
    """ocv_pack_split3_fwd / ocv_pack_split_h2_fwd with ldw = K + 3 (NaN in the slack): bit-equal to the packing of a contiguous
    copy; the three-term buffer also bit-equal to the header's layout formula built element by element on the host (ragged last
    channel tile and K step: zeros beyond N and K)."""
    W = gen.randn("W", (N, K), 400 + N, 1.0 / math.sqrt(K))
    (Pb, Pv), (Db, Dv) = lay(W, (K + 3, 1)), lay(W, (K, 1))
    padded, dense = pack(lib, kind, Pv, K + 3, N, K), pack(lib, kind, Dv, K, N, K)
    assert torch.equal(padded, dense)
    if kind == "split3":
        assert torch.equal(padded.cpu(), split3_layout_host(W))


def lay_packed3(lib, W):
    N, K = W.shape
    Wb, Wv = lay(W, (K, 1))
    return pack(lib, "split3", Wv, K, N, K)


@pytest.mark.parametrize("M,N,K,act,with_bias", [(33, 40, 24, tac.ACT_RELU, True), (70, 130, 72, tac.ACT_LEAKY, False),
                                                 (33, 384, 128, tac.ACT_NONE, True), (1, 160, 136, tac.ACT_NONE, True)])
def test_linear_split3_layouts(lib, M, N, K, act, with_bias):
    """ocv_linear_split3_fwd (lin3_kernel<1>, <2> at 5 channel tiles, <3> at 12; one short chunk, a ragged second one) with lda
    padded by 4 and 8 and ldo by 3 and 4: float64 bar, padding untouched, bit-equal to the dense call."""
    seed = 500 + N
    A, W = gen.randn("A", (M, K), seed), gen.randn("W", (N, K), seed, 1.0 / math.sqrt(K))
    bias_cpu = gen.randn("bias", (N,), seed, 0.5) if with_bias else None
    bias = None if bias_cpu is None else bias_cpu.cuda()
    wp = lay_packed3(lib, W)
    ref64, ref32 = linear_ref(A, W, bias_cpu, act, torch.float64), linear_ref(A, W, bias_cpu, act, torch.float32)
    outs = []
    for lda, ldo in ((K, N), (K + 4, N + 3), (K + 8, N + 4)):
        Ab, Av = lay(A, (lda, 1))
        ob, ov = lay_out((M, N), (ldo, 1))
        rc = lib.ocv_linear_split3_fwd(Av.data_ptr(), lda, wp.data_ptr(), _ptr(bias), ov.data_ptr(), ldo, M, N, K, act, _stream())
        assert rc == 0, lib.ocv_last_error()
        torch.cuda.synchronize()
        outs.append(take(ob, ov))
        check_dev("linear_split3", EXACT, outs[-1], ref64, ref32)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("K", [24, 136])
def test_linear_residual_layernorm_split3_layouts(lib, K, M):
    """ocv_linear_residual_layernorm_split3_fwd (lin3_kernel<1, L3_RES_LN>) with padded lda (multiples of 4), ldres and ldo, with
    and without a zero_row_mask."""
    N = 128
    seed = 600 + K + M
    A, W = gen.randn("A", (M, K), seed), gen.randn("W", (N, K), seed, 1.0 / math.sqrt(K))
    bias, res = gen.randn("bias", (N,), seed, 0.5), gen.randn("res", (M, N), seed)
    gamma, beta = 1.0 + gen.randn("gamma", (N,), seed, 0.1), gen.randn("beta", (N,), seed, 0.1)
    ref64 = ln_linear_ref(A, W, bias, res, gamma, beta, torch.float64)
    ref32 = ln_linear_ref(A, W, bias, res, gamma, beta, torch.float32)
    dev = [t.cuda() for t in (bias, gamma, beta)]
    wp = lay_packed3(lib, W)
    mask_cpu = torch.arange(M) % 3 == 0
    mask, z = mask_cpu.to(torch.uint8).cuda(), mask_cpu.cuda()
    plain = []
    for lda, ldres, ldo in ((K, N, N), (K + 4, N + 1, N + 3), (K + 12, N + 4, N + 4)):
        (Ab, Av), (Rb, Rv) = lay(A, (lda, 1)), lay(res, (ldres, 1))
        outs = []
        for m in (None, mask):
            ob, ov = lay_out((M, N), (ldo, 1))
            rc = lib.ocv_linear_residual_layernorm_split3_fwd(Av.data_ptr(), lda, wp.data_ptr(), dev[0].data_ptr(), Rv.data_ptr(), ldres,
                                                              dev[1].data_ptr(), dev[2].data_ptr(), 1e-5, _ptr(m), ov.data_ptr(), ldo, M, N, K,
                                                              _stream())
            assert rc == 0, lib.ocv_last_error()
            torch.cuda.synchronize()
            outs.append(take(ob, ov))
        check_dev("linear_ln_split3", EXACT, outs[0], ref64, ref32)
        assert float(outs[1][z].abs().max()) == 0.0 and torch.equal(outs[1][~z], outs[0][~z])
        plain.append(outs[0])
    assert torch.equal(plain[0], plain[1]) and torch.equal(plain[0], plain[2])


# ------------------------------------------------------------------ d. ocv_attention_fwd
FORMS = {"h2": 0, "fp32": 1}


@contextlib.contextmanager
def attention_form(ops, lib, form):
    """The attention core's form for the calls inside; afterwards the library holds again what the environment names (the state
    objcavit_amd.hip_ops.attention_form_sync keeps track of)."""
    ops.attention_form_sync()
    back = FORMS[os.environ.get("OCV_ATTN_FORM", "h2")]
    assert lib.ocv_attention_set_dispatch(FORMS[form]) == 0
    try:
        yield
    finally:
        assert lib.ocv_attention_set_dispatch(back) == 0


def dense3(S):
    return (S * E, E, 1)


def attn_vec(q, k, v, ctx):
    """ocv_attention_launch's ``vec`` (csrc/attention.hip) on the actual addresses and strides."""
    return all(t.data_ptr() % 16 == 0 for t in (q, k, v, ctx)) and all(t.stride(i) % 4 == 0 for t in (k, v, ctx) for i in (0, 1))


def call_attention(lib, q, k, v, mask, ctx_strides, ctx_off=0):
    """ocv_attention_fwd on device views q [B, Sq, E], k / v [B, Sk, E] (unit stride on E) -> (logical ctx, vec)."""
    B, Sq, _ = q.shape
    Sk = k.shape[1]
    ob, ov = lay_out((B, Sq, E), ctx_strides, ctx_off)
    rc = lib.ocv_attention_fwd(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0),
                               v.stride(1), _ptr(mask), ov.data_ptr(), ov.stride(0), ov.stride(1), B, HEADS, Sq, Sk, SCALE, _stream())
    assert rc == 0, lib.ocv_last_error()
    torch.cuda.synchronize()
    vec = attn_vec(q, k, v, ov)
    return take(ob, ov), vec


def attention_inputs(B, Sq, Sk, seed):
    return gen.randn("q", (B, Sq, E), seed), gen.randn("k", (B, Sk, E), seed), gen.randn("v", (B, Sk, E), seed)


def attention_refs(q, k, v, mask_cpu):
    return tr._core(q.double(), k.double(), v.double(), mask_cpu, HEADS), tr._core(q, k, v, mask_cpu, HEADS)


# (operand, its seq stride, offset of its base in floats): each alone makes ocv_attention_launch's ``vec`` false
SCALAR_BY = [("k", 385, 0), ("v", 129, 0), ("ctx", 129, 0), ("k", E, 1), ("v", E, 1), ("ctx", E, 1)]


@pytest.mark.parametrize("B,Sq,Sk,counts", [(2, 33, 33, [33, 7]), (1, 5, 130, [129])])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("which,ss,off", SCALAR_BY, ids=[f"{w}-ss{s}-off{o}" for w, s, o in SCALAR_BY])
@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_attention_scalar_form(ops, lib, form, which, ss, off, masked, B, Sq, Sk, counts):
    """attention_h2_kernel<false> / attention_kernel<false>, selected by ONE operand whose seq stride (385, 129) or base (one float
    off) is no multiple of 16 bytes: two ragged 32-key tiles in two images, and 130 keys (for the two-term core: two keys in a
    second 128-key chunk, the last of them masked in the masked run).  Float64 bar, NaN between the rows, ctx padding untouched,
    and the bits of the vector form on dense operands."""
    q, k, v = attention_inputs(B, Sq, Sk, 700 + Sk)
    mask_cpu = tc.key_mask(counts, Sk) if masked else None
    mask = None if mask_cpu is None else mask_cpu.to(torch.uint8).cuda()
    ref64, ref32 = attention_refs(q, k, v, mask_cpu)

    def strides(name, S):
        return (S * ss, ss, 1) if (name == which) else dense3(S)

    def offset(name):
        return off if name == which else 0

    (qb, qv), (kb, kv), (vb, vv) = lay(q, dense3(Sq)), lay(k, strides("k", Sk), offset("k")), lay(v, strides("v", Sk), offset("v"))
    (kdb, kdv), (vdb, vdv) = lay(k, dense3(Sk)), lay(v, dense3(Sk))
    with attention_form(ops, lib, form):
        got, vec = call_attention(lib, qv, kv, vv, mask, strides("ctx", Sq), offset("ctx"))
        got_d, vec_d = call_attention(lib, qv, kdv, vdv, mask, dense3(Sq))
    assert not vec and vec_d
    check_dev(f"attention_{form} scalar", H2 if form == "h2" else EXACT, got, ref64, ref32)
    assert torch.equal(got, got_d)


@pytest.mark.parametrize("layout", ["seq_first", "kv_of_two_buffers", "ctx_padded"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_attention_layouts(ops, lib, form, masked, layout):
    """B = 3, S = 37.  seq_first: q / k / v / ctx stored [S, B, E] (batch stride E, seq stride B E) -- the header's "seq-first layouts
    need no copies"; kv_of_two_buffers: q and k with the strides of a packed [B, S, 3E] projection (k 128 floats into its buffer),
    v out of a buffer with rows of 132 floats and a gap between the images; ctx_padded: o_ss = 132, o_bs = S 132 + 8.  All of them vector forms: the dense call's
    bits."""
    B, S, counts = 3, 37, [37, 20, 1]
    q, k, v = attention_inputs(B, S, S, 800)
    mask_cpu = tc.key_mask(counts, S) if masked else None
    mask = None if mask_cpu is None else mask_cpu.to(torch.uint8).cuda()
    ref64, ref32 = attention_refs(q, k, v, mask_cpu)
    sq = sk = sv = so = dense3(S)
    offs = {"q": 0, "k": 0, "v": 0}
    if layout == "seq_first":
        sq = sk = sv = so = (E, B * E, 1)
    elif layout == "kv_of_two_buffers":
        sq = sk = (S * 3 * E, 3 * E, 1)
        offs["k"] = E
        sv = (S * 132 + 8, 132, 1)
    else:
        so = (S * 132 + 8, 132, 1)
    (qb, qv), (kb, kv), (vb, vv) = lay(q, sq, offs["q"]), lay(k, sk, offs["k"]), lay(v, sv, offs["v"])
    (qdb, qdv), (kdb, kdv), (vdb, vdv) = lay(q, dense3(S)), lay(k, dense3(S)), lay(v, dense3(S))
    with attention_form(ops, lib, form):
        got, vec = call_attention(lib, qv, kv, vv, mask, so)
        got_d, vec_d = call_attention(lib, qdv, kdv, vdv, mask, dense3(S))
    assert vec and vec_d
    check_dev(f"attention_{form} {layout}", H2 if form == "h2" else EXACT, got, ref64, ref32)
    assert torch.equal(got, got_d)


# ------------------------------------------------------------------ e. ocv_mha_fwd: the five-launch route behind a declined fused launch
@pytest.mark.parametrize("form", ["h2", "fp32"])
def test_mha_falls_back_on_a_misaligned_query_source(ops, lib, form):
    """ocv_cross_attn_fused_launch declines a q_src that is not 16-byte aligned; ocv_mha_fwd then runs three projections
    (linear_kernel<.., scalar> for q; the batched linear_stream_kernel with strideO = kv_limit E for k and v), the attention core
    in ``form`` and the output projection -- with 7 and 1 live keys of 12 (kv_limit 7; key rows >= kv_limit hold NaN: they are
    neither projected nor scored), Sq = 45.  Float64 bar for it, and the same bar for the aligned call (one fused exact-fp32
    launch) on the same values."""
    B, Sq, Sk, lim, counts = 2, 45, 12, 7, [7, 1]
    mha = nn.MultiheadAttention(E, HEADS, batch_first=True).eval()
    gen.load_into(mha, 41, gen.PEAKY)
    w = [t.detach().clone() for t in (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias)]
    wd = [t.cuda() for t in w]
    qs, ks, vs = gen.randn("q_src", (B, Sq, E), 41), gen.randn("k_src", (B, Sk, E), 41), gen.randn("v_src", (B, Sk, E), 41)
    mask_cpu = tc.key_mask(counts, Sk)
    mask = mask_cpu.to(torch.uint8).cuda()
    ref64 = tr.mha(qs.double(), ks[:, :lim].double(), vs[:, :lim].double(), *w, mask_cpu[:, :lim])
    ref32 = tr.mha(qs, ks[:, :lim], vs[:, :lim], *w, mask_cpu[:, :lim])
    ks_nan, vs_nan = ks.clone(), vs.clone()
    ks_nan[:, lim:], vs_nan[:, lim:] = NAN, NAN
    (kb, kv), (vb, vv) = lay(ks_nan, dense3(Sk)), lay(vs_nan, dense3(Sk))
    nb = int(lib.ocv_mha_workspace_bytes(B, Sq, Sk, E))
    outs = {}
    with attention_form(ops, lib, form):
        for name, off in (("fallback", 1), ("fused", 0)):
            qb, qv = lay(qs, dense3(Sq), off)
            ws = torch.full((nb // 4 + 4,), NAN, dtype=torch.float32, device="cuda")
            ob, ov = lay_out((B, Sq, E), dense3(Sq))
            rc = lib.ocv_mha_fwd(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), mask.data_ptr(), *[t.data_ptr() for t in wd], ov.data_ptr(),
                                 B, Sq, Sk, lim, E, HEADS, ws.data_ptr(), nb, _stream())
            assert rc == 0, lib.ocv_last_error()
            torch.cuda.synchronize()
            outs[name] = (take(ob, ov), ws)
    margin = H2 if form == "h2" else EXACT
    assert bool(torch.isnan(outs["fused"][1]).all())                      # one launch: the workspace was not touched ...
    assert not bool(torch.isnan(outs["fallback"][1][:B * Sq * E]).any())  # ... five launches: the projected queries lie in it
    check_dev(f"mha fallback ({form} core)", margin, outs["fallback"][0], ref64, ref32)
    check_dev(f"mha fused (bar of the {form} fallback)", margin, outs["fused"][0], ref64, ref32)


# ------------------------------------------------------------------ f. ocv_encoder_layer_fwd, aliasing
class Layer:
    """A seeded nn.TransformerEncoderLayer on the device with its pointer table: exact fp32, or (packed) + the split weights."""

    def __init__(self, ops, module, packed):
        self.cpu = tc.params(module)
        self.mod = copy.deepcopy(module).cuda()
        self.cache = {} if packed else None
        self.st, self.keep = ops.layer_params(self.mod, self.cache)
        assert bool(self.st.in_proj_p3) == bool(self.st.linear2_p3) == packed


def generic_layer(FF):
    lay_ = nn.TransformerEncoderLayer(E, HEADS, FF, batch_first=True).eval()
    gen.load_into(lay_, 50 + FF, gen.PEAKY)
    return lay_


def call_encoder_layer(ops, lib, L, x_ptr, out_ptr, mask, B, S, FF):
    """ocv_encoder_layer_fwd on a workspace that holds NaN (nothing may be read from it that the call did not write)."""
    nb = int(lib.ocv_encoder_layer_workspace_bytes(B, S, E, FF))
    ws = torch.full((nb // 4,), NAN, dtype=torch.float32, device="cuda")
    with attention_form(ops, lib, "h2"):
        rc = lib.ocv_encoder_layer_fwd(x_ptr, C.byref(L.st), _ptr(mask), 0 if mask is None else 1, out_ptr, B, S, E, HEADS, FF, 1e-5,
                                       ws.data_ptr(), nb, _stream())
    assert rc == 0, lib.ocv_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("FF", [100, 130, 200])
def test_encoder_layer_generic_hidden_size(ops, lib, FF, masked):
    """FF % 128 != 0, exact-fp32 weights: ocv_linear_fwd with ldo = FF, then the LayerNorm linear with lda = K = FF -- FF = 100:
    linear_kernel<EPI_RES_LN, false, VEC>; 130: <.., scalar>; 200: linear_stream_kernel<EPI_RES_LN> with a 72-long last chunk.
    B = 2, S = 37, with and without key_padding_mask + zero_padded_rows, against token_ref.encoder_layer on a seeded layer of that
    FF.  Margin 4: the layer's attention core is the two-term fp16 one."""
    B, S, counts = 2, 37, [37, 20]
    M = B * S
    assert tac.variant_of(0, FF, 0, 0, FF, 0, 0, FF) == {100: "vec", 130: "scalar", 200: "stream"}[FF]
    L = Layer(ops, generic_layer(FF), False)
    x_cpu = gen.randn("x", (B, S, E), 900 + FF)
    mask_cpu = tc.key_mask(counts, S) if masked else None
    mask = None if mask_cpu is None else mask_cpu.to(torch.uint8).cuda()
    ref64, ref32 = tr.encoder_layer(x_cpu.double(), L.cpu, mask_cpu), tr.encoder_layer(x_cpu, L.cpu, mask_cpu)
    if masked:
        ref64, ref32 = ref64.masked_fill(mask_cpu[..., None], 0.0), ref32.masked_fill(mask_cpu[..., None], 0.0)
    x = x_cpu.cuda()
    ob, ov = lay_out((M, E), (E, 1))
    call_encoder_layer(ops, lib, L, x.data_ptr(), ov.data_ptr(), mask, B, S, FF)
    assert torch.equal(x.cpu(), x_cpu)
    got = take(ob, ov).view(B, S, E)
    check_dev(f"encoder_layer FF={FF}", H2, got, ref64, ref32)
    if masked:
        assert float(got[mask_cpu.cuda()].abs().max()) == 0.0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("FF,packed", [(1024, False), (128, False), (1024, True), (128, True)])
def test_encoder_layer_out_may_alias_x(ops, lib, FF, packed, masked):
    """``out`` == ``x`` gives the bits of a call with a separate ``out``: FF = 1024 on 74 rows (the feed-forward block shared out
    over ocv_ffn_split_count(74, 1024) = 8 workgroups per row tile + the finish pass, which reads x again), FF = 128 (one fused
    launch), and both on the three-term split weights.  The separate call also meets the float64 bar."""
    B, S, counts = 2, 37, [37, 20]
    M = B * S
    assert tac.ffn_split_count(M, FF) == (8 if FF == 1024 else 1)
    L = Layer(ops, tc.layer_module(tc.encoder(), 0, FF), packed)
    x_cpu = gen.randn("x", (B, S, E), 950 + FF)
    mask_cpu = tc.key_mask(counts, S) if masked else None
    mask = None if mask_cpu is None else mask_cpu.to(torch.uint8).cuda()
    x = x_cpu.cuda()
    ob, ov = lay_out((M, E), (E, 1))
    call_encoder_layer(ops, lib, L, x.data_ptr(), ov.data_ptr(), mask, B, S, FF)
    sep = take(ob, ov)
    ref64, ref32 = tr.encoder_layer(x_cpu.double(), L.cpu, mask_cpu), tr.encoder_layer(x_cpu, L.cpu, mask_cpu)
    if masked:
        ref64, ref32 = ref64.masked_fill(mask_cpu[..., None], 0.0), ref32.masked_fill(mask_cpu[..., None], 0.0)
    check_dev(f"encoder_layer FF={FF} {'split3' if packed else 'fp32'}", H2, sep.view(B, S, E), ref64, ref32)
    xb, xv = lay(x_cpu.view(M, E), (E, 1), 0, SENT)
    call_encoder_layer(ops, lib, L, xv.data_ptr(), xv.data_ptr(), mask, B, S, FF)
    assert torch.equal(take(xb, xv), sep)


def ffn_ref(x, p, dt):
    x = x.to(dt)
    h = torch.relu(x @ p["linear1.weight"].to(dt).t() + p["linear1.bias"].to(dt))
    return tr.layernorm(x + h @ p["linear2.weight"].to(dt).t() + p["linear2.bias"].to(dt), p["norm2.weight"], p["norm2.bias"], 1e-5)


@pytest.mark.parametrize("FF", [128, 1024])
def test_ffn_out_may_alias_x(ops, lib, FF):
    """ocv_ffn_residual_layernorm_fwd(out = x): ffn_fused_kernel stages a tile's rows of x into LDS before anything is written and
    takes the residual from there.  Bits of the separate call, which meets the float64 bar; with a zero_row_mask too."""
    M = 74
    L = Layer(ops, tc.layer_module(tc.encoder(), 1, FF), False)
    x_cpu = gen.randn("x", (M, E), 970 + FF)
    mask_cpu = torch.arange(M) % 3 == 0
    for m in (None, mask_cpu.to(torch.uint8).cuda()):
        outs = []
        for alias in (False, True):
            xb, xv = lay(x_cpu, (E, 1), 0, SENT)
            ob, ov = (xb, xv) if alias else lay_out((M, E), (E, 1))
            st = L.st
            rc = lib.ocv_ffn_residual_layernorm_fwd(xv.data_ptr(), st.linear1_w, st.linear1_b, st.linear2_w, st.linear2_b, st.norm2_w,
                                                    st.norm2_b, 1e-5, _ptr(m), ov.data_ptr(), M, E, FF, _stream())
            assert rc == 0, lib.ocv_last_error()
            torch.cuda.synchronize()
            outs.append(take(ob, ov))
        assert torch.equal(outs[0], outs[1])
        if m is None:
            check_dev(f"ffn FF={FF}", LONG_K if FF >= 512 else EXACT, outs[0], ffn_ref(x_cpu, L.cpu, torch.float64), ffn_ref(x_cpu, L.cpu, torch.float32))
        else:
            assert float(outs[0][mask_cpu.cuda()].abs().max()) == 0.0


def test_object_tokens_pad_out_may_alias_tokens(lib):
    """ocv_object_tokens_pad_fwd(out = tokens): a thread reads the four floats it overwrites.  Rows >= count become the pad value,
    mask = (j >= count); a count of 0 keeps one live key that holds the pad value (csrc/objects_pad.hip).  Exact, and the bits of
    the separate call."""
    B, cap, pad = 3, 9, 1e-4
    counts = [9, 4, 0]
    tok = gen.randn("tok", (B, cap, E), 990)
    cnt = torch.tensor(counts, dtype=torch.int32).cuda()
    want = tok.clone()
    want_mask = torch.zeros(B, cap, dtype=torch.uint8)
    for b, n in enumerate(counts):
        want[b, n:] = pad
        want_mask[b, max(n, 1):] = 1
    outs = []
    for alias in (False, True):
        tb, tv = lay(tok, (cap * E, E, 1), 0, SENT)
        ob, ov = (tb, tv) if alias else lay_out((B, cap, E), (cap * E, E, 1))
        mask = torch.full((B * cap + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        rc = lib.ocv_object_tokens_pad_fwd(tv.data_ptr(), cnt.data_ptr(), pad, ov.data_ptr(), mask.data_ptr(), B, cap, E, _stream())
        assert rc == 0, lib.ocv_last_error()
        torch.cuda.synchronize()
        assert bool((mask[B * cap:] == 0x5A).all()) and torch.equal(mask[:B * cap].view(B, cap).cpu(), want_mask)
        outs.append(take(ob, ov))
    assert torch.equal(outs[0].cpu(), want) and torch.equal(outs[0], outs[1])
