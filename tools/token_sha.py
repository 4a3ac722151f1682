"""SHA-1 of every output of the token path (csrc/linear.hip, attention.hip, bin_head.hip, token_h2.hip, token_split3.hip,
xattn_h2.hip, xattn_split3.hip, token_pack.hip) on fixed seeded operands, one line per case, so that two library builds
(OCV_LIB_PATH) can be compared bit for bit from their logs -- run once per build, in a process of its own:

    python tools/token_sha.py > new.log;  OCV_LIB_PATH=objcavit_amd/lib/variants/parent.so python tools/token_sha.py > parent.log

Cases, at the smallest shapes that reach every kernel instantiation of the eight sources: the two weight packers (aligned, long-K
and ragged matrices; for fp16 one weight beyond +-65504 and one NaN); ocv_linear_split3_fwd (M = 45; one, two and three channel
tiles per wavefront; a short and a two-chunk K; the three activations; no bias); the residual + LayerNorm and feed-forward units on
split3 and fp32 (row mask on / off; FF = 256 with and without the workspace = with and without the shared finish pass);
ocv_linear_fwd on the streamed and the plain kernels; the stand-alone LayerNorm; the layer tails h2 / h2_ws / split3 (G = 1, 2, 4,
8; with a next projection, and without one plus a row mask); the encoder stack and layer under OCV_TOKENS = h2 / split3 / fp32;
few-key attention (h2 in one and in two launches, split3, fp32, and the two-sub-tile form of both fused kernels); many-key
attention; the attention core under both OCV_ATTN_FORMs on contiguous inputs and on the strided views of a packed projection; the
bin head on h2, h2dense and split3.  The last line is a SHA-1 over all the others.
"""
import contextlib, ctypes as C, hashlib, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from objcavit_amd import hip_ops as ops

lib = ops._lib.load()
lines = []
EPS = 1e-5


def rnd(seed, shape, scale=1.0):
    return scale * torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def sha(t):
    t = t.contiguous()
    return hashlib.sha1(t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().tobytes()).hexdigest()[:12]


def note(name, *outs):
    torch.cuda.synchronize()
    lines.append(f"{name:<72s} " + " ".join(sha(o) for o in outs))
    print(lines[-1], flush=True)


def ok(rc):
    assert rc == 0, lib.ocv_last_error().decode(errors="replace")


def p(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def row_mask(M):
    m = torch.zeros(M, dtype=torch.uint8, device="cuda")
    m[3::7] = 1
    return m


def key_mask(B, S, counts):
    return (torch.arange(S, device="cuda")[None, :] >= torch.tensor(counts, device="cuda")[:, None]).contiguous()


def layer(seed, FF):
    torch.manual_seed(seed)
    return torch.nn.TransformerEncoderLayer(128, 4, FF, dropout=0.0, batch_first=True).cuda().eval()


# ---- packers
for (N, K) in [(384, 128), (128, 1024), (40, 72)]:
    w = rnd(1, (N, K))
    note(f"pack3|{(N, K)}", ops.SplitWeight3(w).packed)
    w[1, 3], w[2, 5], w[N - 1, K - 1] = 1.0e5, -7.0e4, float("nan")
    note(f"pack_h2|{(N, K)}|saturated, NaN", ops.SplitWeightH2(w).packed)

# ---- ocv_linear_split3_fwd
M = 45
for N in (128, 160, 384):
    for K in (72, 136):
        w3 = ops.SplitWeight3(rnd(2, (N, K), K ** -0.5))
        for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY_RELU):
            note(f"linear_split3|M{M} N{N} K{K}|act{act}", ops.linear_split3(rnd(3, (M, K)), w3, rnd(4, (N,), 0.3), act))
note(f"linear_split3|M{M} N160 K136|no bias", ops.linear_split3(rnd(3, (M, 136)), ops.SplitWeight3(rnd(2, (160, 136), 136 ** -0.5))))

# ---- residual + LayerNorm, feed-forward: split3 and fp32
x, res = rnd(5, (M, 128)), rnd(6, (M, 128))
wo, bo, g, be = rnd(7, (128, 128), 128 ** -0.5), rnd(8, (128,), 0.3), 1 + rnd(9, (128,), 0.1), rnd(10, (128,), 0.1)
wo3 = ops.SplitWeight3(wo)
FF = 256
w1, b1, w2, b2 = rnd(11, (FF, 128), 128 ** -0.5), rnd(12, (FF,), 0.3), rnd(13, (128, FF), FF ** -0.5), rnd(14, (128,), 0.3)
w13, w23 = ops.SplitWeight3(w1), ops.SplitWeight3(w2)
for masked in (False, True):
    mk = row_mask(M) if masked else None
    out = torch.full((M, 128), float("nan"), device="cuda")
    ok(lib.ocv_linear_residual_layernorm_split3_fwd(p(x), 128, p(wo3.packed), p(bo), p(res), 128, p(g), p(be), EPS, p(mk), p(out), 128, M, 128, 128, st()))
    note(f"linear_res_ln_split3|M{M}|mask {masked}", out)
    note(f"linear_res_ln_fp32|M{M}|mask {masked}", ops.linear_residual_layernorm(x, wo, bo, res, g, be, EPS, mk))
    nb = int(lib.ocv_ffn_split3_workspace_bytes(M, FF))
    assert nb > 0
    for with_ws in (True, False):
        ws = torch.empty(nb // 4, device="cuda") if with_ws else None
        out = torch.full((M, 128), float("nan"), device="cuda")
        ok(lib.ocv_ffn_residual_layernorm_split3_fwd(p(x), p(w13.packed), p(b1), p(w23.packed), p(b2), p(g), p(be), EPS, p(mk), p(out), M, 128, FF,
                                                     p(ws), nb if with_ws else 0, st()))
        note(f"ffn_split3|M{M} FF{FF}|workspace {with_ws}|mask {masked}", out)
    note(f"ffn_fp32|M{M} FF{FF}|mask {masked}", ops.ffn_residual_layernorm(x, w1, b1, w2, b2, g, be, EPS, mk))

# ---- ocv_linear_fwd: the streamed kernel (K % 8 == 0) and the plain one (vector loads at K = 36, scalar at K = 35; both weight layouts)
for K in (128, 36, 35):
    for w_kn in (0, 1):
        for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY_RELU):
            N = 160
            a, w, b = rnd(15, (M, K)), rnd(16, (K, N) if w_kn else (N, K), K ** -0.5), rnd(17, (N,), 0.3)
            out = torch.full((M, N), float("nan"), device="cuda")
            ok(lib.ocv_linear_fwd(p(a), K, 0, p(w), N if w_kn else K, 0, w_kn, p(b), p(out), N, 0, 1, M, N, K, act, st()))
            note(f"linear_fp32|M{M} N{N} K{K}|w_kn {w_kn}|act{act}", out)
    note(f"linear_res_ln_fp32|M{M} K{K}", ops.linear_residual_layernorm(rnd(15, (M, K)), rnd(16, (128, K), K ** -0.5), bo, res, g, be, EPS, None))
note("layernorm_residual", ops.layernorm(x, g, be, EPS, residual=res), ops.layernorm(x, g, be, EPS))

# ---- layer tails
with env(OCV_TOKENS="h2"):
    tails = {}
    for FFt in (128, 256, 1024):
        mods = layer(20, FFt), layer(21, FFt)
        tails[FFt] = [ops.layer_params(m, {}) for m in mods]
for (Mt, FFt) in [(45, 128), (45, 1024), (45, 256), (950, 1024)]:
    (s0, keep0), (s1, keep1) = tails[FFt]
    ctx, xt = rnd(22, (Mt, 128)), rnd(23, (Mt, 128))
    for kind in ("h2", "h2_ws", "split3"):
        for with_next in (True, False):
            out = torch.full((Mt, 128), float("nan"), device="cuda")
            qkv = torch.full((Mt, 384), float("nan"), device="cuda") if with_next else None
            wq = None if not with_next else (s1.in_proj_p3 if kind == "split3" else s1.in_proj_h2)
            mk = None if with_next else row_mask(Mt)
            args = (p(ctx), p(xt), C.byref(s0), wq, s1.in_proj_b if with_next else None, EPS, p(mk), p(out), p(qkv),
                    Mt, 128, FFt)
            G = 1
            if kind == "split3":
                ok(lib.ocv_layer_tail_split3_fwd(*args, st()))
            elif kind == "h2":
                ok(lib.ocv_layer_tail_h2_fwd(*args, st()))
            else:
                G = int(lib.ocv_layer_tail_h2_groups(Mt, FFt))
                ws = torch.zeros(max(int(lib.ocv_layer_tail_h2_workspace_bytes(Mt, FFt)), 16), dtype=torch.uint8, device="cuda")
                ok(lib.ocv_layer_tail_h2_ws_fwd(*args, p(ws), ws.numel(), st()))
            note(f"layer_tail_{kind}|M{Mt} FF{FFt} G{G}|{'next' if with_next else 'row mask'}", *([out, qkv] if with_next else [out]))

# ---- encoder stack and layer
enc = [layer(30 + i, 1024) for i in range(4)]
for mode in ("h2", "split3"):
    with env(OCV_TOKENS=mode):
        caches = [{} for _ in enc]
        params = [ops.layer_params(m, c) for m, c in zip(enc, caches)]
        for (B, S, counts) in [(3, 7, [7, 3, 1]), (2, 132, None)]:
            km = None if counts is None else key_mask(B, S, counts)
            note(f"encoder_stack|{mode}|{(B, S)}|{'masked' if counts else 'full'}",
                 ops.encoder_stack(rnd(34, (B, S, 128)), [q[0] for q in params], km, zero_padded_rows=counts is not None))
        note(f"encoder_layer|{mode}|packed", ops.encoder_layer(rnd(35, (3, 7, 128)), params[0][0], key_mask(3, 7, [7, 3, 1]), True))
with env(OCV_TOKENS="fp32"):
    note("encoder_layer|fp32|not packed", ops.encoder_layer(rnd(35, (3, 7, 128)), ops.layer_params(enc[0], None)[0], key_mask(3, 7, [7, 3, 1]), True),
         ops.encoder_layer(rnd(36, (2, 132, 128)), ops.layer_params(enc[0], None)[0]))

# ---- multi-head attention
torch.manual_seed(40)
mh = torch.nn.MultiheadAttention(128, 4, batch_first=True).cuda().eval()
mh_w = [t.detach() for t in (mh.in_proj_weight, mh.in_proj_bias, mh.out_proj.weight, mh.out_proj.bias)]
with torch.no_grad():
    mh_w[1].copy_(rnd(41, (384,), 0.3)); mh_w[3].copy_(rnd(42, (128,), 0.3))


vk = rnd(45, (2, 300, 128))
for tag, mode, disp in (("h2 one launch", "h2", 1 << 30), ("h2 two launches", "h2", 0), ("split3", "split3", None), ("fp32", "fp32", None)):
    q, k = rnd(43, (2, 45, 128)), rnd(44, (2, 300, 128))
    if disp is not None:
        ok(lib.ocv_mha_few_keys_h2_set_dispatch(disp))
    try:
        with env(OCV_TOKENS=mode):
            out = ops.mha(q, k, vk, *mh_w, key_mask(2, 300, [5, 0]), 4, 5, packed={})
    finally:
        if disp is not None:
            ok(lib.ocv_mha_few_keys_h2_set_dispatch(-1))
    note(f"mha_few|{tag}|(2, 45, 300, 5) counts [5, 0]", out)
for tag, mode in (("h2", "h2"), ("split3", "split3")):      # cdiv(100, 64) * 1024 = 2048 workgroups: two sub-tiles per workgroup
    q, k, v = rnd(46, (1024, 100, 128)), rnd(47, (1024, 8, 128)), rnd(48, (1024, 8, 128))
    cnt = [(i % 6) for i in range(1024)]
    with env(OCV_TOKENS=mode):
        out = ops.mha(q, k, v, *mh_w, key_mask(1024, 8, cnt), 4, 5, packed={})
    note(f"mha_few|{tag} two sub-tiles|(1024, 100, 8, 5)", out)
for mode in ("split3", "fp32"):
    with env(OCV_TOKENS=mode):
        out = ops.mha(rnd(49, (3, 33, 128)), rnd(50, (3, 45, 128)), rnd(51, (3, 45, 128)), *mh_w, key_mask(3, 45, [45, 20, 1]), 4, 0, packed={})
    note(f"mha_many|{mode}|(3, 33, 45) masked", out)

# ---- the attention core
for form in ("h2", "fp32"):
    with env(OCV_ATTN_FORM=form):
        B, S = 3, 45
        qkv = rnd(52, (B * S, 384))
        q, k, v = (qkv[:, i * 128:(i + 1) * 128].reshape(B, S, 128) for i in range(3))
        km = key_mask(B, S, [45, 20, 1])
        note(f"attention|{form}|contiguous", ops.attention_core(q.contiguous(), k.contiguous(), v.contiguous(), km, 4))
        note(f"attention|{form}|strided views of [B S, 384]", ops.attention_core(q, k, v, km, 4), ops.attention_core(q, k, v, None, 4))

# ---- bin head: B = 5 on a ragged 37 x 53 map (its row of tests/test_hip_memory_bounds.py)
feat = rnd(60, (5, 128, 37, 53)).contiguous(memory_format=torch.channels_last)
qs = rnd(61, (5, 300, 128), 0.5)[:, 1:129, :]
wout, bout = rnd(62, (256, 128, 1, 1), 6 / math.sqrt(128)), rnd(63, (256,), 0.5)
widths = torch.rand(5, 256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(64)) + 0.1
centers = (1e-3 + 10.0 * (torch.cumsum(widths / widths.sum(1, keepdim=True), 1) - 0.5 * widths / widths.sum(1, keepdim=True))).contiguous()
for route in ("h2", "h2dense", "split3"):
    with env(OCV_BINHEAD=route):
        note(f"bin_head|{route}|(5, 37, 53)", ops.bin_head(feat, qs, wout, bout, centers), *ops.bin_head(feat, qs, wout, bout, centers, stats=True))

print(f"{len(lines)} cases  sha1 of all lines {hashlib.sha1(chr(10).join(lines).encode()).hexdigest()}  [{os.environ.get('OCV_LIB_PATH', 'product build')}]")
