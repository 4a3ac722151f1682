"""The case table of tests/test_hip_token_abi.py for ocv_linear_fwd, and launch_linear's choice of kernel (csrc/linear.hip)
restated on the host, so that every row can be shown to select the variant it is listed under before anything runs.

A row gives the LOGICAL problem (batch, M, N, K, w_kn, act, bias) and its layout: leading dimensions (None = dense), the
offset in floats of A / W / out behind their 512-byte aligned allocations, and the batch strides (None = dense, i.e. rows x
leading dimension; 0 = the operand is shared by the batch)."""
from collections import namedtuple

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2

Lin = namedtuple("Lin", "variant M N K w_kn act bias lda ldw ldo offA offW batch sA sW sO")


def lin(variant, M, N, K, w_kn=0, act=ACT_NONE, bias=True, lda=None, ldw=None, ldo=None, offA=0, offW=0, batch=1, sA=None, sW=None,
        sO=None):
    lda = K if lda is None else lda
    ldw = (N if w_kn else K) if ldw is None else ldw
    ldo = N if ldo is None else ldo
    sA = M * lda if sA is None else sA
    sW = (K if w_kn else N) * ldw if sW is None else sW
    sO = M * ldo if sO is None else sO
    return Lin(variant, M, N, K, w_kn, act, bias, lda, ldw, ldo, offA, offW, batch, sA, sW, sO)


def dense_twin(c):
    """The same logical problem with dense rows, aligned bases and dense batch strides (shared operands stay shared)."""
    return lin(None, c.M, c.N, c.K, c.w_kn, c.act, c.bias, batch=c.batch, sA=0 if c.sA == 0 else None, sW=0 if c.sW == 0 else None)


def variant_of(ptrA, lda, sA, ptrW, ldw, sW, w_kn, K):
    """launch_linear (csrc/linear.hip):
        vecA = lda % 4 == 0 && sA % 4 == 0 && aligned16(A);  vecW = ldw % 4 == 0 && sW % 4 == 0 && aligned16(W)
        vec = vecA && vecW && (w_kn || K % 4 == 0)
        !w_kn && vec && K % 8 == 0 -> linear_stream_kernel;  else linear_kernel<EPI, w_kn, vec>"""
    vec_a = lda % 4 == 0 and sA % 4 == 0 and ptrA % 16 == 0
    vec_w = ldw % 4 == 0 and sW % 4 == 0 and ptrW % 16 == 0
    vec = vec_a and vec_w and (bool(w_kn) or K % 4 == 0)
    if not w_kn and vec and K % 8 == 0:
        return "stream"
    return ("kn_" if w_kn else "") + ("vec" if vec else "scalar")


def same_arithmetic(v1, v2):
    """linear_kernel<.., VEC> and linear_kernel<.., scalar> differ in how a tile reaches LDS and in nothing behind that;
    linear_stream_kernel walks K in another order than either."""
    return v1 == v2 or {v1, v2} in ({"vec", "scalar"}, {"kn_vec", "kn_scalar"})


def case_variant(c):
    """The variant a row selects; allocations are 512-byte aligned, so a base is aligned iff its offset is a multiple of 4 floats.
    (launch_linear looks at the batch strides whatever the batch: the test hands them over for batch = 1 too.)"""
    return variant_of(4 * c.offA, c.lda, c.sA, 4 * c.offW, c.ldw, c.sW, c.w_kn, c.K)


LINEAR_CASES = [
    # ---- stream: "!w_kn && vec && a.K % 8 == 0" -> linear_stream_kernel<EPI>.  K = 8, 24, 72: one chunk shorter than 128;
    # 136, 520: full chunks and a ragged last one of 8
    lin("stream", 1, 1, 8),
    lin("stream", 33, 40, 24, act=ACT_RELU, lda=28, ldw=28, ldo=41),
    lin("stream", 70, 130, 72, act=ACT_LEAKY, bias=False, ldo=133),
    lin("stream", 33, 160, 136, lda=140),
    lin("stream", 70, 130, 520, act=ACT_RELU, ldw=524, ldo=134),
    lin("stream", 1, 160, 520, act=ACT_LEAKY, lda=524, ldw=524),
    lin("stream", 33, 40, 72, batch=3),                                         # dense batch strides
    lin("stream", 33, 40, 72, batch=3, sW=0, act=ACT_RELU),                     # one weight for the batch
    lin("stream", 33, 130, 72, batch=3, sA=0, bias=False),                      # one activation for the batch
    lin("stream", 33, 40, 72, batch=3, sA=33 * 72 + 8, sW=40 * 72 + 4, sO=33 * 40 + 3),   # gaps; sO is not in "vec": odd
    # ---- <w_kn 0, VEC>: "!w_kn", "vec" (lda, ldw, sA, sW multiples of 4, both bases 16-byte aligned, K % 4 == 0), K % 8 != 0
    lin("vec", 1, 40, 4),
    lin("vec", 33, 130, 36, act=ACT_RELU, bias=False, lda=40, ldw=40, ldo=133),
    lin("vec", 70, 160, 132, act=ACT_LEAKY, ldo=164),
    lin("vec", 70, 1, 132, lda=136),
    lin("vec", 33, 130, 36, batch=3, sW=0),
    lin("vec", 33, 40, 36, batch=3, sA=33 * 36 + 4, sO=33 * 40 + 1, act=ACT_LEAKY),
    # ---- <w_kn 0, scalar>: "vec" false -- K % 4 != 0; A off 16 bytes; lda % 4 != 0; W off 16 bytes; sA % 4 != 0
    lin("scalar", 33, 40, 35, act=ACT_RELU),
    lin("scalar", 70, 130, 35, lda=36, ldw=38, ldo=131, act=ACT_LEAKY, bias=False),
    lin("scalar", 70, 130, 128, offA=1),
    lin("scalar", 33, 160, 128, lda=129, ldw=131, act=ACT_LEAKY),
    lin("scalar", 1, 1, 128, offW=1, bias=False),
    lin("scalar", 33, 40, 128, batch=3, sA=33 * 128 + 1, act=ACT_RELU),
    # ---- <w_kn 1, VEC>: "w_kn" and "vec" (lda % 4 == 0 and ldw % 4 == 0; K itself may be odd: "(w_kn || a.K % 4 == 0)")
    lin("kn_vec", 33, 40, 35, w_kn=1, lda=36),
    lin("kn_vec", 70, 130, 128, w_kn=1, ldw=132, act=ACT_RELU, bias=False, ldo=133),
    lin("kn_vec", 1, 40, 128, w_kn=1, ldw=44, act=ACT_LEAKY),
    lin("kn_vec", 33, 130, 35, w_kn=1, lda=36, ldw=132, batch=3, sW=0, sA=33 * 36),
    lin("kn_vec", 70, 40, 128, w_kn=1, batch=3, sO=70 * 40 + 4),
    # ---- <w_kn 1, scalar>: "w_kn" and "vec" false -- ldw = 130, or lda = 35
    lin("kn_scalar", 33, 130, 128, w_kn=1, ldw=130, act=ACT_RELU),
    lin("kn_scalar", 70, 40, 35, w_kn=1, lda=35, act=ACT_LEAKY, bias=False),
    lin("kn_scalar", 1, 160, 35, w_kn=1, lda=35, ldw=163, ldo=161),
    lin("kn_scalar", 33, 130, 128, w_kn=1, ldw=133, batch=3, sA=0),
]


def lin_id(c):
    pads = "".join(f" {n}={v}" for n, v, d in (("lda", c.lda, c.K), ("ldw", c.ldw, c.N if c.w_kn else c.K), ("ldo", c.ldo, c.N)) if v != d)
    offs = (" A+1" if c.offA else "") + (" W+1" if c.offW else "")
    bat = f" batch={c.batch} sA={c.sA} sW={c.sW} sO={c.sO}" if c.batch > 1 else ""
    return f"{c.variant} M={c.M} N={c.N} K={c.K} act={c.act}{'' if c.bias else ' nobias'}{pads}{offs}{bat}"


def ffn_split_count(M, FF):
    """ocv_ffn_split_count (csrc/linear.hip) restated: workgroups per 32-row tile of the fused feed-forward block."""
    nchunk, tiles, ns = FF // 128, (M + 31) // 32, 1
    while 2 * ns <= nchunk and nchunk % (2 * ns) == 0 and tiles * 2 * ns <= 256:
        ns *= 2
    return ns
