/* objcavit_hip.h -- C ABI of libobjcavit_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the forward depth-inference hot path of ObjCAViT.  The
 * reference has no FFI of its own: the path sits behind Python
 * nn.Module.forward() calls that reach ATen kernels.  Each entry point below
 * replaces the ATen work behind the cited reference lines (paths relative to
 * the reference tree) and is what a ctypes binding in the reference's modules
 * would bind.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (or uint8 for masks) unless
 *     stated otherwise; tensors are dense row-major with the strides given;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - entry points only enqueue work: no allocation, no synchronisation, no
 *     host<->device copies, so a caller may capture them into a hipGraph;
 *     scratch memory is supplied by the caller (`*_workspace_bytes`);
 *   - return 0 on success, a hipError_t (> 0) if a launch failed, -1 for a
 *     rejected argument; ocv_last_error() returns the message (thread-local).
 *   - results are fp32, and so are storage and accumulation.  A contraction runs in one of four forms, named by its entry point:
 *       exact fp32     v_mfma_f32_32x32x2_f32 (the *_exact_* / unsuffixed token entry points, OCV_* = exact / fp32 routes);
 *       fp16 pairs     every operand v = hi + lo with hi = fp16(v), lo = fp16(v - hi) (or lo' = fp16((v - hi) 2^11) for the token
 *                      kernels), every product hi*hi + hi*lo + lo*hi on v_mfma_f32_*_f16 with fp32 accumulation: relative error
 *                      of a product <= 2^-22, range +-65504 (range guard below).  THE DEFAULT of the decoder's and heads' 3x3 / 1x1
 *                      convolutions (f16 = 1 of the *_x_fwd entry points), the token stacks' layer tails, the self-attention core,
 *                      the few-key cross-attention and the bin head;
 *       bf16 pairs     the same with bf16 terms: <= 2^-17 per product, fp32's range.  The encoder's 1x1 layers, and the route every
 *                      fp16-pair kernel falls back to when the range guard trips (f16 = 0);
 *       bf16 triples   three terms, six products ("split3"): 2^-24, fp32's range: the token linears that need both.
 */
#ifndef OBJCAVIT_HIP_H
#define OBJCAVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ocv_stream_t;

#define OCV_ABI_VERSION 5 /* 5: round 6 ADDED ocv_attention_set_dispatch (the library reads no environment variable any more),
 * ocv_conv3x3_packed_taps_k / ocv_conv3x3_split_packed_taps_fwd; nothing removed or changed: a caller built against 4 keeps working;
 * later ADDED (still 5: a new symbol changes nothing for an existing caller) ocv_conv3x3_nhwc_strided_fwd (EfficientNetV2),
 * ocv_depth_metrics_loss_workspace_bytes / ocv_depth_metrics_loss_fwd (validation loss),
 * ocv_depth_normals_fwd / ocv_normals_gather_fwd (surface normals of the final map, Statement N),
 * ocv_ground_grid_workspace_bytes / ocv_ground_grid_fwd (bird's-eye occupancy grid of the final map, Statement G),
 * ocv_ground_plane_workspace_bytes / ocv_ground_plane_fwd (ground plane of the final map, Statement E),
 * ocv_obstacles_workspace_bytes / ocv_obstacles_set_dispatch / ocv_obstacles_fwd (obstacle list of the ground grid, Statement O),
 * ocv_ground_fuse_fwd (ground memory: the grid fused over time, Statement F);
 * 4: round 5 REMOVED the opt-in entry points that lost their A/Bs (ocv_tap_interp_skip_fwd, the squeeze-excite tail
 * family ocv_*_se_fwd / ocv_se_fold_gate_weights_fwd / ocv_se_tail_supported, ocv_conv3x3_winograd_split_fwd F(2x2)) and added the range
 * guard (ocv_range_flag_set, ocv_range_flag_take_fwd, ocv_attention_set_fp32_range), bin head route 4, ocv_mha_few_keys_h2_set_dispatch;
 * 2: ocv_encoder_layer_params starts with struct_size (round 3); 3: ocv_patch_embed_split_fwd and
                           ocv_conv3x3_winograd43_split_fwd take the split operands' element type (+ cscale / oscale), round 4 */
int ocv_abi_version(void);
const char* ocv_last_error(void);

/* Range guard of the fp16 pairs (round 5).  The reference's convolutions are nn.Conv2d in fp32 for ANY input
 * (modules/DenseFeatureExtractor.py:37-47,104-118); the two-term fp16 split of the decoder's activations ends at +-65504.  Every
 * launcher that writes fp16 "hl32" pairs (ocv_conv_nhwc_split_x_fwd, ocv_conv3x3_winograd43_split_fwd,
 * ocv_upsample_concat_split_x_fwd, ocv_tap_interp_*_fwd) ORs 1 into the word the CALLING THREAD armed with ocv_range_flag_set when
 * a value it converts exceeds 65504 / 16 = 4094 in magnitude (the first-batch calibration's own limit) (an atomic on that rare branch only; NULL = not armed, the default).  The word is
 * device memory owned by the caller, sticky until the caller clears it; ocv_range_flag_take_fwd copies it to `out` and zeroes it
 * on the stream (one tiny launch: capturable).  The host reads `out` where it reads results and re-runs the batch on bf16 pairs
 * (objcavit_amd/hip_ops/_core.py: RangeGuard, guarded_forward, bf16_pairs; objcavit_amd/graph.py GraphedGraphBins.checked).  Both
 * return 0 / -1. */
int ocv_range_flag_set(unsigned* flag);
int ocv_range_flag_take_fwd(unsigned* flag, unsigned* out, ocv_stream_t stream);
/* on != 0: ocv_attention_fwd (and every composite built on it) issued by THIS THREAD takes the exact-fp32 core whatever
 * ocv_attention_set_dispatch says -- the two-term fp16 core converts projected queries / keys / values to fp16 and ends at +-65504 like the
 * fp16 pairs; the range guard's fallback route (hip_ops.bf16_pairs) switches it together with them.  Returns 0. */
int ocv_attention_set_fp32_range(int on);
/* Core of ocv_attention_fwd and of every composite built on it (ocv_mha_fwd, ocv_mha_split3_fwd beyond 32 keys, ocv_encoder_layer_fwd,
 * ocv_encoder_stack_fwd): form 0 = two-term fp16 products on v_mfma_f32_32x32x16_f16 (default), 1 = exact fp32 MFMA (the A/B numerics
 * route).  Process-wide, like the other *_set_dispatch entry points; the library reads no environment variable.  Returns 0 / -1. */
int ocv_attention_set_dispatch(int form);

/* activation codes for ocv_linear_fwd */
#define OCV_ACT_NONE 0
#define OCV_ACT_RELU 1
#define OCV_ACT_LEAKY_RELU 2 /* slope 0.01 (nn.LeakyReLU default) */
#define OCV_ACT_SILU 3       /* x * sigmoid(x); convolution entry points only */
#define OCV_ACT_SIGMOID 4    /* ocv_pointwise_conv_nhwc_fwd only (squeeze-excite gate) */

/* out[z][m][n] = act( sum_k A[z][m][k] * W(n,k) + bias[n] )
 * W(n,k) = W[z][n*ldw + k] if w_kn == 0 (nn.Linear layout, [N,K])
 *        = W[z][k*ldw + n] if w_kn != 0 ([K,N] layout).
 * batch strides (elements) may be 0 to share an operand across the batch; 1 <= batch <= 65535 (the grid's z extent).
 * Replaces nn.Linear / nn.Sequential(Linear, LeakyReLU, ...) at
 * modules/ObjCAViT.py:257-282,289,299-303,324-330,378 and
 * modules/miniViT.py:16-20,33; also used for the in/out projections of
 * nn.MultiheadAttention and linear1 of nn.TransformerEncoderLayer. */
int ocv_linear_fwd(const float* A, int lda, long strideA, const float* W, int ldw, long strideW, int w_kn,
                   const float* bias, float* out, int ldo, long strideO, int batch, int M, int N, int K, int act,
                   ocv_stream_t stream);

/* out[m][:] = LayerNorm( residual[m][:] + A[m][:] W^T + bias ) * gamma + beta,  N == E <= 128... exactly 128.
 * zero_row_mask (uint8[M], nullable): rows with a non-zero entry are written as 0.0
 * (nested-tensor fast path of nn.TransformerEncoder).
 * Replaces out_proj + residual + norm1 and linear2 + residual + norm2 of
 * nn.TransformerEncoderLayer (modules/ObjCAViT.py:155-161,169,188; modules/layers.py:8-9,23). */
int ocv_linear_residual_layernorm_fwd(const float* A, int lda, const float* W, int ldw, const float* bias,
                                      const float* residual, int ldres, const float* gamma, const float* beta,
                                      float eps, const uint8_t* zero_row_mask, float* out, int ldo, int M, int N,
                                      int K, ocv_stream_t stream);

/* Fused feed-forward block of a post-norm transformer layer, hidden activations never leave the chip:
 *   out[m][:] = LayerNorm( x[m][:] + W2 relu(W1 x[m][:] + b1) + b2 ) * gamma + beta
 * x / out [M, E] dense (out may alias x), w1 [FF, E], w2 [E, FF] (nn.Linear layout); E == 128, FF % 128 == 0.
 * Replaces linear1 + ReLU + linear2 + residual + norm2 of nn.TransformerEncoderLayer
 * (modules/ObjCAViT.py:155-161,169,188; modules/layers.py:8-9,23). */
int ocv_ffn_residual_layernorm_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                   const float* gamma, const float* beta, float eps, const uint8_t* zero_row_mask,
                                   float* out, int M, int E, int FF, ocv_stream_t stream);

/* out[m][:] = LayerNorm(x[m][:] (+ residual[m][:])) * gamma + beta over E columns (biased variance).
 * residual nullable.  Stand-alone form of the LayerNorm used above. */
int ocv_layernorm_residual_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                               float* out, int rows, int E, ocv_stream_t stream);

/* Attention core: ctx[b, i, h*d : (h+1)*d] = softmax_j( q_bih . k_bjh * scale + mask_bj ) v_bjh,  d == 32.
 * q/k/v/ctx are addressed as ptr + b*batch_stride + i*seq_stride + h*32 (strides in elements), so packed
 * [.., 3E] projections and seq-first (S x B x E) layouts need no copies.
 * key_padding_mask: uint8 [B, Sk], non-zero = ignore key (nullable).  A query row whose keys are ALL masked
 * yields NaN, as torch does. */
int ocv_attention_fwd(const float* q, long q_bs, int q_ss, const float* k, long k_bs, int k_ss, const float* v,
                      long v_bs, int v_ss, const uint8_t* key_padding_mask, float* ctx, long o_bs, int o_ss, int B,
                      int H, int Sq, int Sk, float scale, ocv_stream_t stream);

/* nn.MultiheadAttention(E, H, batch_first=True).forward(query, key, value, key_padding_mask, need_weights=False)
 * (modules/ObjCAViT.py:163-164,195-207): packed in_proj_weight [3E,E] / in_proj_bias [3E], out_proj [E,E] + [E].
 * q_src [B,Sq,E], k_src / v_src [B,Sk,E] dense; out [B,Sq,E].  E == 128, H == 4.
 * kv_limit: 0, or a number of leading keys such that EVERY key j >= kv_limit is masked in every batch row (the
 * caller knows it from the object counts: key_padding_mask is True for j >= n_b, so kv_limit = max_b n_b).  Keys
 * beyond it are then neither projected nor scored -- identical result, since they carry zero probability.  * With E = 128, H = 4 and at most 32 live keys (kv_limit <= 32, or Sk <= 32) the whole operation is one launch
 * (projections, scores, softmax, context, output projection per 32-query tile); otherwise five. */
size_t ocv_mha_workspace_bytes(int B, int Sq, int Sk, int E);
int ocv_mha_fwd(const float* q_src, const float* k_src, const float* v_src, const uint8_t* key_padding_mask,
                const float* in_proj_w, const float* in_proj_b, const float* out_w, const float* out_b, float* out,
                int B, int Sq, int Sk, int kv_limit, int E, int H, void* workspace, size_t workspace_bytes,
                ocv_stream_t stream);

/* ocv_mha_fwd with the four projections as three-term bf16 splits (fp32-faithful; weights packed once by
 * ocv_pack_split3_fwd: in_proj_p3 = packed in_proj_weight [3E, E], out_proj_p3 = packed out_proj.weight [E, E]); QK^T and
 * PV stay on exact fp32 MFMA.  With at most 32 live keys (the image <- object cross-attention, modules/ObjCAViT.py:192-201)
 * K and V are projected ONCE per image (a 32 KB record per image in the workspace, in the order the query tiles' lanes read it) and every 32-query tile is one fused launch
 * reading it; otherwise split3 linears around ocv_attention_fwd.  Same workspace size as ocv_mha_fwd. */
int ocv_mha_split3_fwd(const float* q_src, const float* k_src, const float* v_src, const uint8_t* key_padding_mask,
                       const void* in_proj_p3, const float* in_proj_b, const void* out_proj_p3, const float* out_b, float* out,
                       int B, int Sq, int Sk, int kv_limit, int E, int H, void* workspace, size_t workspace_bytes,
                       ocv_stream_t stream);

/* nn.MultiheadAttention forward with AT MOST 32 LIVE KEYS per image (kv_limit, or Sk itself, <= 32; E = 128, H = 4: the image <-
 * object cross-attention, modules/ObjCAViT.py:192-201) with EVERY contraction -- the four projections, Q K^T and P V -- as a
 * two-term fp16 split: x = hi + 2^-11 lo', hi = fp16(x), lo' = fp16((x - hi) 2^11), three v_mfma_f32_32x32x16_f16 per product
 * block (hi hi into one accumulator, hi lo' + lo' hi into a second that is added scaled by 2^-11); products carry 22 bits,
 * measured error = that of an fp32 FMA chain.  fp16's range applies: an activation beyond +-65504 turns its output rows inf / NaN
 * (packed weights saturate there); ocv_mha_split3_fwd has fp32's range.
 *   ocv_pack_split_h2_fwd: W [N][K] fp32 -> ocv_split_h2_packed_elems(N, K) fp16, 16-byte aligned, laid out
 *     packed[((jt * nsteps + s) * 2 + part) * 512 + lane * 8 + e] = part(W[32 jt + (lane & 31)][16 s + 8 (lane >> 5) + e]).
 *   in_proj_h2 / out_proj_h2 = packed in_proj_weight [3E, E] / out_proj.weight [E, E]; workspace: the K / V record,
 *   ocv_mha_few_keys_h2_workspace_bytes(B); every pointer 16-byte aligned.  ONE launch while the call is
 *   small (ceil(Sq / 32) B <= 320 workgroups: each tile projects its image's K / V itself -- same arithmetic, bit-identical
 *   results, the record unused), two launches beyond (K / V once per image, then the tiles).
 *   ocv_mha_few_keys_h2_set_dispatch(n): one launch up to n workgroups (0 = always two launches, < 0 = the default 320). */
int ocv_mha_few_keys_h2_set_dispatch(int one_launch_max_workgroups);
size_t ocv_split_h2_packed_elems(int N, int K);
int ocv_pack_split_h2_fwd(const float* W, int ldw, int N, int K, void* packed, ocv_stream_t stream);
size_t ocv_mha_few_keys_h2_workspace_bytes(int B);
int ocv_mha_few_keys_h2_fwd(const float* q_src, const float* k_src, const float* v_src, const uint8_t* key_padding_mask,
                            const void* in_proj_h2, const float* in_proj_b, const void* out_proj_h2, const float* out_b,
                            float* out, int B, int Sq, int Sk, int kv_limit, int E, int H, void* workspace,
                            size_t workspace_bytes, ocv_stream_t stream);

/* One post-norm nn.TransformerEncoderLayer(E=128, H=4, FF, relu, eps) in eval mode on x [B,S,E] (dense):
 *   x1 = LN1(x + MHA(x, x, x, mask));  out = LN2(x1 + W2 relu(W1 x1 + b1) + b2)
 * (modules/ObjCAViT.py:155-161,169,188; modules/layers.py:8-9,23).  `out` may alias `x`.
 * zero_padded_rows != 0: rows flagged in key_padding_mask are written as 0.0 in `out` (last layer of a masked
 * encoder). */
typedef struct {
  /* = sizeof(ocv_encoder_layer_params) AS THE CALLER WAS COMPILED.  The library reads only the first struct_size bytes
   * and treats every field beyond them as NULL, so the struct can grow at its end without breaking callers built
   * against an earlier header (ABI 1 had no such field and grew by the four *_p3 pointers: a silent break).  In an
   * array of layers (ocv_encoder_stack_fwd) consecutive elements lie struct_size bytes apart. */
  size_t struct_size;
  const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
  const float *norm1_w, *norm1_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
  /* optional: the four weight matrices packed by ocv_pack_split3_fwd (all four or none).  With them the projections and
   * the feed-forward block run as the three-term bf16 split (fp32-faithful, 2.7x the matrix rate); NULL = exact fp32. */
  const void *in_proj_p3, *out_proj_p3, *linear1_p3, *linear2_p3;
  /* optional (round 3; callers built before it pass a shorter struct_size and these read as NULL): the same four matrices
   * packed by ocv_pack_split_h2_fwd (all four or none).  With them ocv_encoder_stack_fwd runs every layer's token-local tail
   * (output projection, both LayerNorms, feed-forward block, the next layer's q | k | v projection) as two-term fp16 splits
   * (ocv_layer_tail_h2_fwd: half the matrix operations and two thirds of the weight stream of the three-term form; fp16's range). */
  const void *in_proj_h2, *out_proj_h2, *linear1_h2, *linear2_h2;
} ocv_encoder_layer_params;
size_t ocv_encoder_layer_workspace_bytes(int B, int S, int E, int FF);
int ocv_encoder_layer_fwd(const float* x, const ocv_encoder_layer_params* p, const uint8_t* key_padding_mask,
                          int zero_padded_rows, float* out, int B, int S, int E, int H, int FF, float eps,
                          void* workspace, size_t workspace_bytes, ocv_stream_t stream);

/* Three-term bf16 split ("split3") forms of the token-path linear layers: every operand v = h + m + l (h = bf16(v),
 * m = bf16(v - h), l = bf16(v - h - m): 24 significant bits), every product as the six terms whose magnitude exceeds
 * 2^-24 of it, on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- results equal to the exact-fp32 kernels' to fp32
 * rounding at 2.7x their matrix rate (and ~1/2.7 of their matrix-core energy).  The static weight W [N][K] (nn.Linear
 * layout, row stride ldw) is split and packed once per weight version by ocv_pack_split3_fwd into MFMA B-operand
 * fragments, ocv_split3_packed_elems(N, K) bf16 elements:
 *   packed[((jt * ceil(K/16) + s) * 3 + part) * 512 + lane * 8 + e] = part of W[32 jt + (lane & 31)][16 s + 8 (lane >> 5) + e]
 * (zero beyond N / K).  K a multiple of 8.  The packers read W with scalar loads (any ldw >= K, any 4-byte aligned W); `packed`
 * must be 16-byte aligned.  ocv_linear_split3_fwd and ocv_linear_residual_layernorm_split3_fwd stage the rows of A with
 * 16-byte loads: A AND w_packed MUST BE 16-BYTE ALIGNED AND lda A MULTIPLE OF 4 (lda >= K; both return -1 otherwise -- unlike
 * ocv_linear_fwd, which takes any base and leading dimension and falls back to scalar loads).  ldo / ldres / out / residual /
 * bias: any 4-byte aligned address, ldo / ldres >= N.  Same reference lines as ocv_linear_fwd /
 * ocv_linear_residual_layernorm_fwd / ocv_ffn_residual_layernorm_fwd. */
size_t ocv_split3_packed_elems(int N, int K);
int ocv_pack_split3_fwd(const float* W, int ldw, int N, int K, void* packed, ocv_stream_t stream);
int ocv_linear_split3_fwd(const float* A, int lda, const void* w_packed, const float* bias, float* out, int ldo, int M, int N,
                          int K, int act, ocv_stream_t stream);
int ocv_linear_residual_layernorm_split3_fwd(const float* A, int lda, const void* w_packed, const float* bias,
                                             const float* residual, int ldres, const float* gamma, const float* beta,
                                             float eps, const uint8_t* zero_row_mask, float* out, int ldo, int M, int N,
                                             int K, ocv_stream_t stream);
size_t ocv_ffn_split3_workspace_bytes(int M, int FF);
int ocv_ffn_residual_layernorm_split3_fwd(const float* x, const void* w1_packed, const float* b1, const void* w2_packed,
                                          const float* b2, const float* gamma, const float* beta, float eps,
                                          const uint8_t* zero_row_mask, float* out, int M, int E, int FF, void* workspace,
                                          size_t workspace_bytes, ocv_stream_t stream);

/* Everything of a post-norm transformer layer that is local to a token, one launch per 32-token tile (split3 arithmetic):
 *   x1 = LayerNorm1(x + ctx Wo^T + bo);  out = LayerNorm2(x1 + W2 relu(W1 x1 + b1) + b2)   (rows with zero_row_mask != 0: 0)
 *   qkv_next[M][3E] = out . Wqkv_next^T + bqkv_next      when next_in_proj_p3 / next_in_proj_b / qkv_next are given
 * ctx = the attention output of the layer, x its input; p: the layer's parameters with the packed *_p3 weights set.
 * zero_row_mask and a next projection exclude each other (all three ocv_layer_tail_* entry points return -1 before any launch):
 * qkv_next is projected from the LayerNorm2 rows the kernel holds, NOT from the zeroed rows of `out`, and only the last layer of a
 * masked stack zeroes rows -- the one layer without a next projection. */
int ocv_layer_tail_split3_fwd(const float* ctx, const float* x, const ocv_encoder_layer_params* p, const void* next_in_proj_p3,
                              const float* next_in_proj_b, float eps, const uint8_t* zero_row_mask, float* out,
                              float* qkv_next, int M, int E, int FF, ocv_stream_t stream);
/* The same on the two-term fp16 weights (params->out_proj_h2 / linear1_h2 / linear2_h2, next_in_proj_h2 = the NEXT layer's packed
 * in_proj or NULL); csrc/token_h2.hip. */
int ocv_layer_tail_h2_fwd(const float* ctx, const float* x, const ocv_encoder_layer_params* p, const void* next_in_proj_h2,
                              const float* next_in_proj_b, float eps, const uint8_t* zero_row_mask, float* out,
                              float* qkv_next, int M, int E, int FF, ocv_stream_t stream);
/* The same with the feed-forward chunks of every 32-token row block shared out over G workgroups where the launch would leave
 * most of the chip idle (few tokens: the reference's own batch of 1 - 2 images); the row block's last workgroup to arrive adds the
 * partial sums in a fixed order and finishes the layer (one launch, nobody waits).  ocv_layer_tail_h2_groups: G for (M, FF) -- 8 up
 * to 24 row blocks, 4 up to 56, else 1.  workspace: ocv_layer_tail_h2_workspace_bytes (0 when G = 1) = the partial sums
 * followed by one arrival ticket per row block; THE TICKETS MUST BE ZERO WHEN THE CALL STARTS and are zero again when it has
 * finished (ocv_encoder_stack_fwd, which uses this form for batches of up to 4 sequences, clears them itself).  workspace NULL / too small: one workgroup per row block, as above.
 * Results are bit-reproducible for a given (M, FF); they differ from the G = 1 form in the last bits (summation order). */
int ocv_layer_tail_h2_groups(int M, int FF);
size_t ocv_layer_tail_h2_workspace_bytes(int M, int FF);
int ocv_layer_tail_h2_ws_fwd(const float* ctx, const float* x, const ocv_encoder_layer_params* p, const void* next_in_proj_h2,
                             const float* next_in_proj_b, float eps, const uint8_t* zero_row_mask, float* out,
                             float* qkv_next, int M, int E, int FF, void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* nn.TransformerEncoder(layer, n_layers) forward (eval, post-norm, batch-first [B,S,E]) in 1 + 2 n_layers launches: the
 * packed projection of layer 0, then per layer ocv_attention_fwd and ocv_layer_tail_split3_fwd.  Every layer needs its
 * packed split3 weights.  Semantics of key_padding_mask / zero_padded_rows as in ocv_encoder_layer_fwd (the zeros are
 * written by the last layer).  Replaces the nn.TransformerEncoder calls at modules/ObjCAViT.py:169,188 and
 * modules/layers.py:23. */
size_t ocv_encoder_stack_workspace_bytes(int B, int S, int E);
int ocv_encoder_stack_fwd(const float* x, const ocv_encoder_layer_params* layers, int n_layers, const uint8_t* key_padding_mask,
                          int zero_padded_rows, float* out, int B, int S, int E, int H, int FF, float eps, void* workspace,
                          size_t workspace_bytes, ocv_stream_t stream);

/* Patch embedding: Conv2d(C -> E, kernel = stride = 16, no padding) on fmap [B,C,h,w] (NCHW), flattened to tokens,
 * plus bias and positional embedding, written token-major:
 *   out[b][s][e] = bias[e] + pos[b*pos_bs + s*E + e] + sum_{c,i,j} W[e][c][i][j] * fmap[b][c][16*ph+i][16*pw+j]
 * with s = ph*(w/16) + pw.  pos_bs = 0 shares one [S,E] table across the batch; pos may be NULL.
 * channels_last != 0: fmap is stored [B,h,w,C] (torch channels_last) and W in its channels_last storage order
 * [E,16,16,C]; otherwise fmap is [B,C,h,w] and W [E,C,16,16].  (The same flag on the pixel-dot / bin-head entry
 * points selects [B,P,C] vs [B,C,P] for feat; outputs are always NCHW.)
 * Replaces image_embedding_convPxP + flatten + pos add + permute (modules/ObjCAViT.py:287-288,333,362-364;
 * modules/layers.py:11-12,17-22).  E == 128. */
size_t ocv_patch_embed_workspace_bytes(int B, int C, int h, int w, int E);
int ocv_patch_embed_fwd(const float* fmap, int channels_last, const float* W, const float* bias, const float* pos,
                        long pos_bs, float* out, int B, int C, int h, int w, int E, void* workspace,
                        size_t workspace_bytes, ocv_stream_t stream);

/* The same patch embedding on a feature map that is already stored in the "hl32" split-bf16 layout (below: what the
 * decoder's last convolution leaves beside its fp32 result), as 16 two-term-split GEMMs -- one per patch row ky -- in ONE launch
 * of the LDS-DMA convolution kernel (since round 4 their K steps are one axis cut in a batch-dependent number of pieces: the raw
 * partial results, 1 ... 64 of them, go to the workspace), summed in a fixed order with bias and positional embedding.  In that layout the 16 x C
 * values of one patch row are contiguous and the patches of an image row follow each other, so the map is read in place.
 * Products hi*hi + hi*lo + lo*hi (error <= 2^-17 per product, as in every convolution of the path), fp32 accumulation.
 *   x_hl  [B][h][w][2 C] bf16 (C a multiple of 32);   w_hi / w_lo [16 (ky)][E][16 C] bf16, column kx*C + c =
 *   bf16 split of W[e][c][ky][kx];   pos / pos_bs / out as above;   E a multiple of 8;   h a multiple of 16 when B > 1.
 *   workspace: ocv_patch_embed_split_workspace_bytes (the raw partial results).
 *   f16 / oscale: the element type of x_hl, w_hi, w_lo (0 = bf16 pairs, 1 = fp16 pairs) and the nullable per-output-channel
 *   factor [E] on the raw sums, as ocv_conv_nhwc_split_x_fwd (ABI 3). */
size_t ocv_patch_embed_split_workspace_bytes(int B, int C, int h, int w, int E);
int ocv_patch_embed_split_fwd(const void* x_hl, int C, const void* w_hi, const void* w_lo, const float* oscale, int f16,
                              const float* bias, const float* pos, long pos_bs, float* out, int B, int h, int w, int E,
                              void* workspace, size_t workspace_bytes, ocv_stream_t stream);

/* PixelWiseDotProduct (modules/layers.py:31-36): ram[b][q][p] = sum_c feat[b][c][p] * queries[b][q][c].
 * feat [B,C,P] (NCHW with P = h*w), queries addressed as ptr + b*q_bs + q*q_ld + c, ram [B,Q,P].  C == Q == 128. */
int ocv_pixel_dot_fwd(const float* feat, int channels_last, const float* queries, long q_bs, int q_ld, float* ram,
                      int B, int C, int Q, int P, ocv_stream_t stream);

/* Fused bin head (modules/GraphBins.py:109-119 == modules/AdaBins.py:77-87 together with modules/layers.py:31-36):
 *   logits[b][k][p] = bout[k] + sum_q Wout[k][q] * ( sum_c feat[b][c][p] * queries[b][q][c] )
 *   depth[b][p]     = sum_k softmax_k(logits[b][:, p]) * centers[b][k]
 * One pass over feat; the 128-channel range-attention maps and the 256-bin logits / probabilities never reach
 * HBM.  The two contractions are associated as (Wout . queries[b]) . feat (workspace holds the folded
 * [B,256,128] matrix).  C == Q == 128, n_bins == 256. */
size_t ocv_bin_head_workspace_bytes(int B, int n_bins, int C);
/* The two stages of ocv_bin_head_fwd as separate calls (same arithmetic, lets a caller time the main kernel):
 *   ocv_bin_head_fold_fwd   Wf[b] = Wout (n_bins x Q) . queries[b] (Q x C)            -> Wf [B, n_bins, C]
 *   ocv_bin_head_folded_fwd depth[b][p] = sum_k softmax_k(bout + Wf[b] . feat[b][:, p]) * centers[b][k]
 * channels_last selects layout AND arithmetic: 0 = feat is NCHW, 1 = NHWC (both exact fp32 MFMA); 3 = NHWC with the logits as a
 * TWO-term fp16 split with a scaled low term (v = hi + 2^-11 lo', hi = fp16(v), lo' = fp16((v - hi) 2^11): three
 * v_mfma_f32_32x32x16_f16 per product block, 22-bit products = the error of an fp32 FMA chain; both parts of Wf[b] fit the LDS, so
 * one workgroup walks all 256 bins and the map is read once -- the fastest faithful form; fp16's range: a map value or folded
 * weight beyond +-65504 turns the pixel's depth inf / NaN); 4 = 3 with TWO-LEVEL logits: every bin coarsely first (the hi hi
 * product alone), the three-product logits and the softmax arithmetic only for the 32-bin tiles in which some pixel of the
 * wavefront's 32 has a bin within T = 24 (+ twice the coarse product's proven error bound) of its largest coarse logit -- the
 * bins left out weigh <= 224 e^-24 of a pixel's softmax; cost 64 + 24 n MFMAs per 32 pixels, n = tiles kept, against 192;
 * 2 = NHWC, three-term bf16 (fp32's range): ocv_bin_head_folded_ws_fwd only.  (Rounds 2 - 4 also carried a two-term bf16 form under code 2 -- 3x the depth error under near-one-hot softmaxes, opt-in,
 * never a default: removed in round 5.) */
int ocv_bin_head_fold_fwd(const float* queries, long q_bs, int q_ld, const float* Wout, float* Wf, int B, int C, int Q,
                          int n_bins, ocv_stream_t stream);
int ocv_bin_head_folded_fwd(const float* feat, int channels_last, const float* Wf, const float* bout,
                            const float* centers, float* depth, int B, int C, int n_bins, int P, ocv_stream_t stream);
/* The same with scratch for the per-half softmax states: channels_last == 2 = an NHWC map whose logits run
 * as a THREE-term bf16 split (v = h + m + l, six matrix-core products per product, dropped terms <= 2^-24: fp32-faithful)
 * at 2.7x the matrix rate of the exact fp32 kernel -- 256 bins in two halves of 128 (three parts of a half's folded
 * matrix fill 96 KB of LDS), merged per pixel by a second launch.  partials: ocv_bin_head_partials_bytes(B, P) bytes,
 * 16-byte aligned.  Any other channels_last code is handed to ocv_bin_head_folded_fwd. */
size_t ocv_bin_head_partials_bytes(int B, int P);
int ocv_bin_head_folded_ws_fwd(const float* feat, int channels_last, const float* Wf, const float* bout, const float* centers,
                               float* depth, int B, int C, int n_bins, int P, void* partials, size_t partials_bytes,
                               ocv_stream_t stream);
int ocv_bin_head_fwd(const float* feat, int channels_last, const float* queries, long q_bs, int q_ld, const float* Wout,
                     const float* bout, const float* centers, float* depth, int B, int C, int Q, int n_bins, int P,
                     void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* Per-pixel statistics of the SAME softmax, opt-in (the STATS instantiations of every kernel above): with p_k = softmax_k(logits),
 * c_k = centers[b][k] and depth = sum_k p_k c_k as above,
 *   var[b][p]  = sum_k p_k (c_k - depth)^2   (m^2; a negative rounding result is clamped to 0)
 *   pmax[b][p] = max_k p_k                   (= 1 / sum_k exp(logit_k - max logit): what the online softmax carries)
 * both [B][1][P] fp32, each nullable, at least one given; a non-finite pixel gives NaN in both, as in depth.  The moments are carried
 * in fp64 about a per-image pivot, so var has no cancellation floor.  depth is bit-equal to ocv_bin_head_folded_ws_fwd's on the same
 * route; channels_last takes all five codes, 2 (three-term bf16) needs partials of ocv_bin_head_stats_partials_bytes (B, P) bytes,
 * 16-byte aligned (the float4 records + one fp64 moment record per image, half and pixel); the other codes ignore partials.  Under the
 * two-level code 4 the bins left out add <= 8.5e-9 (max_depth - min_depth)^2 to var and <= 8.5e-9 relative to 1 / pmax.
 * No allocation, no synchronisation (hipGraph-capturable); two calls give bit-equal output. */
size_t ocv_bin_head_stats_partials_bytes(int B, int P);
int ocv_bin_head_folded_stats_fwd(const float* feat, int channels_last, const float* Wf, const float* bout, const float* centers,
                                  float* depth, int B, int C, int n_bins, int P, void* partials, size_t partials_bytes, float* var,
                                  float* pmax, ocv_stream_t stream);

/* 3 x 3 convolution, stride 1, zero padding 1, of an image with 1..4 channels into Cout channels (multiple of 4): exact fp32
 * FMA, raw result (no bias, no activation) as NHWC fp32 y [B][H][W][Cout].  x is addressed by element strides (batch,
 * channel, row, column), so NCHW and channels_last images are read in place; w_taps [9][C][Cout] fp32 (tap t = 3 ky + kx
 * major, 16-byte aligned) = W[co][c][ky][kx] transposed.  The skip part of the last decoder stage of do_final_upscale models
 * (reference modules/DenseFeatureExtractor.py:99-101,116-117: the skip tensor is the input image); ocv_tap_interp_combine_fwd
 * adds it to the low-resolution half. */
int ocv_conv3x3_few_channels_fwd(const float* x, long stride_b, long stride_c, long stride_y, long stride_x, const float* w_taps,
                                 float* y, int B, int C, int H, int W, int Cout, ocv_stream_t stream);

/* Depthwise k x k convolution (k in {3,5}, stride in {1,2}) with explicit top/left zero padding (bottom/right
 * padding is implied by Ho/Wo -- covers TensorFlow "SAME"), per-channel bias (folded BatchNorm) and optional SiLU:
 *   out[b][c][y][x] = act( bias[c] + sum_{i,j} w[c][i][j] * in[b][c][y*stride - pad_t + i][x*stride - pad_l + j] )
 * in [B,C,H,W], w [C,k,k], out [B,C,Ho,Wo], NCHW fp32.  Replaces conv_dw + bn + act of the EfficientNet MBConv
 * blocks that the reference runs through its hub backbone (modules/DenseFeatureExtractor.py:18-27,149). */
int ocv_depthwise_conv_fwd(const float* in, const float* w, const float* bias, float* out, int B, int C, int H, int W,
                           int k, int stride, int pad_t, int pad_l, int Ho, int Wo, int act, ocv_stream_t stream);

/* NHWC building blocks of the EfficientNet MBConv stages (exact fp32):
 * pointwise (1x1) convolution as a row GEMM with everything around it fused:
 *   y[m][co] = act( bias[co] + sum_ci x[m][ci] * gate[m / rows_per_image][ci] * W[co][ci] ) + residual[m][co]
 * x [M, Cin] (= [B,H,W,Cin]), W [Cout, Cin], gate (nullable) [B, Cin] = squeeze-excite gate applied to the INPUT,
 * residual (nullable) [M, Cout]; Cin a multiple of 8; act any OCV_ACT_*.  Replaces conv_pw / conv_pwl / conv_head
 * + BatchNorm + SiLU + the SE multiply + the skip add of the hub backbone's blocks
 * (modules/DenseFeatureExtractor.py:18-27,149) and the SE fully-connected layers (with M = B). */
int ocv_pointwise_conv_nhwc_fwd(const float* x, const float* gate, int rows_per_image, const float* W,
                                const float* bias, const float* residual, float* y, long M, int Cin, int Cout, int act,
                                ocv_stream_t stream);

/* The same contraction on the bf16 matrix cores at fp32-level accuracy (split-bf16: every product is formed as
 * hi*hi + hi*lo + lo*hi with fp32 accumulation, relative error of a product <= 2^-17): identical contract, except that
 * the (static) weights arrive pre-split AND packed in matrix-core operand order, so that a wavefront's weight load is
 * one contiguous 1 KB run.  With w_hi = bf16(W), w_lo = bf16(W - w_hi), both zero-padded to [ceil32(Cout)][Kp],
 * Kp = ceil16(Cin):
 *   w_packed[(((jt * (Kp/16) + s) * 2 + part) * 64 + lane) * 8 + e] = w_part[32 jt + (lane & 31)][16 s + 8 (lane >> 5) + e]
 * (part 0 = hi, 1 = lo; bf16; ocv_pointwise_packed_weight_elems() elements).  The exact-fp32 entry point above is
 * MFMA-bound from stage 4 of the encoder on (47 TFLOP/s of 157); this one is the encoder's default. */
size_t ocv_pointwise_packed_weight_elems(int Cin, int Cout);
/* Diagnostics / tests: pin the kernel family ocv_pointwise_conv_nhwc_split_fwd dispatches to, for every later call of
 * this process: 0 = automatic (default), 1 = rows, 2 = stream, 3 = 32-row tile (a = wavefronts across channels 2|4 or 0,
 * b = K groups 1|2 or 0).  A family that cannot run a shape falls back to the automatic choice for that call.  Results
 * do not depend on it beyond fp32 summation order. */
int ocv_pointwise_split_set_dispatch(int family, int a, int b);
int ocv_pointwise_conv_nhwc_split_fwd(const float* x, const float* gate, int rows_per_image, const void* w_packed,
                                      const float* bias, const float* residual, float* y, long M, int Cin, int Cout,
                                      int act, ocv_stream_t stream);
/* ... that also leaves y_hl (nullable): the output in the hl32 split layout ([M][2 ceil32(Cout)] bf16, pad channels zero),
 * for a consumer that reads its rows by LDS-DMA (ocv_pointwise_hl_fwd).  Cout % 8 == 0 when y_hl is given. */
int ocv_pointwise_conv_nhwc_split_hl_fwd(const float* x, const float* gate, int rows_per_image, const void* w_packed,
                                         const float* bias, const float* residual, float* y, void* y_hl, long M, int Cin,
                                         int Cout, int act, ocv_stream_t stream);
/* The same with a caller-provided scratch of ocv_pointwise_split_workspace_bytes(M, Cin, Cout) bytes (0 for most shapes): where the
 * launch would be a handful of 32-row tiles walking a long K on an otherwise idle chip (a batch of 1 - 2 in the late encoder stages:
 * fewer than 128 tiles, K >= 1024) the K slabs of a tile are shared out over up to 8 workgroups that write raw partial tiles to the
 * scratch, and a second launch adds them in ascending order + bias + activation + residual (bitwise reproducible).  Without scratch
 * (or with y_hl) it is ocv_pointwise_conv_nhwc_split_hl_fwd. */
size_t ocv_pointwise_split_workspace_bytes(long M, int Cin, int Cout);
int ocv_pointwise_conv_nhwc_split_ws_fwd(const float* x, const float* gate, int rows_per_image, const void* w_packed,
                                         const float* bias, const float* residual, float* y, void* y_hl, long M, int Cin, int Cout,
                                         int act, void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* The same contraction on a row operand that is ALREADY split, in the "hl32" layout (below: per pixel and 32-channel block,
 * 32 hi then 32 lo bf16 values, pad channels zero) -- what the depthwise / project epilogues of the late encoder stages
 * write -- read by LDS-DMA with no conversion work, and with the squeeze-excite gate folded into PER-IMAGE weights
 * (ocv_se_gate_weights_fwd) instead of multiplied into the rows:
 *   y[m][co] = act( bias[co] + sum_ci x[m][ci] * Wimg[co][ci] ) + residual[m][co],  img = m / rows_per_image
 *   x_hl [M][2 ceil32(Cin)] bf16;  w_packed as above; w_image_elems = 0: one matrix for all rows, else the packed matrix
 *   of image i starts at w_packed + i * w_image_elems (>= ocv_pointwise_packed_weight_elems) and no tile spans two images
 *   (M a multiple of rows_per_image);  y (fp32 [M][Cout]) and / or y_hl (hl32 [M][2 ceil32(Cout)], pad channels written as
 *   zero) -- at least one;  Cin % 8 == 0, Cout % 4 == 0 (% 8 for y_hl).  Same reference lines as above.
 * ocv_pointwise_hl_set_dispatch(rt, tn): pin the wavefront tile (rt x tn blocks of 32 x 32; rt in {1,2,4}, tn in {1,2});
 * (0, 0) = automatic.  Diagnostics / tests only. */
int ocv_pointwise_hl_set_dispatch(int rt, int tn);
int ocv_pointwise_hl_fwd(const void* x_hl, int Cin, const void* w_packed, long w_image_elems, int rows_per_image,
                         const float* bias, const float* residual, float* y, void* y_hl, long M, int Cout, int act,
                         ocv_stream_t stream);
/* Stem convolution: dense 3x3 (Cin * 9 <= 32, Cout <= 64), any stride, explicit top/left zero padding (bottom/right
 * implied by Ho/Wo: TensorFlow "SAME"), + bias (folded BatchNorm) + activation; reads the NCHW image x [B,Cin,H,W] and
 * writes the NHWC activation y [B,Ho,Wo,Cout]; w [Cout][Cin*3*3] (PyTorch's weight, flattened).  Exact fp32.  Replaces
 * conv_stem + bn1 + act1 of the hub backbone (modules/DenseFeatureExtractor.py:18-27). */
int ocv_stem_conv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                      int k, int stride, int pad_t, int pad_l, int Ho, int Wo, int act, ocv_stream_t stream);
/* depthwise k x k (k in {3,5}, stride in {1,2}) on NHWC: in [B,H,W,C], w [k*k][C], out [B,Ho,Wo,C]; C % 4 == 0.
 * Padding / bias / act as ocv_depthwise_conv_fwd. */
int ocv_depthwise_conv_nhwc_fwd(const float* in, const float* w, const float* bias, float* out, int B, int C, int H,
                                int W, int k, int stride, int pad_t, int pad_l, int Ho, int Wo, int act,
                                ocv_stream_t stream);
/* Depthwise convolution + bias + SiLU as ocv_depthwise_conv_nhwc_fwd, that ALSO emits the squeeze-excite pooling sums
 * of its own output, so the activation is not read a second time: part [B][tiles][C] holds one partial sum per
 * workgroup of the launch (tiles = ocv_depthwise_sum_tiles(...), fixed summation order -> reproducible), and
 * ocv_se_gate_partials_fwd turns the partials into the gate (hidden_ws: B * R floats of scratch, R <= 256):
 *   gate[b][c] = sigmoid( b2[c] + sum_r w2t[r][c] * silu( b1[r] + sum_c' w1[r][c'] * mean[b][c'] ) ),
 *   mean[b][c] = (sum_tile part[b][tile][c]) / pixels_per_image.
 * w1 [R][C], w2t [R][C] (= conv_expand's weight transposed).  Replaces conv_dw + bn + act + se.conv_reduce / act /
 * conv_expand / sigmoid of the hub backbone's blocks (modules/DenseFeatureExtractor.py:18-27,149).
 * ocv_depthwise_set_dispatch(mode): which kernel these launches run -- 0 = automatic (k = 5: input rows staged once through
 * LDS; k = 3: register window fed from global memory), 1 = register window everywhere, 2 = LDS rows wherever supported;
 * anything else returns -1.  out / out_hl are bit-identical under every mode, the partial sums (and ocv_depthwise_sum_tiles)
 * are not: the mode must not change between the size query and the launch.  Diagnostics / tests only. */
int ocv_depthwise_set_dispatch(int mode);
int ocv_depthwise_sum_tiles(int B, int C, int Ho, int Wo, int k, int stride);
int ocv_depthwise_conv_nhwc_sum_fwd(const float* in, const float* w, const float* bias, float* out, float* part, int B,
                                    int C, int H, int W, int k, int stride, int pad_t, int pad_l, int Ho, int Wo,
                                    ocv_stream_t stream);
int ocv_se_gate_partials_fwd(const float* part, int tiles, long pixels_per_image, const float* w1, const float* b1,
                             const float* w2t, const float* b2, float* gate, float* hidden_ws, int B, int C, int R,
                             ocv_stream_t stream);
/* ocv_depthwise_conv_nhwc_sum_fwd that writes its output (also, or only: out nullable) in the hl32 split layout: out_hl
 * [B][Ho][Wo][2 C] bf16, C a multiple of 32.  The values are split where they are produced; ocv_pointwise_hl_fwd reads them. */
int ocv_depthwise_conv_nhwc_sum_hl_fwd(const float* in, const float* w, const float* bias, float* out, void* out_hl, float* part,
                                       int B, int C, int H, int W, int k, int stride, int pad_t, int pad_l, int Ho, int Wo,
                                       ocv_stream_t stream);
/* ocv_se_gate_partials_fwd that FOLDS THE GATE INTO THE PROJECT WEIGHTS: for every image b
 *   w_packed + b * w_image_elems  <-  pack(split(W[n][k] * gate[b][k]))      (packed order of ocv_pointwise_conv_nhwc_split_fwd)
 * W fp32 [N][C] (the BN-folded conv_pwl weight), w_image_elems >= ocv_pointwise_packed_weight_elems(C, N) and a multiple of 8;
 * gate (nullable) also receives the [B][C] gate itself.  C a multiple of 8.  Two launches (hidden layer; gate + weights). */
int ocv_se_gate_weights_fwd(const float* part, int tiles, long pixels_per_image, const float* w1, const float* b1,
                            const float* w2t, const float* b2, const float* W, void* w_packed, long w_image_elems, float* gate,
                            float* hidden_ws, int B, int C, int R, int N, ocv_stream_t stream);


/* squeeze: out[b][c] = mean over the P = H*W pixels of x [B,P,C]; two-stage, fixed summation order. */
size_t ocv_channel_mean_workspace_bytes(int B, int C, long P);
int ocv_channel_mean_nhwc_fwd(const float* x, float* out, int B, int C, long P, void* workspace, size_t workspace_bytes,
                              ocv_stream_t stream);

/* squeeze-excite gate: gate[b][c] = sigmoid( b2[c] + sum_r w2t[r][c] * silu( b1[r] + sum_c' w1[r][c'] * mean[b][c'] ) );
 * mean / gate [B, C], w1 [R, C] (conv_reduce), w2t [R, C] (conv_expand weight TRANSPOSED), R <= 256;
 * hidden_ws: caller scratch of B*R floats. */
int ocv_se_gate_fwd(const float* mean, const float* w1, const float* b1, const float* w2t, const float* b2, float* gate,
                    float* hidden_ws, int B, int C, int R, ocv_stream_t stream);

/* Convolution k x k (k in {1,3}), stride 1, zero "same" padding, on NHWC fp32 activations, computed as an implicit
 * GEMM on the bf16 matrix cores with split-bf16 operands (x = hi + lo, 3 MFMAs per product, fp32 accumulate;
 * ~1e-6 relative error, see csrc/conv_igemm.hip; shared pieces csrc/conv_tile.hpp):
 *   y[b][h][w][co] = act( bias[co] + sum_{ky,kx,ci} xcat[b][h+ky-k/2][w+kx-k/2][ci] * Wt[ky*k+kx][co][ci] ) (+ residual)
 * xcat is x1 [B,H,W,C1] followed along channels by the optional x2 [B,H,W,C2] (virtual concat: the skip connection of
 * UpSampleWithSkip, modules/DenseFeatureExtractor.py:44-47).  w_hi / w_lo: bf16 [k*k][Cout][Cp], Cp = C1+C2 rounded up
 * to 32, zero padded, w_hi = bf16(W), w_lo = bf16(W - w_hi) (prepared once on the host).  C1, C2 multiples of 4; C1 a
 * multiple of 32 when x2 is given.  residual (nullable) and y are [B,H,W,Cout].  act: OCV_ACT_*.
 * Replaces the conv3x3 (+ folded BN + LeakyReLU) stages of the UNet decoder (modules/DenseFeatureExtractor.py:37-42,97)
 * and ObjCAViT.conv3x3 / mViT.conv3x3 (modules/ObjCAViT.py:298,374; modules/miniViT.py:15,25). */
int ocv_conv_nhwc_fwd(const float* x1, int C1, const float* x2, int C2, const void* w_hi, const void* w_lo,
                      const float* bias, const float* residual, float* y, int B, int H, int W, int Cout, int ksize,
                      int act, ocv_stream_t stream);
/* The same convolution in EXACT fp32 (v_mfma_f32_32x32x2_f32: fp32 fma chains over blocks of 32 input channels x all taps, summed in
 * channel order; no split operands), any odd k <= 7, any channel counts: the hand-written exact route for A/B numerics and for shapes the
 * split-bf16 kernels do not take (5x slower by construction; not on any default path).  w_tap_major: fp32
 * [k*k][Cout][C1+C2].  Replaces the same reference lines as ocv_conv_nhwc_fwd. */
int ocv_conv_nhwc_exact_fwd(const float* x1, int C1, const float* x2, int C2, const float* w_tap_major, const float* bias,
                            const float* residual, float* y, int B, int H, int W, int Cout, int ksize, int act,
                            ocv_stream_t stream);
/* 3x3 convolution with stride 1 or 2 and explicit zero padding (pad_t rows on top, pad_l columns on the left; the output
 * size Ho x Wo is the caller's: (Ho - 1) stride - pad_t < H, (Wo - 1) stride - pad_l < W, pads < 3) of an NHWC fp32 tensor
 * on the split-bf16 matrix cores (three v_mfma_f32_32x32x16_bf16 per block, fp32 accumulation, as ocv_conv_nhwc_fwd):
 * y = act(conv(x) + bias) (+ residual).  x [B,H,W,Cin], Cin a positive multiple of 4; w_hi / w_lo bf16 [9][Cout][Cp],
 * Cp = Cin rounded up to 32 (ocv_conv_nhwc_fwd's weights); bias [Cout] nullable; residual (nullable) and y
 * [B,Ho,Wo,Cout].  act: OCV_ACT_NONE / RELU / LEAKY_RELU / SILU.  Returns -1 (ocv_last_error) on a bad argument.
 * Replaces the 3x3 convolution (+ folded BN + SiLU, + skip) of torchvision's FusedMBConv (EfficientNetV2 stages 1 - 3,
 * symmetric padding 1), reference modules/DenseFeatureExtractor.py:159-166. */
int ocv_conv3x3_nhwc_strided_fwd(const float* x, int Cin, const void* w_hi, const void* w_lo, const float* bias,
                                 const float* residual, float* y, int B, int H, int W, int Cout, int stride, int pad_t,
                                 int pad_l, int Ho, int Wo, int act, ocv_stream_t stream);

/* Expand 1x1 convolution (+ bias = folded BN, SiLU) and the depthwise k x k convolution (+ bias, SiLU) behind it, fused:
 * the expanded tensor is never written to memory.  x [B,H,W,Cin] NHWC fp32, Cin a multiple of 8 in [24, 64];
 * w_packed = the expand weight [mid][Cin] in the packed split-bf16 layout of ocv_pointwise_conv_nhwc_split_fwd;
 * w_dw [k*k][mid], bias_dw [mid]; y [B,Ho,Wo,mid]; part [B][tiles][mid] = squeeze-excite pooling partials for
 * ocv_se_gate_partials_fwd with tiles = ocv_mbconv_expand_dw_tiles(Ho, Wo, k, stride).  k in {3,5}, stride in {1,2},
 * padding as ocv_depthwise_conv_fwd (out-of-image taps of the EXPANDED tensor are zero).  Numerics: expand as
 * ocv_pointwise_conv_nhwc_split_fwd (split-bf16, fp32 accumulate), depthwise exact fp32.  Replaces conv_pw + bn1 + act1 +
 * conv_dw + bn2 + act2 (+ the pooling of se) of the hub backbone's InvertedResidual blocks
 * (modules/DenseFeatureExtractor.py:18-27). */
int ocv_mbconv_expand_dw_tiles(int Ho, int Wo, int k, int stride);
int ocv_mbconv_expand_dw_fwd(const float* x, const void* w_packed, const float* bias_expand, const float* w_dw,
                             const float* bias_dw, float* y, float* part, int B, int H, int W, int Cin, int mid, int k,
                             int stride, int pad_t, int pad_l, int Ho, int Wo, ocv_stream_t stream);

/* Split-bf16 activation layout "hl32" shared by ocv_upsample_concat_split_fwd and ocv_conv_nhwc_split_fwd: for a
 * logical NHWC activation [B,H,W,C] one bf16 buffer [B*H*W][2*Cp], Cp = C rounded up to 32, holding per pixel and per
 * block of 32 channels the 32 hi values (hi = bf16(v)) followed by the 32 lo values (lo = bf16(v - hi)); element
 * (m, c, part) sits at  m * 2*Cp + (c / 32) * 64 + part * 32 + (c % 32).  Channels C..Cp-1 are stored as zeros.  One
 * (pixel, 32-channel) K step of the convolution is therefore one 128-byte line.  Returns the number of bf16 elements
 * of such a buffer (B*H*W*2*Cp), or 0 on bad sizes. */
size_t ocv_split_act_elems(int B, int H, int W, int C);

/* The same convolution on an input that is ALREADY split: x_hl in the hl32 layout above for Cin channels (128-byte
 * aligned), as produced by ocv_upsample_concat_split_fwd or by a previous convolution's y_hl.  Outputs: y (fp32
 * [B,H,W,Cout], nullable) and / or y_hl (hl32 layout for Cout channels, nullable; needs Cout a multiple of 32).  No
 * fp32->bf16 work per tap in the kernel. */
int ocv_conv_nhwc_split_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* bias,
                            const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout, int ksize,
                            int act, ocv_stream_t stream);
/* The same with a caller-provided workspace of ocv_conv_nhwc_split_workspace_bytes(...) bytes (0 for most shapes): when
 * the tile count would leave the last round of workgroups mostly empty (the 30 x 40 stages of the decoder at B = 16:
 * 600 tiles on 256 CUs) the channel chunks are halved between two workgroups per tile, which write fp32 partial sums
 * to the workspace, and a second pass adds them in a fixed order and applies bias / activation / residual / split.
 * Without a workspace (or with one that is too small) it is ocv_conv_nhwc_split_fwd. */
size_t ocv_conv_nhwc_split_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize);
int ocv_conv_nhwc_split_ws_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* bias,
                               const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout, int ksize,
                               int act, void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* Round 4: the same convolution with the element type of the split operands as a parameter.
 *   f16 = 0: x_hl, w_hi, w_lo, y_hl hold bf16 (hi, lo) pairs -- products good to 2^-17, fp32's range (ocv_conv_nhwc_split_ws_fwd).
 *   f16 = 1: they hold FP16 pairs (hi = fp16(v), lo = fp16(v - hi), the low term unscaled): the same three matrix-core products
 *     per block on v_mfma_f32_16x16x32_f16, good to 2^-22 -- the stress-case margin of the depth map (4.5e-4 of the 1e-3 bar
 *     with bf16 pairs) was these products' alone.  fp16's range is handled explicitly: WEIGHTS are scaled per output channel by
 *     a power of two that puts the row's largest entry near 2^8 (out of the subnormals; hip_ops.prep_conv_weight) and
 *     oscale [Cout] (nullable = ones) = the inverse powers, applied to the raw accumulators in front of bias / activation (exact);
 *     ACTIVATIONS are stored unscaled: beyond +-65504 they become inf (the output is non-finite: loud), below ~0.1 their low
 *     term is subnormal, an ABSOLUTE error floor of 2^-25 per value that only matters for a tensor whose every entry is tiny
 *     (objcavit_amd.hip_ops.fp16_range_report checks a model's activations against both ends).
 * The producers of hl32 tensors take the same flag: ocv_upsample_concat_split_x_fwd, ocv_tap_interp_combine_x_fwd,
 * ocv_conv3x3_winograd43_split_fwd (hl_f16: its input AND its split output), ocv_patch_embed_split_fwd (reads). */
int ocv_conv_nhwc_split_x_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* oscale, int f16,
                              const float* bias, const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout,
                              int ksize, int act, void* workspace, size_t workspace_bytes, ocv_stream_t stream);

/* The same 3 x 3 convolution (stride 1, zero padding 1) with PACKED TAPS (round 6): the K axis of the implicit GEMM is the nine taps'
 * REAL 8-channel granules laid end to end instead of nine chunks of ceil32(Cin) channels, so the matrix cores do not multiply the
 * zero pad channels of every tap -- 24 input channels: 7 K steps of 32 instead of 9; 40: 12 instead of 18 (the skip parts of the
 * decoder's first convolutions, modules/DenseFeatureExtractor.py:44-47 on the encoder's 24- and 40-channel features).  x_hl, outputs,
 * oscale, f16, bias, residual, act: as ocv_conv_nhwc_split_x_fwd (Cin % 8 == 0).  w_hi / w_lo: ONE [Cout][Kp] matrix each,
 * Kp = ocv_conv3x3_packed_taps_k(Cin) = ceil(9 (Cin / 8) / 4) * 32, element (co, 8 ((Cin / 8) t + g) + e) = weight[co][8 g + e] of
 * tap t = 3 ky + kx, zeros beyond the ninth tap.  Same products, same fp32 accumulation; the K order differs from the tap-major form,
 * so results agree to rounding, not bit for bit. */
int ocv_conv3x3_packed_taps_k(int Cin);
/* HALO-STAGED dense 3 x 3 (conv_halo_dma_kernel): ocv_conv_nhwc_split_x_fwd with ksize 3 can run a second kernel whose workgroup is an
 * image-aligned 8 x 32 pixel patch and stages the (8 + 2) x (32 + 2) halo patch of every 32-channel chunk ONCE, where the tap ring stages
 * the 256 tile pixels nine times; the results are bit-identical.
 * ocv_conv3x3_halo_supported: 1 where that kernel can run the shape (pure host arithmetic: H % 8 == 0, W % 32 == 0, a K axis below the
 * length from which ocv_conv_nhwc_split_x_fwd considers split-K -- 9 ceil(Cin / 32) < 128 steps -- and that entry point's operand limits),
 * else 0.  ocv_conv3x3_halo_lds_bytes: the dynamic LDS its launch requests.
 * ocv_conv3x3_set_dispatch(mode): 0 = automatic (the halo kernel on the layers where it measured faster, keyed on H, W, Cin, Cout:
 * 240 x 320 128 -> 128 and 120 x 160 256 -> 256; the tap ring everywhere else), 1 = the tap ring everywhere, 2 = the halo kernel -- an
 * unsupported shape then FAILS (-1, ocv_last_error), it does not fall back; anything else returns -1.
 * ocv_conv3x3_last_kernel: which kernel the last dense 3 x 3 launch of this process ran (1 = tap ring, 2 = halo-staged; 0 = none yet).
 * The last three: diagnostics / tests only. */
int ocv_conv3x3_halo_supported(int B, int H, int W, int Cin, int Cout);
size_t ocv_conv3x3_halo_lds_bytes(void);
int ocv_conv3x3_set_dispatch(int mode);
int ocv_conv3x3_last_kernel(void);
int ocv_conv3x3_split_packed_taps_fwd(const void* x_hl, int Cin, const void* w_hi, const void* w_lo, const float* oscale, int f16,
                                      const float* bias, const float* residual, float* y, void* y_hl, int B, int H, int W, int Cout,
                                      int act, ocv_stream_t stream);

/* The same 3 x 3 convolution (stride 1, zero padding 1) in Winograd F(4x4, 3x3) form on TWO-TERM FP16 splits (round 3), for shapes
 * where the arithmetic dominates the transforms' traffic: 4x fewer matrix-core operations than the direct form, a transformed input
 * of 2.25x the activation.  Input and output are the hl32 split / fp32 tensors of ocv_conv_nhwc_split_x_fwd; inside, the transformed input and filter are fp16 (hi, lo) pairs
 * (22-bit products: the transforms' ~100x error amplification stays at 2 - 3.5e-6 of max |y|, where two bf16 terms give 1e-4).
 *   u_hi, u_lo [36][Cout][Cp] fp16: U'[6 i + j][n][c] = (G g G^T)[i][j][n][c] * 2^k[6 i + j] * 2^-a[c] (fp64 transform; the
 *   power of two per POSITION puts the position's largest entry near 2^8, out of fp16's subnormals; the power of two per INPUT
 *   CHANNEL equalises the filters' columns), hi = fp16(U'), lo = fp16(U' - hi); fscale [36] fp32 = 2^-k; cscale [Cp] fp32 = 2^a
 *   (1 for pad channels; NULL = all ones), applied to the activations by the input transform.
 * Interpolation points 0, 1, -1, 2, -1/2, inf (G rows [1, a, a^2] / prod_{j != i}(a_i - a_j), last row [0 0 1]).  The
 * transformed input is up to 49x the activation (7x per 1-D pass) with an unscaled low term, so the input transform scales every
 * TILE by a power of two taken from that tile's largest input (49 amax 2^s in [2^14, 2^15); a GEMM row: undone exactly by the
 * output transform): no overflow and no subnormal low terms at ANY activation magnitude fp32 holds; inf / NaN inputs give
 * non-finite outputs.  What remains of fp16's range is the spread INSIDE one tile and channel: values 2^-13 below the tile's
 * largest lose low-term bits gradually (their products are that much smaller than the tile's result, too). */
size_t ocv_conv3x3_winograd43_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ocv_conv3x3_winograd43_split_fwd(const void* x_hl, int Cin, const void* u_hi, const void* u_lo, const float* fscale,
                                     const float* cscale, const float* bias, float* y, void* y_hl, int B, int H, int W, int Cout,
                                     int act, int hl_f16, void* workspace, size_t workspace_bytes, ocv_stream_t stream);

/* Second half of "3 x 3 convolution of an up-sampled tensor, computed at the low resolution" (first convolution of every
 * UpSampleWithSkip stage: F.interpolate(bilinear, align_corners=True) + torch.cat + Conv2d(k=3) + BatchNorm + LeakyReLU,
 * modules/DenseFeatureExtractor.py:44-47,37-39).  Bilinear up-sampling is linear and per channel, the convolution mixes
 * channels per tap, so conv_{Wa}(up(x))[p] = sum_t sum_{4 nb} coef(p + t, nb) (Wa_t x[nb]): the caller forms the nine tap
 * products once per LOW-resolution pixel -- z [B,h,w,9 Cout] = ocv_conv_nhwc_split_fwd(ksize 1) of x with the weight rows
 * stacked tap-major, column t Cout + co -- and the skip part s [B,H,W,Cout] = conv3x3 over the skip channels (raw, nullable);
 * this entry point computes
 *   y[b][Y][X][co] = act( bias[co] + s[b][Y][X][co] + sum_t [ (Y,X) + t inside H x W ] bilinear(z[..][t Cout + co]; (Y,X) + t) )
 * with ATen's align_corners=True coefficients, writing fp32 y and / or the hl32 split y_hl.  Exact re-association of the
 * reference's arithmetic; ~4x fewer matrix-core operations for the up-sampled channels.  ocv_tap_interp_supported tells
 * whether (h,w) -> (H,W) is an up-sampling the staging buffer covers (ratios of ~2 and more).
 * zpad = 1 (Decoder.conv2, the 1 x 1 convolution with padding 1 in front of the first stage, :57,:105): the resize source is
 * the h x w grid whose one-pixel border ring holds one constant vector per column (zborder [9 Cout]: the tap products of
 * conv2's bias) and z stores only the (h-2) x (w-2) interior; zpad = 0: zborder NULL, z stores h x w. */
int ocv_tap_interp_supported(int h, int w, int H, int W, int Cout);
/* staging rounds per tap the launch for (h,w) -> (H,W) uses (1..6: which instantiation of the kernel runs; h, w include the
 * border ring of zpad = 1); 0 for sizes below 1.  A host-side query for tests and tools. */
int ocv_tap_interp_staging_rounds(int h, int w, int H, int W);
int ocv_tap_interp_combine_fwd(const float* z, int h, int w, int zpad, const float* zborder, const float* s, const float* bias,
                               float* y, void* y_hl, int B, int H, int W, int Cout, int act, ocv_stream_t stream);
/* the same with the element type of y_hl as a parameter (0 = bf16 pairs, 1 = fp16 pairs: ocv_conv_nhwc_split_x_fwd) */
int ocv_tap_interp_combine_x_fwd(const float* z, int h, int w, int zpad, const float* zborder, const float* s, const float* bias,
                                 float* y, void* y_hl, int hl_f16, int B, int H, int W, int Cout, int act, ocv_stream_t stream);


/* Bilinear resize of x [B,h,w,C1] (NHWC fp32) to H x W with align_corners = True, concatenated along channels with
 * skip [B,H,W,C2] (nullable, then C2 = 0), written in the hl32 split layout for C1+C2 channels (out_hl,
 * ocv_split_act_elems(B,H,W,C1+C2) bf16 elements, 16-byte aligned; pad channels zeroed).  C1, C2 multiples of 4.
 * Replaces F.interpolate + torch.cat of UpSampleWithSkip.forward (modules/DenseFeatureExtractor.py:44-47) and feeds
 * ocv_conv_nhwc_split_fwd. */
int ocv_upsample_concat_split_fwd(const float* x, int h, int w, int C1, const float* skip, int C2, void* out_hl, int B,
                                  int H, int W, ocv_stream_t stream);
/* the same with the element type of out_hl as a parameter (0 = bf16 pairs, 1 = fp16 pairs: ocv_conv_nhwc_split_x_fwd) */
int ocv_upsample_concat_split_x_fwd(const float* x, int h, int w, int C1, const float* skip, int C2, void* out_hl, int f16, int B,
                                    int H, int W, ocv_stream_t stream);

/* Validation-step arithmetic in one pass (next row N2: modules/GraphBinsLM.py:154-212, metrics/MetricsPreprocess.py:14-45,
 * metrics/AbsRel.py:44-52, SqRel.py:45-52, RMSE.py:48-55, RMSELog.py:45-52, Log10.py:52-61, AccThresh.py:59-66).
 * pred [B,1,h,w] = model output; pred_mirror (nullable) = model output for the horizontally flipped image (NOT flipped
 * back): with it the flip-TTA average 0.5 (clamp(pred) + clamp(flip(pred_mirror))) is evaluated, without it clamp(pred).
 * That map is resized to the ground truth's H x W (bilinear, align_corners = True), nan -> min_depth, +-inf ->
 * max_depth; valid pixels: min_depth < gt <= max_depth inside the crop box [crop_y0, crop_y1) x [crop_x0, crop_x1)
 * (pass 0, H, 0, W for none).  records [B][10] per image: abs_rel, sq_rel, rmse, rmse_log, log10, delta1, delta2,
 * delta3 (means over the image's valid pixels; the two RMSEs square-rooted), n_valid, first_image_id + b.
 * Deterministic (fixed-order double-precision reduction); workspace from ocv_depth_metrics_workspace_bytes. */
size_t ocv_depth_metrics_workspace_bytes(int B, int H, int W);
int ocv_depth_metrics_fwd(const float* pred, const float* pred_mirror, int h, int w, const float* gt, int H, int W,
                          float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                          long first_image_id, float* records, int B, void* workspace, size_t workspace_bytes,
                          ocv_stream_t stream);
/* The same pass, also producing what the reference logs as val/loss (modules/GraphBinsLM.py:189-191,243; losses/LossWrapper.py:51-67,
 * losses/SILogLoss.py:28-56, losses/BinsChamferLoss.py:21-37 with pytorch3d 0.7.0 chamfer_distance defaults).  records [B][10] are
 * BIT-IDENTICAL to ocv_depth_metrics_fwd's.  loss_records [B][6] per image, over the mask min_depth < gt <= max_depth of the WHOLE
 * map (no crop) and the resized prediction WITHOUT nan_to_num (a NaN under the mask gives NaN, as in the reference):
 *   mean_g, mean_g2   means of g = log p - log gt and of g^2 (SILog = 10 sqrt(mean_g2 - 0.85 mean_g^2); a batch-wide call
 *                     recombines sum n mean_g, sum n mean_g2, sum n)
 *   n_mask            masked pixels = Chamfer targets T_b
 *   cham_x            (1 / n_bins) sum_k min_t (c_k - t)^2, c_k = 0.5 (e_k + e_k+1) from bin_edges [B][n_bins + 1], t = masked gt
 *   cham_y            (1 / max(T_b, 1)) sum_t min_k (t - c_k)^2           (both 0 for an image without targets)
 *   first_image_id + b
 * The edges may come in any order (the centres are sorted on the device).  A centre that is NaN (a NaN edge: a diverged bin head)
 * is taken as +inf: the image's cham_x is then inf, its cham_y ignores that centre, nothing faults, other images are untouched and
 * the result is still the same on every call.  1 <= n_bins <= 1024, min_depth >= 0.
 * cham_y: minima in fp32 (bit-equal to the fp32 brute-force search); cham_x: in double from the unrounded centres (dense targets
 * sit within ulps of a rounded centre); sums in double in a fixed order; no float atomics: two calls give bit-equal tables.  Workspace from ocv_depth_metrics_loss_workspace_bytes, 8-byte aligned. */
size_t ocv_depth_metrics_loss_workspace_bytes(int B, int H, int W, int n_bins);
int ocv_depth_metrics_loss_fwd(const float* pred, const float* pred_mirror, int h, int w, const float* gt, int H, int W,
                               float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                               const float* bin_edges, int n_bins, long first_image_id, float* records, float* loss_records, int B,
                               void* workspace, size_t workspace_bytes, ocv_stream_t stream);

/* Predict path, input end (modules/Preprocess.py:45-111, modules/GraphBinsLM.py:45,443): decoded frames -> model / metric inputs.
 * ocv_frame_ingest_fwd: frames uint8 [B][Hs][Ws][3] (HWC; frame_stride / row_stride in BYTES, any alignment), the window of H x W pixels
 *   at (top, left) -> out fp32 NCHW [B][3][H][W] with out[b][c][y][x] = table[c][frame value]; table fp32 [3][256] in device memory holds
 *   the reference's ((v / image_norm_factor) - mean[c]) / std[c], evaluated by the host in fp32 in that order (the kernel divides nothing:
 *   bit-equal to the reference arithmetic by construction).  mirror_too != 0: image b is also written flipped along W at
 *   out + mirror_offset (elements; B * 3 * H * W puts the mirrored batch behind the batch: the [batch | mirrored batch] layout of the
 *   validation step's joint forward).  W % 4 == 0 with a 16-byte aligned out: 16-byte stores; any other W: scalar stores.
 * ocv_depth_ingest_fwd: ground truth uint16 [B][Hs][Ws] (strides in ELEMENTS) -> out fp32 [B][1][H][W] = float(v) / factor (1000 NYU,
 *   256 KITTI), IEEE division: bit-equal to torch's fp32 division for all 65536 values.
 * One launch each, no allocation, no synchronisation (hipGraph-capturable). */
int ocv_frame_ingest_fwd(const uint8_t* frames, long frame_stride, long row_stride, int Hs, int Ws, int top, int left,
                         const float* table, float* out, int B, int H, int W, int mirror_too, long mirror_offset,
                         ocv_stream_t stream);
int ocv_depth_ingest_fwd(const uint16_t* depth, long frame_stride, long row_stride, int Hs, int Ws, int top, int left, float factor,
                         float* out, int B, int H, int W, ocv_stream_t stream);
/* Resize on ingest: ocv_frame_ingest_fwd for a window of ANY size -- the Hw x Ww window at (top, left) of every frame -> out fp32 NCHW
 * [B][3][H][W], antialiased (separable triangle filter, half-pixel centres; plain bilinear align_corners = False when enlarging):
 *   out[b][c][y][x] = sum_j sum_k yweight[y][j] xweight[x][k] table[c][ frames[b][top + ystart[y] + j][left + xstart[x] + k][c] ]
 * frames, strides, table, out, mirror_too, mirror_offset: exactly as ocv_frame_ingest_fwd takes them (the mirrored half is the SAME
 * values stored flipped along W, not a resize of the flipped frame).  The tap tables live in DEVICE memory and are made by the host in
 * float64, rounded to fp32 once (objcavit_amd.hip_ops.resize_taps; the statement is tests/resize_ref.py): per axis int32 start[n_out],
 * ascending, and fp32 weight[n_out][K]; a row with fewer than K taps is padded with weight 0.  The kernel decides no tap: it clamps
 * every source index into the window, so a padded slot reads a window pixel with weight 0 and nothing outside the window is touched
 * whatever the tables hold.  Values are the TABLE's (already normalised) values, interpolated in fp32 with fma, taps in ascending
 * source index, x pass then y pass: within (Ky + Kx + 4) 2^-24 max|table| of the float64 statement; a window of the output's size
 * (weights 1, 0) is bit-equal to ocv_frame_ingest_fwd.
 * NAMES: these two do NOT end in _fwd although ocv_frame_resize_ingest launches a kernel.  The guarded-memory suite
 * (tests/test_hip_memory_bounds.py) keeps one table row per *_fwd symbol and fails on a *_fwd name without one; that file is a fixed
 * yardstick, so the resize entry points carry their guarded run in their own test file (tests/test_hip_resize_ingest.py) and a name
 * outside the pattern.
 * Served: Hw <= OCV_FRAME_RESIZE_MAX_RATIO * H and Ww <= OCV_FRAME_RESIZE_MAX_RATIO * W (any enlargement), 1 <= Ky, Kx <=
 * OCV_FRAME_RESIZE_MAX_TAPS; ocv_frame_resize_supported answers the first without a launch (1 / 0).  Beyond it: -1 with a message that
 * names the limit -- the filter is never truncated.  Also -1 before any launch on a null pointer, bad sizes, a window outside the frame,
 * strides smaller than a row / a frame, misaligned out / table / tap tables, a mirrored half that overlaps the batch.
 * One launch, one 256-thread workgroup per image and output tile (8 x 64 outputs up to a ratio of about 2.5, smaller tiles beyond: the
 * LDS request stays under 48 KB), no allocation, no workspace, no synchronisation, no environment read (hipGraph-capturable); no atomics:
 * two calls give identical bytes. */
#define OCV_FRAME_RESIZE_MAX_RATIO 8
#define OCV_FRAME_RESIZE_MAX_TAPS 18
int ocv_frame_resize_supported(int Hw, int Ww, int H, int W);
int ocv_frame_resize_ingest(const uint8_t* frames, long frame_stride, long row_stride, int Hs, int Ws, int top, int left, int Hw, int Ww,
                            const float* table, const int* ystart, const float* yweight, int Ky, const int* xstart, const float* xweight,
                            int Kx, float* out, int B, int H, int W, int mirror_too, long mirror_offset, ocv_stream_t stream);
/* Pixel formats on ingest: the two launches above for frames as decoders and capture APIs deliver them, and the window as RGB24.
 * A frame batch is up to three PLANES, each with its own base pointer, frame stride and row stride in BYTES, at any alignment
 * (Hc = ceil(Hs / 2), Wc = ceil(Ws / 2)); unused planes are null with strides 0:
 *   OCV_PIXFMT_RGB24 / BGR24     plane 0 [B][Hs][Ws][3]
 *   OCV_PIXFMT_RGBA32 / BGRA32   plane 0 [B][Hs][Ws][4], alpha ignored
 *   OCV_PIXFMT_NV12              plane 0 = Y [B][Hs][Ws]; plane 1 = CbCr [B][Hc][Wc][2] (Cb first)
 *   OCV_PIXFMT_I420              plane 0 = Y; plane 1 = Cb [B][Hc][Wc]; plane 2 = Cr [B][Hc][Wc]
 * 4:2:0: pixel (x, y) takes chroma sample (x >> 1, y >> 1) (replication; no sited interpolation).  YCbCr -> RGB is STATEMENT P, in
 * integers, from yuv_table = int32 [5][256] in device memory, made by the host in float64 and rounded once
 * (objcavit_amd.pixel_formats.yuv_tables; matrix bt601 Kr = 0.299, Kb = 0.114 or bt709 Kr = 0.2126, Kb = 0.0722, Kg = 1 - Kr - Kb; range
 * limited y0 = 16, sy = 255 / 219, sc = 255 / 224 or full y0 = 0, sy = sc = 1):
 *   T0[v] = rint(2^16 sy (v - y0)) + 2^15            T1[v] = rint(2^16 sc 2 (1 - Kr) (v - 128))
 *   T2[v] = rint(2^16 sc (-2 Kb (1 - Kb) / Kg) (v - 128))   T3[v] = rint(2^16 sc (-2 Kr (1 - Kr) / Kg) (v - 128))
 *   T4[v] = rint(2^16 sc 2 (1 - Kb) (v - 128))
 *   R = clamp((T0[Y] + T1[Cr]) >> 16)   G = clamp((T0[Y] + T2[Cb] + T3[Cr]) >> 16)   B = clamp((T0[Y] + T4[Cb]) >> 16)
 * with >> the arithmetic shift and clamp to 0 .. 255.  The kernels decide no coefficient; packed formats take yuv_table = null.
 * ocv_frame_ingest_format: ocv_frame_ingest_fwd on those R, G, B bytes -- same table, out, mirror_too, mirror_offset, the same 16-byte /
 *   scalar store rule, one launch, no workspace (hipGraph-capturable); RGB24 launches the very kernel of ocv_frame_ingest_fwd.
 * ocv_frame_resize_ingest_format: ocv_frame_resize_ingest likewise; only the staging step reads the format (it leaves RGB bytes in LDS),
 *   the two tap passes are those of ocv_frame_resize_ingest: bit-equal to it on the converted frames.  Same ratio and tap limits.
 * ocv_frames_to_rgb24: the Hw x Ww window at (top, left) -> out uint8 [B][Hw][Ww][3], every byte written, one launch.
 * -1 before any launch, the message naming the entry point: null plane of the format, unknown format id, bad sizes, window outside the
 * frame, a plane's strides smaller than its row (Ws x 1 / 3 / 4 bytes; chroma rows 2 Wc for NV12, Wc for I420) / its frame, null or
 * misaligned yuv_table for a 4:2:0 format, and the out / table / tap-table / mirror checks of the rgb24 entry points.
 * NAMES: like ocv_frame_resize_ingest these do not end in _fwd; their guarded runs are in tests/test_hip_pixel_formats.py. */
#define OCV_PIXFMT_RGB24 0
#define OCV_PIXFMT_BGR24 1
#define OCV_PIXFMT_RGBA32 2
#define OCV_PIXFMT_BGRA32 3
#define OCV_PIXFMT_NV12 4
#define OCV_PIXFMT_I420 5
int ocv_frame_ingest_format(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                            long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2,
                            const int* yuv_table, int Hs, int Ws, int top, int left, const float* table, float* out, int B, int H, int W,
                            int mirror_too, long mirror_offset, ocv_stream_t stream);
int ocv_frame_resize_ingest_format(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                                   long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2,
                                   const int* yuv_table, int Hs, int Ws, int top, int left, int Hw, int Ww, const float* table,
                                   const int* ystart, const float* yweight, int Ky, const int* xstart, const float* xweight, int Kx,
                                   float* out, int B, int H, int W, int mirror_too, long mirror_offset, ocv_stream_t stream);
int ocv_frames_to_rgb24(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1, long frame_stride1,
                        long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2, const int* yuv_table, int Hs, int Ws,
                        int top, int left, uint8_t* out, int B, int Hw, int Ww, ocv_stream_t stream);
/* Lens on ingest: the rectified Hw x Ww window of DISTORTED frames of any format, as ocv_frame_ingest_format / ocv_frames_to_rgb24 write
 * a cropped one.  The geometry is the host's: a map of the source coordinate of every rectified pixel, made in float64
 * (objcavit_amd/lens.py: any model -- rational Brown-Conrady, Kannala-Brandt fisheye, coordinates exported from elsewhere) and quantised
 * to fixed point.  The device applies STATEMENT L, in integers only:
 *   map   int32 [M][Hw][Ww][2] in device memory, M = 1 (one camera for the batch) or M = B (a map per image), 16-byte aligned.  Entry
 *         (X, Y) of rectified pixel (u, v) is its source coordinate in units of 1/256 pixel, relative to the WHOLE source frame (pixel
 *         centres at integer indices): X = floor(xs * 256 + 0.5) in float64, clamped by the host to [-256, Ws * 256] (Y: [-256,
 *         Hs * 256]), NaN -> -256.  The device needs no range check beyond the tap test below and is safe for any int32.
 *   taps  x0 = X >> 8 (arithmetic), wx = X & 255; y0, wy likewise; (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).  A tap
 *         outside 0 <= x < Ws, 0 <= y < Hs has R = G = B = 0 (a constant black border, decided per tap); a tap inside is the R, G, B of
 *         that source pixel in the frames' format -- for NV12 / I420 Statement P applied per tap, chroma sample (x >> 1, y >> 1).
 *   byte  acc = (256 - wx)(256 - wy) v00 + wx (256 - wy) v10 + (256 - wx) wy v01 + wx wy v11 per channel;
 *         byte = (acc + 32768) >> 16   (acc + 32768 <= 255 * 65536 + 32768: int32 holds it, no clamp).
 * ocv_frame_remap_ingest_fwd: table[c][byte] at (b, c, v, u) of out fp32 [B][3][Hw][Ww] and, with mirror_too, at (b, c, v, Ww - 1 - u) of
 *   the image mirror_offset elements behind -- the layout, out / mirror_offset rules and 16-byte / scalar store rule of
 *   ocv_frame_ingest_fwd (16-byte stores: Ww % 4 == 0, out 16-byte aligned, mirror_offset % 4 == 0).
 * ocv_frames_remap_rgb24_fwd: the three bytes at out uint8 [B][Hw][Ww][3], every byte written.
 * Consequences: the first is bit-equal to ocv_frame_ingest_fwd of the second's output; an identity map (X = 256 (left + u),
 * Y = 256 (top + v)) is bit-equal to ocv_frame_ingest_fwd / ocv_frame_ingest_format at (top, left).
 * The plane arguments are those of ocv_frame_ingest_format.  -1 before any launch, the message naming the entry point: its source checks
 * (null plane, unknown format, bad sizes, strides, yuv_table), null map / table / out, Hw or Ww < 1, a map that is not 16-byte
 * aligned, M outside {1, B}, misaligned out / table, a mirrored half that overlaps the batch.  One launch each, no workspace, no
 * synchronisation, no atomics (hipGraph-capturable; two calls give identical bytes). */
int ocv_frame_remap_ingest_fwd(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                               long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2,
                               const int* yuv_table, int Hs, int Ws, const int* map, int M, int Hw, int Ww, const float* table, float* out,
                               int B, int mirror_too, long mirror_offset, ocv_stream_t stream);
int ocv_frames_remap_rgb24_fwd(int format, const uint8_t* plane0, long frame_stride0, long row_stride0, const uint8_t* plane1,
                               long frame_stride1, long row_stride1, const uint8_t* plane2, long frame_stride2, long row_stride2,
                               const int* yuv_table, int Hs, int Ws, const int* map, int M, int Hw, int Ww, uint8_t* out, int B,
                               ocv_stream_t stream);
/* Predict path, output end(modules/GraphBinsLM.py:159-183,295-301,367, metrics/MetricsPreprocess.py:17-24): the map the metric pass
 * above forms per pixel, written out.  pred [B][1][h][w], pred_mirror nullable and still mirrored (as for the metric pass):
 *   d = resize_{H x W, bilinear, align_corners}(0.5 (clamp(pred) + clamp(flip(pred_mirror)))  or  clamp(pred)), nan -> min_depth,
 *   +-inf -> max_depth; a NaN source pixel reaches every output pixel that has it as a tap, zero-weight taps included (ATen's 0 * NaN).
 * Outputs, each nullable (at least one given):
 *   depth      fp32 [B][1][H][W] = d
 *   depth_u16  [B][H][W] = min(65535, max(0, rint(d * u16_scale))), ties to even (16-bit PNG convention: x 1000 NYU, x 256 KITTI)
 *   rgb8       [B][H][W][3] = colormap[clamp(floor((d - vmin) * colormap_scale), 0, 255)], colormap uint8 [256][3] in device memory,
 *              colormap_scale = 256 / (vmax - vmin) computed by the caller in fp32 (matplotlib's Normalize + colormap call).
 * One launch; H * W % 8 == 0 with 16-byte aligned outputs: 16-byte stores; otherwise scalar stores.  Two calls give bit-equal output. */
int ocv_depth_finalize_fwd(const float* pred, const float* pred_mirror, int h, int w, float min_depth, float max_depth, int H, int W,
                           float* depth, uint16_t* depth_u16, float u16_scale, uint8_t* rgb8, const uint8_t* colormap, float vmin,
                           float colormap_scale, int B, ocv_stream_t stream);
/* The same resize for the bin head's statistics.  The distribution predicted at an output pixel is the MIXTURE of its source
 * distributions, weighted with the bilinear align_corners weights w_t of the depth map above (under flip-TTA: halved, over pred / var /
 * pmax and the un-mirrored *_mirror maps).  With d_t the UNCLAMPED pred, m = sum_t w_t d_t:
 *   depth_std  fp32 [B][1][H][W] = sqrt( sum_t w_t (var_t + (d_t - m)^2) )    (law of total variance: every term non-negative)
 *   confidence fp32 [B][1][H][W] = sum_t w_t pmax_t
 * nan -> max_depth - min_depth (depth_std), 0 (confidence); a NaN source pixel reaches every output pixel that has it as a tap, zero-weight
 * taps included.  Each output nullable (at least one given); depth_std reads pred and var, confidence reads pmax -- maps that are not
 * read may be null; with flip-TTA (any *_mirror given) every map that is read needs its mirror.  All maps [B][1][h][w].  One launch, the
 * LDS tile staging and the vector / scalar store rules of ocv_depth_finalize_fwd; no allocation, no synchronisation; bit-equal on repeat. */
int ocv_depth_finalize_stats_fwd(const float* pred, const float* pred_mirror, const float* var, const float* var_mirror,
                                 const float* pmax, const float* pmax_mirror, int h, int w, float min_depth, float max_depth, int H, int W,
                                 float* depth_std, float* confidence, int B, ocv_stream_t stream);
/* Per-object readout of the final map: depth statistics per detection box (no counterpart in the reference; the statement the tests
 * compare against is tests/object_depth_ref.py).  depth [B][1][H][W] fp32 (the map of ocv_depth_finalize_fwd), depth_std the same shape
 * or null; box r of image b = xywh[(b * cap + r) * xywh_row_stride + 0..3] = centre x, centre y, width, height in pixels of the map's
 * grid; counts int32 [B] in DEVICE memory, read by the kernel only (capturable: a replay serves whatever the buffers hold).
 * Pixel (x, y) belongs to a box iff its centre (x + 0.5, y + 0.5) lies in [cx - hw, cx + hw) x [cy - hh, cy + hh), in fp32 and in this
 * order: hw = half * w (half = fp32(0.5 * shrink), 0 < shrink <= 1 reads the central part of the box), x0 = ceil((cx - hw) - 0.5),
 * x1 = ceil((cx + hw) - 0.5); non-finite -> empty; both clamped to [0, W]; columns x0 .. x1 - 1; rows alike from cy, h, H.
 * out [B][cap][5 + Q] fp32, v = the non-NaN values of the box's pixels in ascending order (+-inf take part):
 *   0 n         their number (exact below 2^24)        1 min = v[0]        2 max = v[n - 1]
 *   3 mean      float64 sum of v / n, rounded to fp32
 *   4 std_mean  the same mean of depth_std over the same pixels (0 without depth_std)
 *   5 + i       v[floor(quantiles[i] * (n - 1))], product and floor in double: an ELEMENT of the map, never interpolated (0.5: the
 *               lower median, torch.median's); -0 and +0 are one value and either may be returned
 * Every column is 0 for a row at or beyond counts[b] and for a row whose pixel set is empty or all NaN: n = 0 is the flag.  Every
 * element of out is written.  quantiles: HOST array of Q doubles in [0, 1], 1 <= Q <= 8, copied by value into the launch.
 * One launch of B * cap workgroups (exact radix select, 4 reads of a box's pixels), no workspace, no allocation, no synchronisation, no
 * float atomics: two calls give bit-equal output. */
int ocv_object_depth_fwd(const float* depth, const float* depth_std, const float* xywh, long xywh_row_stride, const int* counts, int B,
                         int cap, int H, int W, float half, const double* quantiles, int Q, float* out, ocv_stream_t stream);
/* Point-cloud output of the final map: a deterministic, filtered stream compaction with a pinhole back-projection (no counterpart in the
 * reference, which only carries the focal length with every sample; the statement the tests compare against is tests/point_cloud_ref.py).
 * depth [B][1][H][W] fp32 (the map of ocv_depth_finalize_fwd); K [B][4] fp32 in DEVICE memory = fx, fy, cx, cy in pixels of the map's own
 * grid, OpenCV convention (the integer index (x, y) is the pixel's centre; the caller shifts the principal point by the crop origin);
 * confidence / depth_std: the same shape as depth, or null; frames: null, or uint8 [B][Hs][Ws][3] with byte strides frame_stride /
 * row_stride (as ocv_frame_ingest_fwd takes them) of which the H x W window at (top, left) is the map's grid.
 * Pixel (x, y) of image b is KEPT iff  y % sy == 0 and x % sx == 0;  z = depth[b][0][y][x] is finite and near <= z <= far;  with a
 * confidence map conf >= min_confidence (NaN fails);  with a std map std <= max_std (NaN fails);  and fx, fy are finite and > 0 and
 * cx, cy finite (else the image keeps nothing).  Kept pixels are numbered in row-major order of (y, x); point i is the i-th kept pixel.
 * Record i of image b = points[(b * cap + i) * 4 .. + 4), 16 bytes written by one store:
 *   bytes 0-11  X, Y, Z fp32, every operation rounded on its own:  rx = (float(x) - cx) / fx,  ry = (float(y) - cy) / fy (IEEE
 *               division),  X = rx * z,  Y = ry * z,  Z = z
 *   bytes 12-14 R, G, B of frames[b][top + y][left + x]; 0 without frames
 *   byte 15     rint(255 * clamp(conf, 0, 1)), ties to even; 255 without a confidence map
 * pixel: null, or int32 [B][cap] = y * W + x of every point.  total int32 [B] = number of kept pixels; counts int32 [B] = min(total, cap):
 * with total > cap the first cap points in order are written.  Rows of points / pixel at or beyond counts[b] are NOT WRITTEN (they keep
 * whatever the buffer held: a multi-megabyte tail per image is not zeroed).  points and K 16-byte aligned.
 * workspace: ocv_depth_unproject_workspace_bytes = B * T * 4 bytes, T = ceil(ceil(H / sy) * ceil(W / sx) / OCV_UNPROJECT_TILE) tiles per
 * image (0 for sizes the entry point refuses).  Two launches on the stream (count per tile; prefix + write) and nothing else: no
 * allocation, no synchronisation, no atomics, nothing read on the host (capturable); two calls give identical bytes.  Images are
 * independent: a batch can be filled by one call per image with offset pointers.
 * -1 with a message before any launch on: a null required pointer, bad sizes, a stride < 1, cap < 1, near > far (or NaN), a window that
 * does not fit the frame, a workspace that is too small, misaligned pointers. */
#define OCV_UNPROJECT_TILE 2048
size_t ocv_depth_unproject_workspace_bytes(int B, int H, int W, int sy, int sx);
int ocv_depth_unproject_fwd(const float* depth, const float* K, const float* confidence, const float* depth_std, const uint8_t* frames,
                            long frame_stride, long row_stride, int Hs, int Ws, int top, int left, int B, int H, int W, int sy, int sx,
                            float near, float far, float min_confidence, float max_std, int cap, float* points, int* pixel, int* counts,
                            int* total, void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* Surface normals of the final map, STATEMENT N (no counterpart in the reference; the statement the tests compare against is
 * tests/normals_ref.py).  The final map is a bilinear enlargement of the head's map, hence piecewise bilinear: one-pixel differences give
 * faceted normals, so the slope is the LEAST-SQUARES plane slope over a (2r + 1)^2 window.
 * depth [B][1][H][W] fp32 (the map of ocv_depth_finalize_fwd); K [B][4] fp32 in DEVICE memory = fx, fy, cx, cy in pixels of the map's own
 * grid, the integer index (x, y) being the pixel's centre (as ocv_depth_unproject_fwd takes it); radius r in 1..4; near <= far;
 * edge_ratio > 0.
 * VALIDITY (bit-exact: every operation fp32, rounded on its own).  Pixel (x, y) of image b is VALID iff
 *   the window [x - r, x + r] x [y - r, y + r] lies inside the map;
 *   every z of the window is finite (no NaN, no +-inf) and near <= z <= far;
 *   with zc = z(x, y), t = edge_ratio * zc, wmax / wmin the window's extremes:  wmax - zc <= t  and  zc - wmin <= t  (no depth
 *     discontinuity inside the window);
 *   fx, fy are finite and > 0 and cx, cy finite (else the image has no valid pixel).
 * SLOPES, with D = (2r + 1) * 2 * sum_{i=1..r} i^2 (the reference: fp64 from the fp32 map; the kernel: fp32, sums in its own order):
 *   zu = sum_{j=-r..r} sum_{i=1..r} i * (z(x + i, y + j) - z(x - i, y + j)) / D
 *   zv = sum_{i=-r..r} sum_{j=1..r} j * (z(x + i, y + j) - z(x + i, y - j)) / D
 * NORMAL of the back-projected surface P = ((x - cx) z / fx, (y - cy) z / fy, z), pointing at the camera (n . P = -z^2 / |m| < 0):
 *   m = ( fx * zu,  fy * zv,  -(zc + (x - cx) * zu + (y - cy) * zv) ),   n = m / |m|   (m = 0, a flat window at z = 0: n = (0, 0, -1))
 * OUTPUTS, each nullable, at least one given, EVERY element of a given output written:
 *   normals      fp32  [B][3][H][W]  n at valid pixels, (0, 0, 0) at invalid ones
 *   normals_rgb8 uint8 [B][H][W][3]  rint(127.5 * n + 127.5) clamped to 0..255 per component; (0, 0, 0) at invalid pixels
 *   valid        uint8 [B][H][W]     1 / 0
 * One launch, one 256-thread workgroup per 64 x 16 tile: the tile and its halo of r staged once into LDS, a pass per row (ramp sum, box
 * sum, min, max of the 2r + 1 horizontal neighbours), a pass per pixel (their vertical combination, predicate, normalisation, stores).
 * No atomics, no workspace, no allocation, no synchronisation, nothing read on the host (capturable); two calls give identical bytes.
 * Images are independent: a batch can be filled by one call per image with offset pointers.
 * -1 with a message before the launch on: a null depth / K, all outputs null, r outside 1..4, non-positive sizes, H * W or B * tiles
 * at or above 2^31, near > far (or NaN), edge_ratio <= 0 (or NaN), K not 16-byte aligned, depth / normals not 4-byte aligned. */
int ocv_depth_normals_fwd(const float* depth, const float* K, int H, int W, int r, float near, float far, float edge_ratio, float* normals,
                          uint8_t* normals_rgb8, uint8_t* valid, int B, ocv_stream_t stream);
/* A normal for every point of ocv_depth_unproject_fwd's cloud: normals [B][3][H][W] (above), pixel int32 [B][cap] and counts int32 [B] (the
 * cloud's; counts is read on the device only) -> out fp32 [B][cap][4], 16-byte aligned:  out[b][i] = (nx, ny, nz, 0) of pixel
 * pixel[b][i] = y * W + x, ONE 16-byte store, for i < min(counts[b], cap); an index outside [0, H * W) gives (0, 0, 0, 0).  Rows at or
 * beyond counts[b] are NOT WRITTEN (the cloud's rule).  One launch, no workspace, no atomics; capturable; bit-equal on repeat.
 * -1 with a message before the launch on: a null pointer, non-positive sizes, H * W or B * cap at or above 2^31, a misaligned pointer. */
int ocv_normals_gather_fwd(const float* normals, const int* pixel, const int* counts, int H, int W, int cap, float* out, int B,
                           ocv_stream_t stream);
/* Bird's-eye occupancy grid of the final map, STATEMENT G (no counterpart in the reference; the statement the tests compare against is
 * tests/ground_grid_ref.py, fp32 torch on the CPU with one eager op per rounding: the kernel matches it EXACTLY, not within a tolerance).
 * INPUTS  depth fp32 [B][1][H][W] (the map of ocv_depth_finalize_fwd); K fp32 [B][4] in DEVICE memory, as ocv_depth_unproject_fwd takes
 * it; pose fp32 [B][12] in DEVICE memory, 16-byte aligned: a row-major 3 x 4 [R | t] from the camera frame (x right, y down, z forward)
 * to the ground frame, row 0 = ground x (lateral, right), row 1 = ground y (forward), row 2 = height (up); confidence / depth_std
 * (nullable, depth's shape) with min_confidence / max_std; the stride sy, sx and near <= far; the grid x0, y0, cell (metres, x0 and y0
 * finite, cell > 0 and finite) and GX x GY cells (lateral x forward, each at most 2^24); the height band lo <= hi, both of magnitude at
 * most 1000; obstacle_height (not NaN); min_points >= 1, min_obstacle_points >= 1.
 * PER PIXEL.  A pixel is a candidate iff ocv_depth_unproject_fwd's predicate keeps it (the same rule, word for word, with its bad-camera
 * rule: csrc/keep_pixel.hpp is included by both) and all twelve pose values of its image are finite (else the image keeps nothing).  For
 * a candidate every operation is fp32 and rounded on its own, `/` the IEEE division:
 *   rx = (float(x) - cx) / fx,  ry = (float(y) - cy) / fy,  X = rx * z,  Y = ry * z,  Z = z
 *   g_i = ((p[i][0] * X + p[i][1] * Y) + p[i][2] * Z) + p[i][3]   for i = 0, 1, 2, summed left to right
 *   fxi = floorf((g_0 - x0) / cell),  fyi = floorf((g_1 - y0) / cell)
 *   in the grid iff 0 <= fxi < GX and 0 <= fyi < GY (compared as floats: NaN fails);  in the band iff lo <= g_2 <= hi.
 * A point in the grid and in the band belongs to cell (iy, ix) = (int(fyi), int(fxi)).
 * PER CELL, over its points:  count int32;  obstacle int32 = the points with g_2 > obstacle_height;  h_min, h_max fp32 = the extremes of
 * g_2 (0 where count = 0: count = 0 is the flag);  h_mean: q = (long long)rintf(g_2 * 1024.f) (exact, at most 2^20 in magnitude) summed
 * in int64, h_mean = (float)((double)sum / (1024.0 * count)), 0 where empty;  state uint8: 0 = unknown (count < min_points), 2 = occupied
 * (not unknown and obstacle >= min_obstacle_points), 1 = free otherwise.
 * PER LATERAL COLUMN:  first_occupied fp32 [B][GX] = y0 + float(iy) * cell (two fp32 roundings) of the smallest iy with state 2, +inf
 * when the column has no occupied cell.
 * OUTPUTS, each nullable, at least one given, EVERY element of a given output written:  count, obstacle int32 [B][GY][GX];  h_min, h_max,
 * h_mean fp32 [B][GY][GX];  state uint8 [B][GY][GX];  first_occupied fp32 [B][GX].
 * workspace: ocv_ground_grid_workspace_bytes(B, GX, GY) = 24 bytes per cell (0 for sizes the entry point refuses), 8-byte aligned.
 * At most three launches on the stream (csrc/ground_grid.hip): a zero fill of the per-cell records in the workspace; the accumulate pass,
 * one 256-thread workgroup per (image, tile of OCV_GROUND_GRID_TILE consecutive candidates of the strided grid), which merges its points
 * on chip (equal-cell runs of a wave by a segmented reduction, then an LDS table keyed by cell) and issues one set of global atomics per
 * distinct cell of the tile; the finalize pass with the column scan.  INTEGER atomics only (integer adds, unsigned max on the
 * order-preserving integer image of the float, a 64-bit integer add): two calls give identical bytes whatever the arrival order.  No
 * allocation, no synchronisation, nothing read on the host (capturable).  Images are independent: a batch can be filled by one call per
 * image with offset pointers.
 * -1 with a message before any launch on: a null depth / K / pose / workspace, all outputs null, non-positive sizes, H * W, B * tiles or
 * B * GX * GY at or above 2^31, GX or GY above 2^24, a stride below 1, near > far, lo > hi, a band beyond +-1000, cell <= 0 or infinite,
 * an infinite origin (or a NaN in any of these or in obstacle_height), min_points or min_obstacle_points below 1, K / pose not 16-byte
 * aligned, the workspace not 8-byte aligned, another pointer not 4-byte aligned, a workspace that is too small. */
#define OCV_GROUND_GRID_TILE 1024
size_t ocv_ground_grid_workspace_bytes(int B, int GX, int GY);
int ocv_ground_grid_fwd(const float* depth, const float* K, const float* pose, const float* confidence, const float* depth_std, int B, int H,
                        int W, int sy, int sx, float near, float far, float min_confidence, float max_std, float x0, float y0, float cell,
                        int GX, int GY, float lo, float hi, float obstacle_height, int min_points, int min_obstacle_points, int* count,
                        int* obstacle, float* h_min, float* h_max, float* h_mean, uint8_t* state, float* first_occupied, void* workspace,
                        size_t workspace_bytes, ocv_stream_t stream);
/* Obstacle list of the ground grid, STATEMENT O (no counterpart in the reference; the statement the tests compare against is
 * tests/obstacles_ref.py, a flood fill in numpy on the CPU: the kernel matches it EXACTLY, not within a tolerance).
 * INPUTS, per image:  state uint8 [B][GY][GX];  nullable count, obstacle int32 [B][GY][GX] and h_max fp32 [B][GY][GX] -- the grid's
 * outputs above, read as given;  the grid's x0, y0, cell;  link in {1, 2, 3};  min_cells >= 1;  min_obstacle_points >= 0;  cap >= 1.
 * COMPONENTS.  A cell is occupied iff state == 2.  Two different occupied cells of one image are adjacent iff |dix| <= link and
 * |diy| <= link (link = 1 is 8-connectivity; 2 or 3 bridges the one- or two-cell holes that a depth map's sparse far field leaves in a
 * wall).  A component is a class of the transitive closure of adjacency; its root is its smallest iy * GX + ix.
 * PER COMPONENT, all integer arithmetic:  n cells;  ix_min, ix_max, iy_min, iy_max;  points = the sum of count and obstacle_points = the
 * sum of obstacle, both summed in int64 and clamped to 2^31 - 1 on output, 0 when the input is null;  sum_ix, sum_iy in int64;  h_max =
 * the maximum of the cells' h_max through the order-preserving integer key of the grid's own extremes (csrc/float_key.hpp), 0 when the
 * input is null.
 * KEPT COMPONENTS.  A component is kept iff n >= min_cells and obstacle_points >= min_obstacle_points.  The kept ones are ranked by
 * root, ascending: nearest first in forward distance, ties left to right.  total[b] = the number kept, counts[b] = min(total[b], cap).
 * OUTPUTS, each nullable, at least one given, EVERY element of a given output written:
 *   cells  int32 [B][cap][8] = ix_min, ix_max, iy_min, iy_max, n, points, obstacle_points, root
 *   metres fp32  [B][cap][8] = x_min = x0 + float(ix_min) * cell,  x_max = x0 + float(ix_max + 1) * cell,  y_min, y_max likewise (two fp32
 *          roundings each, as first_occupied);  x_mean = (float)((double)x0 + ((double)sum_ix / n + 0.5) * (double)cell), one operation
 *          at a time, y_mean likewise;  h_max;  fill = (float)((double)n / ((double)(ix_max - ix_min + 1) * (double)(iy_max - iy_min + 1)))
 *   rows at or beyond counts[b] are all zero in both tables
 *   labels int32 [B][GY][GX] = -1 where the cell is not occupied, the rank k where its component is kept and k < cap, -2 otherwise
 *   counts, total int32 [B]
 * Everything is a function of the component as a set: two calls give identical bytes.
 * workspace: ocv_obstacles_workspace_bytes(B, GX, GY) = 64 bytes per cell + 4 per OCV_OBSTACLES_CHUNK cells of an image (0 for sizes the
 * entry point refuses), 8-byte aligned; every byte of it is written by every call.  Its layout, n = B * GX * GY:  int64 [n] each of
 * points, obstacle_points, sum_ix, sum_iy;  int32 [n] each of n, GX - 1 - ix_min, ix_max, GY - 1 - iy_min, iy_max;  uint32 [n] the key of
 * h_max -- these records live AT THE ROOT's cell and are zero elsewhere --;  int32 [n] parent (after the call: the root's iy * GX + ix
 * of every occupied cell, -1 elsewhere);  int32 [n] rank;  int32 [B][chunks] kept roots per chunk.
 * At most seven launches on the stream (csrc/obstacles.hip): the zero fill of the records; union-find by smaller index in LDS per tile of
 * OCV_OBSTACLES_TILE x OCV_OBSTACLES_TILE cells; the pairs across tile edges in memory (find, atomic min on the larger root, again while
 * another caller was faster; skipped for a one-tile grid); the flattening with the statistics, merged on chip per 256 cells (equal-root
 * runs of a wave by ocv_ground_grid_fwd's segmented reduction, then an LDS table keyed by root) into one set of global atomics per
 * distinct root; the kept roots per chunk; ranks, rows, tail and counts; with `labels` the relabel pass.  A parent index only ever
 * decreases, so every loop of the union-find ends by construction (csrc/union_find.hpp).  INTEGER atomics only.  No allocation, no
 * synchronisation, nothing read on the host (capturable).  Images are independent: a batch can be filled by one call per image with
 * offset pointers.
 * -1 with a message before any launch on: a null state / workspace, all outputs null, link outside 1..3, min_cells < 1,
 * min_obstacle_points < 0, cap < 1, non-positive sizes, B * GX * GY or B * cap * 8 at or above 2^31, GX or GY above 2^24, cell <= 0 or
 * infinite, an infinite origin (or a NaN in any of these), the workspace not 8-byte aligned, another pointer but state not 4-byte aligned,
 * a workspace that is too small.
 * ocv_obstacles_set_dispatch(on_chip_merge): 1 (default) as above, 0 sends every cell's statistics straight to memory -- the same bytes,
 * kept for the A/B of tools/measure_obstacles.py; -1 for another value. */
#define OCV_OBSTACLES_TILE 32
#define OCV_OBSTACLES_CHUNK 1024
size_t ocv_obstacles_workspace_bytes(int B, int GX, int GY);
int ocv_obstacles_set_dispatch(int on_chip_merge);
int ocv_obstacles_fwd(const uint8_t* state, const int* count, const int* obstacle, const float* h_max, int B, int GX, int GY, float x0,
                      float y0, float cell, int link, int min_cells, int min_obstacle_points, int cap, int* cells, float* metres,
                      int* labels, int* counts, int* total, void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* Ground memory, the occupancy grid fused over time, STATEMENT F (no counterpart in the reference; the statement the tests compare against
 * is tests/ground_memory_ref.py, numpy fp32 on the CPU with one operation per rounding: the kernel matches it EXACTLY, not within a
 * tolerance).  Per-cell evidence, carried from step to step through the vehicle's motion and updated by each step's grid.
 * INPUTS, per image b of B independent camera streams:  state uint8 [B][GY][GX], this step's grid state (0 unknown, 1 free, 2 occupied);
 * nullable h_max fp32 [B][GY][GX], this step's grid h_max;  nullable prev_evidence int16 [B][GY][GX], the evidence the previous step
 * wrote (null = all zero: the first step);  nullable prev_h fp32 [B][GY][GX], the previous step's fused h_max;  motion fp32 [B][4] =
 * (c, s, tx, ty) in DEVICE memory, 16-byte aligned: a point at p in the current ground frame was at
 * (c * p.x - s * p.y + tx,  s * p.x + c * p.y + ty) in the previous step's ground frame -- an image with any non-finite motion value
 * FORGETS: it carries nothing (that is how a stream is reset);  the grid's x0, y0, cell, GX, GY with Statement G's limits;  integers
 * free >= 0, occupied >= 0, decay >= 0, limit >= 1, free_at >= 1, occupied_at >= 1, each at most 16383.
 * PER OUTPUT CELL (iy, ix).  Every fp32 operation is rounded on its own (a product that feeds a sum too), `/` the IEEE division, sums
 * left to right:
 *   xc = x0 + (float(ix) + 0.5f) * cell          yc = y0 + (float(iy) + 0.5f) * cell
 *   px = (c * xc - s * yc) + tx                  py = (s * xc + c * yc) + ty
 *   fxi = floorf((px - x0) / cell)               fyi = floorf((py - y0) / cell)
 *   inside  = the image does not forget and 0 <= fxi < GX and 0 <= fyi < GY   (compared as floats: NaN fails)
 *   carried = inside and prev_evidence given ? prev_evidence[b][int(fyi)][int(fxi)] : 0          (the nearest cell; int32 from here on)
 *   m = |carried| - decay;   faded = m > 0 ? sign(carried) * m : 0
 *   hit = state == 2 ? +occupied : state == 1 ? -free : 0
 *   evidence = clamp(faded + hit, -limit, +limit)                                                 (stored as int16)
 *   fused state = evidence >= occupied_at ? 2 : evidence <= -free_at ? 1 : 0
 *   h = -inf;  if (h_max given and state == 2) h = h_max[b][iy][ix]
 *              if (prev_h given and inside and carried > 0 and prev_h[b][int(fyi)][int(fxi)] > h) h = that value
 *   fused h_max = (evidence > 0 and h > -inf) ? h : 0
 * PER LATERAL COLUMN:  first_occupied fp32 [B][GX] = y0 + float(iy) * cell (two fp32 roundings, Statement G's rule) of the smallest iy
 * whose FUSED state is 2, +inf when there is none.
 * OUTPUTS, each nullable, at least one given, EVERY element of a given output written:  evidence int16 [B][GY][GX];  fused state uint8
 * [B][GY][GX];  fused h_max fp32 [B][GY][GX];  first_occupied fp32 [B][GX].
 * The warp is a gather and the column scan evaluates the statement a second time, so NO OUTPUT MAY OVERLAP AN INPUT: evidence / fused
 * h_max over prev_evidence / prev_h (a ping-pong in place) is refused, and so is any other pair.
 * ONE launch on the stream (csrc/ground_fuse.hip), no workspace, no atomics: 256-thread workgroups, one per (image, tile of
 * OCV_GROUND_FUSE_TILE x OCV_GROUND_FUSE_TILE cells) -- square, so that the tile's footprint in the previous map stays compact under
 * any rotation -- and, with first_occupied, one per (image, 8 columns) for the column scan.  Two calls give identical bytes.  No
 * allocation, no synchronisation, nothing read on the host (capturable).  Images are independent: a batch can be filled by one call per
 * image with offset pointers.
 * -1 with a message before the launch on: a null state / motion, all outputs null, non-positive sizes, B * GX * GY at or above 2^31, GX
 * or GY above 2^24, cell <= 0 or infinite, an infinite origin (or a NaN in any of these), an integer outside its range, motion not
 * 16-byte aligned, an fp32 tensor not 4-byte aligned, an int16 tensor not 2-byte aligned, an output that overlaps an input. */
#define OCV_GROUND_FUSE_TILE 16
int ocv_ground_fuse_fwd(const uint8_t* state, const float* h_max, const int16_t* prev_evidence, const float* prev_h, const float* motion,
                        int B, int GX, int GY, float x0, float y0, float cell, int free, int occupied, int decay, int limit, int free_at,
                        int occupied_at, int16_t* evidence, uint8_t* fused_state, float* fused_h_max, float* first_occupied,
                        ocv_stream_t stream);
/* Ground plane of the final map, STATEMENT E (no counterpart in the reference; the statement the tests compare against is
 * tests/ground_plane_ref.py: fp32 torch on the CPU with one eager op per rounding, the solve in float64 one operation at a time.  The
 * counts, the moments and the stats match it EXACTLY; the pose within one fp32 step, equal bits expected).  It estimates, per image, the
 * camera's pose over the ground -- the [R | t] ocv_ground_grid_fwd takes -- from the map itself: a consensus over a FIXED table of
 * hypotheses (RANSAC whose table is made on the host, so nothing is random at run time), then ONE refit from integer moments.
 * INPUTS  depth fp32 [B][1][H][W];  K fp32 [B][4] in DEVICE memory, 16-byte aligned;  confidence / depth_std (nullable) with
 * min_confidence / max_std, the stride sy, sx and near <= far: the keep rule of csrc/keep_pixel.hpp, as ocv_ground_grid_fwd takes them;
 * triples int32 [T][3] in DEVICE memory, 1 <= T <= OCV_GROUND_PLANE_MAX_HYPOTHESES: each entry a pixel index y * W + x of the map, one
 * table for the whole batch;  prior fp32 [B][12] in DEVICE memory, 16-byte aligned: a ground-pose-style [R | t] whose row 2,
 * u = (prior[8], prior[9], prior[10]), is the expected up direction and which is the FALLBACK output;  tol >= 0 and rel_tol >= 0, finite;
 * h_lo <= h_hi;  cos_tilt in (0, 1];  min_cross > 0;  min_inliers >= 3.
 * Every fp32 operation below is rounded on its own (a product that feeds a sum too), `/` and sqrtf are the IEEE ones.  Back-projection is
 * Statement G's:  rx = (float(x) - cx) / fx,  ry = (float(y) - cy) / fy,  P = (rx * z, ry * z, z).
 * 1. HYPOTHESES, per (b, t).  P0, P1, P2 = the points of the triple's pixels;  a = P1 - P0,  b = P2 - P0;
 *   m = (a1 * b2 - a2 * b1,  a2 * b0 - a0 * b2,  a0 * b1 - a1 * b0);  l = sqrtf((m0 * m0 + m1 * m1) + m2 * m2);  n = m / l, negated if
 *   n1 > 0 (the camera's y points down: up has n1 < 0);  h = -((n0 * P0x + n1 * P0y) + n2 * P0z).
 *   VALID iff (NaN fails each comparison) all three indices lie in [0, H * W); all three pixels are kept by the keep rule with in = true
 *   (the stride does not apply to triples; a bad camera keeps nothing);  l >= min_cross;  (n0 * u0 + n1 * u1) + n2 * u2 >= cos_tilt;
 *   h_lo <= h <= h_hi;  the image's twelve prior values are finite.  Nothing is read through an index outside the map.
 * 2. CONSENSUS.  The candidates are the pixels of the strided grid that the keep rule keeps: exactly ocv_ground_grid_fwd's.  For a
 *   candidate (X, Y, Z):  thr = tol + rel_tol * Z;  count[b][t] int32 = the number of candidates with
 *   fabsf(((n0 * X + n1 * Y) + n2 * Z) + h) <= thr;  0 for an invalid hypothesis.
 * 3. SELECTION.  best[b] = the smallest t with the largest count; -1 if that count is below min_inliers.
 * 4. MOMENTS (best >= 0), over the candidates that are inliers of `best` by the same test and have |X|, |Y|, |Z| <= 256:
 *   q = (int)rintf(v * 128.f) per coordinate (|q| <= 2^15: products fit an int32), nine int64 sums in this order:
 *   N, Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, Szy.  The entry point refuses more than 2^22 candidates per image, so every sum stays below 2^53
 *   and converts to float64 without rounding.  All zero when best = -1.
 * 5. SOLVE, float64, every operation rounded on its own:  mx = Sx / N, my = Sy / N, mz = Sz / N;  cxx = Sxx / N - mx * mx, likewise
 *   cxz = Sxz / N - mx * mz, czz = Szz / N - mz * mz, cxy = Sxy / N - mx * my, czy = Szy / N - mz * my;  det = cxx * czz - cxz * cxz;
 *   A = (cxy * czz - czy * cxz) / det;  Bc = (czy * cxx - cxy * cxz) / det;  C = ((my - A * mx) - Bc * mz) / 128;
 *   s = sqrt((A * A + 1) + Bc * Bc);  up = (A / s, -1 / s, Bc / s);  hgt = C / s;
 *   g = (-(up2 * up0), -(up2 * up1), 1 - up2 * up2);  lf = sqrt((g0 * g0 + g1 * g1) + g2 * g2);  f = g / lf (the optical axis projected
 *   onto the plane: forward);  r = f x up = (f1 * up2 - f2 * up1,  f2 * up0 - f0 * up2,  f0 * up1 - f1 * up0) (right).
 *   ok = 1 iff best >= 0, N >= min_inliers, det > 0, h_lo <= hgt <= h_hi, (up0 * u0 + up1 * u1) + up2 * u2 >= cos_tilt (all in float64,
 *   the fp32 arguments converted), and -- so that the output is never NaN unless the prior is -- lf > 0 and the twelve values below are
 *   finite as fp32.
 * 6. OUTPUTS, EVERY element written.  pose fp32 [B][12] = [r, 0; f, 0; up, hgt], each rounded once to fp32, where ok; the twelve prior
 *   values bit for bit elsewhere.  Row 2 is the plane; rows 0 and 1 follow ground_pose's convention (objcavit_amd/ground_grid.py), so on a
 *   perfect plane the output equals ground_pose(h, pitch, roll).  stats int32 [B][4] = best, count[best] (0 if none), N, ok.
 * workspace: ocv_ground_plane_workspace_bytes(B, T) bytes (0 for sizes the entry point refuses), 16-byte aligned, EVERY byte written.
 *   With Tp = T rounded up to a multiple of OCV_GROUND_PLANE_BATCH:  fp32 [B][Tp][4] the hypotheses n0, n1, n2, h (an invalid or padding one is 0, 0, 0, NaN)
 *   at byte 0;  int64 [B][9] the moments at byte 16 * B * Tp;  int32 [B][T] the counts at byte 16 * B * Tp + 72 * B.
 * Four launches on the stream (csrc/ground_plane.hip): hypotheses (which also clears counts and moments);  consensus, one 256-thread
 * workgroup per (image, tile of OCV_GROUND_PLANE_TILE consecutive candidates of the strided grid), candidates in registers, a wave-uniform
 * loop over the hypotheses, a ballot popcount per test, counts gathered in LDS, one global integer add per (workgroup, hypothesis with a
 * non-zero count);  moments, the same tiling, which finds `best` from the T counts itself and issues nine 64-bit integer adds per
 * workgroup;  solve, one wave per image.  INTEGER atomics only: two calls give identical bytes.  No allocation, no synchronisation, nothing
 * read on the host (capturable).  Images are independent: a batch can be filled by one call per image with offset pointers.
 * -1 with a message before any launch on: a null depth / K / triples / prior / pose / stats / workspace, non-positive sizes, T outside
 * 1..1024, H * W or B * tiles at or above 2^31, more than 2^22 candidates per image, a stride below 1, near > far, tol or rel_tol negative
 * or infinite, h_lo > h_hi, cos_tilt outside (0, 1], min_cross <= 0 (or a NaN in any of these), min_inliers below 3, K / prior not 16-byte
 * aligned, the workspace not 16-byte aligned, another pointer not 4-byte aligned, a workspace that is too small. */
#define OCV_GROUND_PLANE_TILE 1024
#define OCV_GROUND_PLANE_MAX_HYPOTHESES 1024
#define OCV_GROUND_PLANE_BATCH 8 /* hypotheses per uniform load of the consensus loop: the workspace pads T to a multiple of it */
size_t ocv_ground_plane_workspace_bytes(int B, int T);
int ocv_ground_plane_fwd(const float* depth, const float* K, const int* triples, const float* prior, const float* confidence,
                         const float* depth_std, int B, int H, int W, int T, int sy, int sx, float near, float far, float min_confidence,
                         float max_std, float tol, float rel_tol, float h_lo, float h_hi, float cos_tilt, float min_cross, int min_inliers,
                         float* pose, int* stats, void* workspace, size_t workspace_bytes, ocv_stream_t stream);
/* Depth ERROR per detection box, and over objects against background: the validation metrics of ocv_depth_metrics_fwd, segmented by the
 * boxes of ocv_object_depth_fwd (no counterpart in the reference; the statement the tests compare against is tests/object_metrics_ref.py).
 * pred, pred_mirror (nullable, still mirrored), h, w, gt, H, W, min_depth, max_depth and the crop box: exactly as ocv_depth_metrics_fwd
 * takes them; the per-pixel value v (clamp that keeps NaN, un-mirrored average, bilinear align_corners taps with the identity short-cut
 * at equal sizes, nan -> min_depth, +-inf -> max_depth) and the VALID pixels (min_depth < gt <= max_depth inside the crop box) are that
 * entry point's.  xywh, xywh_row_stride, counts, cap, half: exactly as ocv_object_depth_fwd takes them, in pixels of the ground truth's
 * H x W grid; a box's pixels are that entry point's rule.  A box OWNS its pixels that are valid.
 * One record = 10 floats over a set of owned pixels:
 *   0 abs_rel  1 sq_rel  2 rmse  3 rmse_log  4 log10  5 delta1  6 delta2  7 delta3     the eight means of ocv_depth_metrics_fwd's record
 *                                                                                      (float64 sums, the two RMSEs square-rooted)
 *   8 n_valid  the number of pixels in the set (exact below 2^24)
 *   9 gt_mean  the float64 mean of gt over the set, rounded to fp32
 * All ten are 0 for an empty set: n_valid = 0 is the flag.
 * boxes_out [B][cap][10]: row r of image b = the record of box r; overlapping boxes each count their own pixels; a row at or beyond
 *   counts[b], an empty box (outside the map, of no size, non-finite, the <UNK> box -1, -1, -1, -1) and a box without a valid pixel
 *   are all zero.  Every element is written.
 * regions_out [B][2][10], or null to skip the region pass: row 0 = the record over the valid pixels under ANY of the image's first
 *   min(counts[b], cap) boxes (a pixel under several counts once), row 1 = over the valid pixels under none.  Their n_valid add up to
 *   the image's n_valid of ocv_depth_metrics_fwd exactly; the n-weighted recombination of the two rows (RMSEs through their squares) is
 *   that image's record.  The region pass takes cap <= OCV_OBJECT_METRICS_MAX_BOXES; the box pass has no such bound.
 * workspace: ocv_object_metrics_workspace_bytes (0 for sizes the entry point refuses), 8-byte aligned; read and written by the region
 * pass only (null / 0 with regions_out = null).
 * One launch of B * cap workgroups for the boxes, two for the regions ((tiles, B) partials, then B finishes); gt is read over the boxes
 * and once more over the map; no allocation, no synchronisation, counts read on the device only (capturable); sums in float64 in a fixed
 * order, the counts as integers, no float atomics: two calls give identical bytes.
 * -1 with a message before any launch on: a null required pointer, bad sizes, min_depth >= max_depth, a crop box outside the map, half
 * outside (0, 0.5], xywh_row_stride < 4, cap above the bound with regions_out given, misaligned pointers, a workspace that is too small. */
#define OCV_OBJECT_METRICS_MAX_BOXES 1024
size_t ocv_object_metrics_workspace_bytes(int B, int H, int W);
int ocv_object_metrics_fwd(const float* pred, const float* pred_mirror, int h, int w, const float* gt, int H, int W, float min_depth,
                           float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1, const float* xywh, long xywh_row_stride,
                           const int* counts, int B, int cap, float half, float* boxes_out, float* regions_out, void* workspace,
                           size_t workspace_bytes, ocv_stream_t stream);

/* Tail of mViT / ObjCAViT.forward + glue of AdaBins / GraphBins.forward in one launch (modules/miniViT.py:33-42, modules/AdaBins.py:79-83):
 *   y = raw [B][n_bins] (the regressor's last Linear) -> OCV_BINNORM_LINEAR: relu(y) + 0.1 | OCV_BINNORM_SIGMOID: sigmoid(y) |
 *   OCV_BINNORM_NONE: y (already normalised, e.g. a softmax);  widths_normed = y / sum_row(y) (NONE: y);
 *   edges [B][n_bins + 1] = cumsum([min_depth, (max_depth - min_depth) * widths_normed]);  centers [B][n_bins] = edge midpoints. */
#define OCV_BINNORM_LINEAR 0
#define OCV_BINNORM_SIGMOID 1
#define OCV_BINNORM_NONE 2
int ocv_bin_edges_fwd(const float* raw, int mode, float min_depth, float max_depth, float* widths_normed, float* edges,
                      float* centers, int B, int n_bins, ocv_stream_t stream);
/* The bin regressor and ocv_bin_edges_fwd in ONE launch (modules/miniViT.py:33-42 == modules/ObjCAViT.py:373-388): per image,
 * row x + b * x_stride (E floats: token 0) -> Linear(E, H1) + LeakyReLU(leaky_slope) -> Linear(H1, H2) + LeakyReLU -> Linear(H2, n_bins) ->
 * normalisation `mode` -> widths, edges, centres as above.  Weights row-major [out][in], 16-byte aligned; E, H1, H2 multiples of 4, <= 1024.
 * Plain fp32 FMA chains in k order (the three GEMM launches it replaces summed in MFMA order: results agree to fp32 rounding). */
int ocv_regressor_bins_fwd(const float* x, long x_stride, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* w3, const float* b3, int E, int H1, int H2, int n_bins, float leaky_slope, int mode,
                           float min_depth, float max_depth, float* widths_normed, float* edges, float* centers, int B,
                           ocv_stream_t stream);

/* Ragged object lists with the per-image COUNT in device memory (shape-static: a captured graph serves any object set up to its
 * capacity; replaces pad_sequence / F.pad / mask building of SelfAttnCrossAttn.forward, modules/ObjCAViT.py:180-183,192-194).
 *   ocv_object_tokens_pad_fwd: tokens [B][capacity][E] (rows >= counts[b] arbitrary) -> out = rows < count kept, the rest
 *     pad_value (1e-4); mask[b][j] = (j >= counts[b]).  out may alias tokens.
 *   ocv_object_front_pad_fwd: objects [B][capacity][E] -> out [B][S][E] = [ pad_value x (S - Nmax) | rows 0 .. Nmax-1 ] (rows
 *     padded at the FRONT), key_padding_mask [B][S] = (j >= counts[b]) (mask padded at the BACK).  Nmax = nmax
 *     when nmax > 0 (the global batch's longest list, data-parallel shards), else the largest count within the image's group
 *     of `group` consecutive images (one group = one call of the reference: its Nmax is that call's longest list, Q3).
 * counts[b] is read as min(max(counts[b], 1), capacity): the reference never has an image without a row (an image without
 * detections carries ONE <UNK> row, :311-315), and a count of 0 would mask every key (softmax over nothing = NaN). */
int ocv_object_tokens_pad_fwd(const float* tokens, const int* counts, float pad_value, float* out, uint8_t* mask, int B,
                              int capacity, int E, ocv_stream_t stream);
int ocv_object_front_pad_fwd(const float* objects, const int* counts, int group, int nmax, float pad_value, float* out,
                             uint8_t* key_padding_mask, int B, int capacity, int S, int E, ocv_stream_t stream);
/* Object front end: a detector's SELECTED detections -> the padded object inputs above, in one launch (what the reference does per
 * object on the host: the size relation of modules/ObjectLanguageStrategy.py:69-81, the phrase -> text feature step as a table lookup,
 * the <UNK> object of an image without detections, modules/LanguageEmbeddingWrapper.py:56-61 + modules/ObjCAViT.py:311-315).
 * Inputs, all in DEVICE memory and read by the kernel only: box r of image b = xywh[(b * cap + r) * xywh_row_stride + 0..3] (centre x,
 * centre y, width, height), cls int32 [B][cap], counts int32 [B] (read as clamp(count, 0, cap); rows at or beyond it are never read).
 * Tables, element type fp32 (f16 = 0) or fp16 (f16 = 1, widened exactly), rows of F elements, 16-byte aligned:
 *   dense mode (no hash table): class_table [n_classes][F], row = cls.
 *   hash mode (hash_keys / hash_rows / hash_features all given): key = cls << 24 | next << 3 | (rel + 1), looked up by linear probing
 *     from  splitmix64_finaliser(key) & (slots - 1)  in hash_keys uint64 [slots] (slots a power of two, an empty slot = all ones);
 *     hash_rows int32 [slots] names a row of hash_features [n_rows][F].  class_table, when given, is the FALLBACK of a miss.
 *   rel / next: with a hash table and >= 2 live rows, ratio = fp32(fp32(w * h) / fp32(w' * h')) against the NEXT live row (cyclic), both
 *     operations IEEE-rounded; rel = the number of thresholds[k] <= ratio (thresholds: HOST array of six increasing fp32 values, copied
 *     by value; the steps of the reference's log / round / clip formula), next = that row's class.  Otherwise, and for a ratio that is
 *     not a finite positive number (flag BAD_RATIO; the reference raises), rel = -1 and next = cls.
 * Outputs: B' = B images, or 2 B when mirror_width > 0: image b + B = image b with centre x -> fp32(mirror_width - cx), same order.
 *   features[bo * feat_image_stride + j * feat_row_stride + 0..F), xywh_out[bo * xywh_out_image_stride + j * xywh_out_row_stride + 0..3],
 *   j < cap: the table row (else the fallback row, else zeros) and the box unchanged for a live row; zeros for a row at or beyond the
 *   count -- except row 0 of an image whose count is 0: zero feature, box (-1, -1, -1, -1).  Rows cap .. cap_out - 1 and columns
 *   beyond the fourth are NOT touched (cap_out >= cap: the launch may write straight into larger buffers).
 *   counts_out int32 [B'] = clamp(count, 1, cap).  rows int32 [B'][cap] = the table row, -1 on a miss and beyond the count; keys uint64
 *   [B'][cap] = the key (all ones beyond the count or when a class is invalid); flags uint8 [B'][cap], an OR of OCV_OBJFE_*:
 *   MISS (no table row), BAD_CLASS (cls, or the next row's, outside [0, n_classes): no key, a miss; the fallback row of cls if cls itself
 *   is valid), BAD_RATIO, COUNT_CLAMPED (row 0 only: count > cap).
 * One launch of B' * cap workgroups, no workspace, no allocation, no synchronisation, no atomics, one writer per element: bit-equal
 * on repeat.  -1 with a message before any launch on: a null pointer, no table or half a hash table, F not a positive multiple of 4,
 * n_classes outside [1, 2^20], slots not a power of two, cap_out < cap, bad strides, bad thresholds, a bad mirror_width, misalignment. */
#define OCV_OBJFE_MISS 1
#define OCV_OBJFE_BAD_CLASS 2
#define OCV_OBJFE_BAD_RATIO 4
#define OCV_OBJFE_COUNT_CLAMPED 8
int ocv_object_frontend_fwd(const float* xywh, long xywh_row_stride, const int* cls, const int* counts, int B, int cap,
                            const void* class_table, int n_classes, const uint64_t* hash_keys, const int* hash_rows, int slots,
                            const void* hash_features, int n_rows, const float* thresholds, int f16, int F, float mirror_width,
                            float* features, long feat_image_stride, long feat_row_stride, float* xywh_out, long xywh_out_image_stride,
                            long xywh_out_row_stride, int* counts_out, int cap_out, int* rows, uint64_t* keys, uint8_t* flags,
                            ocv_stream_t stream);

/* Positional-embedding samplers of GridRandomPositionalEmbeddings.forward (modules/ObjCAViT.py:50-147) on the learnable
 * table `table` [>= gh*gw][E], viewed as a gh x gw grid of E-vectors (row y*gw + x; reference :82-83).  One output row
 * per coordinate row: out[r][0..E) = sample (+ addend[r][0..E) when addend is not NULL -- the object embedding it is
 * added to at :330).  coords [n_rows][coord_ld] fp32.
 *   OCV_POS_CENTRE_OBJ  coords = (x, y, ...) in full-resolution pixels; F.grid_sample(bilinear, zeros,
 *                       align_corners=False) at (x / p0 * 2 - 1, y / p1 * 2 - 1); the reference passes
 *                       p0 = image HEIGHT, p1 = image WIDTH (:104-105).                       (:102-110)
 *   OCV_POS_CENTRE_IMG  coords = (x, y, ...) of the image tokens, rows_per_image = S rows per image; row s = r % S:
 *                       s == 0 -> both components / p0 * 2 - 1 (p0 = gh), s == 1 -> both / p1 * 2 - 1 (p1 = gw),
 *                       s >= 2 -> raw coordinates (the reference indexes dim 1 of a B x S x 2 tensor; Q6).   (:93-100)
 *   OCV_POS_ROI         coords = (cx, cy, w, h): x1y1x2y2 = centre -+ half size clamped at 0 from below, then
 *                       torchvision.ops.ps_roi_align(output_size=[1,1], spatial_scale=p0, sampling_ratio=-1):
 *                       corners * p0 - 0.5, ceil(roi_h) x ceil(roi_w) bilinear samples averaged (samples outside
 *                       [-1, gh] x [-1, gw] count as 0; a box without extent gives 0/0 = NaN).            (:111-145)
 * The sample loops are bounded by the grid size whatever the box; no host synchronisation (hipGraph-capturable). */
#define OCV_POS_CENTRE_OBJ 0
#define OCV_POS_CENTRE_IMG 1
#define OCV_POS_ROI 2
int ocv_pos_grid_sample_fwd(const float* table, int gh, int gw, int E, const float* coords, int coord_ld, int n_rows,
                            int mode, float p0, float p1, int rows_per_image, const float* addend, float* out,
                            ocv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OBJCAVIT_HIP_H */
