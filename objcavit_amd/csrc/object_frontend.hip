// Object front end on the device (row N4 of SURVEY.md section 8f): selected detections -> the padded object inputs
// of ObjCAViT, one launch.  What objects.TableObjectProvider + PaddedObjects.from_lists do per object on the host -- the size relation
// of modules/ObjectLanguageStrategy.py:69-81, the phrase cache lookup, the gather of the 512-d text feature, the padding, the <UNK>
// object of an image without detections (modules/LanguageEmbeddingWrapper.py:56-61, modules/ObjCAViT.py:311-315) -- from tensors a
// detector already holds on the device:
//   xywh [B][cap][>= 4], cls int32 [B][cap], counts int32 [B]
//   -> features [B'][cap_out][F], xywh [B'][cap_out][>= 4], counts [B'], and per input row its table row (-1 = miss), key and flags
//
// One workgroup of 128 threads per output row (image, j).  Everything in front of the copy -- the count, the two areas, their ratio,
// the relation, the key and the probe of the hash table -- depends on blockIdx and on loads from workgroup-uniform addresses only:
// every lane does it redundantly (the compiler keeps it on the scalar unit where it can), so there is no LDS and no barrier.  Then
// the row is copied, one float4 store per thread and trip (F = 512: one trip).  No atomics, one writer per output element: two calls
// are bit-equal.
//
// The relation is a non-decreasing step function of the fp32 ratio of the two box areas; the host has located its six steps as fp32
// values (objects.relative_size_thresholds: bisection over bit patterns on the reference's own formula), so the device compares and
// counts -- no logarithm here.  The product and the quotient are the IEEE-rounded fp32 operations the reference performs on 0-d
// tensors (__fmul_rn / __fdiv_rn: never contracted, never approximated).
#include "common.hpp"
#include "../../include/objcavit_hip.h"

namespace {

constexpr int OF_THREADS = 128;
constexpr unsigned long long OF_EMPTY = ~0ull;

struct ObjFrontArgs {
  const float* xywh;
  const int *cls, *counts;
  const void *class_table, *hash_features;
  const unsigned long long* hash_keys;
  const int* hash_rows;
  float *features, *xywh_out;
  int *counts_out, *rows;
  unsigned long long* keys;
  uint8_t* flags;
  long xywh_row_stride, feat_image_stride, feat_row_stride, xywh_out_image_stride, xywh_out_row_stride;
  int B, cap, n_classes, slots, n_rows, F4;
  float mirror_width;
  float thr[6];
};

// the finaliser of splitmix64: the home slot of a key is its low bits
__device__ __forceinline__ unsigned long long of_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

template <typename T>
__device__ __forceinline__ float4 of_load4(const T* row, int i);
template <>
__device__ __forceinline__ float4 of_load4<float>(const float* row, int i) { return ld4(row + 4 * i); }
template <>
__device__ __forceinline__ float4 of_load4<_Float16>(const _Float16* row, int i) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4 v = *reinterpret_cast<const h4*>(row + 4 * i);                    // (8-byte aligned: F % 4 == 0, table 16-byte aligned)
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);    // fp16 -> fp32 is exact
}

template <typename T>
__global__ __launch_bounds__(OF_THREADS) void object_frontend_kernel(ObjFrontArgs p) {
  const int tid = threadIdx.x;
  const int bo = blockIdx.x / p.cap, j = blockIdx.x - bo * p.cap;             // output image, row
  const bool mirrored = bo >= p.B;
  const int b = mirrored ? bo - p.B : bo;
  const int count = p.counts[b];
  const int n = min(max(count, 0), p.cap);                                   // live input rows of the image
  const long in_row = (long)b * p.cap + j, side_row = (long)bo * p.cap + j;
  float* fout = p.features + bo * p.feat_image_stride + j * p.feat_row_stride;
  float* bout = p.xywh_out + bo * p.xywh_out_image_stride + j * p.xywh_out_row_stride;

  const T* src = nullptr;                                                    // the feature row; null = zeros
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  int row = -1;
  unsigned long long key = OF_EMPTY;
  unsigned flag = 0;

  if (j < n) {
    const float* bx = p.xywh + in_row * p.xywh_row_stride;
    box = make_float4(bx[0], bx[1], bx[2], bx[3]);
    const int c = p.cls[in_row];
    const bool valid = c >= 0 && c < p.n_classes;
    int rel = -1, next = c;
    const bool hashed = p.hash_keys != nullptr;
    if (hashed && n >= 2) {
      const int jn = j + 1 == n ? 0 : j + 1;
      const float* nx = p.xywh + ((long)b * p.cap + jn) * p.xywh_row_stride;
      const float ratio = __fdiv_rn(__fmul_rn(box.z, box.w), __fmul_rn(nx[2], nx[3]));
      if (ratio > 0.f && ratio < __uint_as_float(0x7f800000u)) {             // the reference raises on anything else (NaN fails both)
        rel = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) rel += ratio >= p.thr[k] ? 1 : 0;
        next = p.cls[(long)b * p.cap + jn];
      } else {
        flag |= OCV_OBJFE_BAD_RATIO;
      }
    }
    const bool next_valid = next >= 0 && next < p.n_classes;
    if (!(valid && next_valid)) flag |= OCV_OBJFE_BAD_CLASS;
    else key = ((unsigned long long)c << 24) | ((unsigned long long)next << 3) | (unsigned long long)(rel + 1);

    if (!hashed) {
      row = valid ? c : -1;
      if (valid) src = (const T*)p.class_table + (long)c * p.F4 * 4;
    } else {
      if (key != OF_EMPTY) {
        const unsigned mask = (unsigned)p.slots - 1u;
        unsigned h = (unsigned)of_mix(key) & mask;
        for (int probe = 0; probe < p.slots; ++probe) {                      // (a table built by the host always has an empty slot)
          const unsigned long long k = p.hash_keys[h];
          if (k == key) { row = p.hash_rows[h]; break; }
          if (k == OF_EMPTY) break;
          h = (h + 1u) & mask;
        }
        if (row < 0 || row >= p.n_rows) row = -1;                            // a row the table does not have is a miss, never an address
      }
      if (row >= 0) src = (const T*)p.hash_features + (long)row * p.F4 * 4;
      else if (valid && p.class_table != nullptr) src = (const T*)p.class_table + (long)c * p.F4 * 4;      // the fallback
    }
    if (row < 0) flag |= OCV_OBJFE_MISS;
    if (mirrored) box.x = __fsub_rn(p.mirror_width, box.x);
  } else if (j == 0) {
    box = make_float4(-1.f, -1.f, -1.f, -1.f);                               // no detections: the <UNK> object, zero feature, this box
  }
  if (j == 0 && count > p.cap) flag |= OCV_OBJFE_COUNT_CLAMPED;

  for (int i = tid; i < p.F4; i += OF_THREADS)
    *reinterpret_cast<float4*>(fout + 4 * i) = src != nullptr ? of_load4<T>(src, i) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid == 0) {
    bout[0] = box.x; bout[1] = box.y; bout[2] = box.z; bout[3] = box.w;
    p.rows[side_row] = row;
    p.keys[side_row] = key;
    p.flags[side_row] = (uint8_t)flag;
    if (j == 0) p.counts_out[bo] = max(n, 1);
  }
}

}  // namespace

extern "C" int ocv_object_frontend_fwd(const float* xywh, long xywh_row_stride, const int* cls, const int* counts, int B, int cap,
                                       const void* class_table, int n_classes, const uint64_t* hash_keys, const int* hash_rows, int slots,
                                       const void* hash_features, int n_rows, const float* thresholds, int f16, int F, float mirror_width,
                                       float* features, long feat_image_stride, long feat_row_stride, float* xywh_out,
                                       long xywh_out_image_stride, long xywh_out_row_stride, int* counts_out, int cap_out, int* rows,
                                       uint64_t* keys, uint8_t* flags, ocv_stream_t stream) {
  OCV_CHECK_ARG(xywh && cls && counts, "ocv_object_frontend_fwd: null pointer (xywh, cls, counts)");
  OCV_CHECK_ARG(features && xywh_out && counts_out && rows && keys && flags,
                "ocv_object_frontend_fwd: null pointer (features, xywh_out, counts_out, rows, keys, flags)");
  const bool hashed = hash_keys || hash_rows || hash_features;
  OCV_CHECK_ARG(hashed || class_table, "ocv_object_frontend_fwd: no table (give class_table, or hash_keys / hash_rows / hash_features)");
  OCV_CHECK_ARG(!hashed || (hash_keys && hash_rows && hash_features && thresholds),
                "ocv_object_frontend_fwd: null pointer (a hash table needs hash_keys, hash_rows, hash_features and thresholds)");
  OCV_CHECK_ARG(B >= 1 && cap >= 1 && (long)2 * B * cap <= 0x7fffffffL, "ocv_object_frontend_fwd: bad sizes (B, cap >= 1, 2 * B * cap below 2^31)");
  OCV_CHECK_ARG(F >= 4 && F % 4 == 0, "ocv_object_frontend_fwd: F = %d must be a positive multiple of 4", F);
  OCV_CHECK_ARG(n_classes >= 1 && n_classes <= (1 << 20), "ocv_object_frontend_fwd: n_classes = %d outside [1, 2^20]", n_classes);
  OCV_CHECK_ARG(cap_out >= cap, "ocv_object_frontend_fwd: cap_out = %d is smaller than cap = %d", cap_out, cap);
  OCV_CHECK_ARG(xywh_row_stride >= 4 && xywh_out_row_stride >= 4 && xywh_out_image_stride >= (long)cap_out * xywh_out_row_stride,
                "ocv_object_frontend_fwd: bad box strides (rows >= 4 floats, an output image >= cap_out rows)");
  OCV_CHECK_ARG(feat_row_stride >= F && feat_row_stride % 4 == 0 && feat_image_stride >= (long)cap_out * feat_row_stride &&
                feat_image_stride % 4 == 0,
                "ocv_object_frontend_fwd: bad feature strides (rows >= F, an image >= cap_out rows, both multiples of 4 floats)");
  OCV_CHECK_ARG(mirror_width >= 0.f && mirror_width <= 3.0e38f, "ocv_object_frontend_fwd: mirror_width must be finite and >= 0 (0 = no mirrored half)");
  if (hashed) {
    OCV_CHECK_ARG(slots >= 2 && (slots & (slots - 1)) == 0, "ocv_object_frontend_fwd: slots = %d must be a power of two (>= 2)", slots);
    OCV_CHECK_ARG(n_rows >= 1, "ocv_object_frontend_fwd: n_rows = %d feature rows behind the hash table (>= 1)", n_rows);
    OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(hash_keys) & 7) == 0 && (reinterpret_cast<uintptr_t>(hash_rows) & 3) == 0,
                  "ocv_object_frontend_fwd: misaligned pointer (hash_keys, hash_rows)");
    for (int k = 0; k < 6; ++k)
      OCV_CHECK_ARG(thresholds[k] > (k ? thresholds[k - 1] : 0.f) && thresholds[k] <= 3.0e38f,
                    "ocv_object_frontend_fwd: thresholds must be six finite, positive, strictly increasing values (threshold %d)", k);
  }
  OCV_CHECK_ARG(ocv_aligned16(features) && ocv_aligned16(class_table) && ocv_aligned16(hash_features),
                "ocv_object_frontend_fwd: features / class_table / hash_features must be 16-byte aligned");
  OCV_CHECK_ARG((reinterpret_cast<uintptr_t>(xywh) & 3) == 0 && (reinterpret_cast<uintptr_t>(xywh_out) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(cls) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(counts_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(rows) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(keys) & 7) == 0,
                "ocv_object_frontend_fwd: misaligned pointer (xywh, xywh_out, cls, counts, counts_out, rows, keys)");
  ObjFrontArgs a{};
  a.xywh = xywh; a.cls = cls; a.counts = counts;
  a.class_table = class_table;
  a.hash_features = hashed ? hash_features : nullptr;
  a.hash_keys = hashed ? reinterpret_cast<const unsigned long long*>(hash_keys) : nullptr;
  a.hash_rows = hashed ? hash_rows : nullptr;
  a.features = features; a.xywh_out = xywh_out; a.counts_out = counts_out; a.rows = rows;
  a.keys = reinterpret_cast<unsigned long long*>(keys); a.flags = flags;
  a.xywh_row_stride = xywh_row_stride; a.feat_image_stride = feat_image_stride; a.feat_row_stride = feat_row_stride;
  a.xywh_out_image_stride = xywh_out_image_stride; a.xywh_out_row_stride = xywh_out_row_stride;
  a.B = B; a.cap = cap; a.n_classes = n_classes; a.slots = hashed ? slots : 0; a.n_rows = hashed ? n_rows : 0; a.F4 = F / 4;
  a.mirror_width = mirror_width;
  for (int k = 0; k < 6; ++k) a.thr[k] = hashed ? thresholds[k] : 0.f;
  const unsigned grid = (unsigned)((mirror_width > 0.f ? 2 : 1) * B * cap);
  if (f16) hipLaunchKernelGGL(object_frontend_kernel<_Float16>, dim3(grid), dim3(OF_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(object_frontend_kernel<float>, dim3(grid), dim3(OF_THREADS), 0, (hipStream_t)stream, a);
  OCV_CHECK_LAUNCH("ocv_object_frontend_fwd");
  return 0;
}
