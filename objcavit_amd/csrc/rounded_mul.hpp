// A product rounded ON ITS OWN even where it feeds a sum: what the statements that are matched bit for bit (Statement G, csrc/ground_grid.hip;
// Statement E, csrc/ground_plane.hip) mean by "every operation rounded on its own".  One definition, included by both, so the two cannot
// drift apart.  The library is built with -ffp-contract=fast, under which the backend fuses any product with the sum it feeds, whatever the
// source says (__fmul_rn(a, b) is `a * b` to the compiler, a contraction pragma is not consulted): one rounding where the statements have
// two.  The empty asm makes the product a value the compiler cannot look through; it emits no instruction.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float gg_mul(float a, float b) {
  float v = __fmul_rn(a, b);
  asm("" : "+v"(v));
  return v;
}

// the packed twin: a scalar times two values at once (one v_pk_mul_f32: two IEEE products)
typedef float gg_float2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ gg_float2 gg_mul2(float a, gg_float2 b) {
  gg_float2 v = a * b;
  asm("" : "+v"(v));
  return v;
}

// the float64 twin (a register pair)
__device__ __forceinline__ double gg_mul64(double a, double b) {
  double v = __dmul_rn(a, b);
  asm("" : "+v"(v));
  return v;
}
