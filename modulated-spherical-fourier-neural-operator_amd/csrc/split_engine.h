// The split-precision MFMA engines: fp32 GEMMs on the 16-bit matrix cores of gfx950.
// This header is the one statement of the two formats, the product order and the
// error bound; every x6 / x3h kernel takes its split, fragments and product from here.
//
// x6 (NP = 3): v = t0 + t1 + t2 exactly, three bf16 terms (bf16x3.h: t0 = bf16(v),
//   t1 = bf16(v - t0), t2 = bf16(v - t0 - t1); RNE, exact residuals, 3 x 8 = 24 bits).
//   a·b = a2·b0 + a1·b1 + a0·b2 + a1·b0 + a0·b1 + a0·b0: the six products whose term
//   orders add to <= 2, smallest first.  The dropped ones are below 2^-24 relative.
// x3h (NP = 2): v ~= h0 + h1, two fp16 terms (h0 = fp16(v), h1 = fp16(v - h0); RNE,
//   |v - h0 - h1| <= 2^-22 |v| while v and h1 stay in fp16's normal range).
//   a·b ~= a1·b0 + a0·b1 + a0·b0, smallest first; a1·b1 and the residuals are O(2^-22).
//   fp16 holds |v| < 65504, so every operand is first scaled by an exact power of two
//   taken from a bound (row_scale, pow2_below): largest entry in [2^14, 2^15) or below
//   2^14, undone in fp32 after the contraction.
// Products of 16-bit terms are exact in fp32 and the MFMAs accumulate in fp32, so the
// only error beyond an fp32 GEMM's own accumulation rounding is the representation
// term above.  The derivation, the range argument and the measurements are at the top
// of mlp_fused_h.hip (x3h) and gemm_x6.hip (x6); tests/test_gpu_x3h.py and
// tests/test_gpu_gemm_x6.py hold both against fp64.
#pragma once
#include "bf16x3.h"

namespace msfno {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));  // ds_read_b64_tr_b16 result
typedef short s16x8 __attribute__((ext_vector_type(8)));

// (a, b) -> packed fp16x2 terms h0 + h1 (RNE; v_cvt_pk_f16_f32)
__device__ __forceinline__ void split2h(float a, float b, uint32_t& t0, uint32_t& t1) {
  const f32x2 v = {a, b};
  const half2v h0 = __builtin_convertvector(v, half2v);
  const f32x2 r = v - __builtin_convertvector(h0, f32x2);
  const half2v h1 = __builtin_convertvector(r, half2v);
  t0 = __builtin_bit_cast(uint32_t, h0);
  t1 = __builtin_bit_cast(uint32_t, h1);
}

// four packed pairs -> one term of an MFMA A / B operand (8 k per lane): half8 or bf16x8
template <class Frag>
__device__ __forceinline__ Frag frag_cast(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(Frag, make_uint4(a, b, c, d));
}

// NP terms per value: 3 = x6, 2 = x3h.  frag: the operand term type; split: (a, b) -> NP
// packed pairs; mma: c += a·b in the order above, c's type choosing the MFMA shape
// (floatx16: 32x32x16, floatx4: 16x16x32)
template <int NP>
struct SplitEng;
template <>
struct SplitEng<3> {
  typedef bf16x8 frag;
  __device__ __forceinline__ static void split(float a, float b, uint32_t (&t)[3]) {
    split2(a, b, t[0], t[1], t[2]);
  }
  __device__ __forceinline__ static void mma(const frag (&a)[3], const frag (&b)[3], floatx16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
  }
  __device__ __forceinline__ static void mma(const frag (&a)[3], const frag (&b)[3], floatx4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
  }
};
template <>
struct SplitEng<2> {
  typedef half8 frag;
  __device__ __forceinline__ static void split(float a, float b, uint32_t (&t)[2]) {
    split2h(a, b, t[0], t[1]);
  }
  __device__ __forceinline__ static void mma(const frag (&a)[2], const frag (&b)[2], floatx16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], c, 0, 0, 0);
  }
  __device__ __forceinline__ static void mma(const frag (&a)[2], const frag (&b)[2], floatx4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[0], c, 0, 0, 0);
  }
};

// 2^(t - e) for m = f 2^e, f in [0.5, 1): the largest of a row whose maximum is m lands
// in [2^(t-1), 2^t); 1 for m = 0 / non-finite
__device__ __forceinline__ float row_scale(float m, int t) {
  float sc = 1.f;
  if (m > 0.f && isfinite(m)) {
    int e;
    frexpf(m, &e);
    sc = ldexpf(1.f, t - e);
  }
  return sc;
}

// the same with the exponent clamped to +-clamp (run-time data: the scale and its
// inverse both stay normal fp32)
__device__ __forceinline__ float pow2_below(float v, int t, int clamp) {
  if (!(v > 0.f) || !isfinite(v)) return 1.f;
  int e;
  frexpf(v, &e);
  return ldexpf(1.f, min(max(t - e, -clamp), clamp));
}

}  // namespace msfno
