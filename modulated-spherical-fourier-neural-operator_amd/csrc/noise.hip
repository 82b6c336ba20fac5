// Spherical Gaussian random fields: spectral coefficients of white or red-in-time noise,
// written in the layout msfno_sht_inverse reads (msfno_amd/harmonics/random_fields.py).
//
//   out[i][l][m] = a prev[i][l][m] + b sqrt_eig[(field0 + i) % K][l] xi(seed, draw, field0 + i, l, m)
//
// The stream is a function of (seed, draw, field, l, m) alone, so a result
// does not depend on the grid, the block size or how the fields are split over calls:
//   Philox4x32-10, key (seed lo, seed hi), counter (l P + p, field, draw lo, draw hi),
//   P = ceil(mmax / 2), p = m / 2; words (w0, w1) serve m = 2p, (w2, w3) serve m = 2p + 1;
//   u = ((w >> 9) + 0.5) 2^-23 (exact in fp32, inside (0, 1));
//   r = sqrt(-2 ln u_a), z0 = r cos(2 pi u_b), z1 = r sin(2 pi u_b);
//   m = 0: xi = (z0, 0); 1 <= m <= l: xi = (z0, z1) / sqrt(2); m > l: xi = 0.
// The angle is formed as sincospi(2 u_b): 2 u_b is exact, so no rounding of 2 pi u enters.
// Above the diagonal (m > l) the output is written as exact zeros whatever prev holds there.
//
// One thread per Philox block = two neighbouring coefficients of a row: one 16-byte store
// (and load of prev) where both lie in the row and on the 16-byte grid, 8-byte accesses
// otherwise (an odd mmax alternates the phase by row; an offset view shifts it as a whole).
// The work per stored byte is VALU: ten Philox rounds (four 32-bit multiplies each), a log,
// a square root and a sincospi per coefficient; a block that lies wholly above the diagonal
// stores its zeros without any of it (half of the blocks at mmax = lmax).  256 lanes per workgroup on a capped grid
// with a grid stride, 64-bit element offsets.  No atomics, no workspace, nothing allocated
// or synchronised: both launches record into a graph, and the draw can come from device
// memory so that a replay sees the value the previous replay left.
#include "kernels.h"

namespace msfno {

namespace {
constexpr int kNoiseThreads = 256;
constexpr int kNoiseGridCap = 2048;  // 8 workgroups per CU

struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                 uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float unit_open(uint32_t w) {
  return ((float)(w >> 9) + 0.5f) * 0x1p-23f;
}

// xi(l, m) of the word pair (wa, wb)
__device__ __forceinline__ float2 noise_xi(uint32_t wa, uint32_t wb, uint32_t l, uint32_t m) {
  const float r = sqrtf(-2.f * logf(unit_open(wa)));
  float sn, cs;
  sincospif(2.f * unit_open(wb), &sn, &cs);
  if (m == 0) return make_float2(r * cs, 0.f);
  if (m > l) return make_float2(0.f, 0.f);
  const float h = r * 0.70710678118654752440f;
  return make_float2(h * cs, h * sn);
}

__device__ __forceinline__ float2 noise_mix(float2 prev, float2 xi, float a, float s,
                                            bool inside) {
  return inside ? make_float2(fmaf(a, prev.x, s * xi.x), fmaf(a, prev.y, s * xi.y))
                : make_float2(0.f, 0.f);
}
struct NoiseArgs {
  float2* out;
  const float2* prev;  // null, or as out (may be out itself: a lane reads what it writes)
  const float* sqrt_eig;
  uint32_t K, lmax, mmax, P;
  int64_t field0;
  float a, b;
  uint32_t k0, k1, d0, d1;
};

// Philox block c0 = l P + p of local field i: the coefficients m = 2p and 2p + 1 of row l
__device__ __forceinline__ void noise_block(const NoiseArgs& g, int64_t i, uint32_t c0) {
  const uint32_t l = c0 / g.P, p = c0 - l * g.P;
  const uint32_t m0 = 2 * p, m1 = m0 + 1;
  const int64_t e = (i * g.lmax + l) * (int64_t)g.mmax + m0;
  float2* out = g.out + e;
  const float2* prev = g.prev ? g.prev + e : nullptr;
  const bool two = m1 < g.mmax;
  const bool vec = two && ((reinterpret_cast<uintptr_t>(out) |
                            reinterpret_cast<uintptr_t>(prev)) & 15) == 0;
  if (m0 > l) {  // a block above the diagonal: zeros whatever prev holds, no Philox
    if (vec) {
      *reinterpret_cast<float4*>(out) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      out[0] = make_float2(0.f, 0.f);
      if (two) out[1] = make_float2(0.f, 0.f);
    }
    return;
  }
  const uint64_t f = (uint64_t)(g.field0 + i);  // < 2^32
  const Philox4 x = philox4x32_10(c0, (uint32_t)f, g.d0, g.d1, g.k0, g.k1);
  const float s = g.b * g.sqrt_eig[(int64_t)((uint32_t)f % g.K) * g.lmax + l];
  const float2 xi0 = noise_xi(x.w[0], x.w[1], l, m0);
  if (!two) {
    out[0] = noise_mix(prev ? prev[0] : make_float2(0.f, 0.f), xi0, g.a, s, true);
    return;
  }
  const float2 xi1 = noise_xi(x.w[2], x.w[3], l, m1);
  float2 p0 = make_float2(0.f, 0.f), p1 = p0;
  if (prev) {
    if (vec) {
      const float4 q = *reinterpret_cast<const float4*>(prev);
      p0 = make_float2(q.x, q.y);
      p1 = make_float2(q.z, q.w);
    } else {
      p0 = prev[0];
      p1 = prev[1];
    }
  }
  const float2 o0 = noise_mix(p0, xi0, g.a, s, true);
  const float2 o1 = noise_mix(p1, xi1, g.a, s, m1 <= l);
  if (vec) {
    *reinterpret_cast<float4*>(out) = make_float4(o0.x, o0.y, o1.x, o1.y);
  } else {
    out[0] = o0;
    out[1] = o1;
  }
}
}  // namespace

__global__ __launch_bounds__(kNoiseThreads) void noise_spectral_kernel(
    float2* out, const float2* prev, const float* __restrict__ sqrt_eig, int K,
    int64_t n, int64_t field0, uint32_t lmax, uint32_t mmax, uint32_t P, float a, float b,
    uint64_t seed, uint64_t draw, const uint64_t* __restrict__ draw_dev) {
  if (draw_dev) draw = *draw_dev;
  const NoiseArgs g{out, prev, sqrt_eig, (uint32_t)K, lmax, mmax, P, field0, a, b,
                    (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw,
                    (uint32_t)(draw >> 32)};
  const uint64_t per_field = (uint64_t)lmax * P;  // < 2^32
  const uint64_t total = (uint64_t)n * per_field;
  // the grid stride as (fields, blocks of a field): one 64-bit division per lane, then the
  // (field, block) pair advances by additions
  const uint64_t stride = (uint64_t)gridDim.x * kNoiseThreads;
  const uint64_t stride_i = stride / per_field, stride_c = stride - stride_i * per_field;
  uint64_t t = (uint64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
  uint64_t i = t / per_field, c = t - i * per_field;
  for (; t < total; t += stride) {
    noise_block(g, (int64_t)i, (uint32_t)c);
    i += stride_i;
    c += stride_c;  // < 2^33
    if (c >= per_field) {
      c -= per_field;
      ++i;
    }
  }
}

__global__ void noise_advance_kernel(uint64_t* draw_dev, uint64_t by) {
  if (blockIdx.x == 0 && threadIdx.x == 0) draw_dev[0] = draw_dev[0] + by;
}

int launch_noise_spectral(float* coeffs, const float* prev, const float* sqrt_eig, int K,
                          int64_t n, int64_t field0, int lmax, int mmax, float a, float b,
                          uint64_t seed, uint64_t draw, const uint64_t* draw_dev,
                          hipStream_t s) {
  const uint32_t P = ((uint32_t)mmax + 1) / 2;
  const int64_t total = n * (int64_t)lmax * P;
  const int blocks = (int)std::min<int64_t>(cdiv(total, kNoiseThreads), kNoiseGridCap);
  hipLaunchKernelGGL(noise_spectral_kernel, dim3(blocks), dim3(kNoiseThreads), 0, s,
                     reinterpret_cast<float2*>(coeffs), reinterpret_cast<const float2*>(prev),
                     sqrt_eig, K, n, field0, (uint32_t)lmax, (uint32_t)mmax, P,
                     prev ? a : 0.f, b, seed, draw, draw_dev);
  return launch_check("noise_spectral");
}

int launch_noise_advance(uint64_t* draw_dev, uint64_t by, hipStream_t s) {
  hipLaunchKernelGGL(noise_advance_kernel, dim3(1), dim3(64), 0, s, draw_dev, by);
  return launch_check("noise_advance");
}

}  // namespace msfno
