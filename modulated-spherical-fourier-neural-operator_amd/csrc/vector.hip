// The streaming kernels between the scalar Legendre stages of the vector spherical
// harmonic transforms (msfno_vsht_forward / msfno_vsht_inverse, api.cpp).  A vector
// transform is two scalar transforms per direction: plan_d, whose table is D = dP̄/dθ moved
// up one degree (coefficient index l + 1, lmax + 1 degrees: the shift gives D the parity the
// hemisphere-folded Legendre kernels need), and plan_q with Q = m P̄ / sin θ.
//
//   combine (analysis):   s[l][m] = A_θ[l+1][m] - i B_φ[l][m]
//                         t[l][m] = A_φ[l+1][m] + i B_θ[l][m]      A, B: plan_d's, plan_q's output
//                         and exact zeros where l < m or l = 0, whatever A and B hold there
//   pack (synthesis):     plan_d's input  (s, t) at l + 1, row 0 zero
//                         plan_q's input  (-i t, i s)              zeros where l < m
//   add (synthesis):      v += plan_q's fields (plan_d's are written to v)
//
// All three are HBM streams built like spectrum.hip.  A (b, component) slab of lmax * mmax
// complex numbers is contiguous in every buffer (in plan_d's it starts one row, mmax
// numbers, into the slab), so a slab is a flat run and a lane handles two neighbouring
// complex numbers: 16 bytes, consecutive lanes on consecutive addresses.  A complex tensor
// is on the 8-byte grid only, and with mmax odd the slabs of one buffer alternate between
// the two 16-byte phases; a run that starts off the 16-byte grid is moved as 8-byte halves
// (still consecutive).  One writer per output word, no atomics, no workspace.
#include "kernels.h"

namespace msfno {

namespace {
constexpr int kVecThreads = 256;
constexpr int kVecGridCap = 2048;  // 8 workgroups per CU

__device__ __forceinline__ bool on16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// two neighbouring complex numbers at p; al: p is on the 16-byte grid
__device__ __forceinline__ float4 load2(const float2* p, bool al) {
  if (al) return *reinterpret_cast<const float4*>(p);
  const float2 a = p[0], b = p[1];
  return make_float4(a.x, a.y, b.x, b.y);
}

__device__ __forceinline__ void store2(float2* p, bool al, float4 v) {
  if (al) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = make_float2(v.x, v.y);
    p[1] = make_float2(v.z, v.w);
  }
}

// keep[j] = 1 where element e + j of a slab, (l, m) = ((e + j) / mmax, (e + j) % mmax),
// is a coefficient: l >= m, and l >= lmin (1: the vector transform has no degree 0)
__device__ __forceinline__ void coeff_mask(int64_t e, int mmax, int lmin, float& k0, float& k1) {
  const int l = (int)(e / mmax), m = (int)(e % mmax);
  k0 = (l >= m && l >= lmin) ? 1.f : 0.f;
  const int l1 = m + 1 == mmax ? l + 1 : l, m1 = m + 1 == mmax ? 0 : m + 1;
  k1 = (l1 >= m1 && l1 >= lmin) ? 1.f : 0.f;
}

__device__ __forceinline__ float pick(float keep, float v) { return keep != 0.f ? v : 0.f; }
}  // namespace

// grid: x over pairs of a slab, y over the bc batch entries
__global__ __launch_bounds__(kVecThreads) void vsht_combine_kernel(
    const float2* __restrict__ A, const float2* __restrict__ B, float2* __restrict__ st, int bc,
    int lmax, int mmax) {
  const int64_t n = (int64_t)lmax * mmax, nd = n + mmax;
  const int64_t pairs = (n + 1) >> 1;
  for (int b = blockIdx.y; b < bc; b += gridDim.y) {
    const float2* a0 = A + (2LL * b) * nd + mmax;  // A_θ at degree l + 1
    const float2* a1 = a0 + nd;                     // A_φ
    const float2* b0 = B + (2LL * b) * n;           // B_θ
    const float2* b1 = b0 + n;                      // B_φ
    float2* s = st + (2LL * b) * n;
    float2* t = s + n;
    const bool la0 = on16(a0), la1 = on16(a1), lb0 = on16(b0), lb1 = on16(b1);
    const bool ls = on16(s), lt = on16(t);
    for (int64_t i = blockIdx.x * (int64_t)kVecThreads + threadIdx.x; i < pairs;
         i += (int64_t)gridDim.x * kVecThreads) {
      const int64_t e = 2 * i;
      float k0, k1;
      coeff_mask(e, mmax, 1, k0, k1);
      if (e + 1 < n) {
        const float4 at = load2(a0 + e, la0), ap = load2(a1 + e, la1);
        const float4 bt = load2(b0 + e, lb0), bp = load2(b1 + e, lb1);
        // s = A_θ - i B_φ = (Re A_θ + Im B_φ, Im A_θ - Re B_φ); t = A_φ + i B_θ
        store2(s + e, ls, make_float4(pick(k0, at.x + bp.y), pick(k0, at.y - bp.x),
                                      pick(k1, at.z + bp.w), pick(k1, at.w - bp.z)));
        store2(t + e, lt, make_float4(pick(k0, ap.x - bt.y), pick(k0, ap.y + bt.x),
                                      pick(k1, ap.z - bt.w), pick(k1, ap.w + bt.z)));
      } else {  // the last number of an odd slab
        const float2 at = a0[e], ap = a1[e], bt = b0[e], bp = b1[e];
        s[e] = make_float2(pick(k0, at.x + bp.y), pick(k0, at.y - bp.x));
        t[e] = make_float2(pick(k0, ap.x - bt.y), pick(k0, ap.y + bt.x));
      }
    }
  }
}

__global__ __launch_bounds__(kVecThreads) void vsht_pack_kernel(
    const float2* __restrict__ st, float2* __restrict__ Cd, float2* __restrict__ Cq, int bc,
    int lmax, int mmax) {
  const int64_t n = (int64_t)lmax * mmax, nd = n + mmax;
  const int64_t pairs = (n + 1) >> 1;
  for (int b = blockIdx.y; b < bc; b += gridDim.y) {
    const float2* s = st + (2LL * b) * n;
    const float2* t = s + n;
    float2* d0 = Cd + (2LL * b) * nd;  // plan_d, θ: s at l + 1
    float2* d1 = d0 + nd;              // plan_d, φ: t at l + 1
    float2* q0 = Cq + (2LL * b) * n;   // plan_q, θ: -i t
    float2* q1 = q0 + n;               // plan_q, φ: i s
    // degree 0 of plan_d's input
    if (blockIdx.x == 0)
      for (int m = threadIdx.x; m < mmax; m += kVecThreads) d0[m] = d1[m] = make_float2(0.f, 0.f);
    d0 += mmax;
    d1 += mmax;
    const bool ls = on16(s), lt = on16(t), ld0 = on16(d0), ld1 = on16(d1);
    const bool lq0 = on16(q0), lq1 = on16(q1);
    for (int64_t i = blockIdx.x * (int64_t)kVecThreads + threadIdx.x; i < pairs;
         i += (int64_t)gridDim.x * kVecThreads) {
      const int64_t e = 2 * i;
      float k0, k1;
      coeff_mask(e, mmax, 0, k0, k1);
      if (e + 1 < n) {
        float4 sv = load2(s + e, ls), tv = load2(t + e, lt);
        sv = make_float4(pick(k0, sv.x), pick(k0, sv.y), pick(k1, sv.z), pick(k1, sv.w));
        tv = make_float4(pick(k0, tv.x), pick(k0, tv.y), pick(k1, tv.z), pick(k1, tv.w));
        store2(d0 + e, ld0, sv);
        store2(d1 + e, ld1, tv);
        store2(q0 + e, lq0, make_float4(tv.y, -tv.x, tv.w, -tv.z));  // -i t
        store2(q1 + e, lq1, make_float4(-sv.y, sv.x, -sv.w, sv.z));  // i s
      } else {
        const float2 sv = make_float2(pick(k0, s[e].x), pick(k0, s[e].y));
        const float2 tv = make_float2(pick(k0, t[e].x), pick(k0, t[e].y));
        d0[e] = sv;
        d1[e] = tv;
        q0[e] = make_float2(tv.y, -tv.x);
        q1[e] = make_float2(-sv.y, sv.x);
      }
    }
  }
}

// v[i] += q[i]; both on the 16-byte grid (vec) or any 4-byte phase
__global__ __launch_bounds__(kVecThreads) void vsht_add_kernel(float* v,
                                                                const float* __restrict__ q,
                                                                int64_t n, int vec) {
  const int64_t tid = blockIdx.x * (int64_t)kVecThreads + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kVecThreads;
  if (vec) {
    float4* v4 = reinterpret_cast<float4*>(v);
    const float4* q4 = reinterpret_cast<const float4*>(q);
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += step) {
      const float4 a = v4[i], b = q4[i];
      v4[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += step) v[i] += q[i];
  } else {
    for (int64_t i = tid; i < n; i += step) v[i] += q[i];
  }
}

namespace {
dim3 vsht_grid(int bc, int lmax, int mmax) {
  const int64_t pairs = ((int64_t)lmax * mmax + 1) >> 1;
  const int by = std::min(bc, 1024);
  const int64_t bx = std::max<int64_t>(1, std::min<int64_t>(cdiv(pairs, kVecThreads), cdiv(kVecGridCap, by)));
  return dim3((unsigned)bx, (unsigned)by);
}
}  // namespace

int launch_vsht_combine(const float2* A, const float2* B, float2* st, int bc, int lmax, int mmax,
                        hipStream_t s) {
  hipLaunchKernelGGL(vsht_combine_kernel, vsht_grid(bc, lmax, mmax), dim3(kVecThreads), 0, s, A,
                     B, st, bc, lmax, mmax);
  return launch_check("vsht_combine");
}

int launch_vsht_pack(const float2* st, float2* Cd, float2* Cq, int bc, int lmax, int mmax,
                     hipStream_t s) {
  hipLaunchKernelGGL(vsht_pack_kernel, vsht_grid(bc, lmax, mmax), dim3(kVecThreads), 0, s, st, Cd,
                     Cq, bc, lmax, mmax);
  return launch_check("vsht_pack");
}

int launch_vsht_add(float* v, const float* q, int64_t n, hipStream_t s) {
  const int vec = ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
  const int blocks = (int)std::min<int64_t>(cdiv(cdiv(n, vec ? 4 : 1), kVecThreads), kVecGridCap);
  hipLaunchKernelGGL(vsht_add_kernel, dim3(std::max(blocks, 1)), dim3(kVecThreads), 0, s, v, q, n,
                     vec);
  return launch_check("vsht_add");
}

}  // namespace msfno
