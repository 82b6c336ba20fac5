// Per-degree power spectrum of spherical-harmonic coefficients and its gradient (the
// middle step of MSFNO/Models/losses.py:158-232, spectral_l2loss_sphere,
// spectral_loss_sphere, h1loss_sphere):
//   power[n][l] = |c[n][l][0]|^2 + 2 sum_{m >= 1} |c[n][l][m]|^2
//   dcoeffs[n][l][m] = (2 e_m gpower[n][l]) c[n][l][m],   e_0 = 1, e_m = 2 (m >= 1)
// The weight 2 covers every m >= 1 (Nyquist included, as in the reference) and every m of
// a row is read: the input is any (N, lmax, mmax) complex tensor, not only a transform's.
//
// Both kernels are HBM streams (303 MB read at 73 x 721 x 721; the backward writes as
// much), built like loss.hip.  A row is mmax complex numbers: always 8-byte aligned, 16-byte
// aligned only every other row when mmax is odd, and off the 16-byte grid as a whole in an
// offset view.  m = 0 has its own weight, so it is always a scalar element; with it the
// scalar head is the 1 or 2 complex numbers in front of the first 16-byte boundary past
// m = 0, the body goes in 16-byte loads / stores (two complex numbers), and an odd
// remainder is a scalar tail.  The backward takes that path when the input and the output
// row have the same 16-byte phase and moves single complex numbers otherwise.
//
// Work split: a row belongs to a group of lpr lanes, lpr the power of two in 4 .. 64 that
// covers the row's 16-byte body in one sweep (64 for longer rows, which take several
// sweeps), so a wave holds 64 / lpr rows and short rows idle no whole wave.  Workgroups of
// 256 lanes take batches of 256 / lpr consecutive rows on a capped grid, 64-bit element
// offsets.  No atomics, no workspace: one writer per output, a fixed summation order, the
// result is bitwise reproducible.
//
// Chain bound: a lane keeps one sum per complex slot of its 16-byte loads, 2 terms per
// sweep each, <= 32 sweeps for mmax <= 4096: 64 terms, + 2 for a head or tail element,
// + 1 to join the two sums, + 6 for the shuffle tree, + 1 for p0 + 2 s (the doubling is
// exact): <= 74 sequential fp32 terms, inside the 128 the tolerance (3 + 128) 2^-24 of
// the tests allows.
#include "kernels.h"

namespace msfno {

namespace {
constexpr int kSpecThreads = 256;
constexpr int kSpecGridCap = 2048;  // 8 workgroups per CU

// lanes per row: the power of two in 4 .. 64 that covers the mmax / 2 16-byte loads
int spectrum_lpr(int mmax) {
  int l = 4;
  while (l < 64 && l < mmax / 2) l <<= 1;
  return l;
}

__device__ __forceinline__ float norm2(float2 v, float acc) {
  return fmaf(v.y, v.y, fmaf(v.x, v.x, acc));
}

// complex numbers in front of the 16-byte body: m = 0, and m = 1 when m = 0 itself sits on
// a 16-byte boundary
__device__ __forceinline__ int spectrum_head(const float2* row, int mmax) {
  return min(2 - (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1), mmax);
}
}  // namespace

__global__ __launch_bounds__(kSpecThreads) void spectrum_power_kernel(
    const float2* __restrict__ coeffs, float* __restrict__ power, int64_t rows, int mmax,
    int lpr) {
  const int grp = (int)threadIdx.x / lpr, lane = (int)threadIdx.x % lpr;
  const int ngrp = kSpecThreads / lpr;
  const int64_t batches = (rows + ngrp - 1) / ngrp;
  for (int64_t b = blockIdx.x; b < batches; b += gridDim.x) {
    const int64_t r = b * ngrp + grp;
    float p0 = 0.f, s0 = 0.f, s1 = 0.f;
    if (r < rows) {
      const float2* p = coeffs + r * (int64_t)mmax;
      const int head = spectrum_head(p, mmax);
      const int nvec = (mmax - head) >> 1;
      const float4* p4 = reinterpret_cast<const float4*>(p + head);
      for (int i = lane; i < nvec; i += lpr) {
        const float4 x = p4[i];
        s0 = fmaf(x.y, x.y, fmaf(x.x, x.x, s0));
        s1 = fmaf(x.w, x.w, fmaf(x.z, x.z, s1));
      }
      // m = 0 on lane 0, m = 1 (a two-element head) on lane 1, an odd tail on lane 2
      const int tail = head + 2 * nvec;
      if (lane == 0) p0 = norm2(p[0], 0.f);
      if (lane == 1 && head == 2) s0 = norm2(p[1], s0);
      if (lane == 2 && tail < mmax) s0 = norm2(p[tail], s0);
    }
    float s = s0 + s1;
    for (int o = lpr >> 1; o > 0; o >>= 1) s += __shfl_down(s, o, lpr);
    if (lane == 0 && r < rows) power[r] = fmaf(2.f, s, p0);
  }
}

// dcoeffs = (2 e_m g) coeffs: the coefficient is an exact power-of-two multiple of g, so
// every output component is one rounding
__global__ __launch_bounds__(kSpecThreads) void spectrum_power_backward_kernel(
    const float2* __restrict__ coeffs, const float* __restrict__ gpower,
    float2* __restrict__ dcoeffs, int64_t rows, int mmax, int lpr) {
  const int grp = (int)threadIdx.x / lpr, lane = (int)threadIdx.x % lpr;
  const int ngrp = kSpecThreads / lpr;
  const int64_t batches = (rows + ngrp - 1) / ngrp;
  for (int64_t b = blockIdx.x; b < batches; b += gridDim.x) {
    const int64_t r = b * ngrp + grp;
    if (r >= rows) continue;
    const float2* p = coeffs + r * (int64_t)mmax;
    float2* o = dcoeffs + r * (int64_t)mmax;
    const float c0 = 2.f * gpower[r], c1 = 4.f * gpower[r];
    const int head = spectrum_head(p, mmax);
    if (head == spectrum_head(o, mmax)) {
      const int nvec = (mmax - head) >> 1;
      const float4* p4 = reinterpret_cast<const float4*>(p + head);
      float4* o4 = reinterpret_cast<float4*>(o + head);
      for (int i = lane; i < nvec; i += lpr) {
        const float4 x = p4[i];
        o4[i] = make_float4(c1 * x.x, c1 * x.y, c1 * x.z, c1 * x.w);
      }
      const int tail = head + 2 * nvec;
      if (lane == 0) o[0] = make_float2(c0 * p[0].x, c0 * p[0].y);
      if (lane == 1 && head == 2) o[1] = make_float2(c1 * p[1].x, c1 * p[1].y);
      if (lane == 2 && tail < mmax) o[tail] = make_float2(c1 * p[tail].x, c1 * p[tail].y);
    } else {
      for (int m = lane; m < mmax; m += lpr) {
        const float c = m ? c1 : c0;
        o[m] = make_float2(c * p[m].x, c * p[m].y);
      }
    }
  }
}

int launch_spectrum_power(const float* coeffs, float* power, int64_t rows, int mmax,
                          hipStream_t s) {
  const int lpr = spectrum_lpr(mmax);
  const int64_t batches = cdiv(rows, kSpecThreads / lpr);
  const int blocks = (int)std::min<int64_t>(batches, kSpecGridCap);
  hipLaunchKernelGGL(spectrum_power_kernel, dim3(blocks), dim3(kSpecThreads), 0, s,
                     reinterpret_cast<const float2*>(coeffs), power, rows, mmax, lpr);
  return launch_check("spectrum_power");
}

int launch_spectrum_power_backward(const float* coeffs, const float* gpower, float* dcoeffs,
                                   int64_t rows, int mmax, hipStream_t s) {
  const int lpr = spectrum_lpr(mmax);
  const int64_t batches = cdiv(rows, kSpecThreads / lpr);
  const int blocks = (int)std::min<int64_t>(batches, kSpecGridCap);
  hipLaunchKernelGGL(spectrum_power_backward_kernel, dim3(blocks), dim3(kSpecThreads), 0, s,
                     reinterpret_cast<const float2*>(coeffs), gpower,
                     reinterpret_cast<float2*>(dcoeffs), rows, mmax, lpr);
  return launch_check("spectrum_power_backward");
}

}  // namespace msfno
