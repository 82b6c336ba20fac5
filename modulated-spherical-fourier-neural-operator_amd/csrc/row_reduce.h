// The scaffold of the latitude-weighted row reductions and row maps over (S, nlat, nlon) fp32
// fields, S = B C slabs (loss.hip, verify.hip, ensemble.hip).  A user supplies the per-pixel
// arithmetic, its kernel signature and its dispatch; everything else is here, once.
//
// Decomposition.  A workgroup is 256 / lpr row groups of lpr lanes (whole waves); a group
// sweeps one row at a time.  A unit is (slab, chunk of rows) on a capped grid.
//
// Row sweep.  16-byte accesses on the part of a row where every pointer in play sits on one
// phase of the 16-byte grid (a slab with odd nlat * nlon moves the phase from row to row):
// a float4 body, the up to 3 + 3 elements before and after it one lane each, and an
// all-scalar path where the pointers disagree.
//
// Reduction.  No atomics.  The order of every sum is fixed:
//   1. per lane, sequential over its share of a row (the caller's bodies);
//   2. one fmaf(w[h], s, acc) per row the lane visits (row_weigh);
//   3. the 6-step shuffle tree of a wave;
//   4. the waves added in index order by the lane that writes the unit's partial;
//   5. per slab, an fp64 lane-strided sum over the chunks, then the shuffle tree
//      (row_combine_kernel).
// A lane's sequential fp32 chain (steps 1 and 2) is its share of a row, nlon / lpr terms,
// plus one weighted add per row it visits: <= 128 terms for nlon <= 16384.  Every workspace
// word read is written by the same call; nothing allocates, synchronises or memsets.
#pragma once
#include <algorithm>

#include "common.h"

namespace msfno {

constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / 64;
constexpr int kRowMaxRows = 64;    // rows per unit: bounds a lane's fp32 chain (above)
constexpr int kRowGridCap = 2048;  // 8 workgroups per CU

// a lambda handed to the scaffold inlines like the __forceinline__ function it stands for
#define ROW_BODY __attribute__((always_inline))

// the decomposition of one call: formed on the host, a kernel's last argument
struct RowGeom {
  int64_t units;  // S * chunks
  int S, nlat, nlon;
  int lpr;     // lanes per row group: the one of 256, 128, 64 with the fewest idle lane slots
               // over the row (1440: 360 float4 = 3 sweeps of 128, not 2 of 256 with the
               // second 40 % full)
  int rows;    // rows per unit (a multiple of the group count unless one unit has them all)
  int chunks;  // units per slab
};

inline RowGeom row_geom(int S, int nlat, int nlon) {
  RowGeom g;
  g.S = S;
  g.nlat = nlat;
  g.nlon = nlon;
  const int nvec = std::max(1, nlon / 4);
  g.lpr = 256;
  for (int l = 128; l >= 64; l >>= 1)
    if (cdiv(nvec, l) * l < cdiv(nvec, g.lpr) * g.lpr) g.lpr = l;
  const int ngrp = kRowThreads / g.lpr;
  // enough units to fill the chip at small S, at most kRowMaxRows rows each
  int64_t chunks = std::max<int64_t>(cdiv(kRowGridCap, S), cdiv(nlat, kRowMaxRows));
  chunks = std::min<int64_t>(chunks, nlat);
  g.rows = (int)std::min<int64_t>(round_up(cdiv(nlat, chunks), ngrp), kRowMaxRows);
  g.chunks = (int)cdiv(nlat, g.rows);
  g.units = (int64_t)S * g.chunks;
  return g;
}

// Bytes for floats_per_unit partials per unit.  From an upper bound of S * chunks that is
// non-decreasing in every argument (S * chunks itself is not: more slabs means fewer chunks
// each): chunks <= nlat and chunks <= cdiv(cap, S) + cdiv(nlat, maxrows).
inline size_t row_workspace_bytes(int S, int nlat, int floats_per_unit) {
  const int64_t a = (int64_t)S * nlat;
  const int64_t b = kRowGridCap + (int64_t)S + (int64_t)S * cdiv(nlat, kRowMaxRows);
  return (size_t)round_up(std::min(a, b) * floats_per_unit * (int64_t)sizeof(float), 256);
}

// kernel(args..., g) on the capped grid
template <class... Formal, class... Args>
inline int row_launch(void (*kernel)(Formal...), const char* name, const RowGeom& g,
                      hipStream_t s, Args... args) {
  const unsigned blocks = (unsigned)std::min<int64_t>(g.units, kRowGridCap);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRowThreads), 0, s, args..., g);
  return launch_check(name);
}

// position of p on the 16-byte grid, in floats
__device__ __forceinline__ int misalign4(const float* p) {
  return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
}

// the phase that all the pointers share, or -1
template <class... P>
__device__ __forceinline__ int row_phase(const float* p, const P*... rest) {
  const int a = misalign4(p);
  return ((a == misalign4(rest)) && ...) ? a : -1;
}

// Unit walk: unit(u, s, rows) for every unit u = (slab s, chunk) this workgroup owns, and in
// it rows(row) calls row(h, off, lane) for every row h of the unit that the lane's group
// sweeps, off = (s * nlat + h) * nlon.  UNIFORM: a row group is whole waves, so its index,
// and with it the row and every row pointer, is wave-uniform; saying so keeps them in scalar
// registers (one base per pointer and one lane offset for all), which the ensemble kernels
// need for their M + 1 and 2 M + 1 row pointers.
template <bool UNIFORM, class Unit>
__device__ __forceinline__ void row_walk(const RowGeom& g, Unit&& unit) {
  const int grp0 = (int)threadIdx.x / g.lpr;
  const int grp = UNIFORM ? __builtin_amdgcn_readfirstlane(grp0) : grp0;
  const int lane = (int)threadIdx.x % g.lpr;
  const int ngrp = kRowThreads / g.lpr;
  for (int64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const int64_t s = u / g.chunks;
    const int h0 = (int)(u - s * g.chunks) * g.rows, h1 = min(g.nlat, h0 + g.rows);
    unit(u, s, [&](auto&& row) ROW_BODY {
      for (int h = h0 + grp; h < h1; h += ngrp) row(h, (s * g.nlat + h) * (int64_t)g.nlon, lane);
    });
  }
}

// body(i) for i = lane, lane + lpr, ... < n.  NOUNROLL where the body is hundreds of
// instructions on nearly all the registers (the ensemble's member pairs).
template <bool NOUNROLL, class Body>
__device__ __forceinline__ void row_strided(int lane, int n, int lpr, Body&& body) {
  if constexpr (NOUNROLL) {
#pragma nounroll
    for (int i = lane; i < n; i += lpr) body(i);
  } else {
    for (int i = lane; i < n; i += lpr) body(i);
  }
}

// Row sweep over nlon elements by the lpr lanes of a group.  a is the phase all row pointers
// share (row_phase), or negative.  vec(head, i) handles the elements head + 4 i .. + 3
// (p + head is 16-byte aligned), one(e) the element e.
template <bool NOUNROLL, class Vec, class One>
__device__ __forceinline__ void row_sweep(int a, int nlon, int lane, int lpr, Vec&& vec,
                                          One&& one) {
  if (a >= 0) {
    const int head = min((4 - a) & 3, nlon);
    const int nvec = (nlon - head) >> 2;
    row_strided<NOUNROLL>(lane, nvec, lpr, [&](int i) ROW_BODY { vec(head, i); });
    // the up to 3 + 3 elements before and after the aligned part, one lane each
    const int tail0 = head + 4 * nvec;
    if (lane < head + (nlon - tail0)) one(lane < head ? lane : tail0 + (lane - head));
  } else {
    row_strided<NOUNROLL>(lane, nlon, lpr, one);
  }
}

// step 2: a row's sums into the unit's, under the row's weight
template <int K>
__device__ __forceinline__ void row_weigh(float wh, const float (&s)[K], float (&acc)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = fmaf(wh, s[k], acc[k]);
}

// Steps 3 and 4: the workgroup's sums of acc[0..K) to out[0..K).  Optionally a second group
// of n2 <= K2 sums that each wave's first lane already holds for its wave (acc2; no
// shuffle), to out[K..K + n2).  red (and red2) are reused by the next unit, hence the second
// barrier.
template <int K, int K2 = 0>
__device__ __forceinline__ void row_block_sum(float (&acc)[K], float (&red)[kRowWaves][K],
                                              float* __restrict__ out,
                                              const float* acc2 = nullptr,
                                              float (*red2)[K2 ? K2 : 1] = nullptr,
                                              int n2 = 0) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = acc[k];
#pragma unroll
    for (int r = 0; r < K2; ++r)
      if (r < n2) red2[threadIdx.x >> 6][r] = acc2[r];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < K + n2) {
    float v;
    if (K2 == 0 || k < K) {
      v = red[0][k];
      for (int q = 1; q < kRowWaves; ++q) v += red[q][k];
    } else {
      v = red2[0][k - K];
      for (int q = 1; q < kRowWaves; ++q) v += red2[q][k - K];
    }
    out[k] = v;
  }
  __syncthreads();
}

// Step 5, one wave per slab: lane l adds the partials l, l + 64, ... of each sum in fp64,
// then a fixed tree.  The first n0 sums of a unit's pstride go to out0 (S, n0), the next n1
// to out1 (S, n1).
static __global__ __launch_bounds__(kRowThreads) void row_combine_kernel(
    const float* __restrict__ part, int pstride, int chunks, int S, float* __restrict__ out0,
    int n0, float* __restrict__ out1, int n1) {
  const int s = (int)blockIdx.x * kRowWaves + ((int)threadIdx.x >> 6);
  if (s >= S) return;
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < n0 + n1; ++k) {
    double v = 0.0;
    for (int c = lane; c < chunks; c += 64)
      v += (double)part[((int64_t)s * chunks + c) * pstride + k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) {
      if (k < n0)
        out0[(int64_t)s * n0 + k] = (float)v;
      else
        out1[(int64_t)s * n1 + (k - n0)] = (float)v;
    }
  }
}

inline int row_combine(const char* name, const RowGeom& g, hipStream_t s, const float* part,
                       int pstride, float* out0, int n0, float* out1 = nullptr, int n1 = 0) {
  hipLaunchKernelGGL(row_combine_kernel, dim3((unsigned)cdiv(g.S, kRowWaves)),
                     dim3(kRowThreads), 0, s, part, pstride, g.chunks, g.S, out0, n0, out1, n1);
  return launch_check(name);
}

}  // namespace msfno
