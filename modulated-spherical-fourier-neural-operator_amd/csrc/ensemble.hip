// Ensemble verification sums and the gradient of the (fair) CRPS.  M members x_i and a
// truth y, all fp32 fields of one (real) space; per slab s = (b, c) under the latitude
// weights w, summed over the pixels of the slab, with dbar = (1/M) sum_i (x_i - y):
//   se   = sum w dbar^2                     gini = sum w sum_{i<j} |x_i - x_j|
//   err  = sum w dbar                       sq   = sum w sum_{i<j} (x_i - x_j)^2
//   abs  = sum w (1/M) sum_i |x_i - y|      hist[r] = sum w [#{i : x_i < y} == r], r = 0..M
// from which the ensemble-mean RMSE and bias, the MAE, the spread (sq = M sum_i
// (x_i - xbar)^2), the spread/skill ratio, the CRPS (abs - gini / M^2), the fair CRPS
// (abs - gini / (M (M - 1))) and the rank histogram follow on (B, C) numbers
// (msfno_amd/ensemble.py).  Difference first: every per-pixel quantity is formed from
// x_i - y or x_i - x_j (one correctly rounded fp32 subtraction each), never from the raw
// values or a raw mean, so a 300 K field with 1 K of spread loses nothing.
//
// Member i of slab s starts at ens + i * member_stride + s * nlat * nlon.  Geometry and
// conventions are loss.hip's and verify.hip's (row_geom.h): units of (slab, chunk of rows)
// on a capped grid, 16-byte loads where the M + 1 row pointers share a phase of the
// 16-byte grid (member_stride a multiple of 4 floats and ens, tar in phase; scalar head
// and tail, a scalar path otherwise), no atomics.  The members of a pixel sit in registers
// under a compile-time bound MB (buckets 4 / 8 / 16 / 32, predicated on the wave-uniform
// M); a lane holds 4 pixels of them up to MB = 16 and 1 pixel at MB = 32 (4 x 32 would
// spill), which is VALU-bound whatever the load width.
//
// Summation chains.  Per pixel: dbar is M - 1 adds and a product with the rounded 1 / M;
// the pair sums are a sequential chain of M (M - 1) / 2 non-negative terms.  Per lane: one
// add per pixel of its share of a row (nlon / lpr terms), one weighted add per row it
// visits, as loss.hip (<= 128 terms for nlon <= 16384); then wave + block reduce, one
// partial per unit into the caller's workspace, combined per slab in fp64 in a fixed
// order.  The rank histogram is counted in integers: per row, per wave, the population
// count of the lanes' ballot for each rank (exact), then one weighted add per row and
// rank; the waves' sums are combined like the other partials.  Every workspace and output
// word read or returned is written by the same call; nothing allocates, synchronises or
// memsets.
#include "kernels.h"
#include "row_geom.h"

namespace msfno {

namespace {
constexpr int kESums = 5;

__host__ __device__ constexpr int ens_px(int MB) { return MB <= 16 ? 4 : 1; }
// waves per SIMD the kernels are compiled for (bounds the registers): the small buckets are
// HBM streams and want the loads of many waves in flight
__host__ __device__ constexpr int ens_waves(int MB) { return MB <= 4 ? 6 : MB <= 8 ? 3 : 2; }
// A full bucket (M == MB) has kernels of its own in which every predicate on M folds, except
// at MB = 16: there the folded pair loops of 4 pixels are one basic block of 480 pairs, which
// the scheduler interleaves until it spills inside the loop; the predicated form does not.
constexpr bool ens_has_full(int MB) { return MB != 16; }

// one pixel: members x[i][k] (i < M), truth y
template <int MB, int PX, bool HIST>
__device__ __forceinline__ void ens_pixel(const float (&x)[MB][PX], int k, float y, int M,
                                          float inv_m, float (&s)[kESums],
                                          int (&cnt)[MB + 1]) {
  float sd = 0.f, sa = 0.f;
  int rank = 0;
#pragma unroll
  for (int i = 0; i < MB; ++i)
    if (i < M) {
      const float d = x[i][k] - y;
      sd += d;
      sa += fabsf(d);
      rank += x[i][k] < y ? 1 : 0;
    }
  float pg = 0.f, ps = 0.f;
#pragma unroll
  for (int i = 0; i + 1 < MB; ++i)
    if (i + 1 < M) {
#pragma unroll
      for (int j = i + 1; j < MB; ++j)
        if (j < M) {
          const float d = x[i][k] - x[j][k];
          pg += fabsf(d);
          ps = fmaf(d, d, ps);
        }
    }
  const float dbar = sd * inv_m;
  s[0] = fmaf(dbar, dbar, s[0]);
  s[1] += dbar;
  s[2] = fmaf(sa, inv_m, s[2]);
  s[3] += pg;
  s[4] += ps;
  if (HIST) {
#pragma unroll
    for (int r = 0; r <= MB; ++r)
      if (r <= M) cnt[r] += __popcll(__ballot(rank == r));
  }
}

// the sums and rank counts of one row over the lanes of a row group; e0 is member 0's row
template <int MB, bool HIST>
__device__ __forceinline__ void ens_row(const float* __restrict__ e0, int64_t mstride,
                                        const float* __restrict__ t, int M, float inv_m,
                                        int nlon, int lane, int lpr, float (&s)[kESums],
                                        int (&cnt)[MB + 1]) {
  constexpr int PX = ens_px(MB);
  if (PX == 4 && (mstride & 3) == 0 && misalign4(e0) == misalign4(t)) {
    const int head = min((4 - misalign4(t)) & 3, nlon);
    const int nvec = (nlon - head) >> 2;
    const float4* t4 = reinterpret_cast<const float4*>(t + head);
    #pragma nounroll
    for (int v = lane; v < nvec; v += lpr) {
      float x[MB][PX];
#pragma unroll
      for (int i = 0; i < MB; ++i)
        if (i < M) {
          const float4 q = reinterpret_cast<const float4*>(e0 + i * mstride + head)[v];
          x[i][0] = q.x;
          x[i][1 % PX] = q.y;
          x[i][2 % PX] = q.z;
          x[i][3 % PX] = q.w;
        }
      const float4 y = t4[v];
      const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int k = 0; k < PX; ++k) ens_pixel<MB, PX, HIST>(x, k, yy[k], M, inv_m, s, cnt);
    }
    // the up to 3 + 3 elements before and after the aligned part, one lane each
    const int tail0 = head + 4 * nvec;
    if (lane < head + (nlon - tail0)) {
      const int e = lane < head ? lane : tail0 + (lane - head);
      float x[MB][PX];
#pragma unroll
      for (int i = 0; i < MB; ++i)
        if (i < M) x[i][0] = e0[i * mstride + e];
      ens_pixel<MB, PX, HIST>(x, 0, t[e], M, inv_m, s, cnt);
    }
  } else {
    #pragma nounroll
    for (int e = lane; e < nlon; e += lpr) {
      float x[MB][PX];
#pragma unroll
      for (int i = 0; i < MB; ++i)
        if (i < M) x[i][0] = e0[i * mstride + e];
      ens_pixel<MB, PX, HIST>(x, 0, t[e], M, inv_m, s, cnt);
    }
  }
}

// sign(x_i - y) / M - kappa sum_{j != i} sign(x_i - x_j), sign(0) = 0: both terms from
// exact integers; on return x[i][k] holds the bracket of member i
template <int MB, int PX>
__device__ __forceinline__ void crps_bracket(float (&x)[MB][PX], int k, float y, int M,
                                             float inv_m, float kappa) {
  int c[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) c[i] = 0;
#pragma unroll
  for (int i = 0; i + 1 < MB; ++i)
    if (i + 1 < M) {
#pragma unroll
      for (int j = i + 1; j < MB; ++j)
        if (j < M) {
          const int sg = (x[i][k] > x[j][k] ? 1 : 0) - (x[i][k] < x[j][k] ? 1 : 0);
          c[i] += sg;
          c[j] -= sg;
        }
    }
#pragma unroll
  for (int i = 0; i < MB; ++i)
    if (i < M) {
      const int sy = (x[i][k] > y ? 1 : 0) - (x[i][k] < y ? 1 : 0);
      x[i][k] = fmaf(-kappa, (float)c[i], (float)sy * inv_m);
    }
}
}  // namespace

// the partials of a unit: the five sums, then the M + 1 rank bins
static inline int ens_part_stride(int M) { return kESums + M + 1; }

size_t ens_workspace_bytes(int S, int M, int nlat, int nlon) {
  (void)nlon;
  return (size_t)round_up(
      row_units_bound(S, nlat) * (int64_t)(ens_part_stride(M) * sizeof(float)), 256);
}

template <int MB, bool HIST, bool FULL>
__global__ __launch_bounds__(kRowThreads, ens_waves(MB)) void ens_sums_kernel(
    const float* __restrict__ ens, int64_t mstride, const float* __restrict__ tar,
    const float* __restrict__ w_lat, float* __restrict__ part, int m_rt, float inv_m, int nlat,
    int nlon, int chunks, int rows, int64_t units, int lpr) {
  const int M = FULL ? MB : m_rt;  // a full bucket: every predicate on M folds
  constexpr int kWaves = kRowThreads / 64;
  __shared__ float red[kWaves][kESums];
  __shared__ float redh[kWaves][MB + 1];
  // a row group is whole waves: its index, and with it the row and every row pointer, is
  // wave-uniform (scalar registers, one base per member and one lane offset for all)
  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x / lpr);
  const int lane = (int)threadIdx.x % lpr;
  const int ngrp = kRowThreads / lpr;
  const int pstride = kESums + M + 1;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t bc = u / chunks;
    const int h0 = (int)(u - bc * chunks) * rows, h1 = min(nlat, h0 + rows);
    float acc[kESums] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float hacc[MB + 1];
#pragma unroll
    for (int r = 0; r <= MB; ++r) hacc[r] = 0.f;
    for (int h = h0 + grp; h < h1; h += ngrp) {
      const int64_t off = (bc * nlat + h) * (int64_t)nlon;
      float s[kESums] = {0.f, 0.f, 0.f, 0.f, 0.f};
      int cnt[MB + 1];
#pragma unroll
      for (int r = 0; r <= MB; ++r) cnt[r] = 0;
      ens_row<MB, HIST>(ens + off, mstride, tar + off, M, inv_m, nlon, lane, lpr, s, cnt);
      const float wh = w_lat[h];
#pragma unroll
      for (int k = 0; k < kESums; ++k) acc[k] = fmaf(wh, s[k], acc[k]);
      if (HIST) {
#pragma unroll
        for (int r = 0; r <= MB; ++r)
          if (r <= M) hacc[r] = fmaf(wh, (float)cnt[r], hacc[r]);
      }
    }
#pragma unroll
    for (int k = 0; k < kESums; ++k)
      for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
    // a wave's first lane takes part in every ballot of the wave (its column index is the
    // lowest), so it holds the wave's whole counts
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < kESums; ++k) red[threadIdx.x >> 6][k] = acc[k];
      if (HIST) {
#pragma unroll
        for (int r = 0; r <= MB; ++r)
          if (r <= M) redh[threadIdx.x >> 6][r] = hacc[r];
      }
    }
    __syncthreads();
    const int nout = HIST ? pstride : kESums;
    if ((int)threadIdx.x < nout) {
      const int k = threadIdx.x;
      float v;
      if (k < kESums) {
        v = red[0][k];
        for (int q = 1; q < kWaves; ++q) v += red[q][k];
      } else {
        v = redh[0][k - kESums];
        for (int q = 1; q < kWaves; ++q) v += redh[q][k - kESums];
      }
      part[u * pstride + k] = v;
    }
    __syncthreads();  // red and redh are reused by the next unit
  }
}

// one wave per slab: lane l adds the partials l, l + 64, ... in fp64, then a fixed tree;
// the rank bins only where a histogram was asked for (their partials are not written
// otherwise)
__global__ __launch_bounds__(kRowThreads) void ens_combine_kernel(
    const float* __restrict__ part, int chunks, int S, int M, float* __restrict__ sums,
    float* __restrict__ hist) {
  const int bc = (int)blockIdx.x * (kRowThreads / 64) + ((int)threadIdx.x >> 6);
  if (bc >= S) return;
  const int lane = threadIdx.x & 63;
  const int pstride = kESums + M + 1;
  const int nk = hist ? pstride : kESums;
  for (int k = 0; k < nk; ++k) {
    double v = 0.0;
    for (int c = lane; c < chunks; c += 64)
      v += (double)part[((int64_t)bc * chunks + c) * pstride + k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) {
      if (k < kESums)
        sums[(int64_t)bc * kESums + k] = (float)v;
      else
        hist[(int64_t)bc * (M + 1) + (k - kESums)] = (float)v;
    }
  }
}

// dens_i = (w[h] g[s]) (sign(x_i - y) / M - kappa sum_{j != i} sign(x_i - x_j)): one pass
// over the members and the truth, 16-byte loads and stores where the 2 M + 1 row pointers
// share a phase
template <int MB, bool FULL>
__global__ __launch_bounds__(kRowThreads, ens_waves(MB)) void ens_crps_backward_kernel(
    const float* __restrict__ ens, int64_t mstride, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ g, float kappa,
    float* __restrict__ dens, int64_t dstride, int m_rt, float inv_m, int nlat, int nlon,
    int chunks, int rows, int64_t units, int lpr) {
  constexpr int PX = ens_px(MB);
  const int M = FULL ? MB : m_rt;
  // a row group is whole waves: its index, and with it the row and every row pointer, is
  // wave-uniform (scalar registers, one base per member and one lane offset for all)
  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x / lpr);
  const int lane = (int)threadIdx.x % lpr;
  const int ngrp = kRowThreads / lpr;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t bc = u / chunks;
    const int h0 = (int)(u - bc * chunks) * rows, h1 = min(nlat, h0 + rows);
    const float gs = g[bc];
    for (int h = h0 + grp; h < h1; h += ngrp) {
      const int64_t off = (bc * nlat + h) * (int64_t)nlon;
      const float* e0 = ens + off;
      const float* t = tar + off;
      float* o0 = dens + off;
      const float c = gs * w_lat[h];
      const int a = misalign4(t);
      if (PX == 4 && ((mstride | dstride) & 3) == 0 && a == misalign4(e0) &&
          a == misalign4(o0)) {
        const int head = min((4 - a) & 3, nlon);
        const int nvec = (nlon - head) >> 2;
        const float4* t4 = reinterpret_cast<const float4*>(t + head);
        #pragma nounroll
        for (int v = lane; v < nvec; v += lpr) {
          float x[MB][PX];
#pragma unroll
          for (int i = 0; i < MB; ++i)
            if (i < M) {
              const float4 q = reinterpret_cast<const float4*>(e0 + i * mstride + head)[v];
              x[i][0] = q.x;
              x[i][1 % PX] = q.y;
              x[i][2 % PX] = q.z;
              x[i][3 % PX] = q.w;
            }
          const float4 y = t4[v];
          const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
          for (int k = 0; k < PX; ++k) crps_bracket<MB, PX>(x, k, yy[k], M, inv_m, kappa);
#pragma unroll
          for (int i = 0; i < MB; ++i)
            if (i < M)
              reinterpret_cast<float4*>(o0 + i * dstride + head)[v] = make_float4(
                  c * x[i][0], c * x[i][1 % PX], c * x[i][2 % PX], c * x[i][3 % PX]);
        }
        const int tail0 = head + 4 * nvec;
        if (lane < head + (nlon - tail0)) {
          const int e = lane < head ? lane : tail0 + (lane - head);
          float x[MB][PX];
#pragma unroll
          for (int i = 0; i < MB; ++i)
            if (i < M) x[i][0] = e0[i * mstride + e];
          crps_bracket<MB, PX>(x, 0, t[e], M, inv_m, kappa);
#pragma unroll
          for (int i = 0; i < MB; ++i)
            if (i < M) o0[i * dstride + e] = c * x[i][0];
        }
      } else {
        #pragma nounroll
        for (int e = lane; e < nlon; e += lpr) {
          float x[MB][PX];
#pragma unroll
          for (int i = 0; i < MB; ++i)
            if (i < M) x[i][0] = e0[i * mstride + e];
          crps_bracket<MB, PX>(x, 0, t[e], M, inv_m, kappa);
#pragma unroll
          for (int i = 0; i < MB; ++i)
            if (i < M) o0[i * dstride + e] = c * x[i][0];
        }
      }
    }
  }
}

template <int MB>
static int launch_ens_sums_mb(const float* ens, int64_t mstride, const float* tar,
                              const float* w_lat, float* part, bool with_hist, int M, int S,
                              int nlat, int nlon, const RowGeom& g, hipStream_t s) {
  const int64_t units = (int64_t)S * g.chunks;
  const int blocks = (int)std::min<int64_t>(units, kRowGridCap);
  const float inv_m = 1.f / (float)M;
  auto k = with_hist ? ens_sums_kernel<MB, true, false> : ens_sums_kernel<MB, false, false>;
  if constexpr (ens_has_full(MB)) {
    if (M == MB) k = with_hist ? ens_sums_kernel<MB, true, true> : ens_sums_kernel<MB, false, true>;
  }
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kRowThreads), 0, s, ens, mstride, tar, w_lat, part, M,
                     inv_m, nlat, nlon, g.chunks, g.rows, units, g.lpr);
  return launch_check("ens_sums");
}

int launch_ens_sums(const float* ens, int64_t mstride, const float* tar, const float* w_lat,
                    float* sums, float* hist, int M, int S, int nlat, int nlon, void* ws,
                    hipStream_t s) {
  const RowGeom g = row_geom(S, nlat, nlon);
  float* part = static_cast<float*>(ws);
  const bool wh = hist != nullptr;
  if (M <= 4)
    MSFNO_TRY(launch_ens_sums_mb<4>(ens, mstride, tar, w_lat, part, wh, M, S, nlat, nlon, g, s));
  else if (M <= 8)
    MSFNO_TRY(launch_ens_sums_mb<8>(ens, mstride, tar, w_lat, part, wh, M, S, nlat, nlon, g, s));
  else if (M <= 16)
    MSFNO_TRY(launch_ens_sums_mb<16>(ens, mstride, tar, w_lat, part, wh, M, S, nlat, nlon, g, s));
  else
    MSFNO_TRY(launch_ens_sums_mb<32>(ens, mstride, tar, w_lat, part, wh, M, S, nlat, nlon, g, s));
  hipLaunchKernelGGL(ens_combine_kernel, dim3((unsigned)cdiv(S, kRowThreads / 64)),
                     dim3(kRowThreads), 0, s, part, g.chunks, S, M, sums, hist);
  return launch_check("ens_combine");
}

template <int MB>
static int launch_ens_bwd_mb(const float* ens, int64_t mstride, const float* tar,
                             const float* w_lat, const float* gr, float kappa, float* dens,
                             int64_t dstride, int M, int S, int nlat, int nlon, hipStream_t s) {
  const RowGeom g = row_geom(S, nlat, nlon);
  const int64_t units = (int64_t)S * g.chunks;
  const int blocks = (int)std::min<int64_t>(units, kRowGridCap);
  auto k = ens_crps_backward_kernel<MB, false>;
  if constexpr (ens_has_full(MB)) {
    if (M == MB) k = ens_crps_backward_kernel<MB, true>;
  }
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kRowThreads), 0, s, ens, mstride, tar, w_lat, gr, kappa,
                     dens, dstride, M, 1.f / (float)M, nlat, nlon, g.chunks, g.rows, units, g.lpr);
  return launch_check("ens_crps_backward");
}

int launch_ens_crps_backward(const float* ens, int64_t mstride, const float* tar,
                             const float* w_lat, const float* g, float kappa, float* dens,
                             int64_t dstride, int M, int S, int nlat, int nlon, hipStream_t s) {
  if (M <= 4)
    return launch_ens_bwd_mb<4>(ens, mstride, tar, w_lat, g, kappa, dens, dstride, M, S, nlat,
                                nlon, s);
  if (M <= 8)
    return launch_ens_bwd_mb<8>(ens, mstride, tar, w_lat, g, kappa, dens, dstride, M, S, nlat,
                                nlon, s);
  if (M <= 16)
    return launch_ens_bwd_mb<16>(ens, mstride, tar, w_lat, g, kappa, dens, dstride, M, S, nlat,
                                 nlon, s);
  return launch_ens_bwd_mb<32>(ens, mstride, tar, w_lat, g, kappa, dens, dstride, M, S, nlat,
                               nlon, s);
}

}  // namespace msfno
