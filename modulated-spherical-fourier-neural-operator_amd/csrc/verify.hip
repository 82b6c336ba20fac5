// Forecast verification sums (the scoring of MSFNO/Models/sfno/model.py:737-758 and
// train.py:533-583, done there on the host after a device-to-host copy of every scored
// output).  One pass over a forecast prd, its truth tar and an optional climatology clim,
// all fp32 fields of one (real) space; per (b, c) slab under the latitude weights w
//   se    = sum w (p - t)^2        pa2   = sum w (p - c)^2
//   err   = sum w (p - t)          ta2   = sum w (t - c)^2
//   ae    = sum w |p - t|          cross = sum w (p - c)(t - c)
// from which RMSE, bias, MAE, the climatology skill 1 - se / ta2 and the anomaly
// correlation cross / sqrt(pa2 ta2) follow on (B, C) numbers (msfno_amd/verification.py).
// clim is a stack of (nlat, nlon) slabs and clim_slab[bc] the slab of bc, or -1 for none
// (then pa2 = ta2 = cross = 0, written explicitly): a climatology broadcast over the batch,
// one for some variables only, one per sample.
//
// An HBM stream: 606 MB read at 1 x 73 x 721 x 1440, 909 MB with a climatology for every
// slab.  Geometry and conventions are loss.hip's (row_geom.h): 16-byte loads on the part of
// a row where the 2 or 3 pointers in play share a phase of the 16-byte grid (scalar head
// and tail, a scalar path otherwise), units of (bc, chunk of rows) on a capped grid, no
// atomics: per-lane fp32 sums of a row, weighted once per row, wave + block reduce, one
// partial of six per unit into the caller's workspace, combined per (b, c) in fp64 in a
// fixed order.  A lane's sequential fp32 chain is that of loss.hip (its share of a row plus
// one weighted add per row it visits, <= 128 terms for nlon <= 16384).  Every workspace
// word read is written by the same call; nothing allocates, synchronises or memsets.
#include "kernels.h"
#include "row_geom.h"

namespace msfno {

namespace {
constexpr int kNSums = 6;

template <bool CLIM>
__device__ __forceinline__ void verify_term(float p, float t, float c, float (&s)[kNSums]) {
  const float d = p - t;
  s[0] = fmaf(d, d, s[0]);
  s[1] += d;
  s[2] += fabsf(d);
  if (CLIM) {
    const float a = p - c, b = t - c;
    s[3] = fmaf(a, a, s[3]);
    s[4] = fmaf(b, b, s[4]);
    s[5] = fmaf(a, b, s[5]);
  }
}

// the sums of one row over the lanes of a row group (c is not read unless CLIM)
template <bool CLIM>
__device__ __forceinline__ void verify_row(const float* __restrict__ p,
                                           const float* __restrict__ t,
                                           const float* __restrict__ c, int nlon, int lane,
                                           int lpr, float (&s)[kNSums]) {
  const int a = misalign4(p);
  if (a == misalign4(t) && (!CLIM || a == misalign4(c))) {
    const int head = min((4 - a) & 3, nlon);
    const int nvec = (nlon - head) >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    const float4* t4 = reinterpret_cast<const float4*>(t + head);
    const float4* c4 = CLIM ? reinterpret_cast<const float4*>(c + head) : nullptr;
    for (int i = lane; i < nvec; i += lpr) {
      const float4 x = p4[i], y = t4[i];
      const float4 z = CLIM ? c4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      verify_term<CLIM>(x.x, y.x, z.x, s);
      verify_term<CLIM>(x.y, y.y, z.y, s);
      verify_term<CLIM>(x.z, y.z, z.z, s);
      verify_term<CLIM>(x.w, y.w, z.w, s);
    }
    // the up to 3 + 3 elements before and after the aligned part, one lane each
    const int tail0 = head + 4 * nvec;
    if (lane < head + (nlon - tail0)) {
      const int e = lane < head ? lane : tail0 + (lane - head);
      verify_term<CLIM>(p[e], t[e], CLIM ? c[e] : 0.f, s);
    }
  } else {
    for (int i = lane; i < nlon; i += lpr) verify_term<CLIM>(p[i], t[i], CLIM ? c[i] : 0.f, s);
  }
}
}  // namespace

size_t verify_workspace_bytes(int BC, int nlat, int nlon) {
  (void)nlon;
  return (size_t)round_up(row_units_bound(BC, nlat) * (int64_t)(kNSums * sizeof(float)), 256);
}

__global__ __launch_bounds__(kRowThreads) void verify_sums_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ clim,
    const int* __restrict__ clim_slab, float* __restrict__ part, int nlat, int nlon, int chunks,
    int rows, int64_t units, int lpr) {
  __shared__ float red[kRowThreads / 64][kNSums];
  const int grp = (int)threadIdx.x / lpr, lane = (int)threadIdx.x % lpr;
  const int ngrp = kRowThreads / lpr;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t bc = u / chunks;
    const int h0 = (int)(u - bc * chunks) * rows, h1 = min(nlat, h0 + rows);
    const int cs = clim_slab ? clim_slab[bc] : -1;
    float acc[kNSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int h = h0 + grp; h < h1; h += ngrp) {
      const int64_t off = (bc * nlat + h) * (int64_t)nlon;
      float s[kNSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (cs >= 0)
        verify_row<true>(prd + off, tar + off, clim + ((int64_t)cs * nlat + h) * (int64_t)nlon,
                         nlon, lane, lpr, s);
      else
        verify_row<false>(prd + off, tar + off, nullptr, nlon, lane, lpr, s);
      const float wh = w_lat[h];
#pragma unroll
      for (int k = 0; k < kNSums; ++k) acc[k] = fmaf(wh, s[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < kNSums; ++k)
      for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < kNSums; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < kNSums) {
      float v = red[0][threadIdx.x];
      for (int k = 1; k < kRowThreads / 64; ++k) v += red[k][threadIdx.x];
      part[u * kNSums + threadIdx.x] = v;
    }
    __syncthreads();  // red is reused by the next unit
  }
}

// one wave per (b, c): lane l adds the partials l, l + 64, ... in fp64, then a fixed tree;
// a slab without a climatology gets exact zeros in its last three sums
__global__ __launch_bounds__(kRowThreads) void verify_combine_kernel(
    const float* __restrict__ part, const int* __restrict__ clim_slab, int chunks, int BC,
    float* __restrict__ sums) {
  const int bc = (int)blockIdx.x * (kRowThreads / 64) + ((int)threadIdx.x >> 6);
  if (bc >= BC) return;
  const int lane = threadIdx.x & 63;
  const int nk = (clim_slab && clim_slab[bc] >= 0) ? kNSums : 3;
  double v[kNSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = lane; c < chunks; c += 64) {
    const float* q = part + ((int64_t)bc * chunks + c) * kNSums;
#pragma unroll
    for (int k = 0; k < kNSums; ++k)
      if (k < nk) v[k] += (double)q[k];
  }
#pragma unroll
  for (int k = 0; k < kNSums; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kNSums; ++k) sums[(int64_t)bc * kNSums + k] = k < nk ? (float)v[k] : 0.f;
  }
}

int launch_verify_sums(const float* prd, const float* tar, const float* w_lat, const float* clim,
                       const int* clim_slab, float* sums, int BC, int nlat, int nlon, void* ws,
                       hipStream_t s) {
  const RowGeom g = row_geom(BC, nlat, nlon);
  const int64_t units = (int64_t)BC * g.chunks;
  float* part = static_cast<float*>(ws);
  const int blocks = (int)std::min<int64_t>(units, kRowGridCap);
  hipLaunchKernelGGL(verify_sums_kernel, dim3(blocks), dim3(kRowThreads), 0, s, prd, tar, w_lat,
                     clim, clim_slab, part, nlat, nlon, g.chunks, g.rows, units, g.lpr);
  MSFNO_TRY(launch_check("verify_sums"));
  hipLaunchKernelGGL(verify_combine_kernel, dim3((unsigned)cdiv(BC, kRowThreads / 64)),
                     dim3(kRowThreads), 0, s, part, clim_slab, g.chunks, BC, sums);
  return launch_check("verify_combine");
}

}  // namespace msfno
