// Sphere-weighted training losses (MSFNO/Models/losses.py: L2Sphere, L2Sphere_noSine,
// CosineMSELoss; the validation MSEs of train.py:553-564).  All of them are, per (b, c),
//   num = sum_h w[h] sum_x (prd - tar)^2,   den = sum_h w[h] sum_x tar^2
// with different latitude weights w, finished by a few ops on the (B, C) sums, and
//   d num / d prd[h][x] = 2 w[h] (prd - tar).
//
// Both kernels are HBM streams (606 MB read forward, 606 MB read + 303 MB written
// backward at 1 x 73 x 721 x 1440), so: 16-byte loads / stores on the part of a row where
// every pointer involved is 16-byte aligned (scalar head and tail; a slab with odd
// nlat * nlon moves the alignment from row to row), work units of (bc, chunk of rows)
// on a capped grid (row_geom.h, shared with verify.hip), and no atomics: per-lane fp32 sums of a row's squares, weighted once
// per row, wave + block reduce, one partial per unit into the caller's workspace, combined
// per (b, c) in fp64 in a fixed order by a second kernel.  Every workspace word read is
// written by the same call.
#include "kernels.h"
#include "row_geom.h"

namespace msfno {

size_t loss_workspace_bytes(int BC, int nlat, int nlon) {
  (void)nlon;
  return (size_t)round_up(row_units_bound(BC, nlat) * (int64_t)sizeof(float2), 256);
}

__global__ __launch_bounds__(kRowThreads) void loss_sums_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, float2* __restrict__ part, int nlat, int nlon, int chunks,
    int rows, int64_t units, int lpr) {
  __shared__ float2 red[kRowThreads / 64];
  const int grp = (int)threadIdx.x / lpr, lane = (int)threadIdx.x % lpr;
  const int ngrp = kRowThreads / lpr;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t bc = u / chunks;
    const int h0 = (int)(u - bc * chunks) * rows, h1 = min(nlat, h0 + rows);
    float num = 0.f, den = 0.f;
    for (int h = h0 + grp; h < h1; h += ngrp) {
      const int64_t off = (bc * nlat + h) * (int64_t)nlon;
      const float* p = prd + off;
      const float* t = tar + off;
      float sn = 0.f, sd = 0.f;
      const int a = misalign4(p);
      if (a == misalign4(t)) {
        const int head = min((4 - a) & 3, nlon);
        const int nvec = (nlon - head) >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p + head);
        const float4* t4 = reinterpret_cast<const float4*>(t + head);
        for (int i = lane; i < nvec; i += lpr) {
          const float4 x = p4[i], y = t4[i];
          const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
          sn = fmaf(d0, d0, sn);
          sn = fmaf(d1, d1, sn);
          sn = fmaf(d2, d2, sn);
          sn = fmaf(d3, d3, sn);
          sd = fmaf(y.x, y.x, sd);
          sd = fmaf(y.y, y.y, sd);
          sd = fmaf(y.z, y.z, sd);
          sd = fmaf(y.w, y.w, sd);
        }
        // the up to 3 + 3 elements before and after the aligned part, one lane each
        const int tail0 = head + 4 * nvec;
        if (lane < head + (nlon - tail0)) {
          const int e = lane < head ? lane : tail0 + (lane - head);
          const float y = t[e], d = p[e] - y;
          sn = fmaf(d, d, sn);
          sd = fmaf(y, y, sd);
        }
      } else {
        for (int i = lane; i < nlon; i += lpr) {
          const float y = t[i], d = p[i] - y;
          sn = fmaf(d, d, sn);
          sd = fmaf(y, y, sd);
        }
      }
      const float wh = w_lat[h];
      num = fmaf(wh, sn, num);
      den = fmaf(wh, sd, den);
    }
    for (int o = 32; o > 0; o >>= 1) {
      num += __shfl_down(num, o);
      den += __shfl_down(den, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(num, den);
    __syncthreads();
    if (threadIdx.x == 0) {
      float2 s = red[0];
      for (int k = 1; k < kRowThreads / 64; ++k) {
        s.x += red[k].x;
        s.y += red[k].y;
      }
      part[u] = s;
    }
    __syncthreads();  // red is reused by the next unit
  }
}

// one wave per (b, c): lane l adds the partials l, l + 64, ... in fp64, then a fixed tree
__global__ __launch_bounds__(kRowThreads) void loss_combine_kernel(
    const float2* __restrict__ part, int chunks, int BC, float* __restrict__ sums) {
  const int bc = (int)blockIdx.x * (kRowThreads / 64) + ((int)threadIdx.x >> 6);
  if (bc >= BC) return;
  const int lane = threadIdx.x & 63;
  double n = 0.0, d = 0.0;
  for (int c = lane; c < chunks; c += 64) {
    const float2 v = part[(int64_t)bc * chunks + c];
    n += (double)v.x;
    d += (double)v.y;
  }
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_down(n, o);
    d += __shfl_down(d, o);
  }
  if (lane == 0) {
    sums[2 * (int64_t)bc] = (float)n;
    sums[2 * (int64_t)bc + 1] = (float)d;
  }
}

// dprd = (2 gnum[bc] w[h]) (prd - tar): one rounding each for the coefficient (the
// doubling is exact), the difference and the product
__global__ __launch_bounds__(kRowThreads) void loss_backward_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ gnum, float* __restrict__ dprd,
    int nlat, int nlon, int chunks, int rows, int64_t units, int lpr) {
  const int grp = (int)threadIdx.x / lpr, lane = (int)threadIdx.x % lpr;
  const int ngrp = kRowThreads / lpr;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t bc = u / chunks;
    const int h0 = (int)(u - bc * chunks) * rows, h1 = min(nlat, h0 + rows);
    const float g2 = 2.f * gnum[bc];
    for (int h = h0 + grp; h < h1; h += ngrp) {
      const int64_t off = (bc * nlat + h) * (int64_t)nlon;
      const float* p = prd + off;
      const float* t = tar + off;
      float* o = dprd + off;
      const float c = g2 * w_lat[h];
      const int a = misalign4(p);
      if (a == misalign4(t) && a == misalign4(o)) {
        const int head = min((4 - a) & 3, nlon);
        const int nvec = (nlon - head) >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p + head);
        const float4* t4 = reinterpret_cast<const float4*>(t + head);
        float4* o4 = reinterpret_cast<float4*>(o + head);
        for (int i = lane; i < nvec; i += lpr) {
          const float4 x = p4[i], y = t4[i];
          o4[i] = make_float4(c * (x.x - y.x), c * (x.y - y.y), c * (x.z - y.z),
                              c * (x.w - y.w));
        }
        const int tail0 = head + 4 * nvec;
        if (lane < head + (nlon - tail0)) {
          const int e = lane < head ? lane : tail0 + (lane - head);
          o[e] = c * (p[e] - t[e]);
        }
      } else {
        for (int i = lane; i < nlon; i += lpr) o[i] = c * (p[i] - t[i]);
      }
    }
  }
}

int launch_loss_sums(const float* prd, const float* tar, const float* w_lat, float* sums, int BC,
                     int nlat, int nlon, void* ws, hipStream_t s) {
  const RowGeom g = row_geom(BC, nlat, nlon);
  const int64_t units = (int64_t)BC * g.chunks;
  float2* part = static_cast<float2*>(ws);
  const int blocks = (int)std::min<int64_t>(units, kRowGridCap);
  hipLaunchKernelGGL(loss_sums_kernel, dim3(blocks), dim3(kRowThreads), 0, s, prd, tar, w_lat,
                     part, nlat, nlon, g.chunks, g.rows, units, g.lpr);
  MSFNO_TRY(launch_check("loss_sums"));
  hipLaunchKernelGGL(loss_combine_kernel, dim3((unsigned)cdiv(BC, kRowThreads / 64)),
                     dim3(kRowThreads), 0, s, part, g.chunks, BC, sums);
  return launch_check("loss_combine");
}

int launch_loss_backward(const float* prd, const float* tar, const float* w_lat,
                         const float* gnum, float* dprd, int BC, int nlat, int nlon,
                         hipStream_t s) {
  const RowGeom g = row_geom(BC, nlat, nlon);
  const int64_t units = (int64_t)BC * g.chunks;
  const int blocks = (int)std::min<int64_t>(units, kRowGridCap);
  hipLaunchKernelGGL(loss_backward_kernel, dim3(blocks), dim3(kRowThreads), 0, s, prd, tar,
                     w_lat, gnum, dprd, nlat, nlon, g.chunks, g.rows, units, g.lpr);
  return launch_check("loss_backward");
}

}  // namespace msfno
