// Separable banded regridding of fp32 fields: conservative remapping, bilinear sampling, block
// means and their adjoints (the Python side is msfno_amd/regrid.py).  Per output slab s with
// source slab src = slab ? slab[s] : s, output row j and output column i:
//   num[s][j][i] = sum_{a < cl[j]} sum_{b < co[i]} wlat[j][a] wlon[i][b] v x[src][r(j,a)][c(i,b)]
//   r(j, a) = clamp(la0[j] + a, 0, nlat_in - 1)       c(i, b) = (lo0[i] + b) mod nlon_in
// cl and co are the table counts cut to [0, taps].  A wrong table therefore gives wrong
// values, never a read outside the slab; the slab list is not range-checked, as in pack.hip.
//   linear       v = 1 and y = num.  Padding taps (a >= count) are never read, so a NaN of x
//                reaches exactly the outputs whose counted taps cover it.
//   normalised   v = mask[r][c] (if a mask is given) * (x == x) (if skip_nan); den is the same
//                sum over v alone; y = num / den where den > 0 and den >= min_valid, else fill.
//                Where v == 0 the value of x is not multiplied in, whatever it is.
//
// Decomposition, on the scaffold of row_reduce.h walked over the OUTPUT rows: a unit is (slab,
// chunk of consecutive output rows) on the capped grid, a row group of lpr lanes (whole waves,
// lpr chosen for the SOURCE row length) takes one output row at a time:
//   latitude stage   the group sweeps the source columns once (row_sweep: a float4 body where
//                    every source row of the band sits on one phase of the 16-byte grid, the
//                    up to 3 + 3 elements around it one lane each, all scalar otherwise) and
//                    sums the cl source rows per column, taps in index order, into an LDS row
//                    in the source column layout (two rows, num and den, when normalised);
//   longitude stage  lane i, i + lpr, ... forms output i from the LDS row, taps in index
//                    order, and writes y coalesced.
// A source row shared by two neighbouring output rows is read by both; the rows of a unit are
// consecutive and its groups work on neighbouring rows at once, so the second read is a cache
// hit.  The order of every sum is fixed and involves one output value only: results do not
// depend on S, on the launch geometry or on the slab's position.  No atomics, no workspace;
// every word of y is written; nothing allocates, synchronises or memsets.
//
// LDS.  ngrp * nbuf * (nlon_in + 4) floats, ngrp = 256 / lpr groups, nbuf = 1 or 2; the 4
// floats of padding let the row start where the float4 body of the sweep is 16-byte aligned in
// LDS too.  The group count is halved until that is at most 64 KiB; one group with two rows
// of kRegridMaxLon = 8188 floats is the limit (the same in both modes).
#include "kernels.h"
#include "row_reduce.h"

namespace msfno {

namespace {
constexpr int kRegridLdsBytes = 64 << 10;

enum : int { kRegridLinear = 0, kRegridSkipNan = 1, kRegridMask = 2 };  // MODE bits

__device__ __forceinline__ int regrid_count(int c, int taps) { return min(max(c, 0), taps); }
}  // namespace

struct RegridArgs {
  const float* x;
  const int* slab;
  const float* mask;
  float* y;
  const int *la0, *lac, *lo0, *loc;
  const float *wlat, *wlon;
  int nlat_in, nlon_in, nlon_out, taps_lat, taps_lon;
  int pitch;  // floats of one LDS row
  float min_valid, fill;
};

template <int MODE>
__global__ __launch_bounds__(kRowThreads) void regrid_kernel(RegridArgs p, RowGeom g) {
  constexpr bool NORM = MODE != kRegridLinear;
  constexpr int NBUF = NORM ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) float regrid_lds[];
  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x / g.lpr);
  const int lane = (int)threadIdx.x % g.lpr;
  const int ngrp = kRowThreads / g.lpr;
  float* const buf = regrid_lds + (size_t)grp * NBUF * p.pitch;
  const int n = p.nlon_in;
  for (int64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const int64_t s = u / g.chunks;
    const int h0 = (int)(u - s * g.chunks) * g.rows, h1 = min(g.nlat, h0 + g.rows);
    const int64_t src = p.slab ? (int64_t)p.slab[s] : s;
    const float* const xs = p.x + src * p.nlat_in * (int64_t)n;
    // every group makes the same number of trips: the barriers are the workgroup's
    for (int hb = h0; hb < h1; hb += ngrp) {
      const int j = hb + grp;
      const bool live = j < h1;
      int sh = 0;  // where the LDS row starts in buf
      if (live) {
        const int r0 = p.la0[j];
        const int cl = regrid_count(p.lac[j], p.taps_lat);
        const float* const wl = p.wlat + (int64_t)j * p.taps_lat;
        auto srow = [&](int a) ROW_BODY {
          return (int64_t)min(max(r0 + a, 0), p.nlat_in - 1) * n;
        };
        // the phase the band's rows share: rows a multiple of 4 floats apart, or one row;
        // the mask's rows lie as far apart, so one comparison covers them
        const float* const x0 = xs + srow(0);
        int ph = (n % 4 == 0 || cl <= 1) ? misalign4(x0) : -1;
        if ((MODE & kRegridMask) && ph >= 0 && misalign4(p.mask + srow(0)) != ph) ph = -1;
        // the LDS row starts where column `head` of the sweep lands on LDS's 16-byte grid
        sh = max(ph, 0);
        float* const num = buf + sh;
        float* const den = num + p.pitch;
        // per column: taps in index order; the first product starts the chain, so a single
        // tap of weight 1 copies the bits
        if constexpr (!NORM) {
          row_sweep<false>(
              ph, n, lane, g.lpr,
              [&](int head, int i) ROW_BODY {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int a = 0; a < cl; ++a) {
                  const float w = wl[a];
                  const float4 v = reinterpret_cast<const float4*>(xs + srow(a) + head)[i];
                  if (a == 0) {
                    acc = make_float4(w * v.x, w * v.y, w * v.z, w * v.w);
                  } else {
                    acc.x = fmaf(w, v.x, acc.x);
                    acc.y = fmaf(w, v.y, acc.y);
                    acc.z = fmaf(w, v.z, acc.z);
                    acc.w = fmaf(w, v.w, acc.w);
                  }
                }
                reinterpret_cast<float4*>(num + head)[i] = acc;
              },
              [&](int e) ROW_BODY {
                float acc = 0.f;
                for (int a = 0; a < cl; ++a) {
                  const float w = wl[a], v = xs[srow(a) + e];
                  acc = a == 0 ? w * v : fmaf(w, v, acc);
                }
                num[e] = acc;
              });
        } else {
          // v and the value it admits
          auto term = [&](float w, float xv, float m, float& an, float& ad) ROW_BODY {
            float v = (MODE & kRegridMask) ? m : 1.f;
            if ((MODE & kRegridSkipNan) && !(xv == xv)) v = 0.f;
            const float wv = w * v;
            an = fmaf(wv, v != 0.f ? xv : 0.f, an);
            ad += wv;
          };
          row_sweep<false>(
              ph, n, lane, g.lpr,
              [&](int head, int i) ROW_BODY {
                float4 an = make_float4(0.f, 0.f, 0.f, 0.f), ad = an;
                for (int a = 0; a < cl; ++a) {
                  const float w = wl[a];
                  const int64_t o = srow(a) + head;
                  const float4 v = reinterpret_cast<const float4*>(xs + o)[i];
                  float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
                  if (MODE & kRegridMask) m = reinterpret_cast<const float4*>(p.mask + o)[i];
                  term(w, v.x, m.x, an.x, ad.x);
                  term(w, v.y, m.y, an.y, ad.y);
                  term(w, v.z, m.z, an.z, ad.z);
                  term(w, v.w, m.w, an.w, ad.w);
                }
                reinterpret_cast<float4*>(num + head)[i] = an;
                reinterpret_cast<float4*>(den + head)[i] = ad;
              },
              [&](int e) ROW_BODY {
                float an = 0.f, ad = 0.f;
                for (int a = 0; a < cl; ++a) {
                  const int64_t o = srow(a) + e;
                  term(wl[a], xs[o], (MODE & kRegridMask) ? p.mask[o] : 1.f, an, ad);
                }
                num[e] = an;
                den[e] = ad;
              });
        }
      }
      __syncthreads();
      if (live) {
        const float* const num = buf + sh;
        const float* const den = num + p.pitch;
        float* const yo = p.y + (s * g.nlat + j) * (int64_t)p.nlon_out;
        for (int i = lane; i < p.nlon_out; i += g.lpr) {
          const int co = regrid_count(p.loc[i], p.taps_lon);
          const float* const wo = p.wlon + (int64_t)i * p.taps_lon;
          int c = p.lo0[i] % n;
          if (c < 0) c += n;
          float an = 0.f, ad = 0.f;
          for (int b = 0; b < co; ++b) {
            const float w = wo[b];
            if constexpr (NORM) {
              an = fmaf(w, num[c], an);
              ad = fmaf(w, den[c], ad);
            } else {
              an = b == 0 ? w * num[c] : fmaf(w, num[c], an);
            }
            if (++c == n) c = 0;
          }
          if constexpr (NORM) an = (ad > 0.f && ad >= p.min_valid) ? an / ad : p.fill;
          yo[i] = an;
        }
      }
      __syncthreads();  // the LDS rows are reused by the next trip
    }
  }
}

int launch_regrid(const float* x, const int* slab, int S_out, const RegridAxis& lat,
                  const RegridAxis& lon, const float* mask, bool skip_nan, float min_valid,
                  float fill, float* y, hipStream_t s) {
  const bool norm = mask || skip_nan;
  const int nbuf = norm ? 2 : 1;
  RegridArgs p;
  p.x = x;
  p.slab = slab;
  p.mask = mask;
  p.y = y;
  p.la0 = lat.start;
  p.lac = lat.count;
  p.lo0 = lon.start;
  p.loc = lon.count;
  p.wlat = lat.w;
  p.wlon = lon.w;
  p.nlat_in = lat.n_in;
  p.nlon_in = lon.n_in;
  p.nlon_out = lon.n_out;
  p.taps_lat = lat.taps;
  p.taps_lon = lon.taps;
  p.pitch = (int)round_up(lon.n_in, 4) + 4;
  p.min_valid = min_valid;
  p.fill = fill;
  // units over the output rows, lanes per row for the source row; fewer, wider groups where
  // the LDS rows of all groups would not fit (a unit's rows stay a multiple of the groups)
  RowGeom g = row_geom(S_out, lat.n_out, lon.n_in);
  auto lds = [&] { return (size_t)(kRowThreads / g.lpr) * nbuf * p.pitch * sizeof(float); };
  while (lds() > (size_t)kRegridLdsBytes && g.lpr < kRowThreads) g.lpr *= 2;
  MSFNO_REQUIRE(lds() <= (size_t)kRegridLdsBytes, MSFNO_EUNSUPPORTED,
                "regrid: the source row does not fit the LDS rows");
  const unsigned blocks = (unsigned)std::min<int64_t>(g.units, kRowGridCap);
  auto go = [&](auto kernel, const char* name) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRowThreads), lds(), s, p, g);
    return launch_check(name);
  };
  if (!norm) return go(regrid_kernel<kRegridLinear>, "regrid");
  if (!mask) return go(regrid_kernel<kRegridSkipNan>, "regrid_skipnan");
  if (!skip_nan) return go(regrid_kernel<kRegridMask>, "regrid_mask");
  return go(regrid_kernel<kRegridSkipNan | kRegridMask>, "regrid_mask_skipnan");
}

}  // namespace msfno
