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
// (then pa2 = ta2 = cross = +0 exactly): a climatology broadcast over the batch,
// one for some variables only, one per sample.
//
// An HBM stream (606 MB read at 1 x 73 x 721 x 1440, 909 MB with a climatology for every
// slab) on the scaffold of row_reduce.h, with 2 or 3 row pointers in play: this file holds
// the per-pixel arithmetic only.
#include "kernels.h"
#include "row_reduce.h"

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
  row_sweep<false>(
      CLIM ? row_phase(p, t, c) : row_phase(p, t), nlon, lane, lpr,
      [&](int head, int i) ROW_BODY {
        const float4 x = reinterpret_cast<const float4*>(p + head)[i];
        const float4 y = reinterpret_cast<const float4*>(t + head)[i];
        const float4 z = CLIM ? reinterpret_cast<const float4*>(c + head)[i]
                              : make_float4(0.f, 0.f, 0.f, 0.f);
        verify_term<CLIM>(x.x, y.x, z.x, s);
        verify_term<CLIM>(x.y, y.y, z.y, s);
        verify_term<CLIM>(x.z, y.z, z.z, s);
        verify_term<CLIM>(x.w, y.w, z.w, s);
      },
      [&](int e) ROW_BODY { verify_term<CLIM>(p[e], t[e], CLIM ? c[e] : 0.f, s); });
}
}  // namespace

size_t verify_workspace_bytes(int BC, int nlat, int nlon) {
  (void)nlon;
  return row_workspace_bytes(BC, nlat, kNSums);
}

// a slab without a climatology never touches its last three sums: their partials, and with
// them the fp64 sums of the combine, are exact +0
__global__ __launch_bounds__(kRowThreads) void verify_sums_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ clim,
    const int* __restrict__ clim_slab, float* __restrict__ part, RowGeom g) {
  __shared__ float red[kRowWaves][kNSums];
  row_walk<false>(g, [&](int64_t u, int64_t bc, auto rows) ROW_BODY {
    const int cs = clim_slab ? clim_slab[bc] : -1;
    float acc[kNSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      float s[kNSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (cs >= 0)
        verify_row<true>(prd + off, tar + off,
                         clim + ((int64_t)cs * g.nlat + h) * (int64_t)g.nlon, g.nlon, lane,
                         g.lpr, s);
      else
        verify_row<false>(prd + off, tar + off, nullptr, g.nlon, lane, g.lpr, s);
      row_weigh(w_lat[h], s, acc);
    });
    row_block_sum(acc, red, part + u * kNSums);
  });
}

int launch_verify_sums(const float* prd, const float* tar, const float* w_lat, const float* clim,
                       const int* clim_slab, float* sums, int BC, int nlat, int nlon, void* ws,
                       hipStream_t s) {
  const RowGeom g = row_geom(BC, nlat, nlon);
  float* part = static_cast<float*>(ws);
  MSFNO_TRY(row_launch(verify_sums_kernel, "verify_sums", g, s, prd, tar, w_lat, clim, clim_slab,
                       part));
  return row_combine("verify_combine", g, s, part, kNSums, sums, kNSums);
}

}  // namespace msfno
