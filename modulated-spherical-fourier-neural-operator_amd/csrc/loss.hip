// Sphere-weighted training losses (MSFNO/Models/losses.py: L2Sphere, L2Sphere_noSine,
// CosineMSELoss; the validation MSEs of train.py:553-564).  All of them are, per (b, c),
//   num = sum_h w[h] sum_x (prd - tar)^2,   den = sum_h w[h] sum_x tar^2
// with different latitude weights w, finished by a few ops on the (B, C) sums, and
//   d num / d prd[h][x] = 2 w[h] (prd - tar).
//
// Both kernels are HBM streams (606 MB read forward, 606 MB read + 303 MB written
// backward at 1 x 73 x 721 x 1440) on the scaffold of row_reduce.h: this file holds the
// per-pixel arithmetic only.
#include "kernels.h"
#include "row_reduce.h"

namespace msfno {

namespace {
constexpr int kLSums = 2;

__device__ __forceinline__ void loss_term(float p, float t, float (&s)[kLSums]) {
  const float d = p - t;
  s[0] = fmaf(d, d, s[0]);
  s[1] = fmaf(t, t, s[1]);
}
}  // namespace

size_t loss_workspace_bytes(int BC, int nlat, int nlon) {
  (void)nlon;
  return row_workspace_bytes(BC, nlat, kLSums);
}

__global__ __launch_bounds__(kRowThreads) void loss_sums_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, float* __restrict__ part, RowGeom g) {
  __shared__ float red[kRowWaves][kLSums];
  row_walk<false>(g, [&](int64_t u, int64_t bc, auto rows) ROW_BODY {
    float acc[kLSums] = {0.f, 0.f};
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      const float* p = prd + off;
      const float* t = tar + off;
      float s[kLSums] = {0.f, 0.f};
      row_sweep<false>(
          row_phase(p, t), g.nlon, lane, g.lpr,
          [&](int head, int i) ROW_BODY {
            const float4 x = reinterpret_cast<const float4*>(p + head)[i];
            const float4 y = reinterpret_cast<const float4*>(t + head)[i];
            loss_term(x.x, y.x, s);
            loss_term(x.y, y.y, s);
            loss_term(x.z, y.z, s);
            loss_term(x.w, y.w, s);
          },
          [&](int e) ROW_BODY { loss_term(p[e], t[e], s); });
      row_weigh(w_lat[h], s, acc);
    });
    row_block_sum(acc, red, part + u * kLSums);
  });
}

// dprd = (2 gnum[bc] w[h]) (prd - tar): one rounding each for the coefficient (the
// doubling is exact), the difference and the product
__global__ __launch_bounds__(kRowThreads) void loss_backward_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ gnum, float* __restrict__ dprd,
    RowGeom g) {
  row_walk<false>(g, [&](int64_t, int64_t bc, auto rows) ROW_BODY {
    const float g2 = 2.f * gnum[bc];
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      const float* p = prd + off;
      const float* t = tar + off;
      float* o = dprd + off;
      const float c = g2 * w_lat[h];
      row_sweep<false>(
          row_phase(p, t, o), g.nlon, lane, g.lpr,
          [&](int head, int i) ROW_BODY {
            const float4 x = reinterpret_cast<const float4*>(p + head)[i];
            const float4 y = reinterpret_cast<const float4*>(t + head)[i];
            reinterpret_cast<float4*>(o + head)[i] = make_float4(
                c * (x.x - y.x), c * (x.y - y.y), c * (x.z - y.z), c * (x.w - y.w));
          },
          [&](int e) ROW_BODY { o[e] = c * (p[e] - t[e]); });
    });
  });
}

int launch_loss_sums(const float* prd, const float* tar, const float* w_lat, float* sums, int BC,
                     int nlat, int nlon, void* ws, hipStream_t s) {
  const RowGeom g = row_geom(BC, nlat, nlon);
  float* part = static_cast<float*>(ws);
  MSFNO_TRY(row_launch(loss_sums_kernel, "loss_sums", g, s, prd, tar, w_lat, part));
  return row_combine("loss_combine", g, s, part, kLSums, sums, kLSums);
}

int launch_loss_backward(const float* prd, const float* tar, const float* w_lat,
                         const float* gnum, float* dprd, int BC, int nlat, int nlon,
                         hipStream_t s) {
  return row_launch(loss_backward_kernel, "loss_backward", row_geom(BC, nlat, nlon), s, prd, tar,
                    w_lat, gnum, dprd);
}

}  // namespace msfno
