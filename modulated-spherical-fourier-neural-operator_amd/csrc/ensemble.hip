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
// Member i of slab s starts at ens + i * member_stride + s * nlat * nlon.  On the scaffold
// of row_reduce.h, with M + 1 (2 M + 1 backward) row pointers in play: they share a phase of
// the 16-byte grid where the member strides are multiples of 4 floats and ens, tar (and
// dens) are in phase.  The members of a pixel sit in registers under a compile-time bound MB
// (buckets 4 / 8 / 16 / 32, predicated on the wave-uniform M); a lane holds 4 pixels of
// them up to MB = 16 and 1 pixel at MB = 32 (4 x 32 would spill), which is VALU-bound
// whatever the load width.
//
// Summation chains.  Per pixel: dbar is M - 1 adds and a product with the rounded 1 / M;
// the pair sums are a sequential chain of M (M - 1) / 2 non-negative terms.  Per lane: one
// add per pixel of its share of a row, then as row_reduce.h has it.  The rank histogram is
// counted in integers: per row, per wave, the population count of the lanes' ballot for
// each rank (exact), then one weighted add per row and rank; the waves' sums are combined
// like the other partials (the scaffold's second group of sums).
#include <type_traits>

#include "kernels.h"
#include "row_reduce.h"

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

// the M members of the pixels head + 4 v .. + 3, or of the pixel e, of the row at e0
template <int MB, int PX>
__device__ __forceinline__ void ens_load4(const float* __restrict__ e0, int64_t mstride,
                                          int head, int v, int M, float (&x)[MB][PX]) {
#pragma unroll
  for (int i = 0; i < MB; ++i)
    if (i < M) {
      const float4 q = reinterpret_cast<const float4*>(e0 + i * mstride + head)[v];
      x[i][0] = q.x;
      x[i][1 % PX] = q.y;
      x[i][2 % PX] = q.z;
      x[i][3 % PX] = q.w;
    }
}

template <int MB, int PX>
__device__ __forceinline__ void ens_load1(const float* __restrict__ e0, int64_t mstride,
                                          int e, int M, float (&x)[MB][PX]) {
#pragma unroll
  for (int i = 0; i < MB; ++i)
    if (i < M) x[i][0] = e0[i * mstride + e];
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
  return row_workspace_bytes(S, nlat, ens_part_stride(M));
}

template <int MB, bool HIST, bool FULL>
__global__ __launch_bounds__(kRowThreads, ens_waves(MB)) void ens_sums_kernel(
    const float* __restrict__ ens, int64_t mstride, const float* __restrict__ tar,
    const float* __restrict__ w_lat, float* __restrict__ part, int m_rt, float inv_m,
    RowGeom g) {
  constexpr int PX = ens_px(MB);
  const int M = FULL ? MB : m_rt;  // a full bucket: every predicate on M folds
  __shared__ float red[kRowWaves][kESums];
  __shared__ float redh[kRowWaves][MB + 1];
  row_walk<true>(g, [&](int64_t u, int64_t, auto rows) ROW_BODY {
    float acc[kESums] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float hacc[MB + 1];
#pragma unroll
    for (int r = 0; r <= MB; ++r) hacc[r] = 0.f;
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      const float* e0 = ens + off;
      const float* t = tar + off;
      float s[kESums] = {0.f, 0.f, 0.f, 0.f, 0.f};
      int cnt[MB + 1];
#pragma unroll
      for (int r = 0; r <= MB; ++r) cnt[r] = 0;
      row_sweep<true>(
          PX == 4 && (mstride & 3) == 0 ? row_phase(t, e0) : -1, g.nlon, lane, g.lpr,
          [&](int head, int v) ROW_BODY {
            float x[MB][PX];
            ens_load4<MB, PX>(e0, mstride, head, v, M, x);
            const float4 y = reinterpret_cast<const float4*>(t + head)[v];
            const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int k = 0; k < PX; ++k) ens_pixel<MB, PX, HIST>(x, k, yy[k], M, inv_m, s, cnt);
          },
          [&](int e) ROW_BODY {
            float x[MB][PX];
            ens_load1<MB, PX>(e0, mstride, e, M, x);
            ens_pixel<MB, PX, HIST>(x, 0, t[e], M, inv_m, s, cnt);
          });
      const float wh = w_lat[h];
      row_weigh(wh, s, acc);
      if (HIST) {
#pragma unroll
        for (int r = 0; r <= MB; ++r)
          if (r <= M) hacc[r] = fmaf(wh, (float)cnt[r], hacc[r]);
      }
    });
    // a wave's first lane takes part in every ballot of the wave (its column index is the
    // lowest), so it holds the wave's whole counts
    row_block_sum<kESums, MB + 1>(acc, red, part + u * (kESums + M + 1), hacc, redh,
                                  HIST ? M + 1 : 0);
  });
}

// dens_i = (w[h] g[s]) (sign(x_i - y) / M - kappa sum_{j != i} sign(x_i - x_j)): one pass
// over the members and the truth
template <int MB, bool FULL>
__global__ __launch_bounds__(kRowThreads, ens_waves(MB)) void ens_crps_backward_kernel(
    const float* __restrict__ ens, int64_t mstride, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ gr, float kappa,
    float* __restrict__ dens, int64_t dstride, int m_rt, float inv_m, RowGeom g) {
  constexpr int PX = ens_px(MB);
  const int M = FULL ? MB : m_rt;
  row_walk<true>(g, [&](int64_t, int64_t bc, auto rows) ROW_BODY {
    const float gs = gr[bc];
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      const float* e0 = ens + off;
      const float* t = tar + off;
      float* o0 = dens + off;
      const float c = gs * w_lat[h];
      row_sweep<true>(
          PX == 4 && ((mstride | dstride) & 3) == 0 ? row_phase(t, e0, o0) : -1, g.nlon, lane,
          g.lpr,
          [&](int head, int v) ROW_BODY {
            float x[MB][PX];
            ens_load4<MB, PX>(e0, mstride, head, v, M, x);
            const float4 y = reinterpret_cast<const float4*>(t + head)[v];
            const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int k = 0; k < PX; ++k) crps_bracket<MB, PX>(x, k, yy[k], M, inv_m, kappa);
#pragma unroll
            for (int i = 0; i < MB; ++i)
              if (i < M)
                reinterpret_cast<float4*>(o0 + i * dstride + head)[v] = make_float4(
                    c * x[i][0], c * x[i][1 % PX], c * x[i][2 % PX], c * x[i][3 % PX]);
          },
          [&](int e) ROW_BODY {
            float x[MB][PX];
            ens_load1<MB, PX>(e0, mstride, e, M, x);
            crps_bracket<MB, PX>(x, 0, t[e], M, inv_m, kappa);
#pragma unroll
            for (int i = 0; i < MB; ++i)
              if (i < M) o0[i * dstride + e] = c * x[i][0];
          });
    });
  });
}

// f(the bucket MB of M members, as a compile-time constant)
template <class F>
static int ens_bucket(int M, F&& f) {
  if (M <= 4) return f(std::integral_constant<int, 4>());
  if (M <= 8) return f(std::integral_constant<int, 8>());
  if (M <= 16) return f(std::integral_constant<int, 16>());
  return f(std::integral_constant<int, 32>());
}

int launch_ens_sums(const float* ens, int64_t mstride, const float* tar, const float* w_lat,
                    float* sums, float* hist, int M, int S, int nlat, int nlon, void* ws,
                    hipStream_t s) {
  const RowGeom g = row_geom(S, nlat, nlon);
  float* part = static_cast<float*>(ws);
  const bool wh = hist != nullptr;
  MSFNO_TRY(ens_bucket(M, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    auto k = wh ? ens_sums_kernel<MB, true, false> : ens_sums_kernel<MB, false, false>;
    if constexpr (ens_has_full(MB)) {
      if (M == MB) k = wh ? ens_sums_kernel<MB, true, true> : ens_sums_kernel<MB, false, true>;
    }
    return row_launch(k, "ens_sums", g, s, ens, mstride, tar, w_lat, part, M, 1.f / (float)M);
  }));
  return row_combine("ens_combine", g, s, part, ens_part_stride(M), sums, kESums, hist,
                     wh ? M + 1 : 0);
}

int launch_ens_crps_backward(const float* ens, int64_t mstride, const float* tar,
                             const float* w_lat, const float* gr, float kappa, float* dens,
                             int64_t dstride, int M, int S, int nlat, int nlon, hipStream_t s) {
  return ens_bucket(M, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    auto k = ens_crps_backward_kernel<MB, false>;
    if constexpr (ens_has_full(MB)) {
      if (M == MB) k = ens_crps_backward_kernel<MB, true>;
    }
    return row_launch(k, "ens_crps_backward", row_geom(S, nlat, nlon), s, ens, mstride, tar,
                      w_lat, gr, kappa, dens, dstride, M, 1.f / (float)M);
  });
}

}  // namespace msfno
