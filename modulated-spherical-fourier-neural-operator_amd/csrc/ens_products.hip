// Ensemble products and the counts behind the threshold scores.  M members x_i of fp32
// fields, addressed as in ensemble.hip: member i of slab s = (b, c) starts at
// ens + i * member_stride + s * nlat * nlon.  Inputs are finite: the caller's contract, not
// checked (a NaN member has no place in a sorted order, an infinite one no difference).
//
// Products (a row map, every output optional), per pixel, with d_i = x_i - x_0:
//   mean = x_0 + (1/M) sum_i d_i              std = sqrt(sum_i (d_i - dm)^2 / (M - 1)),
//   min, max: members, bit for bit                  dm = (1/M) sum_i d_i (two passes over
//   quant[l] = x_(lo) + frac (x_(hi) - x_(lo))      the registers; 0 for equal members)
//   prob[t] = #{i : x_i > thr[s][t]} (1/M)    strict >
// Difference first, as ensemble.hip: mean and std never see a raw sum of 300 K values.  The
// order statistics x_(0) <= .. <= x_(M-1) come from a compile-time compare-exchange network
// over the MB registers of the member bucket (Batcher's odd-even merge sort: 5, 19, 63, 191
// comparators at MB = 4, 8, 16, 32, one fminf / fmaxf pair each), the members i >= M of the
// bucket padded with +inf, so they sort last.  The host forms (lo, hi, frac) per level in fp64
// with hi = min(lo + 1, M - 1): the clamp keeps the padding out of fmaf(frac, x_(hi) - x_(lo),
// x_(lo)), which is x_(lo) itself where frac == 0.  x_(lo) for the wave-uniform lo is a chain
// of MB uniform selects: nothing indexes the register array at run time.  The network is
// instantiated only where quantiles are wanted; min and max alone are a reduction.  quant and
// prob are dense level-major arrays (one base, one plane stride of S * nlat * nlon).
//
// Threshold counts (a row reduction), per slab s and threshold t, with
// k = #{i : x_i > thr[s][t]} and o = [y > thr[s][t]]:
//   counts[s][t][0][k] = sum w [count == k]        counts[s][t][1][k] = sum w [count == k][o]
// A unit has nt * 2 * (M + 1) <= 528 sums, more than a lane can hold, so each wave keeps an
// integer bin table in LDS: a lane adds 1 to bin (t, o, k) for each of its pixels (an integer
// LDS add gives the same table in any order; no floating-point and no global atomics), and
// after each row lane b folds bins b, b + 64, .. into at most 9 register accumulators, one
// fmaf(w[h], count, acc) per row and bin (the count of (t, 0, k) being the integer sum of
// the table's o = 0 and o = 1 bins: all the pixels with that k), and clears them.  After the unit the waves are
// added in index order into the unit's partial; the chunks are combined in fp64
// (row_combine).  Every word of counts is written by every call.
#include <type_traits>

#include "kernels.h"
#include "row_reduce.h"

namespace msfno {

namespace {
constexpr int kLevels = kEnsMaxLevels;
constexpr int kThrBins = kLevels * 2 * 33;       // bins of a wave's table at M = 32, nt = 8
constexpr int kThrAcc = (kThrBins + 63) / 64;    // of which a lane folds at most 9

__host__ __device__ constexpr int ep_px(int MB) { return MB <= 16 ? 4 : 1; }
// waves per SIMD the kernels are compiled for: a cap on the registers, not the occupancy
// (the full MB = 8 kernels take about 100 and run 4 waves; the predicated one without the
// network spills under a cap of 168)
__host__ __device__ constexpr int ep_waves(int MB) { return MB <= 4 ? 4 : 2; }

// Batcher's odd-even merge sort on N = 2^k inputs as a list of comparators (a < b)
template <int N>
struct SortNet {
  int n = 0;
  unsigned char a[N * 8] = {}, b[N * 8] = {};
  constexpr SortNet() {
    for (int p = 1; p < N; p *= 2)
      for (int k = p; k >= 1; k /= 2)
        for (int j = k % p; j + k < N; j += 2 * k)
          for (int i = 0; i < k && i + j + k < N; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
              a[n] = (unsigned char)(i + j);
              b[n] = (unsigned char)(i + j + k);
              ++n;
            }
  }
};
static_assert(SortNet<4>().n == 5 && SortNet<8>().n == 19 && SortNet<16>().n == 63 &&
                  SortNet<32>().n == 191,
              "Batcher's odd-even merge sort");

template <int C, int MB, int PX, int NP>
__device__ __forceinline__ void ep_sort_from(float (&x)[MB][PX]) {
  constexpr SortNet<MB> net;
  if constexpr (C < net.n) {
    constexpr int a = net.a[C], b = net.b[C];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const float lo = fminf(x[a][k], x[b][k]), hi = fmaxf(x[a][k], x[b][k]);
      x[a][k] = lo;
      x[b][k] = hi;
    }
    ep_sort_from<C + 1, MB, PX, NP>(x);
  }
}

// the M members of the pixels head + 4 v .. + 3, or of the pixel e, of the row at e0; with
// PAD the members M .. MB - 1 of the bucket are +inf
template <int MB, int PX, bool PAD>
__device__ __forceinline__ void ep_load4(const float* __restrict__ e0, int64_t mstride,
                                         int head, int v, int M, float (&x)[MB][PX]) {
#pragma unroll
  for (int i = 0; i < MB; ++i)
    if (i < M) {
      const float4 q = reinterpret_cast<const float4*>(e0 + i * mstride + head)[v];
      x[i][0] = q.x;
      x[i][1 % PX] = q.y;
      x[i][2 % PX] = q.z;
      x[i][3 % PX] = q.w;
    } else if (PAD) {
#pragma unroll
      for (int k = 0; k < PX; ++k) x[i][k] = __builtin_inff();
    }
}

template <int MB, int PX, bool PAD>
__device__ __forceinline__ void ep_load1(const float* __restrict__ e0, int64_t mstride, int e,
                                         int M, float (&x)[MB][PX]) {
#pragma unroll
  for (int i = 0; i < MB; ++i)
    if (i < M)
      x[i][0] = e0[i * mstride + e];
    else if (PAD)
      x[i][0] = __builtin_inff();
}

// The wanted products of the pixels x[.][0 .. NP): st(base, r) stores r[0 .. NP) at the
// pixels' place of the (S, nlat, nlon) array at base.  Sorts x where SORT.
template <int MB, int PX, int NP, bool SORT, class Store>
__device__ __forceinline__ void ep_pixels(float (&x)[MB][PX], int M, float inv_m, float inv_m1,
                                          const EnsProductsOut& o, const float* __restrict__ th,
                                          int nt, const EnsQuantiles& q, int nq, int64_t plane,
                                          Store&& st) {
  // the vector and the scalar path round alike: only the fmas written here
#pragma clang fp contract(off)
  float r[NP];
  if (o.mean || o.std) {
    float dm[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) dm[k] = 0.f;
#pragma unroll
    for (int i = 1; i < MB; ++i)
      if (i < M) {
#pragma unroll
        for (int k = 0; k < NP; ++k) dm[k] += x[i][k] - x[0][k];
      }
#pragma unroll
    for (int k = 0; k < NP; ++k) dm[k] *= inv_m;
    if (o.mean) {
#pragma unroll
      for (int k = 0; k < NP; ++k) r[k] = x[0][k] + dm[k];
      st(o.mean, r);
    }
    if (o.std) {
      // the member 0 has d_0 = 0
#pragma unroll
      for (int k = 0; k < NP; ++k) r[k] = dm[k] * dm[k];
#pragma unroll
      for (int i = 1; i < MB; ++i)
        if (i < M) {
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const float e = (x[i][k] - x[0][k]) - dm[k];
            r[k] = fmaf(e, e, r[k]);
          }
        }
#pragma unroll
      for (int k = 0; k < NP; ++k) r[k] = sqrtf(r[k] * inv_m1);
      st(o.std, r);
    }
  }
  if (o.prob) {
    // one level at a time (here and below): unrolled, the wave-uniform values of all the
    // levels are hoisted out of the row and the scalar registers spill
#pragma nounroll
    for (int t = 0; t < nt; ++t) {
      const float tv = th[t];
      int c[NP];
#pragma unroll
      for (int k = 0; k < NP; ++k) c[k] = 0;
#pragma unroll
      for (int i = 0; i < MB; ++i)
        if (i < M) {
#pragma unroll
          for (int k = 0; k < NP; ++k) c[k] += x[i][k] > tv ? 1 : 0;
        }
#pragma unroll
      for (int k = 0; k < NP; ++k) r[k] = (float)c[k] * inv_m;
      st(o.prob + t * plane, r);
    }
  }
  if (o.mn || o.mx) {
    float lo[NP], hi[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) lo[k] = hi[k] = x[0][k];
#pragma unroll
    for (int i = 1; i < MB; ++i)
      if (i < M) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          lo[k] = fminf(lo[k], x[i][k]);
          hi[k] = fmaxf(hi[k], x[i][k]);
        }
      }
    if (o.mn) st(o.mn, lo);
    if (o.mx) st(o.mx, hi);
  }
  if constexpr (SORT) {
    ep_sort_from<0, MB, PX, NP>(x);
#pragma nounroll
    for (int l = 0; l < nq; ++l) {
      const int lo = q.lo[l], hi = q.hi[l];
      const float fr = q.frac[l];
      float a[NP], b[NP];
#pragma unroll
      for (int k = 0; k < NP; ++k) a[k] = b[k] = x[0][k];
#pragma unroll
      for (int i = 1; i < MB; ++i) {
        const bool sa = lo == i, sb = hi == i;  // wave-uniform
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          a[k] = sa ? x[i][k] : a[k];
          b[k] = sb ? x[i][k] : b[k];
        }
      }
#pragma unroll
      for (int k = 0; k < NP; ++k) r[k] = fmaf(fr, b[k] - a[k], a[k]);
      st(o.quant + l * plane, r);
    }
  }
}

// the wave's LDS traffic so far is visible to all its lanes
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one pixel into the wave's bin table: bin (t, o, k) at t * 2 (M + 1) + o (M + 1) + k, the
// pixels with o = 0 and o = 1 apart
template <int MB, int PX>
__device__ __forceinline__ void thr_pixel(const float (&x)[MB][PX], int k, float y, int M,
                                          const float (&th)[kLevels], int nt, int* bins) {
#pragma unroll
  for (int t = 0; t < kLevels; ++t)
    if (t < nt) {
      int c = 0;
#pragma unroll
      for (int i = 0; i < MB; ++i)
        if (i < M) c += x[i][k] > th[t] ? 1 : 0;
      atomicAdd(&bins[(2 * t + (y > th[t] ? 1 : 0)) * (M + 1) + c], 1);
    }
}

// f(the bucket MB of M members, as a compile-time constant)
template <class F>
int ep_bucket(int M, F&& f) {
  if (M <= 4) return f(std::integral_constant<int, 4>());
  if (M <= 8) return f(std::integral_constant<int, 8>());
  if (M <= 16) return f(std::integral_constant<int, 16>());
  return f(std::integral_constant<int, 32>());
}
}  // namespace

template <int MB, bool SORT, bool FULL>
__global__ __launch_bounds__(kRowThreads, ep_waves(MB)) void ens_products_kernel(
    const float* __restrict__ ens, int64_t mstride, const float* __restrict__ thr, int nt,
    EnsQuantiles q, int nq, EnsProductsOut o, int64_t plane, int m_rt, float inv_m,
    float inv_m1, RowGeom g) {
  constexpr int PX = ep_px(MB);
  const int M = FULL ? MB : m_rt;  // a full bucket: every predicate on M folds
  row_walk<true>(g, [&](int64_t, int64_t s, auto rows) ROW_BODY {
    const float* th = thr + s * nt;  // read where prob is wanted
    rows([&](int, int64_t off, int lane) ROW_BODY {
      const float* e0 = ens + off;
      // an output that is not wanted takes no part in the phase
      auto at = [&](const float* p) ROW_BODY { return p ? p + off : e0; };
      const bool grid = (mstride & 3) == 0 && (!(o.quant || o.prob) || (plane & 3) == 0);
      row_sweep<true>(
          PX == 4 && grid ? row_phase(e0, at(o.mean), at(o.std), at(o.mn), at(o.mx),
                                      at(o.quant), at(o.prob))
                          : -1,
          g.nlon, lane, g.lpr,
          [&](int head, int v) ROW_BODY {
            float x[MB][PX];
            ep_load4<MB, PX, SORT>(e0, mstride, head, v, M, x);
            ep_pixels<MB, PX, PX, SORT>(
                x, M, inv_m, inv_m1, o, th, nt, q, nq, plane,
                [&](float* base, const float (&r)[PX]) ROW_BODY {
                  reinterpret_cast<float4*>(base + off + head)[v] =
                      make_float4(r[0], r[1 % PX], r[2 % PX], r[3 % PX]);
                });
          },
          [&](int e) ROW_BODY {
            float x[MB][PX];
            ep_load1<MB, PX, SORT>(e0, mstride, e, M, x);
            ep_pixels<MB, PX, 1, SORT>(
                x, M, inv_m, inv_m1, o, th, nt, q, nq, plane,
                [&](float* base, const float (&r)[1]) ROW_BODY { base[off + e] = r[0]; });
          });
    });
  });
}

template <int MB, bool FULL>
__global__ __launch_bounds__(kRowThreads, ep_waves(MB)) void ens_threshold_kernel(
    const float* __restrict__ ens, int64_t mstride, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ thr, int nt,
    float* __restrict__ part, int m_rt, RowGeom g) {
  constexpr int PX = ep_px(MB);
  const int M = FULL ? MB : m_rt;
  const int nb = nt * 2 * (M + 1);
  __shared__ int bins[kRowWaves][kThrBins];
  __shared__ float red[kRowWaves][kThrBins];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int wl = (int)threadIdx.x & 63;
  int* mine = bins[wave];
  // the table holds the pixels with o = 0 and with o = 1 apart; a bin of the first row of
  // counts is the (integer) sum of the two
  unsigned both = 0;
#pragma unroll
  for (int j = 0; j < kThrAcc; ++j) {
    if (wl + 64 * j < nb) mine[wl + 64 * j] = 0;
    both |= (unsigned)((wl + 64 * j) % (2 * (M + 1)) < M + 1) << j;
  }
  wave_lds_sync();
  row_walk<true>(g, [&](int64_t u, int64_t s, auto rows) ROW_BODY {
    float th[kLevels];
#pragma unroll
    for (int t = 0; t < kLevels; ++t) th[t] = t < nt ? thr[s * nt + t] : 0.f;
    float acc[kThrAcc];
#pragma unroll
    for (int j = 0; j < kThrAcc; ++j) acc[j] = 0.f;
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      const float* e0 = ens + off;
      const float* t = tar + off;
      row_sweep<true>(
          PX == 4 && (mstride & 3) == 0 ? row_phase(t, e0) : -1, g.nlon, lane, g.lpr,
          [&](int head, int v) ROW_BODY {
            float x[MB][PX];
            ep_load4<MB, PX, false>(e0, mstride, head, v, M, x);
            const float4 y = reinterpret_cast<const float4*>(t + head)[v];
            const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int k = 0; k < PX; ++k) thr_pixel<MB, PX>(x, k, yy[k], M, th, nt, mine);
          },
          [&](int e) ROW_BODY {
            float x[MB][PX];
            ep_load1<MB, PX, false>(e0, mstride, e, M, x);
            thr_pixel<MB, PX>(x, 0, t[e], M, th, nt, mine);
          });
      // the row's counts of this wave, weighed into the lane's bins and cleared
      wave_lds_sync();
      int cnt[kThrAcc];
#pragma unroll
      for (int j = 0; j < kThrAcc; ++j)
        if (wl + 64 * j < nb) {
          cnt[j] = mine[wl + 64 * j];
          if (both >> j & 1) cnt[j] += mine[wl + 64 * j + M + 1];
        }
      wave_lds_sync();  // all read before any is cleared
      const float wh = w_lat[h];
#pragma unroll
      for (int j = 0; j < kThrAcc; ++j)
        if (wl + 64 * j < nb) {
          acc[j] = fmaf(wh, (float)cnt[j], acc[j]);
          mine[wl + 64 * j] = 0;
        }
      wave_lds_sync();
    });
    // the waves in index order; red is reused by the next unit, hence the second barrier
#pragma unroll
    for (int j = 0; j < kThrAcc; ++j)
      if (wl + 64 * j < nb) red[wave][wl + 64 * j] = acc[j];
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kRowThreads) {
      float v = red[0][b];
      for (int w = 1; w < kRowWaves; ++w) v += red[w][b];
      part[u * nb + b] = v;
    }
    __syncthreads();
  });
}

int launch_ens_products(const float* ens, int64_t mstride, const EnsQuantiles& q, int nq,
                        const float* thr, int nt, const EnsProductsOut& out, int M, int S,
                        int nlat, int nlon, hipStream_t s) {
  const RowGeom g = row_geom(S, nlat, nlon);
  const int64_t plane = (int64_t)S * nlat * nlon;
  const bool sort = out.quant != nullptr;
  return ep_bucket(M, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    auto k = sort ? ens_products_kernel<MB, true, false> : ens_products_kernel<MB, false, false>;
    if (M == MB) k = sort ? ens_products_kernel<MB, true, true> : ens_products_kernel<MB, false, true>;
    return row_launch(k, "ens_products", g, s, ens, mstride, thr, out.prob ? nt : 0, q,
                      sort ? nq : 0, out, plane, M, 1.f / (float)M, 1.f / (float)(M - 1));
  });
}

static inline int thr_part_stride(int M, int nt) { return nt * 2 * (M + 1); }

size_t ens_threshold_workspace_bytes(int S, int M, int nt, int nlat) {
  return row_workspace_bytes(S, nlat, thr_part_stride(M, nt));
}

int launch_ens_threshold_sums(const float* ens, int64_t mstride, const float* tar,
                              const float* w_lat, const float* thr, int nt, float* counts,
                              int M, int S, int nlat, int nlon, void* ws, hipStream_t s) {
  const RowGeom g = row_geom(S, nlat, nlon);
  float* part = static_cast<float*>(ws);
  MSFNO_TRY(ep_bucket(M, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    auto k = M == MB ? ens_threshold_kernel<MB, true> : ens_threshold_kernel<MB, false>;
    return row_launch(k, "ens_threshold_sums", g, s, ens, mstride, tar, w_lat, thr, nt, part,
                      M);
  }));
  return row_combine("ens_threshold_combine", g, s, part, thr_part_stride(M, nt), counts,
                     thr_part_stride(M, nt));
}

}  // namespace msfno
