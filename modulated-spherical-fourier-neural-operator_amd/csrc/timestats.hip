// Statistics over time at fixed pixel: streaming Welford moments of a field or of a forecast
// error, per (slab, pixel), and their pairwise merge.  A state is a uint32 count (S, P) and K
// fp32 planes (K, S, P) with a plane stride; a slab is a flat run of P = nlat * nlon elements
// (no latitude weights here).
//
//   FIELD (x [, c])     a = x - c, or a = x            planes [mean, m2] (+ [lo, hi]: MINMAX)
//   ERROR (p, t [, c])  d = p - t                      planes [mean_d, m2_d, mean_abs]
//                       pa = p - c, ta = t - c         (+ [mean_pa, m2_pa, mean_ta, m2_ta,
//                                                          c_pt]: with a climatology)
//
// Update, per valid update of a pixel, in fp32 with a true division:
//   n += 1
//   delta = a - mean;  mean += delta / (float)n;  m2 = fma(delta, a - mean, m2)   (new mean)
//   mean_abs += (|d| - mean_abs) / n
//   c_pt = fma(pa - mean_pa_old, ta - mean_ta_new, c_pt)
//   lo = fminf(lo, a);  hi = fmaxf(hi, a)
// Every quantity is formed from a difference against the running mean, never from raw sums of
// squares: sum x^2 - (sum x)^2 / n in fp32 is garbage on a 300 K field with 1 K of
// variability.  A thread loads its pixels' state once, applies the B updates in the order
// b = 0 .. B - 1 and stores once.  With skip_nan an update whose x or c (FIELD), t or c (ERROR)
// is NaN is selected out, never multiplied by zero: all of that pixel's words keep their
// bits.  A NaN in p is never skipped.
//
// Merge, dst <- dst (+) src, per flat index over S * P:
//   n = na + nb;  delta = mean_b - mean_a;  f = nb / n
//   mean = fma(delta, f, mean_a);  m2 = fma(delta^2, na f, m2_a + m2_b)
//   c_pt likewise with delta_pa delta_ta;  mean_abs as a mean;  lo by min, hi by max
// where nb == 0 dst keeps its bits, where na == 0 it takes src's.
//
// Addressing (as the unpack kernel of pack.hip).  A unit is (slab, block of kTsBlock elements)
// on a capped grid.  P may be odd, so the 16-byte phase of a slab moves from slab to slab, and
// an input at b * stride, the count or a plane at k * plane_stride need not share the state's
// phase.  The body is cut on the 16-byte grid of plane 0 of the state; every other stream
// takes 16-byte accesses where it sits on that grid and 4-byte ones where it does not (the
// same for all lanes of a unit); the up to 3 + 3 elements before and after the body take one
// lane each.  Both paths run the same per-pixel code, so the bits do not depend on the phase.
// No atomics, no workspace; nothing allocates, synchronises or memsets; the running count
// lives on the device, so a recorded call replays.
#include "kernels.h"
#include "row_reduce.h"

// every multiply-add below is an explicit fmaf: the vector and the one-lane paths then
// round alike
#pragma clang fp contract(off)

namespace msfno {

namespace {
constexpr int kTsBlock = 4096;  // elements of a slab one workgroup updates at a time
constexpr int kTsGridCap = 8192;

template <class T>
struct alignas(16) Quad {
  T v[4];
};

// W elements at p: one 16-byte access where W == 4 and p sits on the grid
template <int W, class T>
__device__ __forceinline__ void ts_load(const T* __restrict__ p, T (&v)[W]) {
  if constexpr (W == 4) {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      const Quad<T> q = *reinterpret_cast<const Quad<T>*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q.v[j];
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) v[j] = p[j];
}

template <int W, class T>
__device__ __forceinline__ void ts_store(T* __restrict__ p, const T (&v)[W]) {
  if constexpr (W == 4) {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      Quad<T> q;
#pragma unroll
      for (int j = 0; j < 4; ++j) q.v[j] = v[j];
      *reinterpret_cast<Quad<T>*>(p) = q;
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) p[j] = v[j];
}

__device__ __forceinline__ bool ts_nan(float v) { return v != v; }

// one Welford step of (mean, m2) with the value a and the new count fn; returns the old mean
__device__ __forceinline__ float ts_welford(float& mean, float& m2, float a, float fn) {
  const float old = mean;
  const float delta = a - old;
  mean = old + delta / fn;
  m2 = fmaf(delta, a - mean, m2);
  return old;
}

// for every unit (slab s, block) of this workgroup: body4(s, e) for the four elements from e
// on of the 16-byte body, body1(s, e) for a head or tail element; e counts within the slab
template <class Body4, class Body1>
__device__ __forceinline__ void ts_walk(const float* __restrict__ plane0, int64_t S, int64_t P,
                                        Body4&& body4, Body1&& body1) {
  const int64_t blocks = (P + kTsBlock - 1) / kTsBlock, units = blocks * S;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t s = u / blocks;
    const int64_t e0 = (u - s * blocks) * kTsBlock;
    const int len = P - e0 < kTsBlock ? (int)(P - e0) : kTsBlock;
    const int head = min((4 - misalign4(plane0 + s * P + e0)) & 3, len);
    const int nvec = (len - head) >> 2;
    for (int i = threadIdx.x; i < nvec; i += kRowThreads) body4(s, e0 + head + 4 * i);
    const int tail0 = head + 4 * nvec;
    const int t = threadIdx.x;
    if (t < head + (len - tail0)) body1(s, e0 + (t < head ? t : tail0 + (t - head)));
  }
}
}  // namespace

// the arguments of one update
struct TsUpdate {
  const float* in0;
  const float* in1;
  int64_t bs0, bs1;  // batch strides, in elements
  const float* clim;
  const int* clim_slab;  // (B, S)
  int B, S;
  int64_t P;
  int skip_nan;
  uint32_t* count;
  float* state;
  int64_t ps;  // plane stride
};

template <int KIND, bool CLIM, bool MM>
struct TsPlanes {
  static constexpr int K = KIND == MSFNO_TSTATS_FIELD ? (MM ? 4 : 2) : (CLIM ? 8 : 3);
};

// W pixels of slab s from element e on: the state once, B updates in order, one store
template <int KIND, bool CLIM, bool MM, int W>
__device__ __forceinline__ void ts_update_at(const TsUpdate& a, int64_t s, int64_t e) {
  constexpr int K = TsPlanes<KIND, CLIM, MM>::K;
  const int64_t o = s * a.P + e;
  uint32_t n[W];
  float pl[K][W];
  ts_load<W>(a.count + o, n);
#pragma unroll
  for (int k = 0; k < K; ++k) ts_load<W>(a.state + k * a.ps + o, pl[k]);
  const bool skip = a.skip_nan != 0;
  for (int b = 0; b < a.B; ++b) {
    float x[W], y[W], c[W];
    ts_load<W>(a.in0 + b * a.bs0 + o, x);
    if constexpr (KIND == MSFNO_TSTATS_ERROR) ts_load<W>(a.in1 + b * a.bs1 + o, y);
    if constexpr (CLIM) {
      const int64_t cs = a.clim_slab[(int64_t)b * a.S + s];
      ts_load<W>(a.clim + cs * a.P + e, c);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint32_t nn = n[j] + 1u;
      const float fn = (float)nn;
      float q[K];
#pragma unroll
      for (int k = 0; k < K; ++k) q[k] = pl[k][j];
      bool ok;
      if constexpr (KIND == MSFNO_TSTATS_FIELD) {
        const float v = CLIM ? x[j] - c[j] : x[j];
        ok = !(skip && (ts_nan(x[j]) || (CLIM && ts_nan(c[j]))));
        ts_welford(q[0], q[1], v, fn);
        if constexpr (MM) {
          q[2] = fminf(q[2], v);
          q[3] = fmaxf(q[3], v);
        }
      } else {
        const float d = x[j] - y[j];
        ok = !(skip && (ts_nan(y[j]) || (CLIM && ts_nan(c[j]))));
        ts_welford(q[0], q[1], d, fn);
        q[2] = q[2] + (fabsf(d) - q[2]) / fn;
        if constexpr (CLIM) {
          const float pa = x[j] - c[j], ta = y[j] - c[j];
          const float pa_old = ts_welford(q[3], q[4], pa, fn);
          ts_welford(q[5], q[6], ta, fn);
          q[7] = fmaf(pa - pa_old, ta - q[5], q[7]);
        }
      }
      // a skipped update is selected out: the words keep their bits
      n[j] = ok ? nn : n[j];
#pragma unroll
      for (int k = 0; k < K; ++k) pl[k][j] = ok ? q[k] : pl[k][j];
    }
  }
  ts_store<W>(a.count + o, n);
#pragma unroll
  for (int k = 0; k < K; ++k) ts_store<W>(a.state + k * a.ps + o, pl[k]);
}

template <int KIND, bool CLIM, bool MM>
__global__ __launch_bounds__(kRowThreads) void tstats_update_kernel(TsUpdate a) {
  ts_walk(
      a.state, a.S, a.P,
      [&](int64_t s, int64_t e) ROW_BODY { ts_update_at<KIND, CLIM, MM, 4>(a, s, e); },
      [&](int64_t s, int64_t e) ROW_BODY { ts_update_at<KIND, CLIM, MM, 1>(a, s, e); });
}

// the arguments of one merge
struct TsMerge {
  uint32_t* dcount;
  float* dstate;
  int64_t dps;
  const uint32_t* scount;
  const float* sstate;
  int64_t sps;
  int64_t N;
};

// (mean, m2) of a and b into a; returns delta = mean_b - mean_a.  f = nb / n, g = na f
__device__ __forceinline__ float ts_merge_moments(float& mean_a, float& m2_a, float mean_b,
                                                  float m2_b, float f, float g) {
  const float delta = mean_b - mean_a;
  mean_a = fmaf(delta, f, mean_a);
  m2_a = fmaf(delta * delta, g, m2_a + m2_b);
  return delta;
}

template <int KIND, bool ANOM, bool MM, int W>
__device__ __forceinline__ void ts_merge_at(const TsMerge& a, int64_t o) {
  constexpr int K = TsPlanes<KIND, ANOM, MM>::K;
  uint32_t na[W], nb[W];
  float pa[K][W], pb[K][W];
  ts_load<W>(a.dcount + o, na);
  ts_load<W>(a.scount + o, nb);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    ts_load<W>(a.dstate + k * a.dps + o, pa[k]);
    ts_load<W>(a.sstate + k * a.sps + o, pb[k]);
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const uint32_t n = na[j] + nb[j];
    // n == 0 only where both are fresh: f is then unused (dst keeps its bits)
    const float f = (float)nb[j] / (float)n;
    const float g = (float)na[j] * f;
    float q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = pa[k][j];
    if constexpr (KIND == MSFNO_TSTATS_FIELD) {
      ts_merge_moments(q[0], q[1], pb[0][j], pb[1][j], f, g);
      if constexpr (MM) {
        q[2] = fminf(q[2], pb[2][j]);
        q[3] = fmaxf(q[3], pb[3][j]);
      }
    } else {
      ts_merge_moments(q[0], q[1], pb[0][j], pb[1][j], f, g);
      q[2] = fmaf(pb[2][j] - q[2], f, q[2]);
      if constexpr (ANOM) {
        const float dpa = ts_merge_moments(q[3], q[4], pb[3][j], pb[4][j], f, g);
        const float dta = ts_merge_moments(q[5], q[6], pb[5][j], pb[6][j], f, g);
        q[7] = fmaf(dpa * dta, g, q[7] + pb[7][j]);
      }
    }
    const bool keep = nb[j] == 0u, take = na[j] == 0u;
    na[j] = n;
#pragma unroll
    for (int k = 0; k < K; ++k) pa[k][j] = keep ? pa[k][j] : (take ? pb[k][j] : q[k]);
  }
  ts_store<W>(a.dcount + o, na);
#pragma unroll
  for (int k = 0; k < K; ++k) ts_store<W>(a.dstate + k * a.dps + o, pa[k]);
}

template <int KIND, bool ANOM, bool MM>
__global__ __launch_bounds__(kRowThreads) void tstats_merge_kernel(TsMerge a) {
  // one "slab" of N elements
  ts_walk(
      a.dstate, 1, a.N,
      [&](int64_t, int64_t e) ROW_BODY { ts_merge_at<KIND, ANOM, MM, 4>(a, e); },
      [&](int64_t, int64_t e) ROW_BODY { ts_merge_at<KIND, ANOM, MM, 1>(a, e); });
}

int tstats_planes(int kind, int flags) {
  if (kind == MSFNO_TSTATS_FIELD && (flags & ~MSFNO_TSTATS_MINMAX) == 0)
    return (flags & MSFNO_TSTATS_MINMAX) ? 4 : 2;
  if (kind == MSFNO_TSTATS_ERROR && (flags & ~MSFNO_TSTATS_ANOM) == 0)
    return (flags & MSFNO_TSTATS_ANOM) ? 8 : 3;
  return 0;
}

namespace {
unsigned ts_grid(int64_t S, int64_t P) {
  return (unsigned)std::min<int64_t>(S * cdiv(P, kTsBlock), kTsGridCap);
}

template <int KIND, bool CLIM, bool MM>
int ts_launch_update(const TsUpdate& a, hipStream_t s) {
  hipLaunchKernelGGL((tstats_update_kernel<KIND, CLIM, MM>), dim3(ts_grid(a.S, a.P)),
                     dim3(kRowThreads), 0, s, a);
  return launch_check("tstats_update");
}

template <int KIND, bool ANOM, bool MM>
int ts_launch_merge(const TsMerge& a, hipStream_t s) {
  hipLaunchKernelGGL((tstats_merge_kernel<KIND, ANOM, MM>), dim3(ts_grid(1, a.N)),
                     dim3(kRowThreads), 0, s, a);
  return launch_check("tstats_merge");
}
}  // namespace

int launch_tstats_update(int kind, int flags, const float* in0, const float* in1, int64_t bs0,
                         int64_t bs1, const float* clim, const int* clim_slab, int B, int S,
                         int64_t P, int skip_nan, uint32_t* count, float* state, int64_t ps,
                         hipStream_t s) {
  const TsUpdate a = {in0, in1, bs0, bs1, clim, clim_slab, B, S, P, skip_nan, count, state, ps};
  constexpr int F = MSFNO_TSTATS_FIELD, E = MSFNO_TSTATS_ERROR;
  if (kind == F) {
    const bool mm = flags & MSFNO_TSTATS_MINMAX;
    if (clim) return mm ? ts_launch_update<F, true, true>(a, s) : ts_launch_update<F, true, false>(a, s);
    return mm ? ts_launch_update<F, false, true>(a, s) : ts_launch_update<F, false, false>(a, s);
  }
  return clim ? ts_launch_update<E, true, false>(a, s) : ts_launch_update<E, false, false>(a, s);
}

int launch_tstats_merge(int kind, int flags, uint32_t* dcount, float* dstate, int64_t dps,
                        const uint32_t* scount, const float* sstate, int64_t sps, int64_t N,
                        hipStream_t s) {
  const TsMerge a = {dcount, dstate, dps, scount, sstate, sps, N};
  constexpr int F = MSFNO_TSTATS_FIELD, E = MSFNO_TSTATS_ERROR;
  if (kind == F)
    return (flags & MSFNO_TSTATS_MINMAX) ? ts_launch_merge<F, false, true>(a, s)
                                         : ts_launch_merge<F, false, false>(a, s);
  return (flags & MSFNO_TSTATS_ANOM) ? ts_launch_merge<E, true, false>(a, s)
                                     : ts_launch_merge<E, false, false>(a, s);
}

}  // namespace msfno
