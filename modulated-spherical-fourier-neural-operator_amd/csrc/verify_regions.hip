// Regional and masked forecast verification: the sums of verify.hip per region, for up to 32
// regions of one grid in one call.  Region r owns pixel (h, x) iff bit r of
//   row_bits[h] & col_bits[x] & pix_bits[h][x]          (pix_bits null: all ones)
// is set, and a pixel is valid (v = 1) unless skip_nan is set and its truth, or the
// climatology of a slab that has one, is NaN.  Per (bc, region) over the region's valid pixels
//   n = sum w v, then se, err, ae, pa2, ta2, cross as in verify.hip.
//
// Select, never multiply: a pixel that is out or skipped contributes d = p - c = t - c = 0
// by a select, so a NaN or Inf outside a region never reaches its sums (0 * NaN would).  The
// terms then go through the lines of verify.hip's verify_term in the same order, and
// fmaf(0, 0, s) = s + 0 = s: a region of all ones has bitwise the six sums of
// msfno_verify_sums, a region's sums depend on its own valid pixels only, and a missing
// truth and a cleared pix_bits bit give the same bits.  For that the lane shares of a row
// are those of verify.hip too: the float4 body where prd, tar (and clim) share a phase of the
// 16-byte grid, whatever the phase of the bit tables; the tables ride the body as 16-byte
// loads where they sit on that phase, and as four scalar loads where not.
//
// 7 G accumulators per lane and row for a group of G <= 8 regions, as many again per unit:
// the host launches one pass per group of 8 regions with the bits shifted down, every pass
// writes its own columns of the units' partials, and one combine follows.  A pass skips the
// rows that none of its regions owns (row_bits is wave-uniform): no loads, contribution +0.
#include "kernels.h"
#include "row_reduce.h"

namespace msfno {

namespace {
constexpr int kRSums = 7;  // n and the six of verify.hip
constexpr int kGroup = 8;  // regions per pass

__device__ __forceinline__ int bits_phase(const uint32_t* p) {
  return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
}

// one pixel into the sums of the G regions of bits m (bit r: in region r and valid)
template <bool CLIM, int G>
__device__ __forceinline__ void region_term(float p, float t, float c, uint32_t m,
                                            float (&s)[kRSums * G]) {
  const float d = p - t;
  const float a = CLIM ? p - c : 0.f, b = CLIM ? t - c : 0.f;
#pragma unroll
  for (int r = 0; r < G; ++r) {
    const bool in = (m >> r) & 1u;
    const float dr = in ? d : 0.f;
    s[kRSums * r + 0] += in ? 1.f : 0.f;
    s[kRSums * r + 1] = fmaf(dr, dr, s[kRSums * r + 1]);
    s[kRSums * r + 2] += dr;
    s[kRSums * r + 3] += fabsf(dr);
    if (CLIM) {
      const float ar = in ? a : 0.f, br = in ? b : 0.f;
      s[kRSums * r + 4] = fmaf(ar, ar, s[kRSums * r + 4]);
      s[kRSums * r + 5] = fmaf(br, br, s[kRSums * r + 5]);
      s[kRSums * r + 6] = fmaf(ar, br, s[kRSums * r + 6]);
    }
  }
}

// the row's bits of the pass
struct RowBits {
  const uint32_t* col;  // col_bits
  const uint32_t* pix;  // pix_bits + h * nlon, or null
  uint32_t rb;          // the row's bits of the group, shifted down
  int shift;            // first region of the group
  bool skip;            // skip_nan
};

// the group's bits of a pixel with table bits m: none where the pixel is skipped
template <bool CLIM>
__device__ __forceinline__ uint32_t pixel_bits(const RowBits& q, uint32_t m, float t, float c) {
  const bool missing = q.skip && (t != t || (CLIM && c != c));
  return missing ? 0u : ((m >> q.shift) & q.rb);
}

// the sums of one row over the lanes of a row group (c is not read unless CLIM)
template <bool CLIM, int G>
__device__ __forceinline__ void region_row(const float* __restrict__ p,
                                           const float* __restrict__ t,
                                           const float* __restrict__ c, const RowBits& q,
                                           int nlon, int lane, int lpr,
                                           float (&s)[kRSums * G]) {
  const int a = CLIM ? row_phase(p, t, c) : row_phase(p, t);
  const bool bvec = bits_phase(q.col) == a && (!q.pix || bits_phase(q.pix) == a);
  row_sweep<(G > 2)>(
      a, nlon, lane, lpr,
      [&](int head, int i) ROW_BODY {
        const float4 x = reinterpret_cast<const float4*>(p + head)[i];
        const float4 y = reinterpret_cast<const float4*>(t + head)[i];
        const float4 z = CLIM ? reinterpret_cast<const float4*>(c + head)[i]
                              : make_float4(0.f, 0.f, 0.f, 0.f);
        uint4 m;
        if (bvec) {
          m = reinterpret_cast<const uint4*>(q.col + head)[i];
          if (q.pix) {
            const uint4 k = reinterpret_cast<const uint4*>(q.pix + head)[i];
            m.x &= k.x, m.y &= k.y, m.z &= k.z, m.w &= k.w;
          }
        } else {
          const int e = head + 4 * i;
          m = make_uint4(q.col[e], q.col[e + 1], q.col[e + 2], q.col[e + 3]);
          if (q.pix) m.x &= q.pix[e], m.y &= q.pix[e + 1], m.z &= q.pix[e + 2], m.w &= q.pix[e + 3];
        }
        region_term<CLIM, G>(x.x, y.x, z.x, pixel_bits<CLIM>(q, m.x, y.x, z.x), s);
        region_term<CLIM, G>(x.y, y.y, z.y, pixel_bits<CLIM>(q, m.y, y.y, z.y), s);
        region_term<CLIM, G>(x.z, y.z, z.z, pixel_bits<CLIM>(q, m.z, y.z, z.z), s);
        region_term<CLIM, G>(x.w, y.w, z.w, pixel_bits<CLIM>(q, m.w, y.w, z.w), s);
      },
      [&](int e) ROW_BODY {
        const float te = t[e], ce = CLIM ? c[e] : 0.f;
        const uint32_t m = q.pix ? (q.col[e] & q.pix[e]) : q.col[e];
        region_term<CLIM, G>(p[e], te, ce, pixel_bits<CLIM>(q, m, te, ce), s);
      });
}

// One pass: the regions shift .. shift + G of every unit into the columns
// kRSums * shift .. kRSums * (shift + G) of its partial (pstride floats per unit).  gmask
// has the bits of the group's regions that exist; the others get +0.  A slab without a
// climatology never touches its last three sums, as in verify.hip.
template <int G>
__global__ __launch_bounds__(kRowThreads) void verify_regions_kernel(
    const float* __restrict__ prd, const float* __restrict__ tar,
    const float* __restrict__ w_lat, const float* __restrict__ clim,
    const int* __restrict__ clim_slab, const uint32_t* __restrict__ row_bits,
    const uint32_t* __restrict__ col_bits, const uint32_t* __restrict__ pix_bits, int shift,
    uint32_t gmask, int skip_nan, float* __restrict__ part, int pstride, RowGeom g) {
  __shared__ float red[kRowWaves][kRSums * G];
  row_walk<true>(g, [&](int64_t u, int64_t bc, auto rows) ROW_BODY {
    const int cs = clim_slab ? clim_slab[bc] : -1;
    float acc[kRSums * G];
#pragma unroll
    for (int k = 0; k < kRSums * G; ++k) acc[k] = 0.f;
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      RowBits q;
      q.rb = (row_bits[h] >> shift) & gmask;
      if (q.rb == 0u) return;  // wave-uniform: no region of the group owns the row
      const int64_t roff = (int64_t)h * g.nlon;
      q.col = col_bits;
      q.pix = pix_bits ? pix_bits + roff : nullptr;
      q.shift = shift;
      q.skip = skip_nan != 0;
      float s[kRSums * G];
#pragma unroll
      for (int k = 0; k < kRSums * G; ++k) s[k] = 0.f;
      if (cs >= 0)
        region_row<true, G>(prd + off, tar + off, clim + (int64_t)cs * g.nlat * g.nlon + roff,
                            q, g.nlon, lane, g.lpr, s);
      else
        region_row<false, G>(prd + off, tar + off, nullptr, q, g.nlon, lane, g.lpr, s);
      row_weigh(w_lat[h], s, acc);
    });
    row_block_sum(acc, red, part + u * pstride + kRSums * shift);
  });
}

// Step 5 of row_reduce.h with one wave per (slab, region): the operations of
// row_combine_kernel on each of the region's seven sums
__global__ __launch_bounds__(kRowThreads) void verify_regions_combine_kernel(
    const float* __restrict__ part, int pstride, int chunks, int64_t SR, int R,
    float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  for (int64_t v0 = (int64_t)blockIdx.x * kRowWaves + ((int)threadIdx.x >> 6); v0 < SR;
       v0 += (int64_t)gridDim.x * kRowWaves) {
    const int64_t s = v0 / R;
    const int r = (int)(v0 - s * R);
    for (int k = 0; k < kRSums; ++k) {
      double v = 0.0;
      for (int c = lane; c < chunks; c += 64)
        v += (double)part[(s * chunks + c) * pstride + kRSums * r + k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
      if (lane == 0) sums[v0 * kRSums + k] = (float)v;
    }
  }
}

int regions_pstride(int nregions) { return kRSums * (int)round_up(nregions, kGroup); }

template <int G>
int launch_pass(const float* prd, const float* tar, const float* w_lat, const float* clim,
                const int* clim_slab, const uint32_t* row_bits, const uint32_t* col_bits,
                const uint32_t* pix_bits, int shift, int count, int skip_nan, float* part,
                int pstride, const RowGeom& g, hipStream_t s) {
  const uint32_t gmask = count >= 32 ? 0xffffffffu : ((1u << count) - 1u);
  return row_launch(verify_regions_kernel<G>, "verify_regions", g, s, prd, tar, w_lat, clim,
                    clim_slab, row_bits, col_bits, pix_bits, shift, gmask, skip_nan, part,
                    pstride);
}
}  // namespace

size_t verify_regions_workspace_bytes(int BC, int nlat, int nlon, int nregions) {
  (void)nlon;
  return row_workspace_bytes(BC, nlat, regions_pstride(nregions));
}

int launch_verify_region_sums(const float* prd, const float* tar, const float* w_lat,
                              const float* clim, const int* clim_slab, const uint32_t* row_bits,
                              const uint32_t* col_bits, const uint32_t* pix_bits, int nregions,
                              int skip_nan, float* sums, int BC, int nlat, int nlon, void* ws,
                              hipStream_t s) {
  const RowGeom g = row_geom(BC, nlat, nlon);
  float* part = static_cast<float*>(ws);
  const int pstride = regions_pstride(nregions);
  for (int shift = 0; shift < nregions; shift += kGroup) {
    const int count = std::min(kGroup, nregions - shift);
#define MSFNO_REGION_PASS(G)                                                                 \
  MSFNO_TRY(launch_pass<G>(prd, tar, w_lat, clim, clim_slab, row_bits, col_bits, pix_bits,  \
                           shift, count, skip_nan, part, pstride, g, s))
    if (count <= 1)
      MSFNO_REGION_PASS(1);
    else if (count <= 2)
      MSFNO_REGION_PASS(2);
    else if (count <= 4)
      MSFNO_REGION_PASS(4);
    else
      MSFNO_REGION_PASS(8);
#undef MSFNO_REGION_PASS
  }
  const int64_t SR = (int64_t)BC * nregions;
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(SR, kRowWaves), 1 << 16);
  hipLaunchKernelGGL(verify_regions_combine_kernel, dim3(blocks), dim3(kRowThreads), 0, s, part,
                     pstride, g.chunks, SR, nregions, sums);
  return launch_check("verify_regions_combine");
}

}  // namespace msfno
