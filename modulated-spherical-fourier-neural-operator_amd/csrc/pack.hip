// 16-bit simple packing of fp32 fields for export (GRIB simple packing, the scale_factor /
// add_offset of netCDF and zarr): a reference value and a binary scale per output slab, taken
// over the selected points only.  Per output slab s, in fp32:
//   lo = min x, hi = max x, d = hi - lo, R = lo
//   E  = 0 where d == 0, else the smallest integer with d <= 65535 * 2^E, at least -126
//   q  = (uint16) rint((x - R) * 2^-E)          round to nearest even, clamped to [0, 65535]
//   xhat = R + (float)q * 2^E                   (decode)
// 65535 * 2^E = (2 - 2^-15) * 2^(E + 15) is exact in fp32, so E follows from the exponent
// field of d and one comparison of its mantissa: no logarithm.  Both products with a power of
// two are exact (ldexpf), so a numpy fp32 restatement gives the same bits.  Inputs are finite
// and so is hi - lo: the caller's contract, not checked.
//
// Selection.  slab[s] is the source slab of output slab s (any order, repeats; null: s
// itself; not range-checked, as clim_slab is not), and a window (lat0, lat_step, lon0,
// lon_step) picks rows and columns of a source slab; the output rows are dense.
//
// Two passes on the scaffold of row_reduce.h, walked over the OUTPUT rows:
//   range   min / max per unit -> partials in the workspace (fminf / fmaxf: any order gives
//           the same bits, so no atomics are needed for two calls to agree); a wave per slab
//           folds the chunks and writes ref and exp2.  The scaffold's own combine sums in
//           fp64, hence this one.
//   pack    reads ref and exp2, writes q.  The q rows are 2-byte elements and dense, so the
//           16-byte phase of a q row moves from row to row with odd nlon_out: the body is cut
//           on the q row's 16-byte grid (8 elements, one 16-byte store), read with two
//           16-byte loads where the source sits on the same grid and with eight 4-byte loads
//           where it does not; the up to 7 + 7 elements before and after take one lane each.
//           lon_step > 1 is an all-scalar path.
// Unpack is one streaming kernel over (slab, block of elements) with the same head / body /
// tail on the 16-byte grid of y.
#include "kernels.h"
#include "row_reduce.h"

namespace msfno {

namespace {
constexpr int kUnpackBlock = 4096;  // elements of a slab one workgroup decodes at a time
constexpr int kUnpackGridCap = 8192;

// E of the range d >= 0 (finite)
__device__ __forceinline__ int pack_exp(float d) {
  if (d == 0.f) return 0;
  const unsigned b = __float_as_uint(d);
  const int be = (int)(b >> 23);  // d >= 0: no sign bit
  // a subnormal d is below 65535 * 2^-126 by far
  if (be == 0) return -126;
  // d = m 2^(be - 127), 1 <= m < 2, against (2 - 2^-15) 2^(E + 15)
  const int e = be - 127 - ((b & 0x7fffffu) <= 0x7fff00u ? 15 : 14);
  return max(e, -126);
}

__device__ __forceinline__ unsigned pack_one(float x, float R, int nE) {
  const float v = rintf(ldexpf(x - R, nE));
  return (unsigned)fminf(fmaxf(v, 0.f), 65535.f);
}

__device__ __forceinline__ unsigned pack_two(float a, float b, float R, int nE) {
  return pack_one(a, R, nE) | (pack_one(b, R, nE) << 16);
}

// the source row of output row h of output slab s
__device__ __forceinline__ const float* pack_row(const float* __restrict__ x,
                                                 const int* __restrict__ slab, const PackWin& w,
                                                 int64_t s, int h) {
  const int64_t src = slab ? (int64_t)slab[s] : s;
  return x + (src * w.nlat + w.lat0 + (int64_t)h * w.lat_step) * (int64_t)w.nlon + w.lon0;
}
}  // namespace

__global__ __launch_bounds__(kRowThreads) void pack16_range_kernel(
    const float* __restrict__ x, const int* __restrict__ slab, PackWin w,
    float* __restrict__ part, RowGeom g) {
  __shared__ float red[kRowWaves][2];
  row_walk<true>(g, [&](int64_t u, int64_t s, auto rows) ROW_BODY {
    float lo = __builtin_inff(), hi = -__builtin_inff();
    auto term = [&](float v) ROW_BODY {
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    };
    rows([&](int h, int64_t, int lane) ROW_BODY {
      const float* p = pack_row(x, slab, w, s, h);
      if (w.lon_step == 1) {
        row_sweep<false>(
            misalign4(p), g.nlon, lane, g.lpr,
            [&](int head, int i) ROW_BODY {
              const float4 v = reinterpret_cast<const float4*>(p + head)[i];
              term(v.x);
              term(v.y);
              term(v.z);
              term(v.w);
            },
            [&](int e) ROW_BODY { term(p[e]); });
      } else {
        row_strided<false>(lane, g.nlon, g.lpr,
                           [&](int e) ROW_BODY { term(p[(int64_t)e * w.lon_step]); });
      }
    });
    // a lane or a wave without an element holds (+inf, -inf); a unit has at least one row
    for (int o = 32; o > 0; o >>= 1) {
      lo = fminf(lo, __shfl_down(lo, o));
      hi = fmaxf(hi, __shfl_down(hi, o));
    }
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6][0] = lo;
      red[threadIdx.x >> 6][1] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < kRowWaves; ++k) {
        lo = fminf(lo, red[k][0]);
        hi = fmaxf(hi, red[k][1]);
      }
      part[u * 2] = lo;
      part[u * 2 + 1] = hi;
    }
    __syncthreads();  // red is reused by the next unit
  });
}

// one wave per slab: the range of its chunks, then ref and exp2
__global__ __launch_bounds__(kRowThreads) void pack16_combine_kernel(
    const float* __restrict__ part, int chunks, int S, float* __restrict__ ref,
    int* __restrict__ exp2) {
  const int s = (int)blockIdx.x * kRowWaves + ((int)threadIdx.x >> 6);
  if (s >= S) return;
  const int lane = threadIdx.x & 63;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int c = lane; c < chunks; c += 64) {
    lo = fminf(lo, part[((int64_t)s * chunks + c) * 2]);
    hi = fmaxf(hi, part[((int64_t)s * chunks + c) * 2 + 1]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o));
    hi = fmaxf(hi, __shfl_down(hi, o));
  }
  if (lane == 0) {
    ref[s] = lo;
    exp2[s] = pack_exp(hi - lo);
  }
}

__global__ __launch_bounds__(kRowThreads) void pack16_kernel(
    const float* __restrict__ x, const int* __restrict__ slab, PackWin w,
    const float* __restrict__ ref, const int* __restrict__ exp2,
    unsigned short* __restrict__ q, RowGeom g) {
  row_walk<true>(g, [&](int64_t, int64_t s, auto rows) ROW_BODY {
    const float R = ref[s];
    const int nE = -exp2[s];
    rows([&](int h, int64_t off, int lane) ROW_BODY {
      const float* p = pack_row(x, slab, w, s, h);
      unsigned short* o = q + off;
      const int n = g.nlon;
      if (w.lon_step != 1) {
        row_strided<false>(lane, n, g.lpr, [&](int e) ROW_BODY {
          o[e] = (unsigned short)pack_one(p[(int64_t)e * w.lon_step], R, nE);
        });
        return;
      }
      // the q row's position on the 16-byte grid, in elements
      const int qa = (int)((reinterpret_cast<uintptr_t>(o) >> 1) & 7);
      const int head = min((8 - qa) & 7, n);
      const int nvec = (n - head) >> 3;
      uint4* o8 = reinterpret_cast<uint4*>(o + head);
      if (misalign4(p + head) == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(p + head);
        row_strided<false>(lane, nvec, g.lpr, [&](int i) ROW_BODY {
          const float4 a = p4[2 * i], b = p4[2 * i + 1];
          o8[i] = make_uint4(pack_two(a.x, a.y, R, nE), pack_two(a.z, a.w, R, nE),
                             pack_two(b.x, b.y, R, nE), pack_two(b.z, b.w, R, nE));
        });
      } else {
        row_strided<false>(lane, nvec, g.lpr, [&](int i) ROW_BODY {
          const float* e = p + head + 8 * i;
          o8[i] = make_uint4(pack_two(e[0], e[1], R, nE), pack_two(e[2], e[3], R, nE),
                             pack_two(e[4], e[5], R, nE), pack_two(e[6], e[7], R, nE));
        });
      }
      // the up to 7 + 7 elements before and after the body, one lane each (lpr >= 64)
      const int tail0 = head + 8 * nvec;
      if (lane < head + (n - tail0)) {
        const int e = lane < head ? lane : tail0 + (lane - head);
        o[e] = (unsigned short)pack_one(p[e], R, nE);
      }
    });
  });
}

__global__ __launch_bounds__(kRowThreads) void unpack16_kernel(
    const unsigned short* __restrict__ q, const float* __restrict__ ref,
    const int* __restrict__ exp2, float* __restrict__ y, int64_t n, int64_t blocks,
    int64_t units) {
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t s = u / blocks;
    const int64_t e0 = (u - s * blocks) * kUnpackBlock;
    const int len = n - e0 < kUnpackBlock ? (int)(n - e0) : kUnpackBlock;
    const float R = ref[s];
    const int E = exp2[s];
    const unsigned short* qi = q + s * n + e0;
    float* yo = y + s * n + e0;
    auto one = [&](int e) ROW_BODY { yo[e] = R + ldexpf((float)qi[e], E); };
    const int head = min((4 - misalign4(yo)) & 3, len);
    if ((reinterpret_cast<uintptr_t>(qi + head) & 7) == 0) {
      const int nvec = (len - head) >> 2;
      const uint2* q4 = reinterpret_cast<const uint2*>(qi + head);
      float4* y4 = reinterpret_cast<float4*>(yo + head);
      for (int i = threadIdx.x; i < nvec; i += kRowThreads) {
        const uint2 v = q4[i];
        y4[i] = make_float4(R + ldexpf((float)(v.x & 0xffffu), E),
                            R + ldexpf((float)(v.x >> 16), E),
                            R + ldexpf((float)(v.y & 0xffffu), E),
                            R + ldexpf((float)(v.y >> 16), E));
      }
      const int tail0 = head + 4 * nvec;
      const int t = threadIdx.x;
      if (t < head + (len - tail0)) one(t < head ? t : tail0 + (t - head));
    } else {
      for (int e = threadIdx.x; e < len; e += kRowThreads) one(e);
    }
  }
}

size_t pack16_workspace_bytes(int S_out, int nlat_out) {
  return row_workspace_bytes(S_out, nlat_out, 2);
}

int launch_pack16(const float* x, const int* slab, const PackWin& w, int S_out, int nlat_out,
                  int nlon_out, float* ref, int* exp2, unsigned short* q, void* ws,
                  hipStream_t s) {
  const RowGeom g = row_geom(S_out, nlat_out, nlon_out);
  float* part = static_cast<float*>(ws);
  MSFNO_TRY(row_launch(pack16_range_kernel, "pack16_range", g, s, x, slab, w, part));
  hipLaunchKernelGGL(pack16_combine_kernel, dim3((unsigned)cdiv(S_out, kRowWaves)),
                     dim3(kRowThreads), 0, s, part, g.chunks, S_out, ref, exp2);
  MSFNO_TRY(launch_check("pack16_combine"));
  // the pack body is 8 elements wide: the lanes per row that suit nlon_out / 8 vectors
  RowGeom gp = row_geom(S_out, nlat_out, std::max(1, nlon_out / 2));
  gp.nlon = nlon_out;
  return row_launch(pack16_kernel, "pack16", gp, s, x, slab, w, (const float*)ref,
                    (const int*)exp2, q);
}

int launch_unpack16(const unsigned short* q, const float* ref, const int* exp2, float* y,
                    int64_t n, int S, hipStream_t s) {
  const int64_t blocks = cdiv(n, kUnpackBlock), units = blocks * S;
  hipLaunchKernelGGL(unpack16_kernel, dim3((unsigned)std::min<int64_t>(units, kUnpackGridCap)),
                     dim3(kRowThreads), 0, s, q, ref, exp2, y, n, blocks, units);
  return launch_check("unpack16");
}

}  // namespace msfno
