// Graph-convolution FiLM generator (MSFNO/Models/gcn: GCN_custom, GraphConvolution): the
// sparse aggregation and everything fused into it, the narrow first layer, the pool and
// the head.  The dense K = hidden products are not here: gcn.cpp runs them on gemm_dense.
//
// Layout.  Activations are node-major: row (b, n) of `hid` floats, hid % 4 == 0, so a
// neighbour's row is one contiguous 16-byte aligned stream.  A is CSR with values.
//
// Decomposition (gcn_rows_kernel).  A unit is (sample b, chunk of kGcnRows nodes), one
// workgroup each.  The workgroup is 256 / lpr row groups of lpr lanes, lpr the power of two
// that covers hid / 4 float4 columns (capped at 256: wider rows take several sweeps); a
// group walks its rows of the chunk, a lane owns one float4 column of the row.  A row's
// neighbours are visited in CSR order by every lane, one fmaf each: any degree, and an
// empty row yields the bias alone.
//
// Reduction (the mean pool, the bias gradients).  No atomics.  The order of every sum is
// fixed: per lane over the rows of the chunk it visits, the groups of a workgroup in index
// order through LDS, then per (slab, column) over the chunks in fp64 by row_combine of
// row_reduce.h (a slab is one column: the partials are stored column-major so that the
// combine reads a column's chunks contiguously).  Every partial read is written by the same
// call.
#include "kernels.h"
#include "row_reduce.h"

namespace msfno {
namespace {

constexpr float kGcnSlope = 0.01f;  // nn.LeakyReLU()

enum { GCN_SPMM = 0, GCN_EXPAND = 1, GCN_DP = 2 };

struct GcnRows {
  const int* rp;     // SPMM: CSR of the matrix applied
  const int* ci;
  const float* av;
  const float* X;    // SPMM: the gathered rows; EXPAND: the aggregated input (B N, Fin); DP: dH
  const float* W;    // EXPAND: W0 (Fin, hid)
  const float* bias;   // ACT: b (hid)
  const float* resid;  // ACT: the residual rows, or null
  const float* Pin;    // DP: the pre-activation rows
  float* out;
  float* Pout;  // ACT: the pre-activation rows, or null
  float* part;  // COLSUM: column-major partials
  int N, hid, Fin, lpr, chunks;
  int sum_batch;  // COLSUM: one sum per column over all samples (else per sample)
  int nb;         // samples
};

__device__ __forceinline__ float gcn_leaky(float p) { return p > 0.f ? p : kGcnSlope * p; }
__device__ __forceinline__ void fma4(float w, const float4& x, float4& v) {
  v.x = fmaf(w, x.x, v.x); v.y = fmaf(w, x.y, v.y); v.z = fmaf(w, x.z, v.z); v.w = fmaf(w, x.w, v.w);
}

template <int SRC, bool ACT, bool COLSUM>
__global__ __launch_bounds__(256) void gcn_rows_kernel(GcnRows a) {
  __shared__ float4 red[256];
  const int hid4 = a.hid >> 2;
  const int grp = (int)threadIdx.x / a.lpr, lane = (int)threadIdx.x % a.lpr, ngrp = 256 / a.lpr;
  const int64_t u = blockIdx.x;
  const int b = (int)(u / a.chunks), c = (int)(u - (int64_t)b * a.chunks);
  const int r0 = c * kGcnRows, r1 = min(a.N, r0 + kGcnRows);
  const int64_t base = (int64_t)b * a.N;
  const float4* X4 = reinterpret_cast<const float4*>(a.X);
  // every lane of the workgroup makes the same number of sweeps (the barriers below)
  for (int f0 = 0; f0 < hid4; f0 += a.lpr) {
    const int f = f0 + lane;
    const bool live = f < hid4;
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (ACT) bv = reinterpret_cast<const float4*>(a.bias)[f];
      for (int r = r0 + grp; r < r1; r += ngrp) {
        const int64_t row = base + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (SRC == GCN_SPMM) {
          int e = a.rp[r];
          const int e1 = a.rp[r + 1];
          // four neighbours' loads in flight, added in CSR order
          for (; e + 4 <= e1; e += 4) {
            float w[4];
            float4 x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              w[q] = a.av[e + q];
              x[q] = X4[(base + a.ci[e + q]) * hid4 + f];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) fma4(w[q], x[q], v);
          }
          for (; e < e1; ++e) fma4(a.av[e], X4[(base + a.ci[e]) * hid4 + f], v);
        } else if constexpr (SRC == GCN_EXPAND) {
          for (int k = 0; k < a.Fin; ++k)
            fma4(a.X[row * a.Fin + k], reinterpret_cast<const float4*>(a.W)[(int64_t)k * hid4 + f], v);
        } else {
          const float4 g = X4[row * hid4 + f];
          const float4 p = reinterpret_cast<const float4*>(a.Pin)[row * hid4 + f];
          v = make_float4(p.x > 0.f ? g.x : kGcnSlope * g.x, p.y > 0.f ? g.y : kGcnSlope * g.y,
                          p.z > 0.f ? g.z : kGcnSlope * g.z, p.w > 0.f ? g.w : kGcnSlope * g.w);
        }
        if constexpr (ACT) {
          v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
          if (a.Pout) reinterpret_cast<float4*>(a.Pout)[row * hid4 + f] = v;
          v = make_float4(gcn_leaky(v.x), gcn_leaky(v.y), gcn_leaky(v.z), gcn_leaky(v.w));
          if (a.resid) {
            const float4 h = reinterpret_cast<const float4*>(a.resid)[row * hid4 + f];
            v.x += h.x; v.y += h.y; v.z += h.z; v.w += h.w;
          }
        }
        reinterpret_cast<float4*>(a.out)[row * hid4 + f] = v;
        cs.x += v.x; cs.y += v.y; cs.z += v.z; cs.w += v.w;
      }
    }
    if constexpr (COLSUM) {
      red[threadIdx.x] = cs;
      __syncthreads();
      if (grp == 0 && live) {
        float4 t = red[lane];
        for (int g = 1; g < ngrp; ++g) {
          const float4 o = red[g * a.lpr + lane];
          t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
        }
        // partial of column j: slab (b, j) chunk c, or slab j chunk (b, c)
        const int64_t pch = a.sum_batch ? (int64_t)a.nb * a.chunks : a.chunks;
        const int64_t pc = a.sum_batch ? u : c;
        const int64_t slab0 = (a.sum_batch ? 0 : (int64_t)b * a.hid) + 4 * f;
        a.part[(slab0 + 0) * pch + pc] = t.x;
        a.part[(slab0 + 1) * pch + pc] = t.y;
        a.part[(slab0 + 2) * pch + pc] = t.z;
        a.part[(slab0 + 3) * pch + pc] = t.w;
      }
      __syncthreads();
    }
  }
}

// out[(b, r)][f] = sum_e val[e] x[(b, col[e])][f] for rows of F floats, F small (the first
// layer's input and its gradient): one thread per (row, f), neighbours in CSR order
__global__ __launch_bounds__(256) void gcn_spmm_narrow_kernel(const int* __restrict__ rp,
                                                              const int* __restrict__ ci,
                                                              const float* __restrict__ av,
                                                              const float* __restrict__ x,
                                                              float* __restrict__ out, int nb,
                                                              int N, int F) {
  const int64_t n = (int64_t)nb * N * F;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const int64_t row = i / F;
    const int r = (int)(row % N);
    const int64_t base = row - r;
    float v = 0.f;
    for (int e = rp[r]; e < rp[r + 1]; ++e) v = fmaf(av[e], x[(base + ci[e]) * F + f], v);
    out[i] = v;
  }
}

// dax[row][f] = sum_j dP[row][j] W0[f][j]: a wave per row, the lanes' shares by the shuffle tree
__global__ __launch_bounds__(kRowThreads) void gcn_dax_kernel(const float* __restrict__ dP,
                                                              const float* __restrict__ W0,
                                                              float* __restrict__ dax, int64_t rows,
                                                              int hid, int Fin) {
  const int64_t row = (int64_t)blockIdx.x * kRowWaves + ((int)threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  for (int f = 0; f < Fin; ++f) {
    float s = 0.f;
    for (int j = lane; j < hid; j += 64) s = fmaf(dP[row * hid + j], W0[(int64_t)f * hid + j], s);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) dax[row * Fin + f] = s;
  }
}

// y[b][o] = bh[o] + (1 / N) sum_j poolsum[b][j] Wh[o][j]
__global__ void gcn_head_kernel(const float* __restrict__ poolsum, const float* __restrict__ Wh,
                                const float* __restrict__ bh, float* __restrict__ y, int nb,
                                int hid, int out, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * out) return;
  const int b = i / out, o = i % out;
  double s = 0.0;
  for (int j = 0; j < hid; ++j) s += (double)poolsum[(int64_t)b * hid + j] * (double)Wh[(int64_t)o * hid + j];
  y[i] = (float)((double)bh[o] + s / (double)N);
}

// dpool[b][j] = (1 / N) sum_o dy[b][o] Wh[o][j];  dWh[o][j] = sum_b dy[b][o] poolsum[b][j] / N;
// dbh[o] = sum_b dy[b][o]
__global__ void gcn_head_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ poolsum,
                                    const float* __restrict__ Wh, float* __restrict__ dpool,
                                    float* __restrict__ dWh, float* __restrict__ dbh, int nb,
                                    int hid, int out, int N) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t n0 = (int64_t)nb * hid, n1 = n0 + (int64_t)out * hid;
  const double inv = 1.0 / (double)N;
  if (i < n0) {
    const int b = (int)(i / hid), j = (int)(i % hid);
    double s = 0.0;
    for (int o = 0; o < out; ++o) s += (double)dy[(int64_t)b * out + o] * (double)Wh[(int64_t)o * hid + j];
    dpool[i] = (float)(s * inv);
  } else if (i < n1) {
    const int64_t k = i - n0;
    const int o = (int)(k / hid), j = (int)(k % hid);
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += (double)dy[(int64_t)b * out + o] * (double)poolsum[(int64_t)b * hid + j];
    dWh[k] = (float)(s * inv);
  } else if (i < n1 + out) {
    const int o = (int)(i - n1);
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += (double)dy[(int64_t)b * out + o];
    dbh[o] = (float)s;
  }
}

// dH[(b, n)][:] = dpool[b][:]
__global__ void gcn_bcast_kernel(const float4* __restrict__ dpool, float4* __restrict__ dH, int nb,
                                 int N, int hid4) {
  const int64_t n = (int64_t)nb * N * hid4, per = (int64_t)N * hid4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per;
    dH[i] = dpool[b * hid4 + (i % hid4)];
  }
}

GcnRows rows_args(int nb, int N, int hid) {
  GcnRows a{};
  a.nb = nb; a.N = N; a.hid = hid;
  const int hid4 = hid / 4;
  a.lpr = 1;
  while (a.lpr < hid4 && a.lpr < 256) a.lpr <<= 1;
  a.chunks = gcn_chunks(N);
  return a;
}

template <int SRC, bool ACT>
int rows_launch(const GcnRows& a, const char* name, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.nb * a.chunks));
  if (a.part)
    hipLaunchKernelGGL((gcn_rows_kernel<SRC, ACT, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gcn_rows_kernel<SRC, ACT, false>), grid, dim3(256), 0, s, a);
  return launch_check(name);
}

}  // namespace

int gcn_chunks(int N) { return (int)cdiv(N, kGcnRows); }

size_t gcn_partial_bytes(int nb, int N, int hid) {
  return (size_t)round_up((int64_t)nb * gcn_chunks(N) * hid * (int64_t)sizeof(float), 256);
}

int launch_gcn_aggregate(const int* rp, const int* ci, const float* av, const float* S,
                         const float* bias, const float* resid, float* out, float* Pout,
                         float* part, int nb, int N, int hid, hipStream_t s) {
  GcnRows a = rows_args(nb, N, hid);
  a.rp = rp; a.ci = ci; a.av = av; a.X = S; a.bias = bias; a.resid = resid;
  a.out = out; a.Pout = Pout; a.part = part;
  if (bias) return rows_launch<GCN_SPMM, true>(a, "gcn_aggregate", s);
  return rows_launch<GCN_SPMM, false>(a, "gcn_aggregate_t", s);
}

int launch_gcn_expand(const float* ax, const float* W0, const float* b0, float* out, float* Pout,
                      float* part, int nb, int N, int Fin, int hid, hipStream_t s) {
  GcnRows a = rows_args(nb, N, hid);
  a.X = ax; a.W = W0; a.Fin = Fin; a.bias = b0; a.out = out; a.Pout = Pout; a.part = part;
  return rows_launch<GCN_EXPAND, true>(a, "gcn_expand", s);
}

int launch_gcn_act_grad(const float* dH, const float* P, float* dP, float* part, int nb, int N,
                        int hid, hipStream_t s) {
  GcnRows a = rows_args(nb, N, hid);
  a.X = dH; a.Pin = P; a.out = dP; a.part = part; a.sum_batch = 1;
  return rows_launch<GCN_DP, false>(a, "gcn_act_grad", s);
}

int launch_gcn_colsum_combine(const float* part, float* out, int slabs, int chunks,
                              hipStream_t s) {
  RowGeom g{};
  g.S = slabs;
  g.chunks = chunks;
  return row_combine("gcn_colsum", g, s, part, 1, out, 1);
}

int launch_gcn_spmm_narrow(const int* rp, const int* ci, const float* av, const float* x,
                           float* out, int nb, int N, int F, hipStream_t s) {
  const int64_t n = (int64_t)nb * N * F;
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, 256), 65536);
  hipLaunchKernelGGL(gcn_spmm_narrow_kernel, dim3(blocks), dim3(256), 0, s, rp, ci, av, x, out, nb,
                     N, F);
  return launch_check("gcn_spmm_narrow");
}

int launch_gcn_dax(const float* dP, const float* W0, float* dax, int64_t rows, int hid, int Fin,
                   hipStream_t s) {
  hipLaunchKernelGGL(gcn_dax_kernel, dim3((unsigned)cdiv(rows, kRowWaves)), dim3(kRowThreads), 0, s,
                     dP, W0, dax, rows, hid, Fin);
  return launch_check("gcn_dax");
}

int launch_gcn_head(const float* poolsum, const float* Wh, const float* bh, float* y, int nb,
                    int hid, int out, int N, hipStream_t s) {
  hipLaunchKernelGGL(gcn_head_kernel, dim3((unsigned)cdiv((int64_t)nb * out, 256)), dim3(256), 0, s,
                     poolsum, Wh, bh, y, nb, hid, out, N);
  return launch_check("gcn_head");
}

int launch_gcn_head_bwd(const float* dy, const float* poolsum, const float* Wh, float* dpool,
                        float* dWh, float* dbh, int nb, int hid, int out, int N, hipStream_t s) {
  const int64_t n = (int64_t)nb * hid + (int64_t)out * hid + out;
  hipLaunchKernelGGL(gcn_head_bwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, dy,
                     poolsum, Wh, dpool, dWh, dbh, nb, hid, out, N);
  return launch_check("gcn_head_bwd");
}

int launch_gcn_bcast(const float* dpool, float* dH, int nb, int N, int hid, hipStream_t s) {
  const int64_t n = (int64_t)nb * N * (hid / 4);
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, 256), 65536);
  hipLaunchKernelGGL(gcn_bcast_kernel, dim3(blocks), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(dpool), reinterpret_cast<float4*>(dH), nb, N,
                     hid / 4);
  return launch_check("gcn_bcast");
}

}  // namespace msfno
