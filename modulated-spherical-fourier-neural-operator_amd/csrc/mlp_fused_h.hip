// Fused block MLP on the "x3h" engine (gfx950): out = W2·GELU(W1·(a ⊙ x1 + t) + b1)
// + b2 + resid, C = 256, H = 512, hidden activation on-chip — the tiling of
// the round-2 MLP re-tiled (16x16x32 MFMAs, 16 pixels per wave, 64 per workgroup, two
// workgroups per CU, x1 straight from global memory into registers) with fp32
// emulated by TWO fp16 terms instead of three bf16 ones:
//
//   v = v0 + v1,  v0 = fp16(v) (RNE), v1 = fp16(v - v0)   (|v - v0 - v1| <= 2^-22 |v|)
//   a·b ~= a1·b0 + a0·b1 + a0·b0     (three fp16 MFMAs, fp32 accumulation; a1·b1 and
//                                     the representation residuals are O(2^-22))
//
// (split_engine.h: split2h, SplitEng<2>; x3h_tile.h: the tile layout and the pipeline's
// steps, shared with mlp_gen_h.hip and skip_h.hip; the split of Ootomo & Yokota, "Recovering
// single precision accuracy from Tensor Cores while surpassing the FP32 theoretical
// peak performance", 2022).  Products of
// fp16 values are exact in fp32, so the only errors beyond an fp32 GEMM's own
// accumulation rounding are the O(2^-22) representation terms; measured against
// fp64 the GEMM error equals that of the fp32-MFMA and x6 engines (DESIGN.md §4,
// tests/test_gpu_x3h.py).  Half the MFMAs of x6 (the x6 kernels sit at the chip's
// sustained bf16 MFMA rate: MFMA-busy × clock is the same for every x6 kernel,
// DESIGN.md §8), two planes instead of three (a third less weight stream and
// register image).
//
// Range: fp16 holds |v| < 65504.  Every operand is scaled by exact powers of two chosen
// from a bound, so nothing overflows whatever the weights or the data:
//   - weights: every W1 row and every row of W2' = W2 · diag(1 / eta) (below) so that
//     its largest entry lies in [2^14, 2^15), undone in fp32 after the contraction;
//   - fc1 input x^ = a ⊙ x1 + t: per field by xi_b = 2^(14 - e), where
//     B_b = max_c abound[b][c] = f 2^e and abound = |a| sqrt(M2) + |a mu + t| >= |x^|
//     (chan_affine, from the norm1 statistics: |x1 - mu| <= sqrt(M2));
//   - hidden h_j = GELU(z_j), |h_j| <= |z_j| <= ||W1_j||_1 B_b + |b1_j|
//     <= L_j (B_b + 1), L_j = max(||W1_j||_1, |b1_j|): h is multiplied by
//     eta_j = 2^-ceil(log2 L_j) (from the weights, folded into W2's columns) and by
//     eta_b = 2^(14 - e'), B_b + 1 = f' 2^e' (per field), so |h'| < 2^14; the output
//     is unscaled by 1 / eta_b with W2's row scales.
// A term far below its bound keeps the bound's absolute precision (2^-38 of it), far
// under the fp32 rounding of the sums it enters.
//
// Slices (the 24-KB bf16x3 slices of mlp_fused.hip become 16 KB):
//   W1(j,kh): hidden rows 32j..+31, channels 128kh..+127: [pl 2][ks 4][t 2][r 16][32]
//   W2(j,oh): out rows 128oh..+127, hidden block j:       [pl 2][ot 8][r 16][32 (perm)]
// ring of four 16-KB slots; image = 64 slices, then the row scales (inverse) of W1
// (512) and W2' (256), then eta (512), as fp32.
#include "kernels.h"
#include "x3h_tile.h"

#include <cstdio>
#include <vector>
#include <type_traits>

namespace msfno {

namespace {

// (MH_C, MH_PLANE, MH_SLICE, MH_NS: x3h_tile.h, shared with skip_h.hip)
constexpr int MH_H = 512;
constexpr int MH_WAVES = 4;
constexpr int MH_HB = MH_H / 32;                    // hidden blocks
constexpr int MH_NSLICE = 4 * MH_HB;                // slices per tile
constexpr int64_t MH_IMG_ELEMS = (int64_t)MH_NSLICE * MH_SLICE;  // before the scales

struct MlpHParams {
  const float* x1;      // [B][C][P]
  const float* scale;   // [B][C]  x1 affine (norm1 + FiLM): a
  const float* shift;   // [B][C]  t
  const float* resid;   // [B][C][P] or null
  float* out;           // [B][C][P]
  const unsigned short* w1img;  // [HB][2 kh] slices
  const unsigned short* w2img;  // [HB][2 oh] slices
  const float* inv_s1;  // [H] 1 / (W1 row scale)
  const float* inv_s2;  // [C] 1 / (W2 row scale)
  const float* eta;     // [H] hidden-row scales eta_j (folded into W2's columns)
  const float* abound;  // [B][C] bound of |a ⊙ x1 + t| per channel
  const float* b1;      // [H]
  const float* b2;      // [C] or null
  int64_t P;
  int tiles_per_field;
  uint64_t* trace;      // MSFNO_MH_TRACE: 5 words per workgroup, or null
};

// (eta_j and the row scales: launch_x3h_eta, launch_x3h_row_scales of mlp_gen_h.hip.  The image
// keeps only the inverse scales, so the writers below take those: 1 / (1 / s) = s, the
// scales being powers of two)
// W1 (H x C fp32) · diag(s1) -> [j][kh][pl][ks][t][r][32]; one thread per pair of columns
__global__ void mh_w1_image_kernel(const float* __restrict__ W1, const float* __restrict__ is1,
                                   unsigned short* __restrict__ img) {
  constexpr int64_t PAIRS = (int64_t)MH_HB * 2 * 4 * 2 * 16 * 16;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < PAIRS;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int kkp = (int)(e & 15);
    const int r = (int)((e >> 4) & 15);
    const int t = (int)((e >> 8) & 1);
    const int ks = (int)((e >> 9) & 3);
    const int kh = (int)((e >> 11) & 1);
    const int j = (int)(e >> 12);
    const int row = 32 * j + 16 * t + r;
    const float* src = W1 + (int64_t)row * MH_C + 128 * kh + 32 * ks + 2 * kkp;
    const float sc = 1.f / is1[row];
    uint32_t t0, t1;
    split2h(src[0] * sc, src[1] * sc, t0, t1);
    uint32_t* o = reinterpret_cast<uint32_t*>(
        img + (int64_t)(j * 2 + kh) * MH_SLICE + x3h_w1_slice_pos(ks, t, r, 2 * kkp));
    o[0] = t0;
    o[MH_PLANE / 2] = t1;
  }
}

// W2' (C x H fp32, W2 diag(1 / eta)) · row scales -> [j][oh][pl][ot][r][32], hidden index
// permuted by mlph_perm; one thread per pair of k positions kap, kap + 1
__global__ void mh_w2_image_kernel(const float* __restrict__ W2, const float* __restrict__ eta,
                                   const float* __restrict__ is2, unsigned short* __restrict__ img) {
  constexpr int64_t PAIRS = (int64_t)MH_HB * 2 * 8 * 16 * 16;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < PAIRS;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int kkp = (int)(e & 15);
    const int r = (int)((e >> 4) & 15);
    const int ot = (int)((e >> 8) & 7);
    const int oh = (int)((e >> 11) & 1);
    const int j = (int)(e >> 12);
    const int kap = 2 * kkp;
    const int orow = 128 * oh + 16 * ot + r;
    const float* row = W2 + (int64_t)orow * MH_H + 32 * j;
    const float* er = eta + 32 * j;
    const float sc = 1.f / is2[orow];
    const int k0 = mlph_perm(kap), k1 = mlph_perm(kap + 1);
    uint32_t t0, t1;
    split2h(row[k0] / er[k0] * sc, row[k1] / er[k1] * sc, t0, t1);
    uint32_t* o = reinterpret_cast<uint32_t*>(
        img + (int64_t)(j * 2 + oh) * MH_SLICE + ot * 512 + x3h_tile_pos(r, kap));
    o[0] = t0;
    o[MH_PLANE / 2] = t1;
  }
}

__device__ __forceinline__ const unsigned short* mh_slice_src(const MlpHParams& p, int q) {
  if (q < 2) return p.w1img + (int64_t)q * MH_SLICE;
  if (q >= MH_NSLICE - 2)
    return p.w2img + (int64_t)(2 * (MH_HB - 1) + (q - (MH_NSLICE - 2))) * MH_SLICE;
  const int j = 1 + ((q - 2) >> 2), r = (q - 2) & 3;
  return r < 2 ? p.w1img + (int64_t)(2 * j + r) * MH_SLICE
               : p.w2img + (int64_t)(2 * (j - 1) + (r - 2)) * MH_SLICE;
}

// The block MLP for one tile of 64 pixels (4 waves of 16; two workgroups per CU).
// Prologue: the weight slices 0..3 go in flight by LDS-DMA; the field's range scalars
// (xi_b from max_c abound, eta_b from B_b + 1) are reduced over the workgroup; x1 of the
// wave's 16 pixels is normalised (a ⊙ x1 + t, times xi_b) and split into fp16x2 B
// fragments kept in registers.  Then 64 slice steps: W1(j, 0..1) into the fc1
// accumulator of block j while block j - 1 is unscaled, + b1, GELU'd, scaled by
// eta_j eta_b and split into fc2's B fragment (in place: mf_perm orders W2's columns),
// W2(j - 1, 0..1) into the 256 x 16 output accumulators.  Epilogue: unscale + b2 +
// residual, one store per output.
constexpr int MH_LDS = MH_NS * MH_SLICE * 2 + (3 * MH_H + 2 * MH_C + 8) * 4;

// BUF: x1, residual and output addressed as raw buffers (32-bit lane offsets, SGPR row
// offsets; the host takes it when a field's C x P fp32 plane is below 2 GB)
template <int AHEAD, bool TRACE, bool BUF, bool ILV = false>
__device__ __forceinline__ void mlp_fused_h_tile(const MlpHParams& p, int lin, char* lds_raw) {
  // AHEAD: A fragments read ahead of the MFMAs (one and three: equal within 1 %)
  static_assert(AHEAD == 2, "only the two-ahead form is instantiated");
  constexpr int W = MH_WAVES, NS = MH_NS;
  constexpr int RING_BYTES = NS * MH_SLICE * 2;
  constexpr int TPX = 16 * W;  // pixels per workgroup tile
  unsigned short* const ring = reinterpret_cast<unsigned short*>(lds_raw);
  float* const b1s = reinterpret_cast<float*>(lds_raw + RING_BYTES);
  float* const is1s = b1s + MH_H;
  float* const hss = is1s + MH_H;  // eta_j eta_b
  float* const b2s = hss + MH_H;   // the epilogue's vectors (no global loads there)
  float* const is2s = b2s + MH_C;
  float* const red = is2s + MH_C;  // per-wave maxima of abound

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int z = lin / p.tiles_per_field;
  uint64_t tr[3] = {0, 0, 0};
  if constexpr (TRACE) tr[0] = __builtin_amdgcn_s_memrealtime();
  const int64_t P = p.P;
  const int64_t px = (int64_t)(lin - z * p.tiles_per_field) * TPX + 16 * wave + r16;

  // ---- slices 0..NS-1 in flight --------------------------------------------------------
  const X3hRing<W, NS> wring(ring, wave, lane);
  auto slice = [&](int q) { return mh_slice_src(p, q); };
#pragma unroll
  for (int q = 0; q < NS; ++q) wring.fill(q, slice(q));

  // ---- x1 loads, the field's bound B_b = max_c abound (thread tid: channel tid) ------
  const int64_t pxc = px < P ? px : P - 1;
  const uint32_t P4 = (uint32_t)(P * 4);
  float xv[8][8];
  if constexpr (BUF) {
    const auto xr = buf_rsrc(p.x1 + (int64_t)z * MH_C * P, (int64_t)MH_C * P * 4);
    const uint32_t vo = (uint32_t)(((int64_t)(8 * g) * P + pxc) * 4);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[ks][e] = buf_ld_nt(xr, vo, (uint32_t)(32 * ks + e) * P4);
  } else {
    const float* xcol = p.x1 + (int64_t)z * MH_C * P + pxc;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        xv[ks][e] = __builtin_nontemporal_load(xcol + (int64_t)(32 * ks + 8 * g + e) * P);
  }
  float bm = p.abound[(int64_t)z * MH_C + tid];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bm = fmaxf(bm, __shfl_xor(bm, o));
  if (lane == 0) red[wave] = bm;
  __syncthreads();  // (also: the first NS slices and the x1 loads landed)
  const float Bb = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const X3hRange rg = x3h_range(Bb);  // |x^ xi| < 2^14, |h eta_j eta_b| < 2^14
  const float xi = rg.xi, etab = rg.eta;

  // ---- normalised x1 -> fp16x2 B fragments (k-step ks: channels 32 ks + 8 g + 0..7) ----
  const float* sc = p.scale + (int64_t)z * MH_C;
  const float* sh = p.shift + (int64_t)z * MH_C;
  half8 xf[8][2];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const int c0 = 32 * ks + 8 * g;
    const float4 sa = *reinterpret_cast<const float4*>(sc + c0);
    const float4 sb = *reinterpret_cast<const float4*>(sc + c0 + 4);
    const float4 ta = *reinterpret_cast<const float4*>(sh + c0);
    const float4 tb = *reinterpret_cast<const float4*>(sh + c0 + 4);
    const float sv[8] = {sa.x * xi, sa.y * xi, sa.z * xi, sa.w * xi,
                         sb.x * xi, sb.y * xi, sb.z * xi, sb.w * xi};
    const float tv[8] = {ta.x * xi, ta.y * xi, ta.z * xi, ta.w * xi,
                         tb.x * xi, tb.y * xi, tb.z * xi, tb.w * xi};
    x3h_split8([&](int e) { return fmaf(sv[e], xv[ks][e], tv[e]); }, xf[ks]);
  }
  floatx4 oacc[16];
#pragma unroll
  for (int ot = 0; ot < 16; ++ot) oacc[ot] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float ixi = rg.ixi, ietab = rg.ieta;
  for (int i = tid; i < MH_H; i += 64 * W) {
    b1s[i] = p.b1[i];
    is1s[i] = p.inv_s1[i] * ixi;
    hss[i] = p.eta[i] * etab;
  }
  for (int i = tid; i < MH_C; i += 64 * W) {
    b2s[i] = p.b2 ? p.b2[i] : 0.f;
    is2s[i] = p.inv_s2[i] * ietab;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if constexpr (TRACE) tr[1] = __builtin_amdgcn_s_memrealtime();

  floatx4 hacc[2][2];  // [parity][tile]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int t = 0; t < 2; ++t) hacc[a][t] = floatx4{0.f, 0.f, 0.f, 0.f};
  uint32_t hfu[2][4];  // fc2 B fragment of the converted block [plane][pair]

  const int a_lane = x3h_a_lane(r16, g);
  auto afrag = [&](const unsigned short* q) -> half8 {
    return *reinterpret_cast<const half8*>(q);
  };

  // step q: slice q landed for every wave (slices up to q + NS - 2 may stay in flight);
  // the slot of slice q - 1 is free and takes slice q + NS - 1
  auto step_begin = [&](int q) { return wring.landed(q, MH_NSLICE); };
  // (the refill stays one burst after the step's first MFMAs: spread over the step as four
  // single pieces it measured 1.964 against 1.970 ms in-block, inside the run-to-run
  // spread, profiles/r09_refill/ab4_table.txt)
  auto refill = [&](int q) { wring.refill(q, MH_NSLICE, slice); };

  // two tiles' products interleaved (no MFMA reads the accumulator its predecessor writes;
  // each accumulator sees the same three products in the same order as SplitEng<2>::mma)
  auto mfma3x2 = [](const half8 (&a)[2], const half8 (&b)[2], floatx4& c,
                    const half8 (&a2)[2], const half8 (&b2)[2], floatx4& c2) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1], b[0], c, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[1], b2[0], c2, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[1], c, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[0], b2[1], c2, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[0], c, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[0], b2[0], c2, 0, 0, 0);
  };
  // ILV: the steps issue tile pairs through mfma3x2 (MLP 1.924 -> 1.905 ms in-block, three
  // interleaved pairs, profiles/r06_p/ab_mfma_pairs.txt; MSFNO_MH_ILV=0 restores the single-tile order)
  constexpr bool ilv = ILV;

  // pair e2 (0..3) of hidden block j in hacc[PAR]: unscale, + b1, GELU(erf), scale, split
  auto conv_pair = [&](int j, int e2, auto par_c) {
    constexpr int PAR = decltype(par_c)::value;
    const int t = e2 >> 1, i = 2 * (e2 & 1);
    const int row = 32 * j + 16 * t + 4 * g + i;
    const float2 b = *reinterpret_cast<const float2*>(b1s + row);
    const float2 is = *reinterpret_cast<const float2*>(is1s + row);
    const float2 hs = *reinterpret_cast<const float2*>(hss + row);
    x3h_hidden_pair(hacc[PAR][t][i], hacc[PAR][t][i + 1], is, 1.f, b, hs, 1.f, hfu[0][e2], hfu[1][e2]);
  };

  // One slice step: the slot's eight A tiles (both planes of tile u at aoff(u, pl)), read
  // AHEAD ahead of their MFMAs, each times the B operand bf(u) into acc(u); the refill
  // behind tile 0's products, after(u) behind tile u's (ILV: behind the pair u, u + 1)
  auto walk = [&](const unsigned short* slot, int q, auto aoff, auto bf, auto acc, auto after) {
    half8 a[AHEAD + 2][2];  // (the pair path rotates over AHEAD + 2)
#pragma unroll
    for (int k = 0; k < AHEAD; ++k)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) a[k][pl] = afrag(slot + aoff(k, pl));
    if constexpr (ilv) {  // tile pairs (u, u + 1): A fragments AHEAD = 2 ahead cover both
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        mfma3x2(a[u % (AHEAD + 2)], bf(u), acc(u), a[(u + 1) % (AHEAD + 2)], bf(u + 1), acc(u + 1));
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (u + k + AHEAD < 8) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
              a[(u + k + AHEAD) % (AHEAD + 2)][pl] = afrag(slot + aoff(u + k + AHEAD, pl));
          }
        if (u == 0) refill(q);
        after(u);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (u + AHEAD < 8) {
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            a[(u + AHEAD) % (AHEAD + 1)][pl] = afrag(slot + aoff(u + AHEAD, pl));
        }
        SplitEng<2>::mma(a[u % (AHEAD + 1)], bf(u), acc(u));
        if (u == 0) refill(q);
        after(u);
      }
    }
  };
  auto fc1_step = [&](const unsigned short* slot, int q, auto kh_c, auto par_c, auto conv_c,
                      int jc) {
    constexpr int KH = decltype(kh_c)::value, PAR = decltype(par_c)::value;
    constexpr bool CONV = decltype(conv_c)::value;
    using PPrev = std::integral_constant<int, PAR ^ 1>;
    walk(
        slot, q, [&](int u, int pl) { return ((pl * 4 + (u >> 1)) * 2 + (u & 1)) * 512 + a_lane; },
        [&](int u) -> const half8(&)[2] { return xf[KH * 4 + (u >> 1)]; },
        [&](int u) -> floatx4& { return hacc[PAR][u & 1]; },
        [&](int u) {
          if constexpr (CONV) {
            if (u == 2 || u == 6) conv_pair(jc, 2 * KH + (u >> 2), PPrev{});
          }
        });
    if constexpr (CONV && KH == 1) {
#pragma unroll
      for (int t = 0; t < 2; ++t) hacc[PAR ^ 1][t] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto fc2_step = [&](const unsigned short* slot, int q, auto oh_c) {
    constexpr int OH = decltype(oh_c)::value;
    half8 hb[2];
    x3h_frags(hfu, hb);
    walk(
        slot, q, [&](int u, int pl) { return (pl * 8 + u) * 512 + a_lane; },
        [&](int) -> const half8(&)[2] { return hb; },
        [&](int u) -> floatx4& { return oacc[OH * 8 + u]; }, [](int) {});
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using F = std::false_type;
  using T = std::true_type;
  auto do_round = [&](int j, auto par_c) {
    const int q = 2 + 4 * (j - 1);
    fc1_step(step_begin(q), q, I0{}, par_c, T{}, j - 1);
    fc1_step(step_begin(q + 1), q + 1, I1{}, par_c, T{}, j - 1);
    fc2_step(step_begin(q + 2), q + 2, I0{});
    fc2_step(step_begin(q + 3), q + 3, I1{});
  };
  fc1_step(step_begin(0), 0, I0{}, I0{}, F{}, 0);
  fc1_step(step_begin(1), 1, I1{}, I0{}, F{}, 0);
  for (int j = 1; j < MH_HB; j += 2) {
    do_round(j, I1{});
    if (j + 1 < MH_HB) do_round(j + 1, I0{});
  }
#pragma unroll
  for (int e2 = 0; e2 < 4; ++e2) conv_pair(MH_HB - 1, e2, I1{});
  // the residual of every output row, all loads in flight at once and under the last
  // two steps' MFMAs (the x1 fragments are dead: their registers take it)
  float rv[16][4];
  if (p.resid && BUF) {
    const auto rr = buf_rsrc(p.resid + (int64_t)z * MH_C * P, (int64_t)MH_C * P * 4);
    const uint32_t vo = (uint32_t)(((int64_t)(4 * g) * P + pxc) * 4);
#pragma unroll
    for (int ot = 0; ot < 16; ++ot)
#pragma unroll
      for (int i = 0; i < 4; ++i) rv[ot][i] = buf_ld_nt(rr, vo, (uint32_t)(16 * ot + i) * P4);
  } else if (p.resid) {
    const float* rs = p.resid + (int64_t)z * MH_C * P + pxc;
#pragma unroll
    for (int ot = 0; ot < 16; ++ot)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        rv[ot][i] = __builtin_nontemporal_load(rs + (int64_t)(16 * ot + 4 * g + i) * P);
  } else {
#pragma unroll
    for (int ot = 0; ot < 16; ++ot)
#pragma unroll
      for (int i = 0; i < 4; ++i) rv[ot][i] = 0.f;
  }
  fc2_step(step_begin(MH_NSLICE - 2), MH_NSLICE - 2, I0{});
  fc2_step(step_begin(MH_NSLICE - 1), MH_NSLICE - 1, I1{});
  if constexpr (TRACE) {
    // diagnostic (MSFNO_MH_TRACE): per workgroup the CU it ran on and the real-time
    // clock (100 MHz) at entry, after the prologue's loads, after the last MFMA step
    // and once its stores are issued
    tr[2] = __builtin_amdgcn_s_memrealtime();
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
    if (tid == 0) {
      uint64_t* t = p.trace + 5 * (int64_t)blockIdx.x;
      t[0] = ((uint64_t)xcc << 32) | hw;
      t[1] = tr[0];
      t[2] = tr[1];
      t[3] = tr[2];
    }
  }

  // ---- epilogue: unscale + b2 + residual, store (rows 16 ot + 4 g + i) ----------------
  if (px >= P) return;
  float* o = p.out + (int64_t)z * MH_C * P + px;
  const auto orr = buf_rsrc(p.out + (int64_t)z * MH_C * P, (int64_t)MH_C * P * 4);
  const uint32_t vo = (uint32_t)(((int64_t)(4 * g) * P + px) * 4);
#pragma unroll
  for (int ot = 0; ot < 16; ++ot) {
    const int r0 = 16 * ot + 4 * g;
    const float4 is = *reinterpret_cast<const float4*>(is2s + r0);
    const float4 b = *reinterpret_cast<const float4*>(b2s + r0);
    const float isv[4] = {is.x, is.y, is.z, is.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = fmaf(oacc[ot][i], isv[i], bv[i]) + rv[ot][i];
      if constexpr (BUF) buf_st_nt(v, orr, vo, (uint32_t)(16 * ot + i) * P4);
      else o[(int64_t)(r0 + i) * P] = v;
    }
  }
  if constexpr (TRACE) {
    if (tid == 0) p.trace[5 * (int64_t)blockIdx.x + 4] = __builtin_amdgcn_s_memrealtime();
  }
}

// TRACE (MSFNO_MH_TRACE, diagnostic): per-workgroup CU id and phase timestamps
template <int AHEAD, bool TRACE, bool BUF, bool ILV = false>
__global__ __launch_bounds__(256, 2) void mlp_fused_h_kernel(MlpHParams p) {
  static_assert(AHEAD == 2, "only the two-ahead form is instantiated");
  __shared__ __attribute__((aligned(16))) char lds_raw[MH_LDS];
  mlp_fused_h_tile<AHEAD, TRACE, BUF, ILV>(p, xcd_remap(blockIdx.x, gridDim.x), lds_raw);
}

}  // namespace

// the x3h engine is the default (measured as accurate as fp32 against fp64, more so
// than x6: tests/test_gpu_x3h.py); MSFNO_ENGINE=x6 selects the six-MFMA bf16 engine
bool mlp_fused_h_env() {
  static const bool on = !sw_eq("MSFNO_ENGINE", "x6");
  return on;
}

size_t mlp_fused_h_image_bytes() {
  return (size_t)MH_IMG_ELEMS * 2 + (size_t)(2 * MH_H + MH_C) * 4;
}

int launch_mlp_fused_h_images(const float* W1, const float* b1, const float* W2,
                              unsigned short* img, hipStream_t s) {
  float* isc = reinterpret_cast<float*>(img + MH_IMG_ELEMS);  // inverse scales: W1's, then W2's
  float* eta = isc + MH_H + MH_C;
  MSFNO_TRY(launch_x3h_eta(W1, b1, MH_H, MH_C, eta, s));
  MSFNO_TRY(launch_x3h_row_scales(W1, W2, eta, MH_H, MH_C, MH_C, MH_C, nullptr, nullptr, isc,
                                  isc + MH_H, s));
  hipLaunchKernelGGL(mh_w1_image_kernel, dim3(256), dim3(256), 0, s, W1, isc, img);
  MSFNO_TRY(launch_check("mh_w1_image"));
  hipLaunchKernelGGL(mh_w2_image_kernel, dim3(256), dim3(256), 0, s, W2, eta, isc + MH_H,
                     img + (int64_t)MH_HB * 2 * MH_SLICE);
  return launch_check("mh_w2_image");
}

int launch_mlp_fused_h(const float* x1, const float* scale, const float* shift,
                       const float* abound, const float* resid, float* out,
                       const unsigned short* img, const float* b1, const float* b2, int B,
                       int64_t P, hipStream_t s) {
  MSFNO_REQUIRE(x1 && scale && shift && abound && out && img && b1 && B > 0 && P >= 1,
                MSFNO_EINVAL, "mlp_fused_h: bad arguments");
  MlpHParams p{};
  p.x1 = x1; p.scale = scale; p.shift = shift; p.resid = resid; p.out = out;
  p.abound = abound;
  p.w1img = img;
  p.w2img = img + (int64_t)MH_HB * 2 * MH_SLICE;
  const float* sc = reinterpret_cast<const float*>(img + MH_IMG_ELEMS);
  p.inv_s1 = sc;
  p.inv_s2 = sc + MH_H;
  p.eta = sc + MH_H + MH_C;
  p.b1 = b1; p.b2 = b2; p.P = P;
  p.tiles_per_field = (int)cdiv(P, 16 * MH_WAVES);
  const int64_t tiles = (int64_t)B * p.tiles_per_field;
  MSFNO_REQUIRE(tiles < (1LL << 31), MSFNO_EINVAL, "mlp_fused_h: grid too large");
  // MSFNO_MH_TRACE=<file> (diagnostic): each launch's per-workgroup CU ids and phase
  // timestamps are appended to <file> (synchronous; tools/mh_trace.py reads it)
  const char* te = sw_raw("MSFNO_MH_TRACE");  // (read on every call)
  if (te && te[0]) {
    uint64_t* tb = nullptr;
    MSFNO_CHECK_HIP(hipMalloc(&tb, (size_t)tiles * 5 * 8));
    MSFNO_CHECK_HIP(hipMemsetAsync(tb, 0, (size_t)tiles * 5 * 8, s));
    p.trace = tb;
    hipLaunchKernelGGL((mlp_fused_h_kernel<2, true, false>), dim3((unsigned)tiles), dim3(64 * MH_WAVES), 0, s, p);
    MSFNO_TRY(launch_check("mlp_fused_h"));
    std::vector<uint64_t> h((size_t)tiles * 5);
    MSFNO_CHECK_HIP(hipMemcpyAsync(h.data(), tb, h.size() * 8, hipMemcpyDeviceToHost, s));
    MSFNO_CHECK_HIP(hipStreamSynchronize(s));
    MSFNO_CHECK_HIP(hipFree(tb));
    if (FILE* f = fopen(te, "ab")) {
      const uint64_t n = (uint64_t)tiles;
      fwrite(&n, 8, 1, f);
      fwrite(h.data(), 8, h.size(), f);
      fclose(f);
    }
    return MSFNO_OK;
  }
  // A fragments read two MFMA triples ahead (one or three: equal within 1 %, profiles/r06_i).
  // MSFNO_MH_BUF=1: raw-buffer addressing of x1 / residual / output (a field's plane below
  // 2 GB).  Not the default: as fast (1.96 ms) but 3.98 instead of 3.36 GB of HBM traffic
  // per launch (profiles/r06_v vs r06_j pmc_traffic.json)
  static const bool buf_env = sw_is1("MSFNO_MH_BUF");
  static const bool ilv_env = sw_on("MSFNO_MH_ILV");
  const bool buf = buf_env && (int64_t)MH_C * P * 4 < (1LL << 31);
  if (buf && ilv_env)
    hipLaunchKernelGGL((mlp_fused_h_kernel<2, false, true, true>), dim3((unsigned)tiles), dim3(64 * MH_WAVES), 0, s, p);
  else if (buf)
    hipLaunchKernelGGL((mlp_fused_h_kernel<2, false, true>), dim3((unsigned)tiles), dim3(64 * MH_WAVES), 0, s, p);
  else if (ilv_env)
    hipLaunchKernelGGL((mlp_fused_h_kernel<2, false, false, true>), dim3((unsigned)tiles), dim3(64 * MH_WAVES), 0, s, p);
  else
    hipLaunchKernelGGL((mlp_fused_h_kernel<2, false, false>), dim3((unsigned)tiles), dim3(64 * MH_WAVES), 0, s, p);
  return launch_check("mlp_fused_h");
}

}  // namespace msfno
