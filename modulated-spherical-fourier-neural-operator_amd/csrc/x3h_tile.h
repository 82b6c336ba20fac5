// The tile pipeline of the x3h MLP kernels (mlp_fused_h.hip, mlp_gen_h.hip, skip_h.hip): 16
// pixels per wave, 16x16x32 fp16 MFMAs through SplitEng<2> (split_engine.h has the engine
// and its error bound), 16-row x 32-k weight tiles, 16-KB slices of them through a four-slot
// LDS ring filled by LDS-DMA, x split into fp16 pairs in registers, a hidden block unscaled,
// GELU'd, rescaled and split in place.  Each step the three units share is defined here,
// once; what differs between them (widths, the unit order of the slices, the epilogues, the
// persistent kernels' own DMA groups) stays in the units.
#pragma once
#include "dma.h"
#include "gemm_common.h"

namespace msfno {

// ---- tile layout -----------------------------------------------------------------------
// The weight tile: 16 rows x 32 k fp16, the four 16-B k-groups of row r XORed with
// mlph_swz(r) (conflict-free ds_read_b128 fragments); mlph_perm: the hidden row within a
// block of 32 that fc2's k position kappa reads (the C layout of the fc1 accumulators is
// fc2's B fragment in place)
__host__ __device__ __forceinline__ int mlph_swz(int r) { return ((r >> 2) & 1) << 1; }
__host__ __device__ __forceinline__ int mlph_perm(int kappa) {
  const int g = kappa >> 3, e = kappa & 7;
  return e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4);
}
// stored position (fp16 index within one plane of the tile) of row r, column k; the
// swizzle is an XOR, so it is also the column that position k of the row holds
__host__ __device__ __forceinline__ int x3h_tile_pos(int r, int k) {
  return r * 32 + 8 * ((k >> 3) ^ mlph_swz(r)) + (k & 7);
}
// a lane's A fragment of a tile, x3h_tile_pos(r16, 8 g): row r16 = lane & 15, the 8 columns
// of k-group g = lane >> 4 (spelled out, and taking the kernel's own r16 and g: through
// x3h_tile_pos, or from the lane index, the kernels' register allocation changed)
__device__ __forceinline__ int x3h_a_lane(int r16, int g) { return r16 * 32 + 8 * (g ^ mlph_swz(r16)); }

// The 16-KB fp16 weight slice built from those tiles and the depth of the LDS ring it streams
// through; MH_C: the width of the block MLP (mlp_fused_h.hip) and the inner skip (skip_h.hip)
constexpr int MH_C = 256;
constexpr int MH_PLANE = 4096;          // fp16 per plane within a slice
constexpr int MH_SLICE = 2 * MH_PLANE;  // fp16 per 16-KB slice
constexpr int MH_NS = 4;                // ring slots
// stored position of (row r16 of tile (ks, t), column kk) in plane 0 of a W1 slice
// [pl 2][ks 4][t 2][r 16][32]: 32 rows of one hidden / output block, 128 channels
__host__ __device__ __forceinline__ int x3h_w1_slice_pos(int ks, int t, int r16, int kk) {
  return (ks * 2 + t) * 512 + x3h_tile_pos(r16, kk);
}

// ---- fragments ---------------------------------------------------------------------------
// an MFMA operand's two half8 terms from its packed pairs [plane][pair]
__device__ __forceinline__ void x3h_frags(const uint32_t (&t)[2][4], half8 (&f)[2]) {
#pragma unroll
  for (int pl = 0; pl < 2; ++pl) f[pl] = frag_cast<half8>(t[pl][0], t[pl][1], t[pl][2], t[pl][3]);
}
// val(0..7), a lane's 8 fp32 of a k-step -> the two half8 terms of the MFMA operand
template <class Val>
__device__ __forceinline__ void x3h_split8(Val&& val, half8 (&f)[2]) {
  uint32_t t[2][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split2h(val(2 * e), val(2 * e + 1), t[0][e], t[1][e]);
  x3h_frags(t, f);
}

// ---- range -------------------------------------------------------------------------------
// a pixel's maximum over the four lanes that hold it (lane & 15 equal)
__device__ __forceinline__ float x3h_pixel_max(float m) {
  m = fmaxf(m, __shfl_xor(m, 16));
  return fmaxf(m, __shfl_xor(m, 32));
}
// the range scalars from a bound m of |x|: |x xi| < 2^14, |h eta_j eta| < 2^14 (|h_j| <=
// L_j (m + 1), the top of mlp_fused_h.hip), and their inverses
struct X3hRange {
  float xi, eta, ixi, ieta;
};
__device__ __forceinline__ X3hRange x3h_range(float m) {
  X3hRange r;
  r.xi = pow2_below(m, 14, 120);
  r.eta = pow2_below(m + 1.f, 14, 120);
  r.ixi = 1.f / r.xi;
  r.ieta = 1.f / r.eta;
  return r;
}

// ---- hidden block --------------------------------------------------------------------------
// a pair (h0, h1) of fc1 accumulators: unscale (is fi = 1 / (W1 row scale xi)), + b1,
// GELU(erf), scale (hs fh = eta_j eta), split into the fc2 B fragment's pair.  fi, fh: the
// part of the two factors that the caller's tables do not hold (mlp_gen_h.hip: the pixel's
// 1 / xi and eta; mlp_fused_h.hip folds the field's into its tables and passes 1, which the
// compiler drops).  Taken apart so that each product stays where the kernels had it: with
// the folded factors as arguments hs fh moved ahead of the GELU and every mlp_gen_h kernel's
// schedule changed
__device__ __forceinline__ void x3h_hidden_pair(float h0, float h1, float2 is, float fi, float2 b,
                                                float2 hs, float fh, uint32_t& t0, uint32_t& t1) {
  f32x2 v = {fmaf(h0, is.x * fi, b.x), fmaf(h1, is.y * fi, b.y)};
  v = gelu_erf2(v) * f32x2{hs.x * fh, hs.y * fh};
  split2h(v.x, v.y, t0, t1);
}

// (The b1 / 1 / s1 / eta / b2 / 1 / s2 tables are staged into LDS by each kernel itself:
// mlp_fused_h.hip folds the field's range factors into them, mlp_gen_h.hip stores them as
// they are.  One function with the three factors as arguments serves both without a caller
// flag, but with it 758 of the 10163 lines of mlp_gen_hp_kernel<3, 16, true, 4, 2> and 216 of
// mlp_fused_h_kernel's 4058 differed from before, against 2 and 184 without.)

// ---- waits ---------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void x3h_wait_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
// LDS written by the wave's own lanes is read by others of the same wave
__device__ __forceinline__ void x3h_wave_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the one-tile slice ring ---------------------------------------------------------------
// NS slots of 16 KB in LDS, a slice filled by the W waves of the workgroup together: wave w
// moves PIECES 1-KB pieces (piece i at byte (i W + w) 1024 of the slice), one LDS-DMA each.
// The DMAs are inline asm, so the kernel owns their completion (dma.h): a wave's vmcnt
// counts PIECES per slice it filled, and landed() derives its immediates from that same
// PIECES (four pieces: vmcnt(8) / vmcnt(4) / vmcnt(0)).  A kernel that issues other
// vector-memory instructions between its first step and its last must drain them first.
template <int W, int NS>
struct X3hRing {
  static constexpr int PIECES = 4;  // per wave and slice: what glds16x4 issues
  static_assert(W * PIECES * 1024 == MH_SLICE * 2, "the waves' pieces make one slice");
  static_assert(NS >= 3 && NS <= 4, "landed() leaves at most two younger slices in flight");
  const unsigned short* ring;
  uint32_t lds;
  int wave_u;
  uint32_t piece_off[PIECES];

  __device__ __forceinline__ X3hRing(const unsigned short* ring_, int wave, int lane)
      : ring(ring_), lds(lds_addr(ring_)), wave_u(__builtin_amdgcn_readfirstlane(wave)) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) piece_off[i] = (uint32_t)(i * W * 1024 + lane * 16);
  }
  // slice q <- the 16 KB at src
  __device__ __forceinline__ void fill(int q, const unsigned short* src) const {
    glds16x4<W * 1024>(reinterpret_cast<uint64_t>(src) + (uint64_t)wave_u * 1024, piece_off,
                       lds + (uint32_t)((q % NS) * MH_SLICE * 2 + wave_u * 1024));
  }
  // Step q of n: slice q landed for every wave (the min(NS - 2, n - 1 - q) younger slices may
  // stay in flight) and every read of slice q - 1's slot is retired, so that slot is free
  __device__ __forceinline__ const unsigned short* landed(int q, int n) const {
    const int after = min(NS - 2, n - 1 - q);
    if (after >= 2) x3h_wait_vm<2 * PIECES>();
    else if (after == 1) x3h_wait_vm<PIECES>();
    else x3h_wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    return ring + (q % NS) * MH_SLICE;
  }
  // the slot freed at step q takes slice q + NS - 1 from src(q + NS - 1), if there is one
  template <class Src>
  __device__ __forceinline__ void refill(int q, int n, Src&& src) const {
    if (q >= 1 && q + NS - 1 < n) fill(q + NS - 1, src(q + NS - 1));
  }
};

// ---- weight preparation ----------------------------------------------------------------------
// the maximum of m over a 256-thread workgroup, in every thread (wmax: 4 floats of LDS)
__device__ __forceinline__ float x3h_block_max(float m, float* wmax) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

}  // namespace msfno
