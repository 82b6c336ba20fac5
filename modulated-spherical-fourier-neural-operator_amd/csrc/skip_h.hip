// Inner skip at C = 256 on the "x3h" engine (gfx950): out = Ws·x + bs as a 1x1
// convolution over pixels, on the block MLP's fc1 tiling (mlp_fused_h.hip: 16x16x32 fp16
// MFMAs, 16 pixels per wave, fp32 as two fp16 terms and three MFMAs per product,
// split_engine.h).  It shares that unit's 16-KB weight slice layout and ring depth
// and the steps of the tile pipeline (x3h_tile.h) and nothing else.
//   sk_prep_kernel          the per-batch weight image and its row scales
//   skip_hp_kernel          the default: persistent, software-pipelined (P % 4 == 0)
//   skip_h_kernel           one tile per workgroup (MSFNO_SKIP_P=0, any P)
//   chan_pow2_scale_kernel  the input's channel scales where no norm statistics give them
// Unlike mlp_fused_h.hip this unit is built WITH packed FP32 (csrc/Makefile: not in
// NOPK_SRCS): without it skip_hp_kernel measured 1 % slower and took 20 bytes more
// scratch (profiles/r11_mlp_io).  It has none of the op_sel form of DESIGN.md §5;
// tests/test_mlp_packed_fp32.py and tests/test_isa_audit.py check the built library.
#include "kernels.h"
#include "x3h_tile.h"

#include <algorithm>
#include <cstdlib>

namespace msfno {

namespace {

// The fc1 half of mlp_fused_h_kernel with 256 output rows and no hidden layer:
// a wave's 16 pixels of x, scaled per channel by the power of two xs (chan_affine's
// norm0 bound, |xs x| < 2^14) and split into fp16x2 B fragments in registers; the
// per-batch weight image W'[c][k] = rs_c Ws[c][k] / xs_k (rs_c puts the row's maximum
// into [2^14, 2^15)) streams through the four-slot LDS ring as 16 slices of 16 KB
// (output block j of 32 rows, channel half kh: the W1 slice layout); all 256 x 16
// outputs stay in the accumulators and are stored once, unscaled by 1 / rs_c, + bs.
// (gemm_x3 with in-kernel split, 256 x 256 tiles: 0.83 ms at config 2.)
constexpr int SK_NSLICE = 16;

struct SkipHParams {
  const float* x;       // [B][C][P]
  const float* xs;      // [B][C] power-of-two channel scales
  float* out;           // [B][C][P]
  const unsigned short* img;  // [B][16 slices]
  const float* inv_rs;  // [B][C]
  const float* bias;    // [C] or null
  int64_t P;
  int tiles_per_field;
};

// The per-batch skip weight image in one launch (it was two: the row scales, then the
// image, 5.6 us each per block and batch at the network's 120 x 240 blocks): one
// 256-thread workgroup per (row c, batch b).  rs[b][c] = 2^(15 - e) for
// max_k |Ws[c][k] / xs[b][k]| = f 2^e, inv_rs = 1 / rs; then the row of
// W' = rs Ws / xs split into fp16x2 in mh_w1_image_kernel's slice layout
// [b][j][kh][pl][ks][t][r][32] (8 blocks j; thread k < 128 writes the pair 2k, 2k + 1)
__global__ __launch_bounds__(256) void sk_prep_kernel(const float* __restrict__ W,
                                                      const float* __restrict__ xs,
                                                      float* __restrict__ rs,
                                                      float* __restrict__ inv_rs,
                                                      unsigned short* __restrict__ img) {
  __shared__ float wmax[4];
  const int b = blockIdx.y, c = blockIdx.x, k = threadIdx.x;
  const float* row = W + (int64_t)c * MH_C;
  const float* xsb = xs ? xs + (int64_t)b * MH_C : nullptr;
  const float sc = row_scale(x3h_block_max(fabsf(xsb ? row[k] / xsb[k] : row[k]), wmax), 15);
  if (k == 0) {
    rs[(int64_t)b * MH_C + c] = sc;
    inv_rs[(int64_t)b * MH_C + c] = 1.f / sc;
  }
  if (k >= 128) return;
  const int k0 = 2 * k;  // the pair (k0, k0 + 1): one kh, ks, 8-channel group
  const int j = c >> 5, t = (c >> 4) & 1, r = c & 15;
  const int kh = k0 >> 7, ks = (k0 >> 5) & 3;
  uint32_t t0, t1;
  if (xsb)
    split2h(row[k0] / xsb[k0] * sc, row[k0 + 1] / xsb[k0 + 1] * sc, t0, t1);
  else
    split2h(row[k0] * sc, row[k0 + 1] * sc, t0, t1);
  unsigned short* ib = img + (int64_t)b * SK_NSLICE * MH_SLICE;
  uint32_t* o = reinterpret_cast<uint32_t*>(ib + (int64_t)(j * 2 + kh) * MH_SLICE + x3h_w1_slice_pos(ks, t, r, k0 & 31));
  o[0] = t0;
  o[MH_PLANE / 2] = t1;
}

template <int NS, int MINB>
__global__ __launch_bounds__(256, MINB) void skip_h_kernel(SkipHParams p) {
  // NS: ring slots; MINB: workgroups per CU of the launch bounds
  static_assert(NS == MH_NS && MINB == 2, "only the four-slot, two-per-CU form is instantiated");
  constexpr int W = 4;
  constexpr int RING_BYTES = NS * MH_SLICE * 2;
  __shared__ __attribute__((aligned(16))) char lds_raw[RING_BYTES + 2 * MH_C * 4];
  unsigned short* const ring = reinterpret_cast<unsigned short*>(lds_raw);
  float* const irs = reinterpret_cast<float*>(lds_raw + RING_BYTES);
  float* const bs = irs + MH_C;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int z = lin / p.tiles_per_field;
  const int64_t P = p.P;
  const int64_t px = (int64_t)(lin - z * p.tiles_per_field) * 64 + 16 * wave + r16;
  const unsigned short* img = p.img + (int64_t)z * SK_NSLICE * MH_SLICE;

  const X3hRing<W, NS> wring(ring, wave, lane);
  auto slice = [&](int q) { return img + (int64_t)q * MH_SLICE; };
#pragma unroll
  for (int q = 0; q < NS; ++q) wring.fill(q, slice(q));

  // x -> scaled fp16x2 B fragments (k-step ks: channels 32 ks + 8 g + 0..7)
  const float* xcol = p.x + (int64_t)z * MH_C * P + (px < P ? px : P - 1);
  half8 xf[8][2];
  {
    const float* xsb = p.xs + (int64_t)z * MH_C;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int c0 = 32 * ks + 8 * g;
      float xv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = __builtin_nontemporal_load(xcol + (int64_t)(c0 + e) * P);
      const float4 sa = *reinterpret_cast<const float4*>(xsb + c0);
      const float4 sb = *reinterpret_cast<const float4*>(xsb + c0 + 4);
      const float sv[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
      x3h_split8([&](int e) { return sv[e] * xv[e]; }, xf[ks]);
    }
  }
  for (int i = tid; i < MH_C; i += 256) {
    irs[i] = p.inv_rs[(int64_t)z * MH_C + i];
    bs[i] = p.bias ? p.bias[i] : 0.f;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  floatx4 oacc[16];
#pragma unroll
  for (int ot = 0; ot < 16; ++ot) oacc[ot] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int a_lane = x3h_a_lane(r16, g);

  // (the refill stays one burst: as four spread pieces the kernel alone measured 1.598
  // against 1.611 ms at config 2, 0.8 %, under twice the parent's own 0.44 % spread,
  // profiles/r09_refill/skip_h_alone.txt)
#pragma unroll
  for (int q = 0; q < SK_NSLICE; ++q) {
    const unsigned short* slot = wring.landed(q, SK_NSLICE);
    const int j = q >> 1, kh = q & 1;
    auto aoff = [&](int u, int pl) { return ((pl * 4 + (u >> 1)) * 2 + (u & 1)) * 512 + a_lane; };
    half8 a[3][2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) a[k][pl] = *reinterpret_cast<const half8*>(slot + aoff(k, pl));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u + 2 < 8) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
          a[(u + 2) % 3][pl] = *reinterpret_cast<const half8*>(slot + aoff(u + 2, pl));
      }
      SplitEng<2>::mma(a[u % 3], xf[kh * 4 + (u >> 1)], oacc[2 * j + (u & 1)]);
      if (u == 0) wring.refill(q, SK_NSLICE, slice);
    }
  }

  // epilogue: rows 16 ot + 4 g + i of pixel px
  if (px >= P) return;
  float* o = p.out + (int64_t)z * MH_C * P + px;
#pragma unroll
  for (int ot = 0; ot < 16; ++ot) {
    const int r0 = 16 * ot + 4 * g;
    const float4 is = *reinterpret_cast<const float4*>(irs + r0);
    const float4 b = *reinterpret_cast<const float4*>(bs + r0);
    const float isv[4] = {is.x, is.y, is.z, is.w};
    const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) o[(int64_t)(r0 + i) * P] = fmaf(oacc[ot][i], isv[i], bv[i]);
  }
}

// Persistent, pipelined form of skip_h_kernel (one workgroup of 4 waves per CU, one
// wave per SIMD with the whole register file: 32 pixels per wave as two 16-pixel
// groups, 128 per tile; a contiguous range of tiles per workgroup).  skip_h_kernel
// runs one tile per workgroup: its x loads, its 16 slice steps and its 64 four-byte
// stores per lane are three phases that every CU enters at the same time, so HBM idles
// while the MFMAs run and the MFMAs idle while x streams in.  Here one ring carries,
// per slice step, the weight slice of this tile AND one 16-channel piece of the NEXT
// tile's x (8 KB, LDS-DMA), which the step converts into the next tile's B fragments
// in registers; the outputs leave through a per-wave LDS transpose as 16-B stores
// (whole 128-B lines, 32 per lane instead of 128).  HBM then streams x and out under
// the MFMAs, and each A fragment read from LDS feeds both pixel groups.
//
// vmcnt accounting (each wave, in issue order): group n = 6 LDS-DMAs (four 1-KB weight
// pieces + two x-piece rows pairs), issued at step n - (NS - 1); a tile's 32 output
// stores come after its step 15.  The wait for group n at step n leaves NS - 2 younger
// groups in flight, plus the previous tile's stores when n is one of the first NS - 1
// steps of a tile (tile 0: those groups were drained in the prologue).  The tail
// issues dummy groups (the last tile again) so the counts stay exact, and the kernel
// drains every DMA before it exits.
//
// Within a step the group's six DMAs are spread, one after each of the MFMA pairs
// u = 0..5 (the prologue's NS - 1 groups stay bursts: there are no MFMAs yet):
//   WAR   group n + NS - 1 refills slot (n - 1) % NS, last read (weights and x piece) in
//         step n - 1; those reads are retired (lgkmcnt(0)) before step n's barrier, which
//         every DMA of the step follows in program order.
//   RAW   the group is first read in step n + NS - 1, after that step's counted wait (the
//         wave's own six) and barrier (the other waves').
//   count six VMEM instructions per wave and step in the order w0..w3, x0, x1, all issued
//         before the next step's wait; a tile's 32 output stores still come after the
//         sixth DMA of its step 15 and before the first wait of the next tile, so
//         vmcnt(50) / vmcnt(18) count what they counted.
constexpr int SP_NS = 5, SP_W = 4, SP_PX = 32 * SP_W;
constexpr int SP_XPAIR = 1024 + 32;                  // two 512-B x rows + bank pad
constexpr int SP_WBYTES = MH_SLICE * 2;              // 16 KB of weights
constexpr int SP_SLOT = SP_WBYTES + 8 * SP_XPAIR;    // 24,832 B
constexpr int SP_ERS = 36;                           // epilogue row stride (floats)
constexpr int SP_EPI = 32 * SP_ERS * 4;              // per wave: 32 channels x 32 pixels
constexpr int SP_LDS = SP_NS * SP_SLOT + SP_W * SP_EPI + 3 * MH_C * 4;
constexpr int SP_GROUP = 6;                          // DMAs per wave and step
static_assert(SP_LDS <= 160 * 1024, "skip_hp LDS");
static_assert(SP_SLOT % 16 == 0 && SP_EPI % 16 == 0, "skip_hp LDS alignment");
static_assert(SP_GROUP * (SP_NS - 2) + 32 <= 63, "skip_hp vmcnt range");

struct SkipHPParams {
  const float* x;
  const float* xs;
  float* out;
  const unsigned short* img;
  const float* inv_rs;
  const float* bias;
  int64_t P;
  int tiles_per_field;
  int tiles;
};

__global__ __launch_bounds__(64 * SP_W, 1) void skip_hp_kernel(SkipHPParams p) {
  constexpr int NS = SP_NS;
  __shared__ __attribute__((aligned(16))) char lds[SP_LDS];
  float* const epi_all = reinterpret_cast<float*>(lds + NS * SP_SLOT);
  float* const xsl = reinterpret_cast<float*>(lds + NS * SP_SLOT + SP_W * SP_EPI);
  float* const irsl = xsl + MH_C;
  float* const bl = irsl + MH_C;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int64_t P = p.P;
  const int t0 = (int)((int64_t)blockIdx.x * p.tiles / gridDim.x);
  const int t1 = (int)((int64_t)(blockIdx.x + 1) * p.tiles / gridDim.x);
  const int ntile = t1 - t0;  // >= 1: the host launches at most `tiles` workgroups
  const int tpf = p.tiles_per_field;
  const uint32_t ring_lds = lds_addr(lds);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  // x piece of step q: 16 channels 32 (q >> 1) + 8 g' + 4 (q & 1) + e (g' 0..3, e 0..3),
  // piece row i = 4 g' + e, rows (2k, 2k + 1) at k * SP_XPAIR.  This wave's two DMAs move
  // rows 4 wave + 2 h2 + (lane >> 5), pixels 4 (lane & 31) .. + 3 of the tile.
  const uint32_t w_voff = (uint32_t)lane * 16;
  uint32_t x_voff_row[2];
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    const int xrow = 4 * wave + 2 * h2 + (lane >> 5);
    x_voff_row[h2] = (uint32_t)(8 * (xrow >> 2) + (xrow & 3)) * (uint32_t)P * 4;
  }
  const int xcol = 4 * (lane & 31);

  // per-tile DMA sources (uniform): the tile's weight image, the x base of the tile
  // after it (or of itself at the end: never read) and that tile's pixel limit
  struct Src {
    uint64_t w, x;
    uint32_t xo[2];
  };
  auto src_of = [&](int tl) {
    if (tl >= ntile) tl = ntile - 1;  // tail: dummy groups
    const int t = t0 + tl;
    const int z = t / tpf;
    const int tn = tl + 1 < ntile ? t + 1 : t;
    const int zn = tn / tpf;
    const int64_t pxt = (int64_t)(tn - zn * tpf) * SP_PX;
    const int64_t room = P - 4 - pxt;  // >= 0: P % 4 == 0 and pxt < P
    const int lim = room < SP_PX - 4 ? (int)room : SP_PX - 4;
    Src r;
    r.w = reinterpret_cast<uint64_t>(p.img + (int64_t)z * SK_NSLICE * MH_SLICE) + (uint64_t)(wave_u * 1024);
    r.x = reinterpret_cast<uint64_t>(p.x + (int64_t)zn * MH_C * P + pxt);
    const uint32_t c4 = (uint32_t)min(xcol, lim) * 4;
    r.xo[0] = x_voff_row[0] + c4;
    r.xo[1] = x_voff_row[1] + c4;
    return r;
  };
  auto issue = [&](const Src& sr, int n, int q) {
    // opaque copies: keep the per-step address arithmetic at the step (hoisted to the
    // tile start, 16 steps of addresses overflow the SGPRs)
    uint64_t wb = sr.w, xb0 = sr.x, p4 = (uint64_t)P * 4;
    asm volatile("" : "+s"(wb), "+s"(xb0), "+s"(p4));
    const uint32_t slot = ring_lds + (uint32_t)((n % NS) * SP_SLOT);
    const uint64_t wq = wb + (uint64_t)q * MH_SLICE * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      glds16s(wq + (uint64_t)(i * 4096), w_voff, slot + (uint32_t)(i * 4096 + wave_u * 1024));
    const uint64_t xq = xb0 + (uint64_t)(32 * (q >> 1) + 4 * (q & 1)) * p4;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
      glds16s(xq, sr.xo[h2], slot + (uint32_t)(SP_WBYTES + (2 * wave_u + h2) * SP_XPAIR));
  };
  // DMA k (0..SP_GROUP - 1) of issue(sr, n, q) on its own: 0..3 the weight pieces, 4 and 5
  // the x row pairs, in the order of the group above
  auto issue_piece = [&](const Src& sr, int n, int q, int k) {
    const uint32_t slot = ring_lds + (uint32_t)((n % NS) * SP_SLOT);
    if (k < 4) {
      uint64_t wb = sr.w;
      asm volatile("" : "+s"(wb));
      glds16s(wb + (uint64_t)q * MH_SLICE * 2 + (uint64_t)(k * 4096), w_voff,
              slot + (uint32_t)(k * 4096 + wave_u * 1024));
    } else {
      uint64_t xb0 = sr.x, p4 = (uint64_t)P * 4;
      asm volatile("" : "+s"(xb0), "+s"(p4));
      glds16s(xb0 + (uint64_t)(32 * (q >> 1) + 4 * (q & 1)) * p4, sr.xo[k - 4],
              slot + (uint32_t)(SP_WBYTES + (2 * wave_u + (k - 4)) * SP_XPAIR));
    }
  };

  int zc = t0 / tpf, zx = (ntile > 1 ? t0 + 1 : t0) / tpf;
  for (int i = tid; i < MH_C; i += 64 * SP_W) {
    bl[i] = p.bias ? p.bias[i] : 0.f;
    irsl[i] = p.inv_rs[(int64_t)zc * MH_C + i];
    xsl[i] = p.xs[(int64_t)zx * MH_C + i];
  }
  {
    const Src s0 = src_of(0);
#pragma unroll
    for (int n = 0; n < NS - 1; ++n) issue(s0, n, n);
  }

  // the first tile's x -> B fragments (plain loads, once per workgroup)
  half8 xf[2][8][2];
  {
    const float* xsb = p.xs + (int64_t)zc * MH_C;
#pragma unroll
    for (int pg = 0; pg < 2; ++pg) {
      int64_t px = (int64_t)(t0 - zc * tpf) * SP_PX + 32 * wave + 16 * pg + r16;
      if (px > P - 1) px = P - 1;  // past the field's end (never stored)
      const float* xw = p.x + (int64_t)zc * MH_C * P;
      const uint32_t lo = (uint32_t)(8 * g) * (uint32_t)P + (uint32_t)px;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int c0 = 32 * ks + 8 * g;
        float xv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          xv[e] = __builtin_nontemporal_load(xw + (int64_t)(32 * ks + e) * P + lo);
        const float4 sa = *reinterpret_cast<const float4*>(xsb + c0);
        const float4 sb = *reinterpret_cast<const float4*>(xsb + c0 + 4);
        const float sv[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
        x3h_split8([&](int e) { return sv[e] * xv[e]; }, xf[pg][ks]);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int a_lane = x3h_a_lane(r16, g);
  float* const ep = epi_all + wave * 32 * SP_ERS;
  uint32_t xn[2][8][2][4];

  for (int tl = 0; tl < ntile; ++tl) {
    const int t = t0 + tl;
    if (tl > 0) {
      const int zc2 = t / tpf, zx2 = (tl + 1 < ntile ? t + 1 : t) / tpf;
      if (zc2 != zc || zx2 != zx) {  // a field boundary: new scale tables (drains the ring)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int i = tid; i < MH_C; i += 64 * SP_W) {
          irsl[i] = p.inv_rs[(int64_t)zc2 * MH_C + i];
          xsl[i] = p.xs[(int64_t)zx2 * MH_C + i];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        zc = zc2;
        zx = zx2;
      }
    }
    const Src s_cur = src_of(tl), s_nxt = src_of(tl + 1);
    floatx4 oacc[2][16];
#pragma unroll
    for (int pg = 0; pg < 2; ++pg)
#pragma unroll
      for (int ot = 0; ot < 16; ++ot) oacc[pg][ot] = floatx4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int q = 0; q < SK_NSLICE; ++q) {
      const int n = tl * SK_NSLICE + q;
      if (q < NS - 1) asm volatile("s_waitcnt vmcnt(50)" ::: "memory");  // 6 (NS-2) + 32
      else asm volatile("s_waitcnt vmcnt(18)" ::: "memory");              // 6 (NS-2)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const char* slot = lds + (n % NS) * SP_SLOT;
      // the next tile's x piece -> its B fragments (channels 32 ks + 8 g + 4 h + 0..3)
      {
        const int ks = q >> 1, h = q & 1;
        const float4 sv = *reinterpret_cast<const float4*>(xsl + 32 * ks + 8 * g + 4 * h);
#pragma unroll
        for (int pg = 0; pg < 2; ++pg) {
          const char* xb = slot + SP_WBYTES + 4 * (32 * wave + 16 * pg + r16);
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = *reinterpret_cast<const float*>(xb + (2 * g + (e >> 1)) * SP_XPAIR + (e & 1) * 512);
          split2h(sv.x * v[0], sv.y * v[1], xn[pg][ks][0][2 * h], xn[pg][ks][1][2 * h]);
          split2h(sv.z * v[2], sv.w * v[3], xn[pg][ks][0][2 * h + 1], xn[pg][ks][1][2 * h + 1]);
        }
      }
      const unsigned short* ws = reinterpret_cast<const unsigned short*>(slot);
      const int j = q >> 1, kh = q & 1;
      auto aoff = [&](int u, int pl) { return ((pl * 4 + (u >> 1)) * 2 + (u & 1)) * 512 + a_lane; };
      half8 a[3][2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a[k][pl] = *reinterpret_cast<const half8*>(ws + aoff(k, pl));
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (u + 2 < 8) {
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            a[(u + 2) % 3][pl] = *reinterpret_cast<const half8*>(ws + aoff(u + 2, pl));
        }
#pragma unroll
        for (int pg = 0; pg < 2; ++pg)
          SplitEng<2>::mma(a[u % 3], xf[pg][kh * 4 + (u >> 1)], oacc[pg][2 * j + (u & 1)]);
        if (u < SP_GROUP) {  // DMA u of group n + NS - 1, after the step's MFMA triples 2u, 2u + 1
          if (q + NS - 1 < SK_NSLICE) issue_piece(s_cur, n + NS - 1, q + NS - 1, u);
          else issue_piece(s_nxt, n + NS - 1, q + NS - 1 - SK_NSLICE, u);
        }
      }
    }

    // epilogue: row 16 ot + 4 g + i, pixel 32 wave + 16 pg + r16; 32 rows per round
    // through the wave's LDS patch, out as 16-B stores (a row's 32 pixels = one line)
    {
      const int64_t px0 = (int64_t)(t - zc * tpf) * SP_PX + 32 * wave;
      float* const ob = p.out + (int64_t)zc * MH_C * P + px0;
      const uint32_t so = (uint32_t)(lane >> 3) * (uint32_t)P + 4u * (uint32_t)(lane & 7);
      const bool in = px0 + 4 * (lane & 7) < P;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int o2 = 0; o2 < 2; ++o2) {
          const int r0 = 16 * (2 * c + o2) + 4 * g;
          const float4 is = *reinterpret_cast<const float4*>(irsl + r0);
          const float4 bb = *reinterpret_cast<const float4*>(bl + r0);
#pragma unroll
          for (int pg = 0; pg < 2; ++pg) {
            const floatx4 acc = oacc[pg][2 * c + o2];
            float* e0 = ep + (16 * o2 + 4 * g) * SP_ERS + 16 * pg + r16;
            e0[0] = fmaf(acc[0], is.x, bb.x);
            e0[SP_ERS] = fmaf(acc[1], is.y, bb.y);
            e0[2 * SP_ERS] = fmaf(acc[2], is.z, bb.z);
            e0[3 * SP_ERS] = fmaf(acc[3], is.w, bb.w);
          }
        }
        x3h_wave_handover();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int row = 8 * k + (lane >> 3), col = 4 * (lane & 7);
          const floatx4 v = *reinterpret_cast<const floatx4*>(ep + row * SP_ERS + col);
          if (in)
            __builtin_nontemporal_store(
                v, reinterpret_cast<floatx4*>(ob + (int64_t)(32 * c + 8 * k) * P + so));
        }
        x3h_wave_handover();
      }
    }
#pragma unroll
    for (int pg = 0; pg < 2; ++pg)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
        x3h_frags(xn[pg][ks], xf[pg][ks]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the tail's dummy DMAs land before exit
}

// xs[r] = 2^(14 - e), max_p |x[r][p]| = f 2^e (f in [0.5, 1)): every |xs x| < 2^14 (the
// x3h B-row scale of a standalone 1x1 conv, whose input has no norm statistics); one
// 256-thread workgroup per row r
__global__ __launch_bounds__(256) void chan_pow2_scale_kernel(const float* __restrict__ x,
                                                              int64_t P, float* __restrict__ xs) {
  __shared__ float wmax[4];
  const float* row = x + (int64_t)blockIdx.x * P;
  float m = 0.f;
  for (int64_t p = threadIdx.x; p < P; p += 256) m = fmaxf(m, fabsf(row[p]));
  m = x3h_block_max(m, wmax);
  if (threadIdx.x == 0) xs[blockIdx.x] = pow2_below(m, 14, 120);
}

}  // namespace

int launch_chan_pow2_scale(const float* x, int64_t rows, int64_t P, float* xs, hipStream_t s) {
  MSFNO_REQUIRE(x && xs && rows > 0 && rows < (1LL << 31) && P >= 1, MSFNO_EINVAL,
                "chan_pow2_scale: bad arguments");
  hipLaunchKernelGGL(chan_pow2_scale_kernel, dim3((unsigned)rows), dim3(256), 0, s, x, P, xs);
  return launch_check("chan_pow2_scale");
}

size_t skip_h_workspace(int B) {
  return (size_t)B * SK_NSLICE * MH_SLICE * 2 + (size_t)B * MH_C * 4 * 2 + 256;
}

// MSFNO_SKIP_H=0 keeps gemm_x3 for the inner skip
bool skip_h_env() {
  static const bool on = sw_on("MSFNO_SKIP_H");
  return on;
}

int launch_skip_h(const float* W, const float* xs, const float* x, float* out, const float* bias,
                  int B, int64_t P, void* ws, size_t ws_bytes, hipStream_t s, bool side) {
  MSFNO_REQUIRE(W && xs && x && out && ws && B > 0 && P >= 1 && ws_bytes >= skip_h_workspace(B),
                MSFNO_EINVAL, "skip_h: bad arguments");
  unsigned short* img = static_cast<unsigned short*>(ws);
  float* rs = reinterpret_cast<float*>(img + (int64_t)B * SK_NSLICE * MH_SLICE);
  float* inv_rs = rs + (int64_t)B * MH_C;
  hipLaunchKernelGGL(sk_prep_kernel, dim3(MH_C, B), dim3(256), 0, s, W, xs, rs, inv_rs, img);
  MSFNO_TRY(launch_check("sk_prep"));
  SkipHParams p{};
  p.x = x; p.xs = xs; p.out = out; p.img = img; p.inv_rs = inv_rs; p.bias = bias; p.P = P;
  p.tiles_per_field = (int)cdiv(P, 64);
  const int64_t tiles = (int64_t)B * p.tiles_per_field;
  MSFNO_REQUIRE(tiles < (1LL << 31), MSFNO_EINVAL, "skip_h: grid too large");
  // the persistent pipelined kernel (MSFNO_SKIP_P=0: one tile per workgroup, read on
  // every call so one process can run both); its x pieces and output stores move 4
  // pixels per lane (P % 4 == 0)
  const bool persist = sw_on("MSFNO_SKIP_P");
  if (persist && P % 4 == 0) {
    SkipHPParams q{};
    q.x = x; q.xs = xs; q.out = out; q.img = img; q.inv_rs = inv_rs; q.bias = bias; q.P = P;
    q.tiles_per_field = (int)cdiv(P, SP_PX);
    const int64_t t = (int64_t)B * q.tiles_per_field;
    MSFNO_REQUIRE(t < (1LL << 31), MSFNO_EINVAL, "skip_hp: grid too large");
    q.tiles = (int)t;
    // Workgroups per CU.  A workgroup fills its CU (142 KB of LDS, the whole register
    // file).  Alone (inline, or in a graph): 2 per CU, the second half of the grid starting
    // as the first retires.  On the block's side stream the grid size is the share of CUs
    // taken from the main stream's SHT kernels while the skip runs: 0.25 (64 of 256 CUs;
    // the skip then spans 2.35 ms under the SHT) measured 166.9 / 165.4 / 166.1 fields/s
    // against 163.6 / 164.3 / 162.8 for 2 per CU, 158.7 / 156.1 / 158.9 for 0.1875 and
    // 164.4 / 162.6 / 163.9 for 0.3125, three interleaved rounds (profiles/r06_f).
    // MSFNO_SKIP_GRID overrides both.
    const char* ge = sw_raw("MSFNO_SKIP_GRID");  // (read on every call)
    const double per_cu = ge ? atof(ge) : (side ? 0.25 : 2.0);
    const int64_t want = std::max<int64_t>(1, (int64_t)(per_cu * device_cus() + 0.5));
    const int grid = (int)std::min<int64_t>(t, want);
    hipLaunchKernelGGL(skip_hp_kernel, dim3((unsigned)grid), dim3(64 * SP_W), 0, s, q);
    return launch_check("skip_hp");
  }
  hipLaunchKernelGGL((skip_h_kernel<MH_NS, 2>), dim3((unsigned)tiles), dim3(256), 0, s, p);
  return launch_check("skip_h");
}

}  // namespace msfno
