// Spectral-MLP layer as a Gauss three-multiplication complex GEMM on the x6
// engine ("x6c"), for gfx950.
//
// One layer of SpectralAttentionS2.forward_mlp (layers.py:604-620; the
// contraction compl_mul2d_fwd_c, contractions.py:132-137) is Y = W · X over the
// channels of every (l, m) column, W (co x ci) and X (ci x T) complex.  With
//   P1 = Wr·Xr,  P2 = Wi·Xi,  P3 = (Wr + Wi)·(Xr + Xi)
// Re Y = P1 - P2 and Im Y = P3 - P1 - P2: three real products instead of the four
// of the real-ified [[Wr, -Wi], [Wi, Wr]] GEMM, 25 % fewer matrix-core cycles.
// Each product is an x6 product (gemm_x6p.hip) of bf16x3 planes, so both
// operands carry a third "matrix": Ws = Wr + Wi (weight prep) and Xs = Xr + Xi,
// which the producer of X writes next to Xr and Xi (the previous layer's
// epilogue; layer 0 forms it while it stages its fp32 input).  ComplexReLU(real) (activations.py:42-46)
// is applied to Re in the epilogue, before Ys = Re + Im is formed.
//
// Activations ("3M planes"): matrices 0 = real, 1 = imaginary, 2 = real + imaginary, three
// bf16 planes each (x3h: two fp16 planes), stored between the layers in MFMA fragment
// order (described below X6CParams): a hidden layer's epilogue stores its accumulator
// registers as they stand, and the next layer reads them back as B fragments with no
// transpose; the permutation of the contraction index that this implies is carried
// by the next layer's weight image.
// Tile 128 complex rows x 128 columns x 16 (k), 8 waves as 4 (M) x 2 (N), each
// wave 32 x 64 with three accumulator sets (P1, P2, P3).  Stage (72 KB) = A: 3
// matrices x 3 planes x [128][16] + B: 3 x 3 x 16 x 128 (DMA-fed layers: four
// 32-column blocks of 64 lanes x 8 k; layer 0: [16][128] rows, swizzled as in
// gemm_x6p_kernel); two stages, one k-tile in flight (LDS-DMA, dma.h).

#include "dma.h"
#include "gemm_common.h"

#include <type_traits>

namespace msfno {

// NP planes per value (split_engine.h): 3 = the x6 engine, 2 = the x3h engine (operands
// power-of-two scaled into fp16 range, see the scale arrays of X6CParams and
// spec_scales_x3h_kernel)
constexpr int X6C_BM = 128, X6C_BN = 128, X6C_BK = 16;

struct X6CParams {
  const unsigned short* Aw;  // [mat][plane][kt][Mp][16]
  int64_t a_mat, a_plane;
  int Mp;
  const unsigned short* X;   // [b][mat][plane][ci][ldx]
  int64_t x_b, x_mat, x_plane;
  int ldx;
  unsigned short* Y;         // planes out [b][mat][plane][co][ldy] (hidden layers)
  int64_t y_b, y_mat, y_plane;
  int ldy;
  float* S;                  // fp32 out (output layer): Re rows at S + b*s_b, Im at + s_im
  int64_t s_b, s_im;
  int ldS;
  int co, ci, N;
  int tiles_m, tiles_n;
  int relu;
  // BF32 (layer 0): X given as fp32 rows instead of 3M planes: Re rows at
  // Xf + b*xf_b, Im rows at + xf_im, ld ldxf; split (and Re + Im formed) while staged
  const float* Xf;
  int64_t xf_b, xf_im;
  int ldxf;
  // LAY (tiled activations): k-tiles per column tile of the planes input / output
  // (round_up(rows, 128) / 16 of the producing layer)
  int kt_in, kt_out;
  // x3h (NP = 2) scaling, all powers of two: *lscale multiplies the accumulators
  // before the epilogue (layer constant: weight scale undone, output range set);
  // colscale[b * cs_b + column] multiplies the fp32 B values while staged (BF32 layer
  // 0: the per-column input scale) or the outputs in the epilogue (output layer)
  const float* lscale;
  const float* colscale;
  int64_t cs_b;
};

// Tiled 3M activations (LAY): the planes of a layer's activation stored as the MFMA
// B fragments of the next layer, [b][tn][kt][mat*NP+plane][cb = 0..3][lane 0..63][8]:
// the 16 bytes of (cb, lane) are what lane (n = lane & 31, h = lane >> 5) feeds a
// 32x32x16 MFMA as the B operand of column 32 cb + n of the tile, k positions
// 8 h .. 8 h + 7 of k-tile kt.  That is also where the producing layer's accumulators
// sit: of a 32-row output block, registers 8 t .. 8 t + 7 (t = 0, 1) of lane (n, h) are
// rows 16 t + 8 (e >> 2) + 4 h + (e & 3), e = 0..7, of column n, so they are stored as
// they stand as k-tile (row0 >> 4) + t, and k position kp = 8 h + e of a k-tile holds
// channel 16 kt + x6c_kperm(kp).  The consuming layer's weight image carries the same
// permutation of k (spec_weights_3m_kernel), and a sum over k does not see it.
// One (matrix-plane, cb) is a contiguous 1 KB: one DMA piece, one wave store, and a
// linear (conflict-free) ds_read_b128 per fragment.  Pad rows (>= co) and columns
// (>= N) hold 0.
__device__ __forceinline__ int x6c_kperm(int kp) {  // swaps the middle quads; an involution
  return (kp & 3) | ((kp & 4) << 1) | ((kp & 8) >> 1);
}
// Layer 0 (BF32) stages its fp32 input itself, as a row-major [16 rows][128 columns]
// LDS image with 8-column chunks XOR-swizzled by 4 (row & 3), read with transposing loads
__device__ __forceinline__ int x6c_tile_swz(int r, int c) {
  return ((((c >> 3) ^ (4 * (r & 3)))) << 3) + (c & 7);
}

// x3h scales of the spectral MLP (one workgroup): per layer l a weight scale
// tau_l = 2^(15 - e) for the largest of |Wr|, |Wi|, |Wr + Wi| (= f 2^e, f in
// [0.5, 1)), and the row bound nu_l = max_o sum_i (|Wr| + |Wi|): a layer whose
// inputs are bounded by 2^14 in absolute value (re and im) has outputs bounded by
// nu_l 2^14, which sigma_l = 2^-ceil(log2 nu_l) brings back under 2^14 (so the next
// B operand Xr + Xi stays under 2^15 < 65504).  The hidden layers' epilogue
// multiplier is sigma_l / tau_l; the output layer's 1 / (tau_L prod sigma_l) (the
// per-column input scale of layer 0 is undone separately).  scl[2 l] = tau_l,
// scl[2 l + 1] = the multiplier.
__global__ void spec_scales_x3h_kernel(SpecWeightsX6p a) {
  __shared__ float red_m[256], red_n[256];
  float prod_sigma = 1.f;
  for (int l = 0; l < a.nlayers; ++l) {
    const int ci = a.ci[l], co = a.co[l];
    float m = 0.f, nu = 0.f;
    for (int o = threadIdx.x; o < co; o += blockDim.x) {
      float rsum = 0.f;
      for (int i = 0; i < ci; ++i) {
        const float wr = a.w[l][((int64_t)i * co + o) * 2], wi = a.w[l][((int64_t)i * co + o) * 2 + 1];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(wr), fabsf(wi)), fabsf(wr + wi)));
        rsum += fabsf(wr) + fabsf(wi);
      }
      nu = fmaxf(nu, rsum);
    }
    red_m[threadIdx.x] = m;
    red_n[threadIdx.x] = nu;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        red_m[threadIdx.x] = fmaxf(red_m[threadIdx.x], red_m[threadIdx.x + s]);
        red_n[threadIdx.x] = fmaxf(red_n[threadIdx.x], red_n[threadIdx.x + s]);
      }
      __syncthreads();
    }
    m = red_m[0];
    nu = red_n[0];
    __syncthreads();
    // row_scale(m, 15), spelled out (the call changes this kernel's register allocation)
    int e = 0;
    float tau = 1.f;
    if (m > 0.f && isfinite(m)) {
      frexpf(m, &e);
      tau = ldexpf(1.f, 15 - e);
    }
    float sigma = 1.f;
    if (nu > 0.f && isfinite(nu)) sigma = ldexpf(1.f, -(int)ceilf(log2f(nu)));
    const bool last = l == a.nlayers - 1;
    if (threadIdx.x == 0) {
      a.scl[2 * l] = tau;
      a.scl[2 * l + 1] = last ? 1.f / (tau * prod_sigma) : sigma / tau;
    }
    prod_sigma *= sigma;
  }
}

// A image of one layer: Wr, Wi, Ws = Wr + Wi (co x ci each) from the reference
// weight w (ci, co, 2), each split into [plane][kt][Mp][16]; NP = 2: scaled by
// tau_l (a.scl) and split into two fp16 terms.  Layer 0 reads fp32 rows and has its
// channels in order along k; every later layer reads fragment-order planes and has
// them in the planes' order within each k-tile (x6c_kperm; channels >= ci stay 0)
template <int NP = 3>
__global__ void spec_weights_3m_kernel(SpecWeightsX6p a) {
  const int64_t total = a.start[a.nlayers];
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * blockDim.x) {
    int l = 0;
    while (l + 1 < a.nlayers && g >= a.start[l + 1]) ++l;
    const int ci = a.ci[l], co = a.co[l];
    const int Mp = (co + X6C_BM - 1) / X6C_BM * X6C_BM, KT = (ci + X6C_BK - 1) / X6C_BK;
    const int64_t n = (int64_t)Mp * KT * 8;  // pairs per plane
    const int64_t e = g - a.start[l];
    const int mat = (int)(e / n);
    const int64_t f = e - mat * n;
    const int64_t idx = 2 * f;
    const int kt = (int)(idx / ((int64_t)Mp * 16));
    const int rem = (int)(idx - (int64_t)kt * Mp * 16);
    // l >= 1: the B operand arrives as fragment-order planes, whose k position kp of
    // k-tile kt holds channel 16 kt + x6c_kperm(kp) (kp even: the pair stays a pair)
    const int kp = rem & 15;
    const int o = rem >> 4, k0 = kt * 16 + (l > 0 ? x6c_kperm(kp) : kp);
    const float tau = NP == 2 ? a.scl[2 * l] : 1.f;
    float v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int i = k0 + t;
      float x = 0.f;
      if (o < co && i < ci) {
        const float wr = a.w[l][((int64_t)i * co + o) * 2], wi = a.w[l][((int64_t)i * co + o) * 2 + 1];
        x = mat == 0 ? wr : (mat == 1 ? wi : wr + wi);
      }
      v[t] = x * tau;
    }
    uint32_t t[NP];
    SplitEng<NP>::split(v[0], v[1], t);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out[l]) + mat * NP * n + f;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) out[pl * n] = t[pl];
  }
}

// WGM x WGN waves: 4 x 2 (32 x 64 per wave, two waves per SIMD) or 2 x 2 (64 x 64
// per wave, one wave per SIMD: a third fewer LDS fragment reads per MFMA)
// BF32: the B operand arrives as fp32 Re / Im rows (layer 0, straight from the
// forward Legendre GEMM): each thread loads a float4 of Re and of Im for the next
// k-tile before the current one's MFMAs, and after them forms Re + Im, splits the
// three into bf16x3 and writes the nine B planes into the LDS stage; only A is DMA'd
// LAY: bit 1 = B planes read in the tiled layout, bit 2 = planes written tiled
// NS: LDS stages (2; 3 for the x3h DMA-fed layers: two k-tiles in flight, 144 KB)
// BM_: tile rows (128, or 64 for grids that would not fill the chip: the 120 x 240
// blocks of the network, N = 7,260 modes, 57 column tiles)
template <bool PLANES_OUT, int WGM = 4, int WGN = 2, bool BF32 = false, int DBG = 0, int LAY = 0,
          int NP = 3, int NS = 2, int BM_ = X6C_BM>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_x6c_kernel(X6CParams p) {
  constexpr int BM = BM_, BN = X6C_BN, BK = X6C_BK;
  constexpr int NW = WGM * WGN;
  constexpr int NMP = 3 * NP;                 // matrix-planes per operand
  constexpr int APC = (BM / 32) * NMP;        // A pieces (1 KB: 32 rows x 16 k) per k-tile
  constexpr int BPC = 4 * NMP;                // B pieces (1 KB: 4 k rows x 128) per k-tile
  static_assert(BM % 32 == 0 && X6C_BM % BM == 0, "tile rows");
  static_assert(BF32 || (APC + BPC) % NW == 0, "DMA pieces per wave");
  constexpr int NPC = BF32 ? (APC + NW - 1) / NW : (APC + BPC) / NW;  // DMA pieces per wave and k-tile
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int MT = WM / 32, NT = WN / 32;
  constexpr int A_PLANE = BM * BK, B_PLANE = BK * BN;  // 16-bit elements per matrix plane
  constexpr int A_ALL = NMP * A_PLANE;
  constexpr int STAGE = NMP * (A_PLANE + B_PLANE);      // 72 KB (x6) / 48 KB (x3h)
  constexpr int NSTAGE = NS;
  static_assert(NS == 2 || (NS == 3 && !BF32), "three stages: DMA-fed B only");
  static_assert(DBG == 0, "DBG: timing builds with wrong results (no DMA wait, no DMA, no MFMAs)");
  constexpr int RING_BYTES = NSTAGE * STAGE * 2;
  constexpr int EPI_BYTES = 32 * WGM * (BN + 8) * 4;
  constexpr int LDS_BYTES = RING_BYTES > EPI_BYTES ? RING_BYTES : EPI_BYTES;
  static_assert(STAGE * 2 == (APC + BPC) * 1024, "stage = A + B pieces of 1 KB");
  // hidden planes leave in the tiled layout only
  static_assert(PLANES_OUT == ((LAY & 2) != 0), "plane output is tiled, fp32 row output is not");
  typedef typename SplitEng<NP>::frag Frag;
  __shared__ __attribute__((aligned(16))) char lds_raw[LDS_BYTES];
  unsigned short* const ring = reinterpret_cast<unsigned short*>(lds_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int half = lane >> 5, l32 = lane & 31;

  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = lin % p.tiles_m, tn = lin / p.tiles_m;
  const int z = blockIdx.z;
  const int m0 = tm * BM, n0 = tn * BN;
  const int K = p.ci, N = p.N;
  const int nk = (K + BK - 1) / BK;
  const unsigned short* X = p.X + z * p.x_b;

  // LDS-DMA pieces c = wave + NW q (q < NPC): c < APC -> A (matrix-plane c / 4, rows
  // 32 (c % 4) ..), else B (matrix-plane (c - APC) / 4, 32-column block (c - APC) % 4)
  // Each piece is addressed as a wave-uniform base that advances with the k-tile (A: the
  // weight image; B: this column tile's planes, tiled layout) plus the lane's 32-bit byte
  // offset voff, computed once (the hosts check that the weight image stays below 4 GB).
  static_assert(BF32 || (LAY & 1) != 0, "DMA-fed B planes come in the tiled layout");
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  uint32_t voff[NPC];
  int dst[NPC];
  int kind[NPC];  // wave-uniform: 0 = A piece, 1 = B piece, -1 = none (BF32: no B pieces)
#pragma unroll
  for (int q = 0; q < NPC; ++q) {
    const int c = wave_u + NW * q;
    if (BF32 && c >= APC) {
      voff[q] = 0;
      dst[q] = 0;
      kind[q] = -1;
    } else if (c < APC) {
      const int mp = c / (BM / 32), mb = c % (BM / 32);
      const int mat = mp / NP, pl = mp - NP * mat;
      const int m = 32 * mb + (lane >> 1);
      const int h = (lane & 1) ^ ((m >> 3) & 1);
      voff[q] = (uint32_t)((mat * p.a_mat + pl * p.a_plane + (int64_t)(m0 + m) * 16 + 8 * h) * 2);
      dst[q] = mp * A_PLANE + mb * 32 * BK;
      kind[q] = 0;
    } else {
      const int bp = c - APC;
      const int mp = bp >> 2, cb = bp & 3;
      voff[q] = (uint32_t)((mp * B_PLANE + cb * 512 + lane * 8) * 2);
      dst[q] = A_ALL + mp * B_PLANE + cb * 512;
      kind[q] = 1;
    }
  }
  const uint64_t a_base = reinterpret_cast<uint64_t>(p.Aw), a_kbytes = (uint64_t)p.Mp * 16 * 2;
  const uint64_t b_base =
      BF32 ? 0 : reinterpret_cast<uint64_t>(X + (int64_t)tn * p.kt_in * NMP * B_PLANE);
  constexpr uint64_t b_kbytes = (uint64_t)NMP * B_PLANE * 2;
  const uint32_t ring_lds = lds_addr(ring);
  // the wave-uniform part of a refill (k-tile kt into stage st), once per k-tile
  struct Refill {
    uint64_t a, b;
    uint32_t lds;
  };
  auto refill_of = [&](int kt, int st) {
    return Refill{a_base + kt * a_kbytes, b_base + kt * b_kbytes,
                  ring_lds + (uint32_t)(st * STAGE * 2)};
  };
  // its piece q
  auto issue_piece = [&](const Refill& r, int q) {
    if (BF32 && kind[q] < 0) return;
    glds16s(kind[q] == 0 ? r.a : r.b, voff[q], r.lds + (uint32_t)(dst[q] * 2));
  };
  // a whole k-tile at once (the prologue: no MFMAs to issue it under)
  auto issue = [&](int kt, int st) {
    const Refill r = refill_of(kt, st);
#pragma unroll
    for (int q = 0; q < NPC; ++q) issue_piece(r, q);
  };
  // BF32 B staging: thread -> (k row, 4 columns); NW * 64 threads cover 16 x 128
  static_assert(!BF32 || NW * 64 * 4 == BK * BN, "BF32 staging: one float4 per thread");
  const int brow_f = tid / (BN / 4), bcol_f = 4 * (tid % (BN / 4));
  const float* Xf = BF32 ? p.Xf + z * p.xf_b : nullptr;
  float4 fre = make_float4(0.f, 0.f, 0.f, 0.f), fim = fre;
  float csb[4] = {1.f, 1.f, 1.f, 1.f};  // x3h BF32: per-column input scale of this thread's columns
  if constexpr (BF32 && NP == 2) {
    if (p.colscale) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        csb[e] = p.colscale[z * p.cs_b + min(n0 + bcol_f + e, N - 1)];
    }
  }
  static_assert(!BF32 || (LAY & 1) == 0, "BF32: fp32 rows in");
  auto load_bf = [&](int kt) {
    const int k = kt * BK + brow_f;
    const int kc = min(k, K - 1);
    const int col = min(n0 + bcol_f, (N - 1) & ~3);
    const float* r = Xf + (int64_t)kc * p.ldxf + col;
    fre = *reinterpret_cast<const float4*>(r);
    fim = *reinterpret_cast<const float4*>(r + p.xf_im);
  };
  auto store_bf = [&](int kt, int st) {
    const int k = kt * BK + brow_f;
    float re[4] = {fre.x, fre.y, fre.z, fre.w}, im[4] = {fim.x, fim.y, fim.z, fim.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // zero what is out of range (K tail, ragged N)
      const bool ok = k < K && n0 + bcol_f + e < N;
      re[e] = ok ? re[e] * csb[e] : 0.f;  // x3h: the column's input scale (else 1)
      im[e] = ok ? im[e] * csb[e] : 0.f;
    }
    const float sm[4] = {re[0] + im[0], re[1] + im[1], re[2] + im[2], re[3] + im[3]};
    const float* v[3] = {re, im, sm};
    unsigned short* base = ring + st * STAGE + A_ALL;
    const int u = bcol_f >> 3, h = (bcol_f >> 2) & 1;
    const int off = brow_f * BN + ((u ^ (4 * (brow_f & 3))) << 3) + 4 * h;
#pragma unroll
    for (int mat = 0; mat < 3; ++mat) {
      uint32_t ta[NP], tb[NP];
      SplitEng<NP>::split(v[mat][0], v[mat][1], ta);
      SplitEng<NP>::split(v[mat][2], v[mat][3], tb);
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        *reinterpret_cast<uint2*>(base + (mat * NP + pl) * B_PLANE + off) = make_uint2(ta[pl], tb[pl]);
    }
  };

  floatx16 acc[3][MT][NT];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][i][j][r] = 0.f;
  int a_off[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = wm * WM + i * 32 + l32;
    a_off[i] = row * BK + 8 * (half ^ ((row >> 3) & 1));
  }
  const int li = lane & 15, g16 = (lane >> 4) & 1;
  const int br = 8 * half + (li >> 2);
  int b_off[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if constexpr (BF32) {
      const int c = wn * WN + j * 32 + 16 * g16 + 4 * (li & 3);
      b_off[j] = A_ALL + br * BN + x6c_tile_swz(br, c);
    } else {  // fragment-order planes: the lane's 16 bytes of 32-column block cb
      b_off[j] = A_ALL + (wn * WN / 32 + j) * 512 + lane * 8;
    }
  }
  // The MFMAs of one k-tile as NG groups (matrix mat, column tile j: MT x NP-engine
  // products), each accumulator seeing its products k-tile by k-tile in engine order.  The
  // fragments of group g + 1 are read before the MFMAs of group g, and after(g) runs
  // behind them: the k-loops put the next refill's DMA pieces there.  (A DMA piece is
  // an asm statement the compiler moves no LDS read across, so the read-ahead is
  // written out here and not left to the scheduler.)
  constexpr int NG = 3 * NT;
  auto mfma_tile = [&](int st, auto&& after) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const unsigned short* base = ring + st * STAGE;
    Frag a[2][MT][NP], b[2][NP];
    auto read_frags = [&](int g) {
      const int mat = g / NT, j = g % NT;
      if (j == 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int pl = 0; pl < NP; ++pl)
            a[mat & 1][i][pl] =
                *reinterpret_cast<const Frag*>(base + (mat * NP + pl) * A_PLANE + a_off[i]);
      }
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) {
        const unsigned short* q = base + (mat * NP + pl) * B_PLANE + b_off[j];
        if constexpr (!BF32) {  // the fragment as stored: one ds_read_b128
          b[g & 1][pl] = *reinterpret_cast<const Frag*>(q);
        } else {
          const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_s16x4*)((__attribute__((address_space(3))) unsigned short*)q));
          const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_s16x4*)((__attribute__((address_space(3))) unsigned short*)(q + 4 * BN)));
          const s16x8 v = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
          b[g & 1][pl] = __builtin_bit_cast(Frag, v);
        }
      }
    };
    read_frags(0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int mat = g / NT, j = g % NT;
      if (g + 1 < NG) read_frags(g + 1);
#pragma unroll
      for (int i = 0; i < MT; ++i) SplitEng<NP>::mma(a[mat & 1][i], b[g & 1], acc[mat][i][j]);
      after(g);
    }
  };
  // piece q of a k-tile's NPC goes behind group q * NG / NPC: in order, spread evenly,
  // the first one behind the first group's MFMAs
  auto refill_after = [&](int g, const Refill& r) {
#pragma unroll
    for (int q = 0; q < NPC; ++q)
      if (q * NG / NPC == g) issue_piece(r, q);
  };

  issue(0, 0);
  if constexpr (NS == 3) {
    if (nk > 1) issue(1, 1);
  }
  if constexpr (BF32) {
    load_bf(0);
    store_bf(0, 0);
  }
  if constexpr (NS == 3) {
    // k-tiles kt and kt + 1 in flight at the top of iteration kt: wait for kt only
    // (NPC DMA instructions per wave and k-tile), then refill the stage kt - 1 left,
    // its NPC pieces spread behind the MFMA groups of this k-tile.
    //   WAR   stage (kt + 2) % 3 = (kt - 1) % 3 was last read in iteration kt - 1; every
    //         wave retired those reads (lgkmcnt(0)) before this iteration's barrier, and
    //         every piece follows the barrier in program order.
    //   RAW   k-tile kt + 2 is first read in iteration kt + 2, after that iteration's wait
    //         (vmcnt(NPC), or vmcnt(0) for the last: the wave's own pieces of kt + 2 are
    //         then retired, only those of kt + 3 may be younger) and barrier (the others').
    //   count the waits assume NPC DMA instructions per wave and k-tile, issued in k-tile
    //         order and all before the next iteration's wait; the loop issues no other
    //         vector-memory instruction (the epilogue's come after vmcnt(0)).
    // (the iterations that refill and the last two that do not are separate loops, so a
    // piece carries no branch)
    auto step = [&](int kt, auto more_c) {
      constexpr bool MORE = decltype(more_c)::value;
      if (kt + 1 < nk)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPC) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const Refill r = refill_of(kt + 2, (kt + 2) % 3);
      __builtin_amdgcn_s_setprio(1);
      mfma_tile(kt % 3, [&](int g) {
        if constexpr (MORE) refill_after(g, r);
      });
      __builtin_amdgcn_s_setprio(0);
    };
    int kt = 0;
    for (; kt + 2 < nk; ++kt) step(kt, std::true_type{});
    for (; kt < nk; ++kt) step(kt, std::false_type{});
  } else {
    // Two stages, one k-tile in flight; the refill of stage (kt + 1) & 1 is spread behind
    // the MFMA groups of k-tile kt.
    //   WAR   stage (kt + 1) & 1 was last read in iteration kt - 1 (MFMA fragments; BF32:
    //         last written by store_bf of iteration kt - 2); lgkmcnt(0) and this
    //         iteration's barrier come before every piece and before store_bf(kt + 1).
    //   RAW   k-tile kt + 1 is read in iteration kt + 1, after its vmcnt(0) (every piece of
    //         the wave, and the BF32 fp32 loads) and barrier.
    //   count vmcnt(0) only: nothing depends on the order of the pieces and the BF32
    //         loads of load_bf, which now go first so their latency has the whole k-tile.
    auto step = [&](int kt, auto more_c) {
      constexpr bool MORE = decltype(more_c)::value;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // my DMA of k-tile kt landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // everyone's landed; stage (kt + 1) & 1 is free
      const Refill r = refill_of(kt + 1, (kt + 1) & 1);
      if constexpr (BF32 && MORE) load_bf(kt + 1);
      __builtin_amdgcn_s_setprio(1);
      mfma_tile(kt & 1, [&](int g) {
        if constexpr (MORE) refill_after(g, r);
      });
      __builtin_amdgcn_s_setprio(0);
      if constexpr (BF32 && MORE) store_bf(kt + 1, (kt + 1) & 1);
    };
    for (int kt = 0; kt + 1 < nk; ++kt) step(kt, std::true_type{});
    if (nk > 0) step(nk - 1, std::false_type{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // the fp32 row epilogue goes through LDS: every wave is done with the ring first.
  // (The plane epilogue stores from registers and touches no LDS.)
  if constexpr (!PLANES_OUT) __syncthreads();

  // x3h: the layer multiplier (weight scale undone, output range) and, for the fp32
  // output rows of the last layer, the per-column factor (layer 0's input scale undone)
  float mul[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) mul[j] = 1.f;
  if constexpr (NP == 2) {
    const float ls = *p.lscale;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      mul[j] = ls;
      if constexpr (!PLANES_OUT) {
        if (p.colscale) mul[j] *= p.colscale[z * p.cs_b + min(n0 + wn * WN + j * 32 + l32, N - 1)];
      }
    }
  }
  // Re = P1 - P2 (ComplexReLU on hidden layers), Im = P3 - P1 - P2, Ys = Re + Im
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p1 = acc[0][i][j][r] * mul[j], p2 = acc[1][i][j][r] * mul[j],
                    p3 = acc[2][i][j][r] * mul[j];
        float re = p1 - p2;
        const float im = p3 - p1 - p2;
        if (p.relu) re = fmaxf(re, 0.f);
        acc[0][i][j][r] = re;
        acc[1][i][j][r] = im;
        acc[2][i][j][r] = re + im;
      }
  if constexpr (PLANES_OUT) {
    // fragment-order planes, every row and column of the tile (pad rows / columns are
    // 0: zero weight rows, zero B columns).  Accumulator register r of lane (l32, half)
    // is row 8 (r >> 2) + 4 half + (r & 3) of column l32 of its 32 x 32 block, so
    // registers 8 t .. 8 t + 7 are, as they stand, the lane's B fragment of k-tile
    // (block row >> 4) + t of the next layer (x6c_kperm): split in pairs and stored as
    // 16 bytes per plane, 1 KB contiguous per wave.  No LDS, no barrier.
    unsigned short* Yt = p.Y + z * p.y_b + (int64_t)tn * p.kt_out * NMP * B_PLANE;
#pragma unroll
    for (int mat = 0; mat < 3; ++mat)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int kt = (m0 + wm * WM + 32 * i) / 16 + t, cb = wn * WN / 32 + j;
            uint32_t w[4][NP];
#pragma unroll
            for (int e = 0; e < 4; ++e)
              SplitEng<NP>::split(acc[mat][i][j][8 * t + 2 * e], acc[mat][i][j][8 * t + 2 * e + 1], w[e]);
            unsigned short* d = Yt + (kt * NMP + mat * NP) * B_PLANE + cb * 512 + lane * 8;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
              *reinterpret_cast<uint4*>(d + pl * B_PLANE) =
                  make_uint4(w[0][pl], w[1][pl], w[2][pl], w[3][pl]);
          }
  } else {
    float* lds = reinterpret_cast<float*>(lds_raw);
    GemmParams q{};
    q.vecC = 1;
#pragma unroll
    for (int mat = 0; mat < 2; ++mat) {
      float* C = p.S + z * p.s_b + (mat ? p.s_im : 0);
      q.vecC = (p.ldS % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 15) == 0);
      gemm_epilogue<BM, BN, 0, WGM, WGN>(q, acc[mat], lds, nullptr, C, nullptr, p.co, N, p.ldS,
                                         m0, n0);
      __syncthreads();
    }
  }
}

// ---- host ---------------------------------------------------------------------

// the kernel addresses the A pieces by 32-bit byte offsets into the layer's weight image
// (three matrices of a_mat 16-bit elements)
static bool x6c_image_fits(const X6CParams& p) { return 3 * p.a_mat * 2 < (1LL << 32); }

size_t gemm_x6c_weight_bytes(int co, int ci) {
  const int64_t Mp = round_up(co, X6C_BM), Kp = round_up(ci, X6C_BK);
  return (size_t)round_up(3 * 3 * Mp * Kp * 2, 256);
}

size_t spec_weights_3m_layout(SpecWeightsX6p& a) {
  size_t bytes = 0;
  a.start[0] = 0;
  for (int l = 0; l < a.nlayers; ++l) {
    a.start[l + 1] = a.start[l] + 3 * round_up(a.co[l], X6C_BM) * cdiv(a.ci[l], X6C_BK) * 8;
    bytes += gemm_x6c_weight_bytes(a.co[l], a.ci[l]);
  }
  return bytes;
}

int launch_spec_weights_3m(const SpecWeightsX6p& a, hipStream_t s) {
  if (a.nlayers <= 0) return MSFNO_OK;
  const int blocks = (int)std::min<int64_t>(cdiv(a.start[a.nlayers], 256), 4096);
  hipLaunchKernelGGL(spec_weights_3m_kernel<3>, dim3(blocks), dim3(256), 0, s, a);
  return launch_check("spec_weights_3m");
}

// layer 0 on fp32 input rows (Re at Sin + b*2*ci*ldSin, Im ci rows later), split while
// staged: out 3M planes Y in the tiled layout
int gemm_x6c_f32b(const unsigned short* Aw, int co, int ci, const float* Sin, int ldSin, int N,
                  unsigned short* Y, int ldy, bool relu, int B, hipStream_t s) {
  if (co <= 0 || N <= 0 || B <= 0) return MSFNO_OK;
  MSFNO_REQUIRE(ldSin % 4 == 0 && (reinterpret_cast<uintptr_t>(Sin) & 15) == 0 && ldSin >= N,
                MSFNO_EINVAL, "gemm_x6c_f32b: fp32 rows need ld % 4 == 0 and 16-B alignment");
  MSFNO_REQUIRE(Y && ldy % 8 == 0, MSFNO_EINVAL, "gemm_x6c_f32b: plane output, ld % 8 == 0");
  X6CParams p{};
  p.Mp = (int)round_up(co, X6C_BM);
  const int KT = (int)cdiv(ci, X6C_BK);
  p.Aw = Aw;
  p.a_plane = (int64_t)p.Mp * KT * 16;
  p.a_mat = 3 * p.a_plane;
  MSFNO_REQUIRE(x6c_image_fits(p), MSFNO_EINVAL, "gemm_x6c: weight image of 4 GB or more");
  p.Xf = Sin;
  p.xf_b = 2LL * ci * ldSin;
  p.xf_im = (int64_t)ci * ldSin;
  p.ldxf = ldSin;
  p.ldx = 8;  // unused (no B planes)
  p.Y = Y;
  p.y_plane = (int64_t)co * ldy;
  p.y_mat = 3 * p.y_plane;
  p.y_b = 3 * p.y_mat;
  p.ldy = ldy;
  p.co = co; p.ci = ci; p.N = N;
  p.tiles_m = p.Mp / X6C_BM;
  p.tiles_n = (int)cdiv(N, X6C_BN);
  p.relu = relu ? 1 : 0;
  const dim3 grid(p.tiles_m * p.tiles_n, 1, B);
  p.kt_out = p.Mp / 16;
  p.y_b = x6c_tiled_elems(co, N);
  hipLaunchKernelGGL((gemm_x6c_kernel<true, 4, 2, true, 0, 2>), grid, dim3(512), 0, s, p);
  return launch_check("gemm_x6c_f32b");
}

// elements of one field's tiled 3M activation with `rows` channel rows, N columns
int64_t x6c_tiled_elems(int rows, int N) {
  return cdiv(N, X6C_BN) * round_up(rows, X6C_BM) * 9 * X6C_BN;
}

// one spectral-MLP layer on tiled 3M planes X (ci rows) -> tiled planes Y (co rows; relu)
// or, with S given, fp32 rows [b][re/im][co] of S (ld ldS)
int gemm_x6c(const unsigned short* Aw, int co, int ci, const unsigned short* X, int N, int ldx,
             unsigned short* Y, float* S, int ldS, bool relu, int B, hipStream_t s) {
  if (co <= 0 || N <= 0 || B <= 0) return MSFNO_OK;
  MSFNO_REQUIRE(ldx % 8 == 0 && ldx >= 8 && (reinterpret_cast<uintptr_t>(X) & 15) == 0,
                MSFNO_EINVAL, "gemm_x6c: X planes need ld % 8 == 0 and 16-B alignment");
  MSFNO_REQUIRE((Y != nullptr) != (S != nullptr), MSFNO_EINVAL, "gemm_x6c: one output");
  X6CParams p{};
  p.Mp = (int)round_up(co, X6C_BM);
  const int KT = (int)cdiv(ci, X6C_BK);
  p.Aw = Aw;
  p.a_plane = (int64_t)p.Mp * KT * 16;
  p.a_mat = 3 * p.a_plane;
  MSFNO_REQUIRE(x6c_image_fits(p), MSFNO_EINVAL, "gemm_x6c: weight image of 4 GB or more");
  p.X = X;
  p.x_plane = (int64_t)ci * ldx;
  p.x_mat = 3 * p.x_plane;
  p.x_b = x6c_tiled_elems(ci, N);
  p.ldx = ldx;
  p.Y = Y;
  p.y_plane = (int64_t)co * ldx;
  p.y_mat = 3 * p.y_plane;
  p.y_b = 3 * p.y_mat;
  p.ldy = ldx;
  p.S = S;
  p.s_b = 2LL * co * ldS;
  p.s_im = (int64_t)co * ldS;
  p.ldS = ldS;
  p.co = co; p.ci = ci; p.N = N;
  p.tiles_m = p.Mp / X6C_BM;
  p.tiles_n = (int)cdiv(N, X6C_BN);
  p.relu = relu ? 1 : 0;
  const dim3 grid(p.tiles_m * p.tiles_n, 1, B);
  p.kt_in = (int)round_up(ci, X6C_BM) / 16;
  p.kt_out = p.Mp / 16;
  if (Y) {
    p.y_b = x6c_tiled_elems(co, N);
    hipLaunchKernelGGL((gemm_x6c_kernel<true, 4, 2, false, 0, 3>), grid, dim3(512), 0, s, p);
  } else {
    hipLaunchKernelGGL((gemm_x6c_kernel<false, 4, 2, false, 0, 1>), grid, dim3(512), 0, s, p);
  }
  return launch_check("gemm_x6c");
}

// ---- x3h spectral chain --------------------------------------------------------

int launch_spec_weights_3m_x3h(const SpecWeightsX6p& a, hipStream_t s) {
  if (a.nlayers <= 0) return MSFNO_OK;
  MSFNO_REQUIRE(a.scl, MSFNO_EINVAL, "spec_weights_3m_x3h: no scale array");
  hipLaunchKernelGGL(spec_scales_x3h_kernel, dim3(1), dim3(256), 0, s, a);
  MSFNO_TRY(launch_check("spec_scales_x3h"));
  const int blocks = (int)std::min<int64_t>(cdiv(a.start[a.nlayers], 256), 4096);
  hipLaunchKernelGGL(spec_weights_3m_kernel<2>, dim3(blocks), dim3(256), 0, s, a);
  return launch_check("spec_weights_3m_x3h");
}

// per (b, column n): m = max over the C rows of |Re|, |Im| (S rows [b][re/im][c], ld
// ldS); alpha = 2^(14 - e) with m = f 2^e, f in [0.5, 1) (1 for an all-zero column).
// A workgroup = 64 columns x 16 row slices (a thread: 4 columns by float4, every 16th
// row), the slices combined through LDS: 16-B coalesced loads, 1024+ workgroups at
// the production shape instead of one latency-bound row walk per thread
__global__ __launch_bounds__(256) void spec_colscale_kernel(const float* __restrict__ S, int C, int N,
                                                            int ldS, float* __restrict__ cs,
                                                            int ldcs, int B) {
  __shared__ float4 red[16][16];
  const int b = blockIdx.y;
  const int cg = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int n = blockIdx.x * 64 + 4 * cg;
  const float* p = S + (int64_t)b * 2 * C * ldS;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n + 3 < N && (ldS & 3) == 0) {
#pragma unroll 4
    for (int r = sl; r < 2 * C; r += 16) {
      const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)r * ldS + n);
      m.x = fmaxf(m.x, fabsf(v.x)); m.y = fmaxf(m.y, fabsf(v.y));
      m.z = fmaxf(m.z, fabsf(v.z)); m.w = fmaxf(m.w, fabsf(v.w));
    }
  } else if (n < N) {
    for (int r = sl; r < 2 * C; r += 16) {
      const float* q = p + (int64_t)r * ldS + n;
      m.x = fmaxf(m.x, fabsf(q[0]));
      if (n + 1 < N) m.y = fmaxf(m.y, fabsf(q[1]));
      if (n + 2 < N) m.z = fmaxf(m.z, fabsf(q[2]));
      if (n + 3 < N) m.w = fmaxf(m.w, fabsf(q[3]));
    }
  }
  red[sl][cg] = m;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int c4 = threadIdx.x >> 2, e = threadIdx.x & 3;
  float mx = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float4 v = red[t][c4];
    mx = fmaxf(mx, e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w)));
  }
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= ldcs) return;
  float a = 1.f;
  if (col < N && mx > 0.f && isfinite(mx)) {
    int ex;
    frexpf(mx, &ex);
    a = ldexpf(1.f, 14 - ex);
  }
  cs[(int64_t)b * ldcs + col] = a;
  cs[(int64_t)(B + b) * ldcs + col] = 1.f / a;
}

int launch_spec_colscale(const float* S, int B, int C, int N, int ldS, float* cs, int ldcs,
                         hipStream_t s) {
  if (B <= 0 || N <= 0) return MSFNO_OK;
  MSFNO_REQUIRE(cs && ldcs >= N && B <= 65535, MSFNO_EINVAL, "spec_colscale: bad arguments");
  hipLaunchKernelGGL(spec_colscale_kernel, dim3((unsigned)cdiv(ldcs, 64), (unsigned)B), dim3(256),
                     0, s, S, C, N, ldS, cs, ldcs, B);
  return launch_check("spec_colscale");
}

int64_t x3c_tiled_elems(int rows, int N) {
  return cdiv(N, X6C_BN) * round_up(rows, X6C_BM) * 6 * X6C_BN;
}

int gemm_x3c(const unsigned short* Aw, int co, int ci, const float* Sin, int ldSin,
             const unsigned short* X, int N, unsigned short* Y, float* Sout, int ldSout,
             bool relu, const float* lscale, const float* colscale, int64_t cs_b, int B,
             hipStream_t s) {
  if (co <= 0 || N <= 0 || B <= 0) return MSFNO_OK;
  MSFNO_REQUIRE((Sin != nullptr) != (X != nullptr), MSFNO_EINVAL, "gemm_x3c: one input");
  MSFNO_REQUIRE((Y != nullptr) != (Sout != nullptr), MSFNO_EINVAL, "gemm_x3c: one output");
  MSFNO_REQUIRE(lscale, MSFNO_EINVAL, "gemm_x3c: no layer scale");
  MSFNO_REQUIRE(!Sin || (ldSin % 4 == 0 && ldSin >= N && (reinterpret_cast<uintptr_t>(Sin) & 15) == 0),
                MSFNO_EINVAL, "gemm_x3c: fp32 rows need ld % 4 == 0 and 16-B alignment");
  MSFNO_REQUIRE(!(Sin && Sout), MSFNO_EINVAL, "gemm_x3c: an fp32 layer writes planes");
  X6CParams p{};
  p.Mp = (int)round_up(co, X6C_BM);
  const int KT = (int)cdiv(ci, X6C_BK);
  p.Aw = Aw;
  p.a_plane = (int64_t)p.Mp * KT * 16;
  p.a_mat = 2 * p.a_plane;
  MSFNO_REQUIRE(x6c_image_fits(p), MSFNO_EINVAL, "gemm_x3c: weight image of 4 GB or more");
  p.Xf = Sin;
  p.xf_b = 2LL * ci * ldSin;
  p.xf_im = (int64_t)ci * ldSin;
  p.ldxf = ldSin;
  p.X = X;
  p.x_b = x3c_tiled_elems(ci, N);
  p.ldx = 8;
  p.kt_in = (int)round_up(ci, X6C_BM) / 16;
  p.Y = Y;
  p.y_b = x3c_tiled_elems(co, N);
  p.kt_out = p.Mp / 16;
  p.S = Sout;
  p.s_b = 2LL * co * ldSout;
  p.s_im = (int64_t)co * ldSout;
  p.ldS = ldSout;
  p.co = co; p.ci = ci; p.N = N;
  p.tiles_m = p.Mp / X6C_BM;
  p.tiles_n = (int)cdiv(N, X6C_BN);
  p.relu = relu ? 1 : 0;
  p.lscale = lscale;
  p.colscale = colscale;
  p.cs_b = cs_b;
  const dim3 grid(p.tiles_m * p.tiles_n, 1, B);
  // three LDS stages for the DMA-fed layers (two k-tiles in flight): layers 1/2
  // 0.51 -> 0.49 ms, output 0.31 -> 0.29 ms against two stages (two interleaved pairs)
  // grids that would not fill the chip twice (the network's 120 x 240 blocks: 57 column
  // tiles) take 64-row tiles of four waves, two stages, two workgroups per CU
  // (MSFNO_X3C_BM64=0 keeps the 128-row tiles; 2 takes 64 rows for every DMA-fed layer:
  // hidden layers 0.65 vs 0.54 ms in-block, the output layer no faster once it is timed
  // beside the same side-stream skip: 0.293 ms with 64 rows in profiles/r06_v vs 0.292
  // with 128 in profiles/r06_t/ab_bm64.txt)
  static const int bm64_on = sw_int("MSFNO_X3C_BM64", 1);
  if (!Sin && bm64_on && ((int64_t)p.tiles_m * p.tiles_n * B < 2 * 256 || bm64_on == 2)) {
    p.tiles_m = p.Mp / 64;
    const dim3 g64(p.tiles_m * p.tiles_n, 1, B);
    if (Y)
      hipLaunchKernelGGL((gemm_x6c_kernel<true, 2, 2, false, 0, 3, 2, 2, 64>), g64, dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((gemm_x6c_kernel<false, 2, 2, false, 0, 1, 2, 2, 64>), g64, dim3(256), 0, s, p);
    return launch_check("gemm_x3c");
  }
  // layer 0 (fp32 rows in) on the small grids too: 64-row tiles, 8 waves of 32 x 32 (the
  // fp32 staging needs 512 threads), two stages, two workgroups per CU: config 3 131.7 /
  // 132.3 / 132.1 vs 131.3 / 131.8 / 131.5 steps/s (three interleaved pairs,
  // profiles/r06_ac; MSFNO_X3C_L0_BM64=0 keeps the 128-row tiles)
  static const bool l0_bm64 = sw_on("MSFNO_X3C_L0_BM64");
  if (Sin && l0_bm64 && bm64_on && (int64_t)p.tiles_m * p.tiles_n * B < 2 * 256) {
    p.tiles_m = p.Mp / 64;
    const dim3 g64(p.tiles_m * p.tiles_n, 1, B);
    hipLaunchKernelGGL((gemm_x6c_kernel<true, 2, 4, true, 0, 2, 2, 2, 64>), g64, dim3(512), 0, s, p);
    return launch_check("gemm_x3c");
  }
  if (Sin)
    hipLaunchKernelGGL((gemm_x6c_kernel<true, 4, 2, true, 0, 2, 2>), grid, dim3(512), 0, s, p);
  else if (Y)
    hipLaunchKernelGGL((gemm_x6c_kernel<true, 4, 2, false, 0, 3, 2, 3>), grid, dim3(512), 0, s, p);
  else
    hipLaunchKernelGGL((gemm_x6c_kernel<false, 4, 2, false, 0, 1, 2, 3>), grid, dim3(512), 0, s, p);
  return launch_check("gemm_x3c");
}

}  // namespace msfno
