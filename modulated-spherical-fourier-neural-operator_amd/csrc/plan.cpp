// SHT plans: the spectral layout, the per-m Legendre GEMM descriptors and their caches,
// plan construction and table loading, and the stand-alone scalar and vector transforms.
#include <algorithm>
#include <cmath>
#include <functional>

#include "block.h"

namespace msfno {

void SpecLayout::build(int lmax_, int mmax_, const std::vector<char>* mask) {
  lmax = lmax_;
  mmax = mmax_;
  L.assign(mmax, 0);
  Lp.assign(mmax, 0);
  Lpe.assign(mmax, 0);
  off.assign(mmax, 0);
  T = Tp = 0;
  mact = 0;
  for (int m = 0; m < mmax; ++m) {
    const int l = (mask && !(*mask)[m]) ? 0 : std::max(lmax - m, 0);
    L[m] = l;
    Lpe[m] = (int)round_up((l + 1) / 2, 8);  // 8: 16-B bf16 chunks of the x6 Legendre GEMM
    Lp[m] = Lpe[m] + (int)round_up(l / 2, 8);
    off[m] = (int)Tp;
    T += l;
    Tp += Lp[m];
    if (l > 0) mact = m + 1;
  }
  ldT = round_up(std::max<int64_t>(Tp, 8), 8);
}

// Legendre GEMM tiles (descriptor layout and launch must agree)
static GemmTile leg_tile(int inverse) { return inverse ? TILE_128x128 : TILE_128x64; }

// the per-(m, parity) Legendre problems of a plan for R rows, in launch order:
// forward A = Xt slab (R x K), B = table, C = S (ld ldT); inverse A = S (ld ldT),
// B = table, C = Yt slab (R x N); symmetric plans: one even- and one odd-parity
// problem per m (tiles not set)
static void leg_problems(const msfno_sht_plan_s* p, int R, int64_t ldT,
                         const std::function<void(GemmDesc)>& push) {
  const SpecLayout& L = p->spec;
  const int ldko = (int)round_up(p->Ko, 4);
  for (int m = 0; m < L.mact; ++m) {
    if (L.L[m] == 0) continue;  // m outside a sharded plan's m-set
    const int64_t slab = (int64_t)p->slab[m] * R * p->ldk;
    const int lpe = L.Lpe[m], lpo = L.Lp[m] - L.Lpe[m];
    const int le = (L.L[m] + 1) / 2, lo = L.L[m] / 2;
    GemmDesc g{};
    g.M = R;
    if (p->band_world) {
      // band plan: A (forward) / C (inverse) is the exchange buffer [p][slab][R][2W],
      // its K / N index the exchange columns (segmented in the launch, legendre_*)
      const int W = p->band_W, ld = 2 * W, Kb = p->band_K();
      const int64_t bs = (int64_t)p->slab[m] * R * ld;
      if (!p->sym) {
        if (!p->inverse) {
          g.N = L.Lp[m]; g.K = Kb; g.lda = ld; g.ldb = L.Lp[m]; g.ldc = (int)ldT;
          g.offA = bs; g.offB = p->tab_off[m]; g.offC = L.off[m];
        } else {
          g.N = Kb; g.K = L.Lp[m]; g.lda = (int)ldT; g.ldb = Kb; g.ldc = ld;
          g.offA = L.off[m]; g.offB = p->tab_off[m]; g.offC = bs;
        }
        push(g);
      } else if (!p->inverse) {
        GemmDesc e = g;  // even: Xs (R x Kb) . We (Kb x Lpe)
        e.N = lpe; e.K = Kb; e.lda = ld; e.ldb = lpe; e.ldc = (int)ldT;
        e.offA = bs; e.offB = p->tab_off[m]; e.offC = L.off[m];
        push(e);
        if (lo > 0) {
          GemmDesc o = g;  // odd: Xa (R x Kb) . Wo (Kb x Lpo)
          o.N = lpo; o.K = Kb; o.lda = ld; o.ldb = lpo; o.ldc = (int)ldT;
          o.offA = bs + W; o.offB = p->tab_off[m] + (int64_t)Kb * lpe; o.offC = L.off[m] + lpe;
          push(o);
        }
      } else {
        GemmDesc e = g;  // even: E (R x Kb) = S_e (R x Le) . Pe (Le x Kb)
        e.N = Kb; e.K = le; e.lda = (int)ldT; e.ldb = Kb; e.ldc = ld;
        e.offA = L.off[m]; e.offB = p->tab_off[m]; e.offC = bs;
        push(e);
        GemmDesc o = g;  // odd: O (R x Kb); K = 0 writes zeros (the receiver reads O)
        o.N = Kb; o.K = lo; o.lda = (int)ldT; o.ldb = Kb; o.ldc = ld;
        o.offA = L.off[m] + lpe; o.offB = p->tab_off[m] + (int64_t)lpe * Kb; o.offC = bs + W;
        push(o);
      }
      continue;
    }
    if (!p->sym) {
      if (!p->inverse) {
        g.N = L.Lp[m]; g.K = p->nlat;
        g.lda = p->ldk; g.ldb = L.Lp[m]; g.ldc = (int)ldT;
        g.offA = slab; g.offB = p->tab_off[m]; g.offC = L.off[m];
      } else {
        g.N = p->nlat; g.K = L.Lp[m];
        g.lda = (int)ldT; g.ldb = p->ldk; g.ldc = p->ldk;
        g.offA = L.off[m]; g.offB = p->tab_off[m]; g.offC = slab;
      }
      push(g);
      continue;
    }
    if (!p->inverse) {
      GemmDesc e = g;  // even: Xs (R x Ke) . We (Ke x Lpe)
      e.N = lpe; e.K = p->Ke; e.lda = p->ldk; e.ldb = lpe; e.ldc = (int)ldT;
      e.offA = slab; e.offB = p->tab_off[m]; e.offC = L.off[m];
      push(e);
      if (lo > 0) {
        GemmDesc o = g;  // odd: Xa (R x Ko) . Wo (Ko x Lpo)
        o.N = lpo; o.K = p->Ko; o.lda = p->ldk; o.ldb = lpo; o.ldc = (int)ldT;
        o.offA = slab + p->ldke; o.offB = p->tab_off[m] + (int64_t)p->Ke * lpe;
        o.offC = L.off[m] + lpe;
        push(o);
      }
    } else {
      GemmDesc e = g;  // even: E (R x Ke) = S_e (R x Le) . Pe (Le x Ke)
      e.N = p->Ke; e.K = le; e.lda = (int)ldT; e.ldb = p->ldke; e.ldc = p->ldk;
      e.offA = L.off[m]; e.offB = p->tab_off[m]; e.offC = slab;
      push(e);
      GemmDesc o = g;  // odd: O (R x Ko) = S_o (R x Lo) . Po (Lo x Ko)
      o.N = p->Ko; o.K = lo; o.lda = (int)ldT; o.ldb = ldko; o.ldc = p->ldk;
      o.offA = L.off[m] + lpe; o.offB = p->tab_off[m] + (int64_t)lpe * p->ldke;
      o.offC = slab + p->ldke;
      push(o);  // also for lo == 0 (K = 0 writes zeros): transpose_inv_sym reads O
    }
  }
}

// descriptor and image builds allocate and copy synchronously: refused while the
// stream is being captured into a HIP graph (run the call once before capturing)
static int require_not_capturing(hipStream_t s, const char* what) {
  if (!s) return MSFNO_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
    set_error(std::string(what) + ": first use of this row count or table under HIP graph "
              "capture; run the call once before capturing");
    return MSFNO_EINVAL;
  }
  return MSFNO_OK;
}

// device copies of a descriptor list and its tile -> descriptor map
static int upload_descs(const std::vector<GemmDesc>& d, int tiles, bool tile_map,
                        msfno_sht_plan_s::DescSet* set) {
  MSFNO_CHECK_HIP(hipMalloc(&set->d, std::max<size_t>(1, d.size()) * sizeof(GemmDesc)));
  if (!d.empty())
    MSFNO_CHECK_HIP(hipMemcpy(set->d, d.data(), d.size() * sizeof(GemmDesc), hipMemcpyHostToDevice));
  if (tile_map) {
    std::vector<int> t2d((size_t)std::max(tiles, 1), 0);
    for (size_t i = 0; i < d.size(); ++i)
      for (int t = 0; t < d[i].tiles_m * d[i].tiles_n; ++t) t2d[d[i].tile_start + t] = (int)i;
    MSFNO_CHECK_HIP(hipMalloc(&set->tile, t2d.size() * sizeof(int)));
    MSFNO_CHECK_HIP(hipMemcpy(set->tile, t2d.data(), t2d.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  set->n = (int)d.size();
  set->tiles = tiles;
  return MSFNO_OK;
}

int ensure_desc(msfno_sht_plan_s* p, int R, int other_ld, int64_t ldT, hipStream_t s) {
  if (p->desc_R == R && p->d_desc) return MSFNO_OK;
  auto hit = p->desc_sets.find(R);
  if (hit != p->desc_sets.end()) {
    p->d_desc = hit->second.d;
    p->ndesc = hit->second.n;
    p->desc_tiles = hit->second.tiles;
    p->desc_R = R;
    return MSFNO_OK;
  }
  MSFNO_TRY(require_not_capturing(s, "Legendre descriptors"));
  int bm, bn;
  gemm_tile_dims(leg_tile(p->inverse), &bm, &bn);
  std::vector<GemmDesc> d;
  int tiles = 0;
  leg_problems(p, R, ldT, [&](GemmDesc g) {
    g.tiles_m = (int)cdiv(g.M, bm);
    g.tiles_n = (int)cdiv(g.N, bn);
    if (g.tiles_m * g.tiles_n == 0) return;
    g.tile_start = tiles;
    tiles += g.tiles_m * g.tiles_n;
    d.push_back(g);
  });
  (void)other_ld;
  msfno_sht_plan_s::DescSet set;
  MSFNO_TRY(upload_descs(d, tiles, false, &set));
  p->desc_sets[R] = set;
  p->d_desc = set.d;
  p->ndesc = set.n;
  p->desc_tiles = set.tiles;
  p->desc_R = R;
  return MSFNO_OK;
}

// ---- x3h Legendre (legendre_x3.hip) -------------------------------------------------
// The same problems on the x3h engine: the table as a column-scaled two-plane fp16
// image ([plane][n][Kp] per problem, built on first use after a table load), A split
// in-kernel under per-(row, k-tile) scales.  Default with the x3h engine (side stream
// off, two interleaved pairs: forward 0.32 vs 0.39 ms, inverse 0.52 vs 0.55 ms for the
// fp32-MFMA descriptor GEMM); MSFNO_LEG_X3=0 keeps the fp32 GEMM.
bool leg_x3_enabled() {
  static const bool on = sw_is1_or("MSFNO_LEG_X3", mlp_fused_h_env()) && gemm_use_x6();
  return on;
}

// inverse problems on the register-resident kernel (legendre_x3r) when every problem
// fits it (K <= X3R_KMAX, N <= X3R_NMAX); MSFNO_LEG_X3R=0 keeps the tiled kernel
static bool x3r_env() {
  static const bool on = sw_on("MSFNO_LEG_X3R");
  return on;
}

static int build_tab3(msfno_sht_plan_s* p, int R, int64_t ldT, hipStream_t s);

static int ensure_desc3(msfno_sht_plan_s* p, int R, int64_t ldT, hipStream_t s) {
  if (p->desc3_R == R && p->d_desc3 && p->tab3_valid) return MSFNO_OK;
  auto hit = p->desc3_sets.find(R);
  if (hit != p->desc3_sets.end()) {
    p->d_desc3 = hit->second.d;
    p->d_tile3 = hit->second.tile;
    p->ndesc3 = hit->second.n;
    p->desc3_tiles = hit->second.tiles;
    p->desc3_res = hit->second.res;
    p->desc3_R = R;
    if (p->tab3_valid) return MSFNO_OK;
  }
  MSFNO_TRY(require_not_capturing(s, "x3h Legendre image"));
  if (hit != p->desc3_sets.end()) return build_tab3(p, R, ldT, s);
  bool res = p->inverse && x3r_env();
  if (res)
    leg_problems(p, R, ldT, [&](GemmDesc g) {
      if (g.K > X3R_KMAX || g.N > X3R_NMAX || g.N <= 0) res = false;
    });
  p->desc3_res = res ? 1 : 0;
  std::vector<GemmDesc> d;
  int tiles = 0;
  int64_t img = 0, sc = 0;
  leg_problems(p, R, ldT, [&](GemmDesc g) {
    g.tiles_m = (int)cdiv(g.M, X3D_BM);
    g.tiles_n = res ? 1 : (int)cdiv(g.N, X3D_BN);
    // every problem gets its image, also K = 0 ones (written as zeros)
    g.offBx = img;
    g.offBs = sc;
    img += 2LL * g.N * round_up(std::max(g.K, 1), X3D_BK);
    sc += g.N;
    if (g.tiles_m * g.tiles_n == 0) return;
    g.tile_start = tiles;
    tiles += g.tiles_m * g.tiles_n;
    d.push_back(g);
  });
  msfno_sht_plan_s::DescSet set;
  MSFNO_TRY(upload_descs(d, tiles, true, &set));
  set.res = p->desc3_res;
  p->desc3_sets[R] = set;
  p->d_desc3 = set.d;
  p->d_tile3 = set.tile;
  p->ndesc3 = set.n;
  p->desc3_tiles = set.tiles;
  p->desc3_R = R;
  (void)img;
  (void)sc;
  return build_tab3(p, R, ldT, s);
}

// the x3h table image and column scales (R-independent: every descriptor set gives the
// same image offsets), rebuilt after a table load
static int build_tab3(msfno_sht_plan_s* p, int R, int64_t ldT, hipStream_t s) {
  int64_t img = 0, sc = 0;
  leg_problems(p, R, ldT, [&](GemmDesc g) {
    img += 2LL * g.N * round_up(std::max(g.K, 1), X3D_BK);
    sc += g.N;
  });
  if (!p->tab3_valid || img > p->tab3_elems || sc > p->tab3s_elems) {
    if (img > p->tab3_elems) {
      if (p->tab3) MSFNO_CHECK_HIP(hipFree(p->tab3));
      p->tab3 = nullptr;
      MSFNO_CHECK_HIP(hipMalloc(&p->tab3, std::max<int64_t>(1, img) * sizeof(unsigned short)));
      p->tab3_elems = img;
    }
    if (sc > p->tab3s_elems) {
      if (p->tab3s) MSFNO_CHECK_HIP(hipFree(p->tab3s));
      p->tab3s = nullptr;
      MSFNO_CHECK_HIP(hipMalloc(&p->tab3s, std::max<int64_t>(1, sc) * sizeof(float)));
      p->tab3s_elems = sc;
    }
    MSFNO_TRY(launch_legendre_x3_image(p->table, p->d_desc3, p->ndesc3, p->tab3, p->tab3s, s));
    p->tab3_valid = 1;
  }
  return MSFNO_OK;
}

// forward problems on legendre_x3f: the image and column scales of desc3, tiles of
// X3F_RB rows x 64 columns (column blocks of one row block adjacent).  Default with the
// x3h Legendre on symmetric, unsharded blocks with norm0 (the slab planes need its
// per-channel bound); MSFNO_LEG_X3F=0 keeps legendre_x3 on the fp32 slab.
bool x3f_env() {
  static const bool on = sw_on("MSFNO_LEG_X3F");
  return on;
}

bool x3f_usable(msfno_sht_plan_s* f) {
  if (!x3f_env() || !leg_x3_enabled() || !f->sym || f->inverse) return false;
  if (f->band_world)  // the receive buffer, segmented by source rank (W % 8 == 0)
    return f->band_W % 8 == 0 && f->band_K() <= X3F_KMAX;
  if (f->nslab != f->mmax) return false;
  return f->Ke <= X3F_KMAX && f->Ko <= X3F_KMAX && f->ldke % 8 == 0 && f->ldk % 8 == 0 &&
         std::max(f->ldke, f->ldk - f->ldke) <= cdiv(f->Ke, 64) * 64;
}

static int ensure_desc3f(msfno_sht_plan_s* p, int R, int64_t ldT, hipStream_t s) {
  MSFNO_TRY(ensure_desc3(p, R, ldT, s));
  if (p->desc3f_R == R && p->d_desc3f) return MSFNO_OK;
  auto hit = p->desc3f_sets.find(R);
  if (hit != p->desc3f_sets.end()) {
    p->d_desc3f = hit->second.d;
    p->d_tile3f = hit->second.tile;
    p->ndesc3f = hit->second.n;
    p->desc3f_tiles = hit->second.tiles;
    p->desc3f_R = R;
    return MSFNO_OK;
  }
  MSFNO_TRY(require_not_capturing(s, "x3h forward Legendre descriptors"));
  std::vector<GemmDesc> d;
  int tiles = 0;
  int64_t img = 0, sc = 0;
  leg_problems(p, R, ldT, [&](GemmDesc g) {  // the offsets ensure_desc3 gave the image
    g.offBx = img;
    g.offBs = sc;
    img += 2LL * g.N * round_up(std::max(g.K, 1), X3D_BK);
    sc += g.N;
    g.tiles_m = (int)cdiv(g.M, X3F_RB);
    g.tiles_n = (int)cdiv(g.N, 64);
    if (g.tiles_m * g.tiles_n == 0 || g.K <= 0) return;
    g.tile_start = tiles;
    tiles += g.tiles_m * g.tiles_n;
    d.push_back(g);
  });
  msfno_sht_plan_s::DescSet set;
  MSFNO_TRY(upload_descs(d, tiles, true, &set));
  p->desc3f_sets[R] = set;
  p->d_desc3f = set.d;
  p->d_tile3f = set.tile;
  p->ndesc3f = set.n;
  p->desc3f_tiles = set.tiles;
  p->desc3f_R = R;
  return MSFNO_OK;
}

// forward Legendre on the slab planes of launch_transpose_fwd_sym_h (Xp: fp16 pairs
// interleaved per 8 k, isr: 1 / sigma per row) -> S
int legendre_fwd_x3f(msfno_sht_plan_s* f, const unsigned short* Xp, const float* isr, float* S,
                     int R, hipStream_t s) {
  MSFNO_TRY(ensure_desc3f(f, R, f->spec.ldT, s));
  const int segw = f->band_world ? f->band_seg() : 0;
  const int64_t segs = f->band_world ? (int64_t)f->nslab * R * 2 * f->band_W : 0;
  return legendre_x3f(Xp, isr, f->tab3, f->tab3s, S, f->d_desc3f, f->d_tile3f,
                      f->ndesc3f, f->desc3f_tiles, s, segw, segs);
}

// Xn (BC, nlat, mmax) -> the plan's slab layout (hemispheres folded when symmetric)
int transpose_fwd_plan(const msfno_sht_plan_s* p, const float2* Xn, float* Xt, int B, int C,
                       const float* nscale, const float* nshift, hipStream_t s) {
  if (p->sym)
    return launch_transpose_fwd_sym(Xn, Xt, B, C, p->geom(), p->mmax, nscale, nshift, s);
  return launch_transpose_fwd(Xn, Xt, B, C, p->nlat, p->mmax, p->ldk, nscale, nshift, s);
}

int transpose_inv_plan(const msfno_sht_plan_s* p, const float* Yt, float2* Yn, int B, int C,
                       hipStream_t s) {
  if (p->sym) return launch_transpose_inv_sym(Yt, Yn, B, C, p->geom(), p->mmax, p->spec.mact, s);
  return launch_transpose_inv(Yt, Yn, B, C, p->nlat, p->mmax, p->spec.mact, p->ldk, s);
}

int legendre_fwd(msfno_sht_plan_s* f, const float* Xt, float* S, int R, hipStream_t s) {
  if (leg_x3_enabled()) {
    MSFNO_TRY(ensure_desc3(f, R, f->spec.ldT, s));
    GemmEpi e;
    if (f->band_world) {
      e.segA_w = f->band_seg();
      e.segA_stride = (int64_t)f->nslab * R * 2 * f->band_W;
    }
    return legendre_x3(Xt, f->tab3, f->tab3s, S, f->d_desc3, f->d_tile3, f->ndesc3,
                       f->desc3_tiles, e, s);
  }
  MSFNO_TRY(ensure_desc(f, R, 0, f->spec.ldT, s));
  GemmEpi e;
  if (f->band_world) {  // Xt is the phase-0 receive buffer: one block per source rank
    e.segA_w = f->band_seg();
    e.segA_stride = (int64_t)f->nslab * R * 2 * f->band_W;
  }
  return gemm_desc(leg_tile(0), Xt, f->table, S, f->d_desc, f->ndesc,
                   f->desc_tiles, e, s);
}

int legendre_inv(msfno_sht_plan_s* g, const float* S, float* Yt, int R, hipStream_t s) {
  if (leg_x3_enabled()) {
    MSFNO_TRY(ensure_desc3(g, R, g->spec.ldT, s));
    GemmEpi e;
    if (g->band_world) {
      e.segC_w = g->band_seg();
      e.segC_stride = (int64_t)g->nslab * R * 2 * g->band_W;
    }
    if (g->desc3_res)
      return legendre_x3r(S, g->tab3, g->tab3s, Yt, g->d_desc3, g->d_tile3, g->ndesc3,
                          g->desc3_tiles, e, s);
    return legendre_x3(S, g->tab3, g->tab3s, Yt, g->d_desc3, g->d_tile3, g->ndesc3,
                       g->desc3_tiles, e, s);
  }
  MSFNO_TRY(ensure_desc(g, R, 0, g->spec.ldT, s));
  GemmEpi e;
  if (g->band_world) {  // Yt is the phase-1 send buffer: one block per destination rank
    e.segC_w = g->band_seg();
    e.segC_stride = (int64_t)g->nslab * R * 2 * g->band_W;
  }
  return gemm_desc(leg_tile(1), S, g->table, Yt, g->d_desc, g->ndesc,
                   g->desc_tiles, e, s);
}


// per-m table offsets of the plan GEMM layout:
//   general:   fwd  W (nlat x Lp) columns in S order;  inv  P (Lp x ldk) rows in S order
//   symmetric: fwd  We (Ke x Lpe), Wo (Ko x Lpo);      inv  Pe (Lpe x ldke), Po (Lpo x ldko)
void set_table_offsets(msfno_sht_plan_s* p, int sym) {
  const SpecLayout& L = p->spec;
  p->tab_off.assign(p->mmax, 0);
  int64_t acc = 0;
  for (int m = 0; m < p->mmax; ++m) {
    p->tab_off[m] = acc;
    if (L.L[m] == 0) continue;
    const int64_t lpe = L.Lpe[m], lpo = L.Lp[m] - L.Lpe[m];
    if (p->band_world) {  // band plans: W / P blocks over the band_K() exchange columns
      acc += (int64_t)p->band_K() * L.Lp[m];
      continue;
    }
    if (!sym)
      acc += p->inverse ? (int64_t)L.Lp[m] * p->ldk : (int64_t)p->nlat * L.Lp[m];
    else
      acc += p->inverse ? lpe * p->ldke + lpo * round_up(p->Ko, 4)
                        : (int64_t)p->Ke * lpe + (int64_t)p->Ko * lpo;
  }
  p->table_elems = acc;
}

int plan_create(int nlat, int nlon, int lmax, int mmax, int inverse,
                const std::vector<char>* mask, msfno_sht_plan_s** plan) {
  MSFNO_REQUIRE(nlat > 0 && nlon > 1 && lmax > 0 && mmax > 0, MSFNO_EINVAL, "bad SHT dims");
  MSFNO_REQUIRE(mmax <= nlon / 2 + 1, MSFNO_EINVAL, "mmax must be <= nlon//2 + 1");
  MSFNO_REQUIRE(!mask || (int)mask->size() == mmax, MSFNO_EINVAL, "m-set mask must have mmax entries");
  auto* p = new msfno_sht_plan_s();
  p->nlat = nlat; p->nlon = nlon; p->lmax = lmax; p->mmax = mmax; p->inverse = inverse ? 1 : 0;
  p->nh = nlat / 2;
  p->Ke = nlat - p->nh;
  p->Ko = p->nh;
  // slab columns padded to 16: whole k-tiles of the x6 Legendre GEMM stay in a row
  p->ldke = (int)round_up(p->Ke, 16);
  p->ldk = (int)std::max<int64_t>(round_up(nlat, 16), p->ldke + round_up(p->Ko, 16));
  p->spec.build(lmax, mmax, mask);
  p->slab.assign(mmax, -1);
  for (int m = 0; m < mmax; ++m) {
    if (!mask) p->slab[m] = m;
    else if (p->spec.L[m] > 0) p->slab[m] = p->nslab++;
  }
  if (!mask) p->nslab = mmax;
  int rc = fft_plan_build(p->fft, nlon);
  if (rc != MSFNO_OK) { delete p; return rc; }
  // table sized for the general (non-symmetric) layout, the larger of the two
  set_table_offsets(p, 0);
  const int64_t acc = p->table_elems;
  p->table_cap = std::max<int64_t>(acc, 4);
  hipError_t e = hipMalloc(&p->table, p->table_cap * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&p->d_tab_off, mmax * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&p->d_Lp, mmax * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&p->d_off, mmax * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&p->d_Lpe, mmax * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(p->d_Lpe, p->spec.Lpe.data(), mmax * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->d_tab_off, p->tab_off.data(), mmax * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->d_Lp, p->spec.Lp.data(), mmax * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->d_off, p->spec.off.data(), mmax * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess && mask) {
    // tril order: row l holds m = 0..min(l, mmax-1) (torch.tril_indices(lmax, mmax),
    // layers.py:368); keep the plan's own modes in ascending global order
    std::vector<int> loc;
    loc.reserve((size_t)lmax * std::min(lmax, mmax));
    for (int l = 0; l < lmax; ++l)
      for (int m = 0; m <= std::min(l, mmax - 1); ++m) {
        if ((*mask)[m]) {
          loc.push_back((int)p->lin_modes.size());
          p->lin_modes.push_back((long long)loc.size() - 1);
        } else {
          loc.push_back(-1);
        }
      }
    e = hipMalloc(&p->d_tril_local, std::max<size_t>(loc.size(), 1) * sizeof(int));
    if (e == hipSuccess)
      e = hipMemcpy(p->d_tril_local, loc.data(), loc.size() * sizeof(int), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && !mask) {
    const SpecLayout& L = p->spec;
    std::vector<int> tcol;
    tcol.reserve((size_t)L.T);
    std::vector<char> used((size_t)L.Tp, 0);
    for (int l = 0; l < lmax; ++l)
      for (int m = 0; m <= std::min(l, mmax - 1); ++m) {
        const int64_t t = L.col(m, l);
        tcol.push_back((int)t);
        used[(size_t)t] = 1;
      }
    std::vector<int> pad;
    for (int64_t t = 0; t < L.Tp; ++t)
      if (!used[(size_t)t]) pad.push_back((int)t);
    p->npad = (int)pad.size();
    e = hipMalloc(&p->d_tcol, std::max<size_t>(tcol.size(), 1) * sizeof(int));
    if (e == hipSuccess)
      e = hipMemcpy(p->d_tcol, tcol.data(), tcol.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->d_tpad, std::max<size_t>(pad.size(), 1) * sizeof(int));
    if (e == hipSuccess && !pad.empty())
      e = hipMemcpy(p->d_tpad, pad.data(), pad.size() * sizeof(int), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    set_error(std::string("plan allocation failed: ") + hipGetErrorString(e));
    msfno_sht_plan_destroy(p);
    return MSFNO_EHIP;
  }
  *plan = p;
  return MSFNO_OK;
}

// workspace of the stand-alone scalar transforms, either direction
struct ShtBufs {
  float2* Xn;  // (bc, nlat, mmax) longitude spectra (the inverse's Yn)
  float* Xt;   // the plan's slab layout (the inverse's Yt)
  float* S;    // (2 bc, ldT) spectral rows
};

static void carve_sht(Carve& cv, ShtBufs& b, const msfno_sht_plan_s* p, int bc) {
  const int64_t R = 2LL * bc;
  b.Xn = cv.take<float2>((int64_t)bc * p->nlat * p->mmax);
  b.Xt = cv.take<float>((int64_t)p->mmax * R * p->ldk);
  b.S = cv.take<float>(R * p->spec.ldT);
}

}  // namespace msfno

using namespace msfno;

extern "C" {

int msfno_sht_plan_create(int nlat, int nlon, int lmax, int mmax, int inverse,
                          msfno_sht_plan_t* plan) {
  MSFNO_REQUIRE(plan, MSFNO_EINVAL, "null plan pointer");
  return plan_create(nlat, nlon, lmax, mmax, inverse, nullptr, plan);
}

int msfno_sht_plan_destroy(msfno_sht_plan_t p) {
  if (!p) return MSFNO_OK;
  fft_plan_free(p->fft);
  if (p->table) (void)hipFree(p->table);
  if (p->d_tab_off) (void)hipFree(p->d_tab_off);
  if (p->d_Lp) (void)hipFree(p->d_Lp);
  if (p->d_off) (void)hipFree(p->d_off);
  if (p->d_tril_local) (void)hipFree(p->d_tril_local);
  if (p->d_tcol) (void)hipFree(p->d_tcol);
  if (p->d_tpad) (void)hipFree(p->d_tpad);
  if (p->d_Lpe) (void)hipFree(p->d_Lpe);
  for (auto* sets : {&p->desc_sets, &p->desc3_sets, &p->desc3f_sets})
    for (auto& kv : *sets) {
      if (kv.second.d) (void)hipFree(kv.second.d);
      if (kv.second.tile) (void)hipFree(kv.second.tile);
    }
  if (p->tab3) (void)hipFree(p->tab3);
  if (p->tab3s) (void)hipFree(p->tab3s);
  if (p->d_kmap) (void)hipFree(p->d_kmap);
  delete p;
  return MSFNO_OK;
}

int msfno_sht_plan_load_table(msfno_sht_plan_t p, const float* table, void* stream) {
  MSFNO_REQUIRE(p && table, MSFNO_EINVAL, "null plan or table");
  hipStream_t s = (hipStream_t)stream;
  // one-time setup: detect the equatorial symmetry of this table (host sync)
  int sym = 0;
  if (!sw_set("MSFNO_NO_SYM") && p->nlat >= 2) {
    int* d_flag = nullptr;
    MSFNO_CHECK_HIP(hipMalloc(&d_flag, sizeof(int)));
    int h_flag = 0;
    hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(int), s);
    int rc = MSFNO_OK;
    if (e == hipSuccess) rc = launch_check_symmetry(table, p->mmax, p->lmax, p->nlat, d_flag, s);
    if (e == hipSuccess && rc == MSFNO_OK)
      e = hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_flag);
    MSFNO_TRY(rc);
    MSFNO_CHECK_HIP(e);
    sym = h_flag == 0;
  }
  p->sym = sym;
  set_table_offsets(p, sym);
  if (p->table_elems > p->table_cap) {  // band plans: the exchange layout can be larger
    MSFNO_CHECK_HIP(hipFree(p->table));
    p->table = nullptr;
    p->table_cap = p->table_elems;
    MSFNO_CHECK_HIP(hipMalloc(&p->table, p->table_cap * sizeof(float)));
  }
  if (p->band_world) {
    const std::vector<int>& km = sym ? p->kmap_sym : p->kmap_gen;
    if (!p->d_kmap)
      MSFNO_CHECK_HIP(hipMalloc(&p->d_kmap, p->kmap_gen.size() * sizeof(int)));
    MSFNO_CHECK_HIP(hipMemcpy(p->d_kmap, km.data(), km.size() * sizeof(int),
                              hipMemcpyHostToDevice));
  }
  MSFNO_CHECK_HIP(hipMemcpy(p->d_tab_off, p->tab_off.data(), p->mmax * sizeof(int64_t),
                            hipMemcpyHostToDevice));
  // descriptors depend on the layout (symmetric or not): every cached set goes
  MSFNO_CHECK_HIP(hipStreamSynchronize(s));
  for (auto* sets : {&p->desc_sets, &p->desc3_sets, &p->desc3f_sets}) {
    for (auto& kv : *sets) {
      if (kv.second.d) MSFNO_CHECK_HIP(hipFree(kv.second.d));
      if (kv.second.tile) MSFNO_CHECK_HIP(hipFree(kv.second.tile));
    }
    sets->clear();
  }
  p->d_desc = p->d_desc3 = p->d_desc3f = nullptr;
  p->d_tile3 = p->d_tile3f = nullptr;
  p->desc_R = -1;
  MSFNO_TRY(launch_relayout_table(*p, table, s));
  p->desc3_R = -1;
  p->desc3f_R = -1;
  p->tab3_valid = 0;  // the x3h image is rebuilt from the new table on first use
  p->table_loaded = 1;
  return MSFNO_OK;
}

size_t msfno_sht_workspace_size(msfno_sht_plan_t p, int bc) {
  if (!p) return 0;
  Carve cv;
  ShtBufs b;
  carve_sht(cv, b, p, bc);
  return cv.off;
}

int msfno_sht_forward(msfno_sht_plan_t p, const float* x, float* out, int bc, void* ws,
                      size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(p && !p->inverse, MSFNO_EINVAL, "msfno_sht_forward needs a forward plan");
  MSFNO_REQUIRE(p->table_loaded, MSFNO_EINVAL, "plan table not loaded");
  Carve cv;
  cv.base = (char*)ws;
  ShtBufs b;
  carve_sht(cv, b, p, bc);
  MSFNO_REQUIRE(ws_bytes >= cv.off, MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t R = 2LL * bc;
  const float scale = (float)(2.0 * M_PI / p->nlon);
  MSFNO_TRY(launch_fft_r2c_rows(p->fft, x, b.Xn, nullptr, (int64_t)bc * p->nlat, p->mmax, scale,
                                s));
  MSFNO_TRY(transpose_fwd_plan(p, b.Xn, b.Xt, 1, bc, nullptr, nullptr, s));
  MSFNO_TRY(legendre_fwd(p, b.Xt, b.S, (int)R, s));
  MSFNO_TRY(launch_spec_to_ref(*p, b.S, reinterpret_cast<float2*>(out), 1, bc, p->d_off, s));
  return MSFNO_OK;
}

int msfno_sht_inverse(msfno_sht_plan_t p, const float* in, float* x, int bc, void* ws,
                      size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(p && p->inverse, MSFNO_EINVAL, "msfno_sht_inverse needs an inverse plan");
  MSFNO_REQUIRE(p->table_loaded, MSFNO_EINVAL, "plan table not loaded");
  Carve cv;
  cv.base = (char*)ws;
  ShtBufs b;
  carve_sht(cv, b, p, bc);
  MSFNO_REQUIRE(ws_bytes >= cv.off, MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t R = 2LL * bc;
  MSFNO_TRY(launch_ref_to_spec(*p, reinterpret_cast<const float2*>(in), b.S, 1, bc, p->d_off, s));
  MSFNO_TRY(legendre_inv(p, b.S, b.Xt, (int)R, s));
  MSFNO_TRY(transpose_inv_plan(p, b.Xt, b.Xn, 1, bc, s));
  MSFNO_TRY(launch_fft_c2r_rows(p->fft, b.Xn, x, nullptr, nullptr, (int64_t)bc * p->nlat, p->mmax,
                                0, s));
  return MSFNO_OK;
}

// ---------------------------------------------------------------------------
// Vector transforms: two scalar transforms per direction (plan_d: D moved up one
// degree, plan_q: Q) joined by the streaming kernels of vector.hip
// ---------------------------------------------------------------------------
namespace {
struct VshtBufs {
  float2* d = nullptr;    // plan_d's spectra (2bc, lmax + 1, mmax)
  float2* q = nullptr;    // plan_q's spectra (2bc, lmax, mmax)
  float* grid = nullptr;  // inverse only: plan_q's fields (2bc, nlat, nlon)
  void* sht = nullptr;    // the scalar transforms' workspace, used by one after the other
  size_t sht_bytes = 0;
};

int vsht_pair_ok(msfno_sht_plan_t pd, msfno_sht_plan_t pq, int bc) {
  MSFNO_REQUIRE(pd && pq, MSFNO_EINVAL, "null vector transform plan");
  MSFNO_REQUIRE(bc >= 1, MSFNO_EINVAL, "vector transform: bc must be >= 1");
  MSFNO_REQUIRE(pd->nlat == pq->nlat && pd->nlon == pq->nlon && pd->mmax == pq->mmax &&
                    pd->inverse == pq->inverse,
                MSFNO_EINVAL, "vector transform: the two plans differ in grid, mmax or direction");
  MSFNO_REQUIRE(pd->lmax == pq->lmax + 1, MSFNO_EINVAL,
                "vector transform: plan_d must have lmax + 1 degrees and plan_q lmax");
  return MSFNO_OK;
}

size_t vsht_carve(Carve& cv, VshtBufs& b, msfno_sht_plan_t pd, msfno_sht_plan_t pq, int bc) {
  const int64_t n2 = 2LL * bc;
  b.d = cv.take<float2>(n2 * pd->lmax * pd->mmax);
  b.q = cv.take<float2>(n2 * pq->lmax * pq->mmax);
  if (pd->inverse) b.grid = cv.take<float>(n2 * pd->nlat * pd->nlon);
  b.sht_bytes = std::max(msfno_sht_workspace_size(pd, (int)n2), msfno_sht_workspace_size(pq, (int)n2));
  b.sht = cv.take<char>(b.sht_bytes);
  return cv.off;
}
}  // namespace

size_t msfno_vsht_workspace_size(msfno_sht_plan_t pd, msfno_sht_plan_t pq, int bc) {
  if (vsht_pair_ok(pd, pq, bc) != MSFNO_OK || bc > INT32_MAX / 2) return 0;
  Carve cv;
  VshtBufs b;
  return vsht_carve(cv, b, pd, pq, bc);
}

int msfno_vsht_forward(msfno_sht_plan_t pd, msfno_sht_plan_t pq, const float* v, float* st,
                       int bc, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(v && st && ws, MSFNO_EINVAL, "msfno_vsht_forward: null pointer");
  MSFNO_TRY(vsht_pair_ok(pd, pq, bc));
  MSFNO_REQUIRE(bc <= INT32_MAX / 2, MSFNO_EINVAL, "vector transform: bc too large");
  MSFNO_REQUIRE(!pd->inverse, MSFNO_EINVAL, "msfno_vsht_forward needs forward plans");
  MSFNO_REQUIRE(pd->table_loaded && pq->table_loaded, MSFNO_EINVAL, "plan table not loaded");
  Carve cv;
  VshtBufs b;
  cv.base = (char*)ws;
  MSFNO_REQUIRE(ws_bytes >= vsht_carve(cv, b, pd, pq, bc), MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  // (bc, 2, nlat, nlon) is a batch of 2 bc scalar fields
  MSFNO_TRY(msfno_sht_forward(pd, v, reinterpret_cast<float*>(b.d), 2 * bc, b.sht, b.sht_bytes, s));
  MSFNO_TRY(msfno_sht_forward(pq, v, reinterpret_cast<float*>(b.q), 2 * bc, b.sht, b.sht_bytes, s));
  return launch_vsht_combine(b.d, b.q, reinterpret_cast<float2*>(st), bc, pq->lmax, pq->mmax, s);
}

int msfno_vsht_inverse(msfno_sht_plan_t pd, msfno_sht_plan_t pq, const float* st, float* v,
                       int bc, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(v && st && ws, MSFNO_EINVAL, "msfno_vsht_inverse: null pointer");
  MSFNO_TRY(vsht_pair_ok(pd, pq, bc));
  MSFNO_REQUIRE(bc <= INT32_MAX / 2, MSFNO_EINVAL, "vector transform: bc too large");
  MSFNO_REQUIRE(pd->inverse, MSFNO_EINVAL, "msfno_vsht_inverse needs inverse plans");
  MSFNO_REQUIRE(pd->table_loaded && pq->table_loaded, MSFNO_EINVAL, "plan table not loaded");
  Carve cv;
  VshtBufs b;
  cv.base = (char*)ws;
  MSFNO_REQUIRE(ws_bytes >= vsht_carve(cv, b, pd, pq, bc), MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  MSFNO_TRY(launch_vsht_pack(reinterpret_cast<const float2*>(st), b.d, b.q, bc, pq->lmax,
                             pq->mmax, s));
  // plan_d's fields go to v, plan_q's beside them; the add joins them in place
  MSFNO_TRY(msfno_sht_inverse(pd, reinterpret_cast<const float*>(b.d), v, 2 * bc, b.sht,
                              b.sht_bytes, s));
  MSFNO_TRY(msfno_sht_inverse(pq, reinterpret_cast<const float*>(b.q), b.grid, 2 * bc, b.sht,
                              b.sht_bytes, s));
  return launch_vsht_add(v, b.grid, 2LL * bc * pd->nlat * pd->nlon, s);
}

}  // extern "C"
