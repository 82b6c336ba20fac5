// Forward orchestration of the fused SFNO block: workspace layout, the side stream, the
// spectral filter (run_filter: one chain per engine), the inner skip (skip_gemm, skip_fork,
// skip_fork_point: shared with band.cpp), run_spectral, the channel MLP and the
// msfno_block_* entry points.
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>

#include "block.h"

namespace msfno {

// ---------------------------------------------------------------------------
// per-device side stream: the inner-skip 1x1 conv (MFMA-bound, depends only on
// the block input) runs concurrently with the HBM-bound SHT stages (fork/join
// through events; capture-safe).  MSFNO_SIDE_STREAM=0 disables it.
// ---------------------------------------------------------------------------

// side stream at the lowest priority: the skip GEMM fills what the spectral path
// leaves (+1 % over equal priority, measured)
static hipError_t create_side_stream(hipStream_t* s) {
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
  return e;
}

int side_ctx(std::shared_ptr<SideCtx>* out, hipStream_t caller) {
  // (read at every call: tests switch it inside one process)
  const bool enabled = sw_on("MSFNO_SIDE_STREAM");
  out->reset();
  if (!enabled) return MSFNO_OK;
  // no fork while the caller's stream is being captured into a HIP graph: the
  // captured fork/join made a 12-block network step 19.0 ms instead of 12.4 ms
  // (replayed, config 3, round 2) and still 8.16 vs 8.10 ms in round 5 (profiles/r05_b);
  // the graph runs the skip GEMM in line
  if (caller) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(caller, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return MSFNO_OK;
  }
  // one side stream per device (pooled: every caller stream of that device forks to
  // it) + one fork/join event pair per (device, caller stream).  The device comes
  // from the caller's stream (not the thread's current device); two caller streams
  // never share fork/join events.  The per-caller map is bounded (LRU, kMaxCallers):
  // the oldest pair is dropped from the map, and its events are destroyed when the
  // last holder releases it (HIP releases an event whose recorded work is still
  // pending once it completes)
  static std::mutex mu;
  static std::map<int, hipStream_t> side_of_dev;
  struct Entry {
    std::shared_ptr<SideCtx> c;
    uint64_t used = 0;
  };
  static std::map<std::pair<int, hipStream_t>, Entry> ctx;
  static uint64_t tick = 0;
  constexpr size_t kMaxCallers = 64;
  int dev = 0;
  if (caller) MSFNO_CHECK_HIP(hipStreamGetDevice(caller, &dev));
  else MSFNO_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto it = ctx.find({dev, caller});
  if (it == ctx.end() && ctx.size() >= kMaxCallers) {
    auto lru = ctx.begin();
    for (auto j = ctx.begin(); j != ctx.end(); ++j)
      if (j->second.used < lru->second.used) lru = j;
    ctx.erase(lru);
  }
  Entry& en = ctx[{dev, caller}];
  en.used = ++tick;
  if (!en.c) {
    auto c = std::make_shared<SideCtx>();
    int cur = 0;
    MSFNO_CHECK_HIP(hipGetDevice(&cur));
    if (cur != dev) MSFNO_CHECK_HIP(hipSetDevice(dev));
    hipError_t e = hipSuccess;
    hipStream_t& pooled = side_of_dev[dev];
    if (!pooled) e = create_side_stream(&pooled);
    c->side = pooled;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->join, hipEventDisableTiming);
    if (cur != dev) (void)hipSetDevice(cur);
    if (e != hipSuccess) {
      ctx.erase({dev, caller});
      set_error(std::string("side stream creation failed: ") + hipGetErrorString(e));
      return MSFNO_EHIP;
    }
    en.c = std::move(c);
  }
  *out = en.c;
  return MSFNO_OK;
}

// spectral MLP on the x6 engine (real-ified 4-multiplication GEMM on the bf16
// matrix cores, fp32-accurate split) whenever the dense GEMMs use it;
// MSFNO_SPEC_X6=0 keeps the fp32 3M kernel for A/B
bool spec_use_x6() {
  static const bool on = gemm_use_x6() && sw_on("MSFNO_SPEC_X6");
  return on;
}

// ---------------------------------------------------------------------------
// block workspace layout (shared by size query and forward)
// ---------------------------------------------------------------------------


void carve_block(Carve& cv, BlockBufs& b, const msfno_block_desc* d,
                        const msfno_sht_plan_s* f, const msfno_sht_plan_s* g, int B,
                        bool with_norms) {
  const int64_t C = d->C, BC = (int64_t)B * C, R = 2 * BC;
  const int64_t P = (int64_t)g->nlat * g->nlon;
  b.Xn = cv.take<float2>(BC * f->nlat * f->mmax);
  b.Xt = cv.take<float>((int64_t)f->mmax * R * f->ldk);
  b.rs0 = cv.take<float2>(BC * f->nlat);
  b.sc0 = cv.take<float>(BC);
  b.sh0 = cv.take<float>(BC);
  carve_filter(cv, b, d, f->spec, B, 0);
  b.Yt = cv.take<float>((int64_t)g->mmax * R * g->ldk);
  b.Yn = cv.take<float2>(BC * g->nlat * g->mmax);
  b.x1 = nullptr;
  b.st1 = nullptr;
  b.sc1 = b.sh1 = b.W1f = b.b1f = b.h = nullptr;
  b.x1p = nullptr;
  b.mfimg = nullptr;
  if (!with_norms) return;
  b.x1 = cv.take<float>(BC * P);
  b.st1 = cv.take<float2>(BC * g->nlat);
  b.sc1 = cv.take<float>(BC);
  b.sh1 = cv.take<float>(BC);
  b.ab1 = cv.take<float>(BC);
  if (mlp_fused(d, P)) {
    b.mfimg = wcache_mfimg(d);
    if (!b.mfimg) b.mfimg = cv.take<unsigned short>(mlp_fused_image_bytes() / 2);
  } else if (d->has_mlp) {
    const int64_t Hd = d->mlp_hidden;
    b.W1f = cv.take<float>((int64_t)B * Hd * C);
    b.b1f = cv.take<float>((int64_t)B * Hd);
    b.h = cv.take<float>(mlp_h_floats(B, Hd, P));
  }
  b.x1p = x1p_buffer(d, g) ? cv.take<unsigned short>(BC * 3 * P) : nullptr;
  b.xs = skip_x3(d) ? cv.take<float>(BC) : nullptr;
  b.lsig = nullptr;
  b.isr = nullptr;
  if (x3f_env() && leg_x3_enabled()) {
    b.lsig = cv.take<float>(BC);
    b.isr = cv.take<float>(R);
  }
  carve_dense_ws(cv, b.dw, d, B);
}

void carve_filter(Carve& cv, BlockBufs& b, const msfno_block_desc* d, const SpecLayout& L, int B,
                  int64_t tril_floor) {
  const int64_t C = d->C, BC = (int64_t)B * C, R = 2 * BC;
  b.Sa = cv.take<float>(R * L.ldT);
  b.Sb = b.Sc = nullptr;
  b.cs = nullptr;
  for (auto& w : b.Wexp) w = nullptr;
  b.dw = DenseWs{};
  b.xt = b.yt = nullptr;
  if (d->filter_type == MSFNO_FILTER_NONLINEAR) {
    const int64_t Hs = d->spec_hidden;
    b.Sb = cv.take<float>(spec_hidden_floats(B, Hs, L));
    b.Sc = cv.take<float>(spec_hidden_floats(B, Hs, L));
    b.cs = cv.take<float>(2LL * B * round_up(L.Tp, 4));
    for (int l = 0; l <= d->spectral_layers && l < 9; ++l) {
      const int64_t ci = (l == 0) ? C : Hs;
      const int64_t co = (l == d->spectral_layers) ? C : Hs;
      b.Wexp[l] = cv.take<float>(4 * ci * co);
    }
    if (d->wcache) {
      Carve wc;
      wc.base = static_cast<char*>(d->wcache);
      carve_spec_ws(wc, b.dw, d);
    } else {
      carve_spec_ws(cv, b.dw, d);
    }
  } else {
    // the gathered copies of the linear filter's input and output (tril order)
    b.xt = cv.take<float>(std::max(2 * BC * L.T, tril_floor));
    b.yt = cv.take<float>(std::max(2 * BC * L.T, tril_floor));
  }
}

void carve_dense_ws(Carve& cv, DenseWs& w, const msfno_block_desc* d, int B) {
  w.skip = w.fc1 = w.fc2 = nullptr;
  w.skip_b = w.fc1_b = w.fc2_b = 0;
  const int C = (int)d->C;
  if (d->inner_skip == MSFNO_SKIP_LINEAR &&
      (w.skip_b = std::max({gemm_dense_workspace(C, C, 1),
                            skip_x3(d) ? gemm_x3_workspace(C, C, B) : 0,
                            skip_x3(d) && C == 256 ? skip_h_workspace(B) : 0})))
    w.skip = cv.take<char>(w.skip_b);
  if (d->has_mlp) {
    const int Hd = (int)d->mlp_hidden;
    if ((w.fc1_b = gemm_dense_workspace(Hd, C, B))) w.fc1 = cv.take<char>(w.fc1_b);
    if ((w.fc2_b = gemm_dense_workspace(C, Hd, 1))) w.fc2 = cv.take<char>(w.fc2_b);
  }
}

// spectral MLP as Gauss 3M complex GEMMs on the x6 engine (gemm_x6c.hip);
// MSFNO_SPEC_3M=0 keeps the real-ified 4M x6p GEMMs for A/B
bool spec_use_3m() {
  static const bool on = sw_on("MSFNO_SPEC_3M");
  return on && spec_use_x6();
}

// spectral MLP on the x3h engine (gemm_x3c: fp32 as two fp16 terms, three fp16 MFMAs
// per product, power-of-two scaled operands) by default; MSFNO_ENGINE=x6 or
// MSFNO_SPEC_X3H=0 keep the x6 chain (A/B)
bool spec_use_x3h() {
  static const bool on = sw_is1_or("MSFNO_SPEC_X3H", mlp_fused_h_env());
  return on && spec_use_3m();
}

// The x3h chain carries its hidden activations as two fp16 terms under fixed scales: layer
// l's output is multiplied by sigma_l = 2^-ceil(log2 nu_l), nu_l the largest row sum of
// |Wr| + |Wi| (spec_scales_x3h_kernel), so that no input bounded by 2^14 overflows.  The
// values a layer really produces are smaller than that bound by nu_l over the layer's
// gain, about 1.3 sqrt(ci) for weights without structure, whatever their scale: with the
// rounding of sigma_l to a power of two, log2(ci) / 2 + 1 bits per hidden layer.  fp16
// holds 2^14 down to the low term's floor of 2^-25, 39 bits, of which a product wants 22:
// 17 bits of headroom.  Measured (DESIGN.md §2, 13 x 26, unit-gain weights): the chain stays
// within 2 x the fp32 oracle's error up to 13.5 bits, 2.5 to 3 x at 17 and 17.5 bits, 50 x
// and more from 20 bits (hidden 32 at six layers, hidden 128 at five).  Chains that would
// drain more than X3H_RANGE_BITS take the x6 engine's 3M chain (bf16 planes: fp32's
// exponent), as MSFNO_SPEC_X3H=0 does for every chain.  The flagship's three layers of 256 ->
// 512 -> 512 drain 16 bits.
constexpr float X3H_RANGE_BITS = 16.5f;

static bool spec_x3h_range_ok(int64_t C, int64_t Hs, int nl) {
  float bits = 0.f;
  for (int l = 0; l < nl; ++l) bits += 0.5f * std::log2((float)(l == 0 ? C : Hs)) + 1.f;
  return bits <= X3H_RANGE_BITS;
}

// floats to reserve for one spectral-MLP hidden buffer (B, 2 Hs, T): fp32, or
// bf16x3 planes with a row stride padded to 8 on the x6 engine
int64_t spec_hidden_floats(int B, int64_t Hs, const SpecLayout& L) {
  if (!spec_use_x6()) return (int64_t)B * 2 * Hs * L.ldT;
  // 4M: re / im rows as 3 planes each, row stride padded to 8; 3M: the tiled layout of
  // re, im, re + im (never smaller than the 4M form)
  return std::max<int64_t>({(int64_t)B * 2 * Hs * L.ldT,
                            cdiv((int64_t)B * 6 * Hs * round_up(L.Tp, 8) * 2, 4),
                            cdiv((int64_t)B * x6c_tiled_elems((int)Hs, (int)L.Tp) * 2, 4)});
}

// prepared-weight cache layout (msfno_block_desc.wcache): the spectral images
// (carve_spec_ws order), then the fused MLP image
static size_t wcache_layout(const msfno_block_desc* d, unsigned short** mfimg) {
  Carve wc;
  wc.base = static_cast<char*>(d->wcache);
  DenseWs w;
  if (d->filter_type == MSFNO_FILTER_NONLINEAR) carve_spec_ws(wc, w, d);
  unsigned short* m = nullptr;
  if (d->has_mlp && gemm_use_x6() && d->fc1_b && mlp_fused_supported((int)d->C, (int)d->mlp_hidden))
    m = wc.take<unsigned short>(mlp_fused_image_bytes() / 2);
  if (mfimg) *mfimg = m;
  return wc.off;
}

unsigned short* wcache_mfimg(const msfno_block_desc* d) {
  if (!d->wcache) return nullptr;
  unsigned short* m = nullptr;
  wcache_layout(d, &m);
  return m;
}

bool wcache_ready(const msfno_block_desc* d) { return d->wcache && d->wcache_valid; }

// split-A planes of the real-ified spectral MLP weights (x6 engine)
void carve_spec_ws(Carve& cv, DenseWs& w, const msfno_block_desc* d) {
  for (auto& p : w.spec) p = nullptr;
  for (auto& n : w.spec_b) n = 0;
  if (!spec_use_x6() || d->filter_type != MSFNO_FILTER_NONLINEAR) return;
  for (int l = 0; l <= d->spectral_layers && l < 9; ++l) {
    const int ci = (l == 0) ? (int)d->C : (int)d->spec_hidden;
    const int co = (l == d->spectral_layers) ? (int)d->C : (int)d->spec_hidden;
    w.spec_b[l] = std::max(gemm_dense_workspace(2 * co, 2 * ci, 1), gemm_x6c_weight_bytes(co, ci));
    if (w.spec_b[l]) w.spec[l] = cv.take<char>(w.spec_b[l]);
  }
}

int check_pair(const msfno_block_desc* d, const msfno_sht_plan_s* f,
                      const msfno_sht_plan_s* g) {
  MSFNO_REQUIRE(d && f && g, MSFNO_EINVAL, "null descriptor or plan");
  MSFNO_REQUIRE(!f->inverse && g->inverse, MSFNO_EINVAL,
                "forward plan must be a RealSHT plan and inverse an InverseRealSHT plan");
  MSFNO_REQUIRE(f->lmax == g->lmax && f->mmax == g->mmax, MSFNO_EINVAL,
                "inverse_transform lmax/mmax must equal forward_transform's (layers.py:364-365)");
  MSFNO_REQUIRE(f->table_loaded && g->table_loaded, MSFNO_EINVAL, "plan tables not loaded");
  MSFNO_REQUIRE(d->C > 0, MSFNO_EINVAL, "C must be > 0");
  if (d->filter_type == MSFNO_FILTER_NONLINEAR) {
    MSFNO_REQUIRE(d->spectral_layers >= 1 && d->spectral_layers <= 8, MSFNO_EUNSUPPORTED,
                  "spectral_layers must be in [1, 8]");
    MSFNO_REQUIRE(d->spec_hidden > 0, MSFNO_EINVAL, "spec_hidden must be > 0");
  } else {
    MSFNO_REQUIRE(d->filter_type == MSFNO_FILTER_LINEAR, MSFNO_EUNSUPPORTED, "unknown filter_type");
  }
  return MSFNO_OK;
}

// the spectral MLP's layers 0 .. spectral_layers (the last is the output layer): each one's
// (ci, co, weight) and A image (b.dw.spec), for every chain and the one-launch weight
// preparations
static int spec_layers(const msfno_block_desc* d, const BlockBufs& b, SpecWeightsX6p& sw) {
  const int nl = d->spectral_layers;
  sw = SpecWeightsX6p{};
  sw.nlayers = nl + 1;
  for (int l = 0; l <= nl; ++l) {
    sw.w[l] = (l == nl) ? d->spec_wout : d->spec_w[l];
    MSFNO_REQUIRE(sw.w[l], MSFNO_EINVAL, "missing spectral weight");
    sw.ci[l] = (int)(l == 0 ? d->C : d->spec_hidden);
    sw.co[l] = (int)(l == nl ? d->C : d->spec_hidden);
    sw.out[l] = static_cast<unsigned short*>(b.dw.spec[l]);
  }
  return MSFNO_OK;
}

// x3h engine (gemm_x3c): two fp16 planes per value, three MFMAs per product; the layer
// scales (2 floats per layer) live behind layer 0's A image (inside wcache when
// the images are cached), the per-column input scales in b.cs
static int filter_x3h(const msfno_block_desc* d, const SpecLayout& L, const BlockBufs& b,
                      SpecWeightsX6p& sw, int B, hipStream_t s) {
  const int nl = d->spectral_layers;
  const int64_t a0 = round_up(6LL * round_up(sw.co[0], 128) * round_up(sw.ci[0], 16) * 2, 256);
  MSFNO_REQUIRE((size_t)a0 + 2 * (nl + 1) * sizeof(float) <= b.dw.spec_b[0], MSFNO_EWORKSPACE,
                "x3h spectral scales do not fit behind layer 0's image");
  sw.scl = reinterpret_cast<float*>(static_cast<char*>(b.dw.spec[0]) + a0);
  if (!wcache_ready(d)) MSFNO_TRY(launch_spec_weights_3m_x3h(sw, s));
  const int ldcs = (int)round_up(L.Tp, 4);
  MSFNO_TRY(launch_spec_colscale(b.Sa, B, (int)d->C, (int)L.Tp, (int)L.ldT, b.cs, ldcs, s));
  unsigned short* cur = nullptr;
  for (int l = 0; l <= nl; ++l) {
    prof(l == nl ? ST_SPEC_OUT : ST_SPEC_L0 + std::min(l, 3), s);
    unsigned short* out = l == nl ? nullptr
                                  : reinterpret_cast<unsigned short*>((l & 1) ? b.Sc : b.Sb);
    MSFNO_TRY(gemm_x3c(sw.out[l], sw.co[l], sw.ci[l], l == 0 ? b.Sa : nullptr, (int)L.ldT,
                       l == 0 ? nullptr : cur, (int)L.Tp, out, l == nl ? b.Sa : nullptr,
                       (int)L.ldT, l < nl, sw.scl + 2 * l + 1,
                       l == 0 ? b.cs : (l == nl ? b.cs + (int64_t)B * ldcs : nullptr), ldcs, B,
                       s));
    cur = out;
  }
  return MSFNO_OK;
}

// x6 engine, Gauss 3M complex GEMMs (gemm_x6c.hip): layer 0 stages S fp32 and splits it
// in-kernel; hidden activations travel in the tiled layout
static int filter_x6_3m(const msfno_block_desc* d, const SpecLayout& L, const BlockBufs& b,
                        const SpecWeightsX6p& sw, int B, hipStream_t s) {
  const int nl = d->spectral_layers;
  if (!wcache_ready(d)) MSFNO_TRY(launch_spec_weights_3m(sw, s));
  const int ldTx = (int)round_up(L.Tp, 8);
  unsigned short* cur = nullptr;
  for (int l = 0; l <= nl; ++l) {
    prof(l == nl ? ST_SPEC_OUT : ST_SPEC_L0 + std::min(l, 3), s);
    unsigned short* out = l == nl ? nullptr
                                  : reinterpret_cast<unsigned short*>((l & 1) ? b.Sc : b.Sb);
    if (l == 0)
      MSFNO_TRY(gemm_x6c_f32b(sw.out[0], sw.co[0], sw.ci[0], b.Sa, (int)L.ldT, (int)L.Tp, out,
                              ldTx, true, B, s));
    else
      MSFNO_TRY(gemm_x6c(sw.out[l], sw.co[l], sw.ci[l], cur, (int)L.Tp, ldTx, out,
                         l == nl ? b.Sa : nullptr, (int)L.ldT, l < nl, B, s));
    cur = out;
  }
  return MSFNO_OK;
}

// x6 engine, real-ified [[Wr, -Wi], [Wi, Wr]] GEMMs (MSFNO_SPEC_3M=0, or C > Hs),
// ComplexReLU(real) = ReLU on the real rows of each batch block, in the epilogue.  Hidden
// activations travel as bf16x3 planes [b][plane][2 Hs][ldTx]: later layers stage planes by
// LDS-DMA (gemm_x6p), the output layer writes fp32 S for the inverse Legendre.
static int filter_x6p(const msfno_block_desc* d, const SpecLayout& L, const BlockBufs& b,
                      SpecWeightsX6p& sw, int B, hipStream_t s) {
  const int nl = d->spectral_layers;
  const bool split_l0 = d->C <= d->spec_hidden;  // layer 0 input split into Sc (below)
  // every layer's real-ified weight straight into its x6p A image, one launch
  spec_weights_x6p_layout(sw);
  if (!wcache_ready(d)) MSFNO_TRY(launch_spec_weights_x6p(sw, s));
  if (!split_l0) MSFNO_TRY(launch_expand_complex_weight(sw.w[0], b.Wexp[0], sw.ci[0], sw.co[0], s));
  const int64_t ldTx = round_up(L.Tp, 8);
  const float* in = b.Sa;
  for (int l = 0; l <= nl; ++l) {
    const int ci = sw.ci[l], co = sw.co[l];
    float* out = (l == nl) ? b.Sa : ((l & 1) ? b.Sc : b.Sb);
    prof(l == nl ? ST_SPEC_OUT : ST_SPEC_L0 + std::min(l, 3), s);
    GemmEpi e;
    if (l < nl) {
      e.relu_period = 2 * co;
      e.relu_rows = co;
      e.c_planes = reinterpret_cast<unsigned short*>(out);
      e.c_plane_stride = 2LL * co * ldTx;
    }
    const int ldc = l < nl ? (int)ldTx : (int)L.ldT;
    const int64_t sC = l < nl ? 3 * 2LL * co * ldTx : 2LL * co * L.ldT;
    if (l == 0 && !split_l0) {  // layer 0 splits its fp32 input in-kernel
      MSFNO_TRY(gemm_dense(TILE_128x128, b.Wexp[l], in, out, 2 * co, (int)L.Tp, 2 * ci, 2 * ci,
                           (int)L.ldT, ldc, 0, 2LL * ci * L.ldT, sC, B, e, b.dw.spec[l],
                           b.dw.spec_b[l], s));
    } else {
      e.a_planes = static_cast<const unsigned short*>(b.dw.spec[l]);
      e.b_planes = reinterpret_cast<const unsigned short*>(in);
      if (l == 0) {  // Sc is free during layer 0
        // layer 0's fp32 input (the forward Legendre output) -> planes in Sc: one
        // streaming pass, then the LDS-DMA kernel (cheaper than splitting the
        // 2C x T operand once per M-tile inside the GEMM)
        unsigned short* inx = reinterpret_cast<unsigned short*>(b.Sc);
        MSFNO_TRY(launch_split_planes(in, inx, 2 * ci, (int)L.Tp, (int)L.ldT, 2LL * ci * L.ldT,
                                      (int)ldTx, 2LL * ci * ldTx, 3 * 2LL * ci * ldTx, B, s));
        e.b_planes = inx;
      }
      e.b_plane_stride = 2LL * ci * ldTx;
      MSFNO_TRY(gemm_x6p(b.Wexp[l], out, 2 * co, (int)L.Tp, 2 * ci, 2 * ci, (int)ldTx, ldc, 0,
                         3 * 2LL * ci * ldTx, sC, B, e, b.dw.spec[l], b.dw.spec_b[l], s));
    }
    in = out;
  }
  return MSFNO_OK;
}

// fp32 engine: Gauss 3-multiplication complex GEMMs (cgemm.hip), ComplexReLU(real) fused
static int filter_f32(const msfno_block_desc* d, const SpecLayout& L, const BlockBufs& b,
                      const SpecWeightsX6p& sw, int B, hipStream_t s) {
  const int nl = d->spectral_layers;
  for (int l = 0; l <= nl; ++l) {
    const int ci = sw.ci[l], co = sw.co[l];
    MSFNO_TRY(launch_split_complex_weight(sw.w[l], b.Wexp[l], b.Wexp[l] + (int64_t)ci * co, ci, co, s));
  }
  const float* in = b.Sa;
  for (int l = 0; l <= nl; ++l) {
    const int ci = sw.ci[l], co = sw.co[l];
    float* out = (l == nl) ? b.Sa : ((l & 1) ? b.Sc : b.Sb);
    prof(l == nl ? ST_SPEC_OUT : ST_SPEC_L0 + std::min(l, 3), s);
    MSFNO_TRY(gemm_c3m(b.Wexp[l], b.Wexp[l] + (int64_t)ci * co, in, out, co, ci, (int)L.Tp,
                       (int)L.ldT, (int)L.ldT, 2LL * ci * L.ldT, 2LL * co * L.ldT, B, l < nl, s));
    in = out;
  }
  return MSFNO_OK;
}

// linear filter: gather S to tril order, per-mode contraction, scatter back
static int filter_linear(const msfno_block_desc* d, const msfno_sht_plan_s& f, const BlockBufs& b,
                         int B, hipStream_t s) {
  const int C = (int)d->C;
  MSFNO_REQUIRE(d->lin_w, MSFNO_EINVAL, "missing linear spectral weight");
  prof(ST_LIN_GATHER, s);
  MSFNO_TRY(launch_spec_to_tril(f, b.Sa, b.xt, B, C, s));
  prof(ST_LIN_CONTRACT, s);
  MSFNO_TRY(launch_compl_contract(b.xt, d->lin_w, b.yt, B, C, C, f.spec.T, s));
  prof(ST_LIN_SCATTER, s);
  MSFNO_TRY(launch_tril_to_spec(f, b.yt, b.Sa, B, C, s));
  return MSFNO_OK;
}

int run_filter(const msfno_block_desc* d, msfno_sht_plan_s* f, const BlockBufs& b, int B,
               hipStream_t s) {
  if (d->filter_type != MSFNO_FILTER_NONLINEAR) return filter_linear(d, *f, b, B, s);
  const int64_t C = d->C, Hs = d->spec_hidden;
  const SpecLayout& L = f->spec;
  prof(ST_SPEC_PREP, s);
  const bool x6 = spec_use_x6() && b.dw.spec[0];
  SpecWeightsX6p sw;
  MSFNO_TRY(spec_layers(d, b, sw));
  if (!x6) return filter_f32(d, L, b, sw, B, s);
  if (!(spec_use_3m() && C <= Hs)) return filter_x6p(d, L, b, sw, B, s);
  // 3M: weights Wr, Wi, Wr+Wi of all layers in one launch
  spec_weights_3m_layout(sw);
  if (spec_use_x3h() && spec_x3h_range_ok(C, Hs, d->spectral_layers) && b.cs && L.ldT % 4 == 0)
    return filter_x3h(d, L, b, sw, B, s);
  return filter_x6_3m(d, L, b, sw, B, s);
}

int run_spectral(const msfno_block_desc* d, msfno_sht_plan_s* f, msfno_sht_plan_s* g,
                 const BlockBufs& b, const float* x, int B, bool norm0, hipStream_t s,
                 const InnerSkip* skip) {
  const int64_t C = d->C, BC = (int64_t)B * C, R = 2 * BC;
  const SkipFork at = skip ? skip->at : SKIP_NONE;
  if (at == SKIP_FIRST) MSFNO_TRY(skip_fork(*skip, s));
  prof(ST_FFT_FWD, s);
  const float scale = (float)(2.0 * M_PI / f->nlon);
  const C2RPlanes xp{b.x1p, (int)C, f->nlat};
  MSFNO_TRY(launch_fft_r2c_rows(f->fft, x, b.Xn, norm0 ? b.rs0 : nullptr, BC * f->nlat, f->mmax,
                                scale, s, at == SKIP_AFTER_FFT ? &xp : nullptr));
  if (at == SKIP_AFTER_FFT) MSFNO_TRY(skip_fork(*skip, s));
  if (norm0) {
    prof(ST_NORM0, s);
    MSFNO_TRY(launch_chan_affine(b.rs0, f->nlat, f->nlon, f->nlon, B, (int)C, d->norm0_w,
                                 d->norm0_b, d->norm_eps, nullptr, nullptr, 0.f, b.sc0, b.sh0,
                                 s, b.xs, b.lsig));
    if (at == SKIP_AFTER_NORM0) MSFNO_TRY(skip_fork(*skip, s));
  }
  prof(ST_TRANSPOSE_FWD, s);
  if (norm0 && b.lsig && b.isr && x3f_usable(f)) {
    // slab as x3h fp16 pairs in the Xt buffer (the fp32 bytes)
    unsigned short* Xp = reinterpret_cast<unsigned short*>(b.Xt);
    MSFNO_TRY(launch_transpose_fwd_sym_h(b.Xn, Xp, B, (int)C, f->geom(), f->mmax, b.sc0, b.sh0,
                                         b.lsig, b.isr, s));
    prof(ST_LEG_FWD, s);
    MSFNO_TRY(legendre_fwd_x3f(f, Xp, b.isr, b.Sa, (int)R, s));
  } else {
    MSFNO_TRY(transpose_fwd_plan(f, b.Xn, b.Xt, B, (int)C, norm0 ? b.sc0 : nullptr,
                                 norm0 ? b.sh0 : nullptr, s));
    prof(ST_LEG_FWD, s);
    MSFNO_TRY(legendre_fwd(f, b.Xt, b.Sa, (int)R, s));
  }
  MSFNO_TRY(run_filter(d, f, b, B, s));
  if (at == SKIP_BEFORE_INV) MSFNO_TRY(skip_fork(*skip, s));
  prof(ST_LEG_INV, s);
  // (the linear filter on S writes its output to Sb)
  MSFNO_TRY(legendre_inv(g, b.Sa, b.Yt, (int)R, s));
  return MSFNO_OK;
}

int run_inverse_fft(msfno_sht_plan_s* g, const BlockBufs& b, int B, int C, float* out,
                    const float* addsrc, float2* rowstats, int act, hipStream_t s,
                    unsigned short* planes) {
  const int64_t BC = (int64_t)B * C;
  prof(ST_TRANSPOSE_INV, s);
  MSFNO_TRY(transpose_inv_plan(g, b.Yt, b.Yn, B, C, s));
  prof(ST_FFT_INV, s);
  if (planes) {
    const C2RPlanes pl{planes, C, g->nlat};
    return launch_fft_c2r_rows(g->fft, b.Yn, out, addsrc, rowstats, BC * g->nlat, g->mmax, act,
                               s, &pl);
  }
  return launch_fft_c2r_rows(g->fft, b.Yn, out, addsrc, rowstats, BC * g->nlat, g->mmax, act, s);
}

// channel MLP of the block (layers.py:145-178) on x1 (B, C, P) with norm1/FiLM
// already folded into (W1f, b1f):  out = W2·GELU(W1f·x1 + b1f) + b2 (+ resid).
// GELU(erf) in fc1's epilogue on 128x64 tiles, bias + outer skip in fc2's
// (measured cheapest split: DESIGN.md §8).
int run_mlp(const msfno_block_desc* d, const float* W1f, const float* b1f, const float* x1,
            float* h, float* out, const float* resid, int B, int64_t P, const DenseWs& dw,
            hipStream_t s, const unsigned short* x1p) {
  const int64_t C = d->C, Hd = d->mlp_hidden;
  // x6 engine: h travels as bf16x3 planes [B][3][Hd][ldh] (fc1 splits it once in its
  // epilogue, fc2 stages it without conversion)
  const bool planes = mlp_h_planes(dw.fc1 != nullptr && dw.fc2 != nullptr);
  const int64_t ldh = planes ? round_up(P, 8) : P;
  unsigned short* hx = planes ? reinterpret_cast<unsigned short*>(h) : nullptr;
  prof(ST_FC1, s);
  GemmEpi e1;
  e1.bias = b1f;
  e1.sBias = Hd;
  e1.act = 1;
  if (planes) { e1.c_planes = hx; e1.c_plane_stride = Hd * ldh; }
  if (planes && x1p) {
    // x1 arrives as planes from the inverse FFT: LDS-DMA GEMM (per-field folded W1)
    e1.b_planes = x1p;
    e1.b_plane_stride = C * P;
    MSFNO_TRY(gemm_x6p(W1f, h, (int)Hd, (int)P, (int)C, (int)C, (int)P, (int)ldh, Hd * C,
                       3 * C * P, 3 * Hd * ldh, B, e1, dw.fc1, dw.fc1_b, s));
  } else
  MSFNO_TRY(gemm_dense(TILE_128x256, W1f, x1, h, (int)Hd, (int)P, (int)C, (int)C,
                       (int)P, (int)ldh, Hd * C, C * P, (planes ? 3 : 1) * Hd * ldh, B, e1,
                       dw.fc1, dw.fc1_b, s));
  prof(ST_FC2, s);
  GemmEpi e2;
  e2.bias = d->fc2_b;
  if (resid) { e2.addend = resid; e2.sD = C * P; e2.ldd = (int)P; }
  if (planes) {
    e2.b_planes = hx;
    e2.b_plane_stride = Hd * ldh;
    return gemm_x6p(d->fc2_w, out, (int)C, (int)P, (int)Hd, (int)Hd, (int)ldh, (int)P, 0,
                    3 * Hd * ldh, C * P, B, e2, dw.fc2, dw.fc2_b, s);
  }
  return gemm_dense(TILE_256x128, d->fc2_w, h, out, (int)C, (int)P, (int)Hd, (int)Hd,
                    (int)ldh, (int)P, 0, (planes ? 3 : 1) * Hd * ldh, C * P, B, e2, dw.fc2,
                    dw.fc2_b, s);
}

// ---------------------------------------------------------------------------
// the inner skip: engine dispatch, fork / join, fork point (block_forward_impl and
// msfno_band_block_stage; DESIGN.md §5 has the table)
// ---------------------------------------------------------------------------

// the inner-skip GEMM reads fp32 x and splits it in-kernel (gemm_x6), forked before
// the forward FFT; MSFNO_SKIP_PLANES=1: x as bf16x3 planes written by the forward FFT
// (into the x1 plane buffer), the GEMM forked after it.  With the fused MLP the fp32
// form measured 2.8 % faster per block (rfft 0.70 -> 0.51 ms without the 1.6 GB of
// plane stores)
static bool skip_planes_env() {
  static const bool on = sw_is1("MSFNO_SKIP_PLANES");
  return on;
}

// the inner skip on the x3h engine by default (MSFNO_ENGINE=x6 or MSFNO_SKIP_X3H=0 keep x6)
bool skip_x3(const msfno_block_desc* d) {
  static const bool on = sw_is1_or("MSFNO_SKIP_X3H", mlp_fused_h_env());
  return on && gemm_use_x6() && !skip_planes_env() && d->inner_skip == MSFNO_SKIP_LINEAR;
}

static bool skip_planes(const msfno_block_desc* d, const msfno_sht_plan_s* f, const BlockBufs& b) {
  return skip_planes_env() && b.x1p && b.dw.skip && d->inner_skip == MSFNO_SKIP_LINEAR &&
         fft_r2c_planes_supported(f->fft, f->mmax);
}

// x3h (b.xs: its per-channel scales come from the norm0 statistics): forked after them.  The
// skip slows whatever it overlaps by about its own length: forked after the forward
// Legendre instead (overlapping only the MFMA-bound spectral layers) measured equal
// (160.8 / 159.9 vs 160.7 / 159.9 fields/s, round 5).  The linear filter forks it after
// the per-mode contraction, so its 2.1 GB do not share HBM with the 34 GB weight stream:
// 94.0 / 94.2 vs 92.2 / 92.3 fields/s (profiles/r05_b).
// x6 planes: the forward FFT also writes x as bf16x3 planes into the x1 plane buffer (dead
// until the inverse FFT, which runs after the skip GEMM); the GEMM is forked after the FFT
// and stages B by LDS-DMA (gemm_x6p) instead of splitting fp32 x in-kernel.  A separate
// skip input is not what the FFT reads: fp32, forked first.
// Otherwise (x6 or fp32 engine on fp32 x: depends only on the input) forked first.
SkipFork skip_fork_point(const msfno_block_desc* d, const msfno_sht_plan_s* f, const BlockBufs& b,
                         bool separate_input) {
  if (d->inner_skip != MSFNO_SKIP_LINEAR) return SKIP_NONE;
  if (b.xs) return d->filter_type == MSFNO_FILTER_NONLINEAR ? SKIP_AFTER_NORM0 : SKIP_BEFORE_INV;
  return skip_planes(d, f, b) && !separate_input ? SKIP_AFTER_FFT : SKIP_FIRST;
}

// the skip GEMM on stream ss: x3h on the scales b.xs (skip_h at C = 256, else gemm_x3), x6
// on the x planes the forward FFT wrote (gemm_x6p), else gemm_dense on fp32 sx
static int skip_gemm(const InnerSkip& k, hipStream_t ss) {
  const msfno_block_desc* d = k.d;
  const BlockBufs& b = *k.b;
  const int64_t C = d->C, P = k.P;
  const int B = k.B;
  prof(ST_SKIP, ss);
  GemmEpi e;
  e.bias = d->skip_b;
  if (k.own_scales) MSFNO_TRY(launch_chan_pow2_scale(k.sx, (int64_t)B * C, P, b.xs, ss));
  if (b.xs && C == 256 && skip_h_env()) {
    MSFNO_TRY(launch_skip_h(d->skip_w, b.xs, k.sx, k.x1, d->skip_b, B, P, b.dw.skip, b.dw.skip_b,
                            ss, k.quarter_cu));
  } else if (b.xs) {
    MSFNO_TRY(gemm_x3(d->skip_w, (int)C, b.xs, k.sx, k.x1, (int)C, (int)P, (int)C, (int)P, (int)P,
                      C * P, C * P, B, e, b.dw.skip, b.dw.skip_b, ss));
  } else if (k.at == SKIP_AFTER_FFT) {
    e.b_planes = b.x1p;
    e.b_plane_stride = C * P;
    MSFNO_TRY(gemm_x6p(d->skip_w, k.x1, (int)C, (int)P, (int)C, (int)C, (int)P, (int)P, 0,
                       3 * C * P, C * P, B, e, b.dw.skip, b.dw.skip_b, ss));
  } else {
    // sx: global_conv's skip input is the residual, not the filter input x
    MSFNO_TRY(gemm_dense(TILE_128x256, d->skip_w, k.sx, k.x1, (int)C, (int)P, (int)C, (int)C,
                         (int)P, (int)P, 0, C * P, C * P, B, e, b.dw.skip, b.dw.skip_b, ss));
  }
  return MSFNO_OK;
}

int skip_fork(const InnerSkip& k, hipStream_t s) {
  hipStream_t ss = s;
  if (k.side) {  // fork
    MSFNO_CHECK_HIP(hipEventRecord(k.side->fork, s));
    MSFNO_CHECK_HIP(hipStreamWaitEvent(k.side->side, k.side->fork, 0));
    ss = k.side->side;
  }
  MSFNO_TRY(skip_gemm(k, ss));
  if (k.side) {
    prof(ST_END, ss);
    MSFNO_CHECK_HIP(hipEventRecord(k.join, ss));
  }
  return MSFNO_OK;
}

// x1 (the MLP input) written by the inverse FFT as bf16x3 planes: x6 engine, an
// MLP, and an LDS-DMA inverse FFT whose rows tile the plane rows (P % 8 == 0);
// MSFNO_X1_PLANES=0 keeps fp32 x1 for A/B
bool x1_planes(const msfno_block_desc* d, const msfno_sht_plan_s* g) {
  static const bool on = sw_on("MSFNO_X1_PLANES");
  return on && d->has_mlp && mlp_h_planes(true) && !mlp_fused(d, (int64_t)g->nlat * g->nlon) &&
         ((int64_t)g->nlat * g->nlon) % 8 == 0 && fft_c2r_planes_supported(g->fft, g->mmax);
}

bool mlp_fused(const msfno_block_desc* d, int64_t P) {
  return d->has_mlp && gemm_use_x6() && d->fc1_b != nullptr && P % 4 == 0 && P >= 4 &&
         mlp_fused_supported((int)d->C, (int)d->mlp_hidden);
}

bool x1p_buffer(const msfno_block_desc* d, const msfno_sht_plan_s* g) {
  return x1_planes(d, g) ||
         (skip_planes_env() && mlp_fused(d, (int64_t)g->nlat * g->nlon) &&
          d->inner_skip == MSFNO_SKIP_LINEAR && mlp_h_planes(true));
}

int run_block_mlp(const msfno_block_desc* d, const float* x1, const unsigned short* x1p,
                  const float* sc1, const float* sh1, const float* ab1, float* W1f, float* b1f, float* h,
                  unsigned short* mfimg, float* out, const float* resid, int B, int64_t P,
                  const DenseWs& dw, hipStream_t s) {
  MSFNO_REQUIRE(d->fc1_w && d->fc2_w, MSFNO_EINVAL, "missing MLP weights");
  if (mfimg) {
    prof(ST_MLP_FUSED, s);
    if (!(wcache_ready(d) && mfimg == wcache_mfimg(d)))
      MSFNO_TRY(launch_mlp_fused_images(d->fc1_w, d->fc1_b, d->fc2_w, mfimg, s));
    return launch_mlp_fused(x1, sc1, sh1, ab1, resid, out, mfimg, d->fc1_b, d->fc2_b, B, P, s);
  }
  const int64_t C = d->C, Hd = d->mlp_hidden;
  MSFNO_TRY(launch_fold_affine(d->fc1_w, d->fc1_b, sc1, sh1, W1f, b1f, B, (int)Hd, (int)C, s));
  return run_mlp(d, W1f, b1f, x1, h, out, resid, B, P, dw, s, x1p);
}

// MLP hidden activation in the bf16x3 plane format (x6 engine; MSFNO_H_PLANES=0
// keeps it fp32 for A/B)
bool mlp_h_planes(bool have_ws) {
  static const bool on = gemm_use_x6() && sw_on("MSFNO_H_PLANES");
  return on && have_ws;
}

// floats to reserve for the MLP hidden activation h (B, Hd, P) in either format
int64_t mlp_h_floats(int B, int64_t Hd, int64_t P) {
  if (!mlp_h_planes(true)) return (int64_t)B * Hd * P;
  return cdiv((int64_t)B * 3 * Hd * round_up(P, 8) * 2, 4);
}
}  // namespace msfno

using namespace msfno;

extern "C" {

size_t msfno_block_wcache_size(const msfno_block_desc* d) {
  if (!d) return 0;
  msfno_block_desc t = *d;
  t.wcache = nullptr;
  return wcache_layout(&t, nullptr);
}

size_t msfno_block_workspace_size(const msfno_block_desc* d, msfno_sht_plan_t f,
                                  msfno_sht_plan_t g, int B) {
  if (!d || !f || !g) return 0;
  Carve cv;
  BlockBufs b;
  carve_block(cv, b, d, f, g, B, true);
  return cv.off;
}

int msfno_filter_forward(const msfno_block_desc* d, msfno_sht_plan_t f, msfno_sht_plan_t g,
                         const float* x, float* y, int B, void* ws, size_t ws_bytes,
                         void* stream) {
  MSFNO_TRY(check_pair(d, f, g));
  MSFNO_REQUIRE(ws_bytes >= msfno_block_workspace_size(d, f, g, B), MSFNO_EWORKSPACE,
                "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carve cv;
  cv.base = (char*)ws;
  BlockBufs b;
  // (sized as the whole block, with its norm and MLP buffers; carved without them: the
  // filter's buffers are a prefix of that layout)
  carve_block(cv, b, d, f, g, B, false);
  MSFNO_TRY(run_spectral(d, f, g, b, x, B, false, s));
  MSFNO_TRY(run_inverse_fft(g, b, B, d->C, y, nullptr, nullptr, 0, s));
  prof(ST_END, s);
  return MSFNO_OK;
}

}  // extern "C"

// x1_ext / aff_out (both or neither; blocks without MLP and outer skip): the block stops
// before its output affine, leaving x1 in x1_ext and the per-(b,c) norm1 (+ FiLM) affine
// in aff_out = [scale (B*C)][shift (B*C)] for the consumer to apply (the decoder MLP)
// skip_x (or null = x): the inner skip's input (global_conv's `residual`); norm_only: stop
// after norm1 (no FiLM, MLP or outer skip: FourierNeuralOperatorBlock_Filmed.global_conv)
static int block_forward_impl(const msfno_block_desc* d, msfno_sht_plan_t f, msfno_sht_plan_t g,
                              const float* x, const float* gamma, const float* beta,
                              float film_scale, float* out, float* x1_ext, float* aff_out, int B,
                              void* ws, size_t ws_bytes, void* stream,
                              const float* skip_x = nullptr, bool norm_only = false) {
  MSFNO_TRY(check_pair(d, f, g));
  MSFNO_REQUIRE(ws_bytes >= msfno_block_workspace_size(d, f, g, B), MSFNO_EWORKSPACE,
                "workspace too small");
  MSFNO_REQUIRE((gamma == nullptr) == (beta == nullptr), MSFNO_EINVAL,
                "gamma and beta must both be given or both be NULL");
  MSFNO_REQUIRE(d->outer_skip != MSFNO_SKIP_LINEAR, MSFNO_EUNSUPPORTED,
                "outer_skip='linear' is not supported by the fused block");
  const bool resample = (f->nlat != g->nlat) || (f->nlon != g->nlon);
  MSFNO_REQUIRE(!resample || (d->inner_skip == MSFNO_SKIP_NONE && d->outer_skip == MSFNO_SKIP_NONE),
                MSFNO_EINVAL, "skips require equal input and output grids");
  hipStream_t s = (hipStream_t)stream;
  Carve cv;
  cv.base = (char*)ws;
  BlockBufs b;
  carve_block(cv, b, d, f, g, B, true);
  const int64_t C = d->C, BC = (int64_t)B * C;
  const int64_t P = (int64_t)g->nlat * g->nlon;
  const int act = d->filter_type == MSFNO_FILTER_LINEAR ? 1 : 0;  // GELU after skip (linear only)

  // ---- inner skip 1x1 conv (depends only on x): x1 = Ws·x + bs, on the side stream ----
  // run_spectral forks it at skip.at (skip_fork_point)
  float* x1 = x1_ext ? x1_ext : b.x1;
  const float* sx = skip_x ? skip_x : x;
  std::shared_ptr<SideCtx> side;
  InnerSkip skip{d, &b, sx, x1, B, P, skip_fork_point(d, f, b, sx != x)};
  if (skip.at != SKIP_NONE) {
    MSFNO_REQUIRE(d->skip_w, MSFNO_EINVAL, "missing inner_skip weight");
    MSFNO_TRY(side_ctx(&side, s));
    skip.side = side.get();
    skip.join = side ? side->join : nullptr;
    // a separate skip input has no norm0 statistics: its x3h B-row scales from its max
    // (the block only: the band's skip input is always the filter's)
    skip.own_scales = b.xs && sx != x;
    // the quarter-CU side grid only where the skip is forked at the block start and
    // overlaps the whole SHT + spectral chain (non-linear filter); the other filters fork
    // it after the contraction (SKIP_BEFORE_INV), where it is on the critical path (1.80 vs
    // 0.79 ms, linear 85.9 vs 97.5 fields/s, profiles/r06_j)
    skip.quarter_cu = side && d->filter_type == MSFNO_FILTER_NONLINEAR;
  }
  MSFNO_TRY(run_spectral(d, f, g, b, x, B, true, s, &skip));
  if (side) MSFNO_CHECK_HIP(hipStreamWaitEvent(s, side->join, 0));  // join
  // ---- filter output + skip (+ GELU for the linear filter) -> x1, norm1 partials ---
  const float* skip_src = d->inner_skip == MSFNO_SKIP_LINEAR ? x1
                          : (d->inner_skip == MSFNO_SKIP_IDENTITY ? sx : nullptr);
  // irfft writes x1 as planes (the unfused MLP's fc1 operand; global_conv reads fp32 x1)
  unsigned short* x1p = !norm_only && x1_planes(d, g) ? b.x1p : nullptr;
  MSFNO_TRY(run_inverse_fft(g, b, B, (int)C, x1, skip_src, b.st1, act, s, x1p));
  const int64_t np = g->nlat, cnt = g->nlon, cnt_last = g->nlon;
  // ---- norm1 (+ FiLM) as a per-(b,c) affine --------------------------------------
  prof(ST_NORM1, s);
  MSFNO_TRY(launch_chan_affine(b.st1, np, cnt, cnt_last, B, (int)C, d->norm1_w, d->norm1_b,
                               d->norm_eps, gamma, beta, film_scale, b.sc1, b.sh1, s, nullptr,
                               nullptr, b.ab1));
  const float* resid = d->outer_skip == MSFNO_SKIP_IDENTITY ? x : nullptr;
  if (norm_only) {
    prof(ST_OUT_AFFINE, s);
    MSFNO_TRY(launch_affine_rows(x1, b.sc1, b.sh1, nullptr, out, BC, P, 0, nullptr, 0, s));
  } else if (aff_out) {
    MSFNO_CHECK_HIP(hipMemcpyAsync(aff_out, b.sc1, BC * sizeof(float), hipMemcpyDeviceToDevice, s));
    MSFNO_CHECK_HIP(
        hipMemcpyAsync(aff_out + BC, b.sh1, BC * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else if (d->has_mlp) {
    MSFNO_TRY(run_block_mlp(d, x1, x1p, b.sc1, b.sh1, b.ab1, b.W1f, b.b1f, b.h, b.mfimg, out, resid, B,
                            P, b.dw, s));
  } else {
    prof(ST_OUT_AFFINE, s);
    MSFNO_TRY(launch_affine_rows(x1, b.sc1, b.sh1, resid, out, BC, P, 0, nullptr, 0, s));
  }
  prof(ST_END, s);
  return MSFNO_OK;
}

extern "C" {

int msfno_block_forward(const msfno_block_desc* d, msfno_sht_plan_t f, msfno_sht_plan_t g,
                        const float* x, const float* gamma, const float* beta, float film_scale,
                        float* out, int B, void* ws, size_t ws_bytes, void* stream) {
  return block_forward_impl(d, f, g, x, gamma, beta, film_scale, out, nullptr, nullptr, B, ws,
                            ws_bytes, stream);
}

int msfno_block_global_conv(const msfno_block_desc* d, msfno_sht_plan_t f, msfno_sht_plan_t g,
                            const float* x, const float* residual, float* out, int B, void* ws,
                            size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(x && out, MSFNO_EINVAL, "global_conv: missing tensors");
  return block_forward_impl(d, f, g, x, nullptr, nullptr, 0.f, out, nullptr, nullptr, B, ws,
                            ws_bytes, stream, residual, true);
}

int msfno_block_forward_deferred(const msfno_block_desc* d, msfno_sht_plan_t f,
                                 msfno_sht_plan_t g, const float* x, const float* gamma,
                                 const float* beta, float film_scale, float* x1_out,
                                 float* affine_out, int B, void* ws, size_t ws_bytes,
                                 void* stream) {
  MSFNO_REQUIRE(d && x1_out && affine_out, MSFNO_EINVAL, "block_forward_deferred: null output");
  MSFNO_REQUIRE(!d->has_mlp && d->outer_skip == MSFNO_SKIP_NONE, MSFNO_EUNSUPPORTED,
                "block_forward_deferred: blocks without MLP and outer skip only");
  return block_forward_impl(d, f, g, x, gamma, beta, film_scale, nullptr, x1_out, affine_out, B,
                            ws, ws_bytes, stream);
}

}  // extern "C"
