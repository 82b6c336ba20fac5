// libmsfno C-ABI: version, last error, and the thin validate-and-launch wrappers
// (contractions, conv1x1, losses, verification, ensemble, export, regridding, statistics over
// time, spectrum).
#include <cmath>

#include "block.h"

namespace msfno {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

struct Conv1x1Bufs {
  float* xs;  // per-(b, channel) power-of-two scale of x
  void* eng;  // the engine's workspace: launch_skip_h (256 -> 256) or gemm_x3
};

static void carve_conv1x1(Carve& cv, Conv1x1Bufs& b, int B, int Cin, int Cout) {
  b.xs = cv.take<float>((int64_t)B * Cin);
  b.eng = cv.take<char>(Cin == 256 && Cout == 256 ? skip_h_workspace(B)
                                                  : gemm_x3_workspace(Cout, Cin, B));
}

}  // namespace msfno

using namespace msfno;

extern "C" {

const char* msfno_last_error(void) { return g_last_error.c_str(); }
int msfno_abi_version(void) { return 6; }

int msfno_compl_contract_fwd_c(const float* a, const float* w, float* y, int B, int Ci, int Co,
                               int T, void* stream) {
  MSFNO_REQUIRE(a && w && y && B > 0 && Ci > 0 && Co > 0 && T > 0, MSFNO_EINVAL,
                "bad compl_contract_fwd_c arguments");
  return launch_compl_contract(a, w, y, B, Ci, Co, T, (hipStream_t)stream);
}

int msfno_compl_mul2d_fwd_c(const float* a, const float* w, float* y, int B, int Ci, int Co,
                            long long XY, int relu_real, void* stream) {
  MSFNO_REQUIRE(a && w && y && B > 0 && Ci > 0 && Co > 0 && XY > 0, MSFNO_EINVAL,
                "bad compl_mul2d_fwd_c arguments");
  return launch_compl_mul2d(a, w, y, B, Ci, Co, XY, relu_real, (hipStream_t)stream);
}

// 1x1 convolution (the block's inner skip as a standalone op): x3h engine, B rows scaled
// per (b, channel) by the power of two below its max |x| (no norm statistics here)
size_t msfno_conv1x1_workspace_size(int B, int Cin, int Cout) {
  if (B <= 0 || Cin <= 0 || Cout <= 0) return 0;
  Carve cv;
  Conv1x1Bufs b;
  carve_conv1x1(cv, b, B, Cin, Cout);
  return cv.off;
}

int msfno_conv1x1(const float* w, const float* bias, const float* x, float* out, int B, int Cin,
                  int Cout, long long P, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(w && x && out && ws && B > 0 && Cin > 0 && Cout > 0 && P > 0 && P < (1LL << 31),
                MSFNO_EINVAL, "bad conv1x1 arguments");
  Carve cv;
  cv.base = (char*)ws;
  Conv1x1Bufs b;
  carve_conv1x1(cv, b, B, Cin, Cout);
  MSFNO_REQUIRE(ws_bytes >= cv.off, MSFNO_EWORKSPACE, "conv1x1: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  // the engine may use all the caller gave behind xs (each engine checks its own need)
  const size_t eng_b = ws_bytes - (size_t)(static_cast<char*>(b.eng) - cv.base);
  MSFNO_TRY(launch_chan_pow2_scale(x, (int64_t)B * Cin, P, b.xs, s));
  if (Cin == 256 && Cout == 256 && skip_h_env())
    return launch_skip_h(w, b.xs, x, out, bias, B, P, b.eng, eng_b, s);
  GemmEpi e;
  e.bias = bias;
  return gemm_x3(w, Cin, b.xs, x, out, Cout, (int)P, Cin, (int)P, (int)P, (int64_t)Cin * P,
                 (int64_t)Cout * P, B, e, b.eng, eng_b, s);
}

size_t msfno_loss_workspace_size(int BC, int nlat, int nlon) {
  if (BC <= 0 || nlat <= 0 || nlon <= 0) return 0;
  return loss_workspace_bytes(BC, nlat, nlon);
}

int msfno_loss_sums(const float* prd, const float* tar, const float* w_lat, float* sums, int BC,
                    int nlat, int nlon, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(prd && tar && w_lat && sums && ws && BC > 0 && nlat > 0 && nlon > 0,
                MSFNO_EINVAL, "bad loss_sums arguments");
  MSFNO_REQUIRE(ws_bytes >= msfno_loss_workspace_size(BC, nlat, nlon), MSFNO_EWORKSPACE,
                "loss_sums: workspace too small");
  return launch_loss_sums(prd, tar, w_lat, sums, BC, nlat, nlon, ws, (hipStream_t)stream);
}

int msfno_loss_backward(const float* prd, const float* tar, const float* w_lat,
                        const float* gnum, float* dprd, int BC, int nlat, int nlon,
                        void* stream) {
  MSFNO_REQUIRE(prd && tar && w_lat && gnum && dprd && BC > 0 && nlat > 0 && nlon > 0,
                MSFNO_EINVAL, "bad loss_backward arguments");
  return launch_loss_backward(prd, tar, w_lat, gnum, dprd, BC, nlat, nlon,
                              (hipStream_t)stream);
}

size_t msfno_verify_workspace_size(int BC, int nlat, int nlon) {
  if (BC <= 0 || nlat <= 0 || nlon <= 0) return 0;
  return verify_workspace_bytes(BC, nlat, nlon);
}

int msfno_verify_sums(const float* prd, const float* tar, const float* w_lat, const float* clim,
                      const int* clim_slab, float* sums, int BC, int nlat, int nlon, void* ws,
                      size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(prd && tar && w_lat && sums && ws && BC > 0 && nlat > 0 && nlon > 0,
                MSFNO_EINVAL, "bad verify_sums arguments");
  MSFNO_REQUIRE((clim == nullptr) == (clim_slab == nullptr), MSFNO_EINVAL,
                "verify_sums: clim and clim_slab must both be set or both be null");
  MSFNO_REQUIRE(ws_bytes >= msfno_verify_workspace_size(BC, nlat, nlon), MSFNO_EWORKSPACE,
                "verify_sums: workspace too small");
  return launch_verify_sums(prd, tar, w_lat, clim, clim_slab, sums, BC, nlat, nlon, ws,
                            (hipStream_t)stream);
}

size_t msfno_verify_regions_workspace_size(int BC, int nlat, int nlon, int nregions) {
  if (BC <= 0 || nlat <= 0 || nlon <= 0 || nregions < 1 || nregions > 32) return 0;
  return verify_regions_workspace_bytes(BC, nlat, nlon, nregions);
}

int msfno_verify_region_sums(const float* prd, const float* tar, const float* w_lat,
                             const float* clim, const int* clim_slab, const uint32_t* row_bits,
                             const uint32_t* col_bits, const uint32_t* pix_bits, int nregions,
                             int skip_nan, float* sums, int BC, int nlat, int nlon, void* ws,
                             size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(prd && tar && w_lat && row_bits && col_bits && sums && ws && BC > 0 &&
                    nlat > 0 && nlon > 0,
                MSFNO_EINVAL, "bad verify_region_sums arguments");
  MSFNO_REQUIRE(nregions >= 1 && nregions <= 32, MSFNO_EINVAL,
                "verify_region_sums: nregions must be in 1..32");
  MSFNO_REQUIRE((clim == nullptr) == (clim_slab == nullptr), MSFNO_EINVAL,
                "verify_region_sums: clim and clim_slab must both be set or both be null");
  MSFNO_REQUIRE(ws_bytes >= msfno_verify_regions_workspace_size(BC, nlat, nlon, nregions),
                MSFNO_EWORKSPACE, "verify_region_sums: workspace too small");
  return launch_verify_region_sums(prd, tar, w_lat, clim, clim_slab, row_bits, col_bits, pix_bits,
                                   nregions, skip_nan, sums, BC, nlat, nlon, ws,
                                   (hipStream_t)stream);
}

size_t msfno_ens_workspace_size(int S, int M, int nlat, int nlon) {
  if (S <= 0 || M < 2 || M > 32 || nlat <= 0 || nlon <= 0) return 0;
  return ens_workspace_bytes(S, M, nlat, nlon);
}

int msfno_ens_sums(const float* ens, long long member_stride, const float* tar,
                   const float* w_lat, float* sums, float* hist, int M, int S, int nlat,
                   int nlon, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(ens && tar && w_lat && sums && ws && S > 0 && nlat > 0 && nlon > 0 && M >= 2,
                MSFNO_EINVAL, "bad ens_sums arguments");
  MSFNO_REQUIRE(member_stride >= (long long)S * nlat * nlon, MSFNO_EINVAL,
                "ens_sums: member_stride is shorter than a member");
  MSFNO_REQUIRE(M <= 32, MSFNO_EUNSUPPORTED, "ens_sums: more than 32 members");
  MSFNO_REQUIRE(ws_bytes >= msfno_ens_workspace_size(S, M, nlat, nlon), MSFNO_EWORKSPACE,
                "ens_sums: workspace too small");
  return launch_ens_sums(ens, member_stride, tar, w_lat, sums, hist, M, S, nlat, nlon, ws,
                         (hipStream_t)stream);
}

int msfno_ens_crps_backward(const float* ens, long long member_stride, const float* tar,
                            const float* w_lat, const float* g, float kappa, float* dens,
                            long long dens_member_stride, int M, int S, int nlat, int nlon,
                            void* stream) {
  MSFNO_REQUIRE(ens && tar && w_lat && g && dens && S > 0 && nlat > 0 && nlon > 0 && M >= 2,
                MSFNO_EINVAL, "bad ens_crps_backward arguments");
  MSFNO_REQUIRE(member_stride >= (long long)S * nlat * nlon &&
                    dens_member_stride >= (long long)S * nlat * nlon,
                MSFNO_EINVAL, "ens_crps_backward: a member stride is shorter than a member");
  MSFNO_REQUIRE(M <= 32, MSFNO_EUNSUPPORTED, "ens_crps_backward: more than 32 members");
  return launch_ens_crps_backward(ens, member_stride, tar, w_lat, g, kappa, dens,
                                  dens_member_stride, M, S, nlat, nlon, (hipStream_t)stream);
}

int msfno_ens_products(const float* ens, long long member_stride, const double* q_levels,
                       int nq, const float* thr, int nt, const msfno_ens_products_out* out,
                       int M, int S, int nlat, int nlon, void* stream) {
  MSFNO_REQUIRE(ens && out && S > 0 && nlat > 0 && nlon > 0 && M >= 2 && nq >= 0 && nt >= 0,
                MSFNO_EINVAL, "bad ens_products arguments");
  MSFNO_REQUIRE(out->mean || out->std || out->min || out->max || out->quant || out->prob,
                MSFNO_EINVAL, "ens_products: no output wanted");
  MSFNO_REQUIRE(member_stride >= (long long)S * nlat * nlon, MSFNO_EINVAL,
                "ens_products: member_stride is shorter than a member");
  MSFNO_REQUIRE(!out->quant || (nq >= 1 && q_levels), MSFNO_EINVAL,
                "ens_products: quant wanted without a level");
  MSFNO_REQUIRE(!out->prob || (nt >= 1 && thr), MSFNO_EINVAL,
                "ens_products: prob wanted without a threshold");
  MSFNO_REQUIRE(M <= 32, MSFNO_EUNSUPPORTED, "ens_products: more than 32 members");
  MSFNO_REQUIRE(nq <= MSFNO_ENS_MAX_LEVELS && nt <= MSFNO_ENS_MAX_LEVELS, MSFNO_EUNSUPPORTED,
                "ens_products: more than 8 levels or thresholds");
  // the position of level q among the sorted members, pos = q (M - 1), in fp64: the kernel
  // never divides.  hi stays below M: the bucket's padding sorts behind the members.
  EnsQuantiles eq = {};
  for (int l = 0; out->quant && l < nq; ++l) {
    const double q = q_levels[l];
    MSFNO_REQUIRE(q >= 0.0 && q <= 1.0, MSFNO_EINVAL,
                  "ens_products: a quantile level outside [0, 1]");
    const double pos = q * (M - 1);
    const int lo = std::min((int)std::floor(pos), M - 1);
    eq.lo[l] = lo;
    eq.hi[l] = std::min(lo + 1, M - 1);
    eq.frac[l] = (float)(pos - lo);
  }
  const EnsProductsOut o = {out->mean, out->std, out->min, out->max, out->quant, out->prob};
  return launch_ens_products(ens, member_stride, eq, nq, thr, nt, o, M, S, nlat, nlon,
                             (hipStream_t)stream);
}

size_t msfno_ens_threshold_workspace_size(int S, int M, int nt, int nlat, int nlon) {
  if (S <= 0 || M < 2 || M > 32 || nt < 1 || nt > MSFNO_ENS_MAX_LEVELS || nlat <= 0 || nlon <= 0)
    return 0;
  return ens_threshold_workspace_bytes(S, M, nt, nlat);
}

int msfno_ens_threshold_sums(const float* ens, long long member_stride, const float* tar,
                             const float* w_lat, const float* thr, int nt, float* counts,
                             int M, int S, int nlat, int nlon, void* ws, size_t ws_bytes,
                             void* stream) {
  MSFNO_REQUIRE(ens && tar && w_lat && thr && counts && ws && S > 0 && nlat > 0 && nlon > 0 &&
                    M >= 2 && nt >= 1,
                MSFNO_EINVAL, "bad ens_threshold_sums arguments");
  MSFNO_REQUIRE(member_stride >= (long long)S * nlat * nlon, MSFNO_EINVAL,
                "ens_threshold_sums: member_stride is shorter than a member");
  MSFNO_REQUIRE(M <= 32, MSFNO_EUNSUPPORTED, "ens_threshold_sums: more than 32 members");
  MSFNO_REQUIRE(nt <= MSFNO_ENS_MAX_LEVELS, MSFNO_EUNSUPPORTED,
                "ens_threshold_sums: more than 8 thresholds");
  MSFNO_REQUIRE(ws_bytes >= msfno_ens_threshold_workspace_size(S, M, nt, nlat, nlon),
                MSFNO_EWORKSPACE, "ens_threshold_sums: workspace too small");
  return launch_ens_threshold_sums(ens, member_stride, tar, w_lat, thr, nt, counts, M, S, nlat,
                                   nlon, ws, (hipStream_t)stream);
}

size_t msfno_pack16_workspace_size(int S_out, int nlat_out, int nlon_out) {
  if (S_out <= 0 || nlat_out <= 0 || nlon_out <= 0) return 0;
  return pack16_workspace_bytes(S_out, nlat_out);
}

int msfno_pack16(const float* x, int S_in, int nlat, int nlon, const int* slab, int S_out,
                 const msfno_window* win, float* ref, int* exp2, unsigned short* q, void* ws,
                 size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(x && ref && exp2 && q && ws && S_in > 0 && nlat > 0 && nlon > 0 && S_out > 0,
                MSFNO_EINVAL, "bad pack16 arguments");
  MSFNO_REQUIRE(slab || S_out <= S_in, MSFNO_EINVAL,
                "pack16: more output slabs than slabs without a slab list");
  const msfno_window whole = {0, 1, nlat, 0, 1, nlon};
  const msfno_window& v = win ? *win : whole;
  MSFNO_REQUIRE(v.lat_step >= 1 && v.lon_step >= 1 && v.nlat_out >= 1 && v.nlon_out >= 1,
                MSFNO_EINVAL, "pack16: a window extent or step below 1");
  MSFNO_REQUIRE(v.lat0 >= 0 && v.lon0 >= 0 &&
                    v.lat0 + (long long)(v.nlat_out - 1) * v.lat_step < nlat &&
                    v.lon0 + (long long)(v.nlon_out - 1) * v.lon_step < nlon,
                MSFNO_EINVAL, "pack16: the window leaves the slab");
  MSFNO_REQUIRE(ws_bytes >= msfno_pack16_workspace_size(S_out, v.nlat_out, v.nlon_out),
                MSFNO_EWORKSPACE, "pack16: workspace too small");
  const PackWin w = {nlat, nlon, v.lat0, v.lat_step, v.lon0, v.lon_step};
  return launch_pack16(x, slab, w, S_out, v.nlat_out, v.nlon_out, ref, exp2, q, ws,
                       (hipStream_t)stream);
}

int msfno_unpack16(const unsigned short* q, const float* ref, const int* exp2, float* y,
                   long long n_per_slab, int S, void* stream) {
  MSFNO_REQUIRE(q && ref && exp2 && y && n_per_slab > 0 && S > 0, MSFNO_EINVAL,
                "bad unpack16 arguments");
  return launch_unpack16(q, ref, exp2, y, n_per_slab, S, (hipStream_t)stream);
}

static bool regrid_axis_ok(const msfno_regrid_axis* a) {
  return a && a->start && a->count && a->w && a->n_in >= 1 && a->n_out >= 1;
}

int msfno_regrid(const float* x, int S_in, const int* slab, int S_out,
                 const msfno_regrid_axis* lat, const msfno_regrid_axis* lon, const float* mask,
                 int skip_nan, float min_valid, float fill, float* y, void* stream) {
  MSFNO_REQUIRE(x && y && S_in > 0 && S_out > 0 && regrid_axis_ok(lat) && regrid_axis_ok(lon),
                MSFNO_EINVAL, "bad regrid arguments");
  MSFNO_REQUIRE(lat->taps >= 1 && lat->taps <= MSFNO_REGRID_MAX_TAPS && lon->taps >= 1 &&
                    lon->taps <= MSFNO_REGRID_MAX_TAPS,
                MSFNO_EINVAL, "regrid: taps outside 1..32");
  MSFNO_REQUIRE(slab || S_out <= S_in, MSFNO_EINVAL,
                "regrid: more output slabs than slabs without a slab list");
  MSFNO_REQUIRE(std::isfinite(min_valid) && min_valid >= 0.f, MSFNO_EINVAL,
                "regrid: min_valid is negative or not finite");
  MSFNO_REQUIRE(lon->n_in <= kRegridMaxLon, MSFNO_EUNSUPPORTED,
                "regrid: source rows longer than 8188 do not fit the LDS rows");
  const RegridAxis la = {lat->n_in, lat->n_out, lat->taps, lat->start, lat->count, lat->w};
  const RegridAxis lo = {lon->n_in, lon->n_out, lon->taps, lon->start, lon->count, lon->w};
  return launch_regrid(x, slab, S_out, la, lo, mask, skip_nan != 0, min_valid, fill, y,
                       (hipStream_t)stream);
}

int msfno_tstats_planes(int kind, int flags) {
  const int K = tstats_planes(kind, flags);
  MSFNO_REQUIRE(K > 0, MSFNO_EINVAL,
                "tstats_planes: unknown kind, or a flag that the kind does not take");
  return K;
}

int msfno_tstats_update(int kind, int flags, const float* in0, const float* in1,
                        long long batch_stride0, long long batch_stride1, const float* clim,
                        const int* clim_slab, int B, int S, long long P, int skip_nan,
                        uint32_t* count, float* state, long long plane_stride, void* stream) {
  MSFNO_REQUIRE(tstats_planes(kind, flags) > 0, MSFNO_EINVAL,
                "tstats_update: unknown kind, or a flag that the kind does not take");
  MSFNO_REQUIRE(in0, MSFNO_EINVAL, "tstats_update: in0 is null");
  MSFNO_REQUIRE(count, MSFNO_EINVAL, "tstats_update: count is null");
  MSFNO_REQUIRE(state, MSFNO_EINVAL, "tstats_update: state is null");
  MSFNO_REQUIRE(B >= 1 && S >= 1 && P >= 1, MSFNO_EINVAL,
                "tstats_update: B, S or P below 1");
  MSFNO_REQUIRE((kind == MSFNO_TSTATS_ERROR) == (in1 != nullptr), MSFNO_EINVAL,
                "tstats_update: in1 is required for ERROR and must be null for FIELD");
  MSFNO_REQUIRE((clim == nullptr) == (clim_slab == nullptr), MSFNO_EINVAL,
                "tstats_update: clim and clim_slab must both be set or both be null");
  MSFNO_REQUIRE(kind != MSFNO_TSTATS_ERROR || ((flags & MSFNO_TSTATS_ANOM) != 0) == (clim != nullptr),
                MSFNO_EINVAL,
                "tstats_update: ERROR has the anomaly planes (flags) iff clim is given");
  MSFNO_REQUIRE(plane_stride >= (long long)S * P, MSFNO_EINVAL,
                "tstats_update: plane_stride is shorter than a plane");
  return launch_tstats_update(kind, flags, in0, in1, batch_stride0, batch_stride1, clim,
                              clim_slab, B, S, P, skip_nan, count, state, plane_stride,
                              (hipStream_t)stream);
}

int msfno_tstats_merge(int kind, int flags, uint32_t* dst_count, float* dst_state,
                       long long dst_plane_stride, const uint32_t* src_count,
                       const float* src_state, long long src_plane_stride, long long N,
                       void* stream) {
  MSFNO_REQUIRE(tstats_planes(kind, flags) > 0, MSFNO_EINVAL,
                "tstats_merge: unknown kind, or a flag that the kind does not take");
  MSFNO_REQUIRE(dst_count && dst_state, MSFNO_EINVAL,
                "tstats_merge: dst_count or dst_state is null");
  MSFNO_REQUIRE(src_count && src_state, MSFNO_EINVAL,
                "tstats_merge: src_count or src_state is null");
  MSFNO_REQUIRE(N >= 1, MSFNO_EINVAL, "tstats_merge: N below 1");
  MSFNO_REQUIRE(dst_plane_stride >= N, MSFNO_EINVAL,
                "tstats_merge: dst_plane_stride is shorter than a plane");
  MSFNO_REQUIRE(src_plane_stride >= N, MSFNO_EINVAL,
                "tstats_merge: src_plane_stride is shorter than a plane");
  return launch_tstats_merge(kind, flags, dst_count, dst_state, dst_plane_stride, src_count,
                             src_state, src_plane_stride, N, (hipStream_t)stream);
}

// N * lmax rows of mmax complex numbers; the interleaved floats of a complex tensor sit on
// the 8-byte grid
static bool spectrum_args_ok(const void* a, const void* b, long long N, int lmax, int mmax) {
  return a && b && N >= 1 && lmax >= 1 && mmax >= 1 &&
         ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0 &&
         N <= INT64_MAX / ((int64_t)lmax * mmax * 2);
}

int msfno_spectrum_power(const float* coeffs, float* power, long long N, int lmax, int mmax,
                         void* stream) {
  MSFNO_REQUIRE(power && spectrum_args_ok(coeffs, coeffs, N, lmax, mmax), MSFNO_EINVAL,
                "bad spectrum_power arguments");
  return launch_spectrum_power(coeffs, power, (int64_t)N * lmax, mmax, (hipStream_t)stream);
}

int msfno_spectrum_power_backward(const float* coeffs, const float* gpower, float* dcoeffs,
                                  long long N, int lmax, int mmax, void* stream) {
  MSFNO_REQUIRE(gpower && spectrum_args_ok(coeffs, dcoeffs, N, lmax, mmax), MSFNO_EINVAL,
                "bad spectrum_power_backward arguments");
  return launch_spectrum_power_backward(coeffs, gpower, dcoeffs, (int64_t)N * lmax, mmax,
                                        (hipStream_t)stream);
}

int msfno_noise_spectral(float* coeffs, const float* prev, const float* sqrt_eig, int K,
                         long long n, long long field0, int lmax, int mmax, float a, float b,
                         unsigned long long seed, unsigned long long draw,
                         const unsigned long long* draw_dev, void* stream) {
  MSFNO_REQUIRE(sqrt_eig && K >= 1 && field0 >= 0 &&
                    spectrum_args_ok(coeffs, prev ? (const void*)prev : (const void*)coeffs, n,
                                     lmax, mmax),
                MSFNO_EINVAL, "bad noise_spectral arguments");
  // the Philox counter holds l * ceil(mmax / 2) + m / 2 and the field index in 32 bits each
  MSFNO_REQUIRE((int64_t)lmax * (((int64_t)mmax + 1) / 2) < (1LL << 32), MSFNO_EINVAL,
                "noise_spectral: lmax * ceil(mmax / 2) must be below 2^32");
  MSFNO_REQUIRE(field0 <= (1LL << 32) && n <= (1LL << 32) - field0, MSFNO_EINVAL,
                "noise_spectral: field0 + n must not exceed 2^32");
  return launch_noise_spectral(coeffs, prev, sqrt_eig, K, (int64_t)n, (int64_t)field0, lmax,
                               mmax, a, b, (uint64_t)seed, (uint64_t)draw,
                               reinterpret_cast<const uint64_t*>(draw_dev),
                               (hipStream_t)stream);
}

int msfno_noise_advance(unsigned long long* draw_dev, unsigned long long by, void* stream) {
  MSFNO_REQUIRE(draw_dev && (reinterpret_cast<uintptr_t>(draw_dev) & 7) == 0, MSFNO_EINVAL,
                "bad noise_advance arguments");
  return launch_noise_advance(reinterpret_cast<uint64_t*>(draw_dev), (uint64_t)by,
                              (hipStream_t)stream);
}

}  // extern "C"
