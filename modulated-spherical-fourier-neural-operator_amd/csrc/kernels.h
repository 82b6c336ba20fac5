// Internal launcher declarations (host-callable, stream-ordered).
#pragma once
#include "common.h"

namespace msfno {

// ---- fft.hip ----------------------------------------------------------------
// x (rows, N) fp32 -> out (rows, mmax) complex, scaled by `scale`; optional
// per-row (mean, M2) over the N inputs.
// planes (optional, LDS-DMA path only): the input rows are also written as bf16x3
// planes in the C2RPlanes layout below (the inner-skip GEMM's B operand)
int launch_fft_r2c_rows(const FFTPlan& f, const float* x, float2* out, float2* rowstats,
                        int64_t rows, int mmax, float scale, hipStream_t s,
                        const struct C2RPlanes* planes = nullptr);
// in (rows, mmax) complex (Hermitian half spectrum, zero beyond mmax) -> x (rows, N);
// act: 0 none, 1 GELU; optional per-row (mean, M2) of the outputs.
// addsrc (may alias x): x = act(addsrc + irfft(in))  (the block's skip branch)
int launch_fft_c2r_rows(const FFTPlan& f, const float2* in, float* x, const float* addsrc,
                        float2* rowstats, int64_t rows, int mmax, int act, hipStream_t s,
                        const struct C2RPlanes* planes = nullptr);
// optional bf16x3 plane output of launch_fft_c2r_rows / _r2c_rows (the next GEMM's B
// operand, gemm_x6p): rows are (b*C + c)*nlat + lat, written to
// xp[b][plane][c][lat*N + n] with plane stride C*nlat*N; x (fp32) is not written
struct C2RPlanes {
  unsigned short* xp;
  int C, nlat;
};
bool fft_c2r_planes_supported(const FFTPlan& f, int mmax);
bool fft_r2c_planes_supported(const FFTPlan& f, int mmax);


// ---- spectral.hip ------------------------------------------------------------
// Xn (BC, nlat, mmax) complex -> Xt (mmax, R=2BC, ldk); per-bc affine of the
// spatial field folded in: m>0 -> s·X, m=0 -> s·X + 2π·t (real part).
// slab (device, optional, size mmax): Xt slab of each m (-1 = skip); default slab = m.
int launch_transpose_fwd(const float2* Xn, float* Xt, int B, int C, int nlat, int mmax, int ldk,
                         const float* nscale, const float* nshift, hipStream_t s,
                         const int* slab = nullptr, int kpad = 0);
// Yt (mmax, R, ldk) -> Yn (BC, nlat, mmax); m >= mact written as 0.
int launch_transpose_inv(const float* Yt, float2* Yn, int B, int C, int nlat, int mmax, int mact,
                         int ldk, hipStream_t s, const int* slab = nullptr);
// Combine per-(bc) partial (mean, M2) statistics (np partials, each over `cnt`
// elements except the last over `cnt_last`) and produce the affine that
// implements InstanceNorm (+ optional FiLM): y = scale·x + shift.  xscale (or null):
// per (b,c) the power of two 2^(14 - e), |mean| + sqrt(M2) = f 2^e (f in [0.5, 1)),
// under which every element of the channel scales below 2^14 in magnitude
// (|x - mean| <= sqrt(sum (x - mean)^2)): the x3h skip GEMM's B-row scales
int launch_chan_affine(const float2* partials, int64_t np, int64_t cnt, int64_t cnt_last,
                       int B, int C, const float* w, const float* b, float eps,
                       const float* gamma, const float* beta, float film_scale, float* scale,
                       float* shift, hipStream_t s, float* xscale = nullptr,
                       float* lsig = nullptr, float* abound = nullptr);
// abound (or null): per (b,c) |scale| sqrt(M2) + |scale mean + shift| (x 1.001), a bound of
// |scale x + shift| over the channel (|x - mean| <= sqrt(M2)): the fused MLP's x3h range
// latitude-band sharding helpers (band.cpp)
// rowstats (BC, np) (mean, M2) over cnt each -> out (BC, 3) fp64 {n, mean, M2}; xscale
// (or null): the local x3h skip B-row scales as in launch_chan_affine
int launch_stats_partial(const float2* rowstats, int64_t np, int64_t cnt, int64_t BC, double* out,
                         hipStream_t s, float* xscale = nullptr);
// parts (nparts, BC, 3) fp64 -> InstanceNorm (+FiLM) per-(b,c) affine
int launch_chan_affine_parts(const double* parts, int nparts, int B, int C, const float* w,
                             const float* b, float eps, const float* gamma, const float* beta,
                             float film_scale, float* scale, float* shift, hipStream_t s,
                             float* xscale = nullptr, float* abound = nullptr,
                             float* lsig = nullptr);
// the all-to-all buffers are the Legendre GEMMs' own operands: [p][slab][R][2W]
// blocks (common.h msfno_sht_plan_s band fields).  g: the rank's local rows as a
// small symmetric grid (Ke = its band, nh = the band rows that have a mirror row,
// stored after the band, ascending), ldke = W, ldk = 2W.  pack: Xn (local rows)
// -> send (slab perm[m], norm0 affine, fold, zero pads); unpack: recv -> Yn.
int launch_band_pack(const float2* Xn, float* send, int B, int C, const LatGeom& g, int mmax,
                     const float* nscale, const float* nshift, const int* perm, int W,
                     hipStream_t s);
int launch_band_unpack(const float* recv, float2* Yn, int B, int C, const LatGeom& g, int mmax,
                       int mact, const int* perm, hipStream_t s);
// W' [b] = W·diag(scale[b]),  b'[b] = bias + W·shift[b]
int launch_fold_affine(const float* W, const float* bias, const float* scale, const float* shift,
                       float* Wf, float* bf, int B, int O, int I, hipStream_t s);
// out[bc][p] = act(scale[bc]·x[bc][p] + shift[bc] + addend[bc][p]) with optional stats
int launch_affine_rows(const float* x, const float* scale, const float* shift,
                       const float* addend, float* out, int64_t BC, int64_t P, int act,
                       float2* stats, int stats_ld, hipStream_t s);
// ---- mlp_fused.hip: the block MLP with the hidden activation on-chip ----------
// out = W2·GELU(W1·(scale ⊙ x1 + shift) + b1) + b2 (+ resid), C = 256, H = 512 only
bool mlp_fused_supported(int C, int H);
size_t mlp_fused_image_bytes();
// W1 (H x C), W2 (C x H) fp32 -> the kernel's bf16x3 weight image (mlp_fused_image_bytes)
int launch_mlp_fused_images(const float* W1, const float* b1, const float* W2,
                            unsigned short* img, hipStream_t s);
// abound: [B][C] bound of |scale ⊙ x1 + shift| (chan_affine), the x3h range scalars
int launch_mlp_fused(const float* x1, const float* scale, const float* shift, const float* abound,
                     const float* resid, float* out, const unsigned short* img, const float* b1,
                     const float* b2, int B, int64_t P, hipStream_t s);
// mlp_fused_h.hip: the MLP on the x3h engine (fp32 as two fp16 terms, three fp16
// MFMAs per product, row-scaled weights); default (MSFNO_ENGINE=x6 selects the x6 engine)
bool mlp_fused_h_env();
// mlp_gen_h.hip: the standalone MLP (network encoder / decoder) fused on the x3h engine,
// per-pixel range scales; widths (Cin + Cin2, Cout) of the instantiated kernels only
bool mlp_gen_h_supported(int Ct, int H, int Cout);
size_t mlp_gen_h_workspace(int Ct, int H, int Cout);
// xa, xt (both or neither): [B][Cin] per-channel affine applied to x first (a deferred
// norm / FiLM of the producing block).  cache (or null): mlp_gen_h_workspace bytes holding
// the prepared weight image across calls, rebuilt only when cache_valid is 0 (ws is then
// unused)
int launch_mlp_gen_h(const float* x, const float* xa, const float* xt, const float* x2, int Cin,
                     int Cin2, const float* W1,
                     const float* b1, const float* W2, const float* b2, int H, int Cout,
                     const float* addend, int64_t add_bstride, float* out, int B, int64_t P,
                     void* ws, size_t ws_bytes, hipStream_t s, void* cache = nullptr,
                     int cache_valid = 0);
// skip_h.hip: inner skip at C = 256 on the mlp_fused_h tiling (x3h): out = Ws·x + bs, x scaled by the
// power-of-two channel scales xs (|xs x| < 2^14), or per pixel in-kernel when xs is null;
// ws >= skip_h_workspace(B)
bool skip_h_env();
size_t skip_h_workspace(int B);
// side_share: the persistent kernel's workgroups per CU when it runs on the block's side
// stream beside the SHT (0: the default for a kernel that runs alone)
int launch_skip_h(const float* W, const float* xs, const float* x, float* out, const float* bias,
                  int B, int64_t P, void* ws, size_t ws_bytes, hipStream_t s,
                  bool side = false);
// xs[r] = the power of two 2^(14 - e) with max_p |x[r][p]| = f 2^e (rows of P values): the
// x3h B-row scales of a 1x1 conv whose input carries no norm statistics
int launch_chan_pow2_scale(const float* x, int64_t rows, int64_t P, float* xs, hipStream_t s);
// The x3h MLPs' weight preparation (mlp_gen_h.hip; the block MLP's image build uses it too),
// one 256-thread workgroup per row.  eta[j] = 2^-ceil(log2 L_j), L_j = max(||W1_j||_1,
// |b1_j|) for the H rows of W1 (H x Ct; b1 or null)
int launch_x3h_eta(const float* W1, const float* b1, int H, int Ct, float* eta, hipStream_t s);
// Row scales 2^(15 - e), max |row| = f 2^e, of W1 (H x Ct) and of W2' = W2 diag(1 / eta)
// (Cout x H): the scales into s1 [H] / s2 [rows2] (both or neither; null: not stored), their
// inverses into is1 / is2; rows Cout .. rows2 - 1 of s2 / is2 are 0
int launch_x3h_row_scales(const float* W1, const float* W2, const float* eta, int H, int Ct,
                          int Cout, int rows2, float* s1, float* s2, float* is1, float* is2,
                          hipStream_t s);
size_t mlp_fused_h_image_bytes();
int launch_mlp_fused_h_images(const float* W1, const float* b1, const float* W2,
                              unsigned short* img, hipStream_t s);
int launch_mlp_fused_h(const float* x1, const float* scale, const float* shift,
                       const float* abound, const float* resid, float* out,
                       const unsigned short* img, const float* b1, const float* b2, int B,
                       int64_t P, hipStream_t s);
// ---- cgemm.hip -----------------------------------------------------------------
// complex (Ci,Co,2) weight -> Ar, Ai (Co x Ci) row-major (Ar[o][i] = Re w[i][o])
int launch_split_complex_weight(const float* w, float* Ar, float* Ai, int Ci, int Co,
                                hipStream_t s);
// Y = W.X complex per column (3M scheme), X/Y rows [b][re|im][ci|co] in the S layout;
// relu: ComplexReLU(real) on the output
int gemm_c3m(const float* Ar, const float* Ai, const float* X, float* Y, int co, int ci, int N,
             int ldx, int ldy, int64_t sX, int64_t sY, int B, bool relu, hipStream_t s);
// complex (Ci,Co,2) weight -> real (2Co x 2Ci) block matrix [[Wr^T,-Wi^T],[Wi^T,Wr^T]]
int launch_expand_complex_weight(const float* w, float* Wexp, int Ci, int Co, hipStream_t s);
// (mmax,lmax,nlat) reference table -> plan GEMM layout (general or symmetric)
int launch_relayout_table(const msfno_sht_plan_s& p, const float* table, hipStream_t s);
// FiLM backward (film_bwd.hip)
int launch_transpose_mat(const float* A, int rows, int cols, int lda, float* AT, hipStream_t s);
int launch_gelu_grad_mul(float* dh, const float* pre, int64_t n, hipStream_t s);
int launch_film_grad_reduce(const float* du, const float* x1, const float* an, const float* tn,
                            float scale, int BC, int64_t P, float* dgamma, float* dbeta,
                            hipStream_t s);
// ---- row reductions over (S, nlat, nlon) fields on the scaffold of row_reduce.h ------------
// ---- loss.hip: sphere-weighted loss sums and their gradient -----------------------------
// sums[bc] = {sum_h w[h] sum_x (prd - tar)^2, sum_h w[h] sum_x tar^2}; prd, tar (BC, nlat,
// nlon); ws >= loss_workspace_bytes (may hold anything on entry)
size_t loss_workspace_bytes(int BC, int nlat, int nlon);
int launch_loss_sums(const float* prd, const float* tar, const float* w_lat, float* sums, int BC,
                     int nlat, int nlon, void* ws, hipStream_t s);
// dprd[bc][h][x] = 2 gnum[bc] w[h] (prd - tar)
int launch_loss_backward(const float* prd, const float* tar, const float* w_lat,
                         const float* gnum, float* dprd, int BC, int nlat, int nlon,
                         hipStream_t s);
// ---- verify.hip: forecast verification sums -----------------------------------------------
// sums[bc] = {se, err, ae, pa2, ta2, cross} (see verify.hip); clim a stack of (nlat, nlon)
// slabs and clim_slab (BC) device int32 slab indices, -1 = none, or both null;
// ws >= verify_workspace_bytes (may hold anything on entry)
size_t verify_workspace_bytes(int BC, int nlat, int nlon);
int launch_verify_sums(const float* prd, const float* tar, const float* w_lat, const float* clim,
                       const int* clim_slab, float* sums, int BC, int nlat, int nlon, void* ws,
                       hipStream_t s);
// ---- verify_regions.hip: the verification sums per region -----------------------------------
// sums[bc][r] = {n, se, err, ae, pa2, ta2, cross} over the valid pixels of region r: bit r of
// row_bits[h] & col_bits[x] & pix_bits[h][x] (pix_bits may be null: all ones), 1 <= nregions
// <= 32; skip_nan drops the pixels whose truth (or climatology, where the slab has one) is
// NaN; ws >= verify_regions_workspace_bytes (may hold anything on entry)
size_t verify_regions_workspace_bytes(int BC, int nlat, int nlon, int nregions);
int launch_verify_region_sums(const float* prd, const float* tar, const float* w_lat,
                              const float* clim, const int* clim_slab, const uint32_t* row_bits,
                              const uint32_t* col_bits, const uint32_t* pix_bits, int nregions,
                              int skip_nan, float* sums, int BC, int nlat, int nlon, void* ws,
                              hipStream_t s);
// ---- ensemble.hip: ensemble verification sums and the CRPS gradient -------------------------
// member i of slab s at ens + i * mstride + s * nlat * nlon (mstride in floats);
// sums[s] = {se, err, abs, gini, sq}, hist[s][0..M] the weighted rank counts or null (see
// ensemble.hip); 2 <= M <= 32; ws >= ens_workspace_bytes (may hold anything on entry)
size_t ens_workspace_bytes(int S, int M, int nlat, int nlon);
int launch_ens_sums(const float* ens, int64_t mstride, const float* tar, const float* w_lat,
                    float* sums, float* hist, int M, int S, int nlat, int nlon, void* ws,
                    hipStream_t s);
// dens_i = w[h] g[s] (sign(x_i - y) / M - kappa sum_{j != i} sign(x_i - x_j))
int launch_ens_crps_backward(const float* ens, int64_t mstride, const float* tar,
                             const float* w_lat, const float* g, float kappa, float* dens,
                             int64_t dstride, int M, int S, int nlat, int nlon, hipStream_t s);
// ---- ens_products.hip: per-pixel ensemble products and the threshold counts -----------------
constexpr int kEnsMaxLevels = 8;  // quantile levels, and thresholds, of one call
// level l of the sorted members: x_(lo) + frac (x_(hi) - x_(lo)), hi = min(lo + 1, M - 1)
struct EnsQuantiles {
  int lo[kEnsMaxLevels], hi[kEnsMaxLevels];
  float frac[kEnsMaxLevels];
};
// (S, nlat, nlon) each, quant (nq, S, nlat, nlon), prob (nt, S, nlat, nlon); null = not wanted
struct EnsProductsOut {
  float *mean, *std, *mn, *mx, *quant, *prob;
};
// members as launch_ens_sums takes them; thr (S, nt) on the device (read where prob is wanted)
int launch_ens_products(const float* ens, int64_t mstride, const EnsQuantiles& q, int nq,
                        const float* thr, int nt, const EnsProductsOut& out, int M, int S,
                        int nlat, int nlon, hipStream_t s);
// counts (S, nt, 2, M + 1): the weighted counts of k members above thr[s][t], and of those
// where the truth is above it too; ws >= ens_threshold_workspace_bytes (may hold anything)
size_t ens_threshold_workspace_bytes(int S, int M, int nt, int nlat);
int launch_ens_threshold_sums(const float* ens, int64_t mstride, const float* tar,
                              const float* w_lat, const float* thr, int nt, float* counts,
                              int M, int S, int nlat, int nlon, void* ws, hipStream_t s);
// ---- pack.hip: 16-bit simple packing of selected fields, and its decode ---------------------
// a source slab's extents, and the origin and step of the window's rows and columns
struct PackWin {
  int nlat, nlon, lat0, lat_step, lon0, lon_step;
};
// q (S_out, nlat_out, nlon_out) dense, ref and exp2 (S_out), all written whole; slab (S_out)
// source slabs on the device or null; ws >= pack16_workspace_bytes (may hold anything)
size_t pack16_workspace_bytes(int S_out, int nlat_out);
int launch_pack16(const float* x, const int* slab, const PackWin& w, int S_out, int nlat_out,
                  int nlon_out, float* ref, int* exp2, unsigned short* q, void* ws,
                  hipStream_t s);
int launch_unpack16(const unsigned short* q, const float* ref, const int* exp2, float* y,
                    int64_t n, int S, hipStream_t s);
// ---- timestats.hip: streaming per-pixel moments over time, and their merge -----------------
// planes of a state of this kind (MSFNO_TSTATS_FIELD / _ERROR) and flags (_MINMAX / _ANOM), 0
// for an unknown kind or a flag the kind does not take
int tstats_planes(int kind, int flags);
// in0, in1 (B, S, P) with batch strides in elements (in1 null for FIELD); clim a stack of (P)
// slabs with clim_slab (B, S) device indices, or both null; count (S, P), state (K, S, P)
// with plane stride ps; the B updates are applied in order
int launch_tstats_update(int kind, int flags, const float* in0, const float* in1, int64_t bs0,
                         int64_t bs1, const float* clim, const int* clim_slab, int B, int S,
                         int64_t P, int skip_nan, uint32_t* count, float* state, int64_t ps,
                         hipStream_t s);
// dst <- dst (+) src over N = S P elements
int launch_tstats_merge(int kind, int flags, uint32_t* dcount, float* dstate, int64_t dps,
                        const uint32_t* scount, const float* sstate, int64_t sps, int64_t N,
                        hipStream_t s);
// ---- regrid.hip: separable banded regridding (conservative, bilinear, block mean) ----------
// one axis as an ELL table on the device: start and count (n_out), w (n_out, taps)
struct RegridAxis {
  int n_in, n_out, taps;
  const int* start;
  const int* count;
  const float* w;
};
constexpr int kRegridMaxLon = 8188;  // the longest source row whose two LDS rows fit 64 KiB
// y (S_out, lat.n_out, lon.n_out) dense, written whole; slab (S_out) source slabs on the
// device or null; mask (lat.n_in, lon.n_in) or null.  Normalised (y = num / den where
// den > 0 and den >= min_valid, else fill) iff a mask is given or skip_nan is set.
int launch_regrid(const float* x, const int* slab, int S_out, const RegridAxis& lat,
                  const RegridAxis& lon, const float* mask, bool skip_nan, float min_valid,
                  float fill, float* y, hipStream_t s);
// ---- graph.hip: the graph-convolution FiLM generator (gcn.cpp) -----------------------------
// node-major activations (nb N, hid), hid % 4 == 0, 16-byte aligned; CSR (rp N + 1, ci, av).
// part (gcn_partial_bytes, may hold anything on entry) receives the fixed-order column
// partials of `out`: per sample (the pool), or over all samples (a bias gradient);
// launch_gcn_colsum_combine(part, out, slabs = nb hid or hid, chunks = gcn_chunks(N) or
// nb gcn_chunks(N)) finishes them in fp64
constexpr int kGcnRows = 32;  // nodes per unit
int gcn_chunks(int N);
size_t gcn_partial_bytes(int nb, int N, int hid);
// bias given: out = resid + leaky(A S + bias) (resid or null), Pout (or null) = A S + bias;
// bias null: out = A S
int launch_gcn_aggregate(const int* rp, const int* ci, const float* av, const float* S,
                         const float* bias, const float* resid, float* out, float* Pout,
                         float* part, int nb, int N, int hid, hipStream_t s);
// out = leaky(ax W0 + b0), ax (nb N, Fin) the aggregated narrow input, W0 (Fin, hid)
int launch_gcn_expand(const float* ax, const float* W0, const float* b0, float* out, float* Pout,
                      float* part, int nb, int N, int Fin, int hid, hipStream_t s);
// dP = dH leaky'(P) (slope where P <= 0), part: the partials of sum_(b, n) dP
int launch_gcn_act_grad(const float* dH, const float* P, float* dP, float* part, int nb, int N,
                        int hid, hipStream_t s);
int launch_gcn_colsum_combine(const float* part, float* out, int slabs, int chunks, hipStream_t s);
// out = A x on rows of F floats, any F (the first layer's input, its gradient)
int launch_gcn_spmm_narrow(const int* rp, const int* ci, const float* av, const float* x,
                           float* out, int nb, int N, int F, hipStream_t s);
// dax (rows, Fin) = dP (rows, hid) W0^T
int launch_gcn_dax(const float* dP, const float* W0, float* dax, int64_t rows, int hid, int Fin,
                   hipStream_t s);
// y (nb, out) = (poolsum / N) Wh^T + bh, and its backward (dpool includes the 1 / N)
int launch_gcn_head(const float* poolsum, const float* Wh, const float* bh, float* y, int nb,
                    int hid, int out, int N, hipStream_t s);
int launch_gcn_head_bwd(const float* dy, const float* poolsum, const float* Wh, float* dpool,
                        float* dWh, float* dbh, int nb, int hid, int out, int N, hipStream_t s);
// dH[(b, n)][:] = dpool[b][:]
int launch_gcn_bcast(const float* dpool, float* dH, int nb, int N, int hid, hipStream_t s);
// ---- spectrum.hip: per-degree power spectrum and its gradient ----------------------------
// coeffs (rows, mmax) complex interleaved, 8-byte aligned, rows = N * lmax:
// power[r] = |c[r][0]|^2 + 2 sum_{m >= 1} |c[r][m]|^2
int launch_spectrum_power(const float* coeffs, float* power, int64_t rows, int mmax,
                          hipStream_t s);
// dcoeffs[r][m] = (2 e_m gpower[r]) coeffs[r][m], e_0 = 1, e_m = 2 (m >= 1)
int launch_spectrum_power_backward(const float* coeffs, const float* gpower, float* dcoeffs,
                                   int64_t rows, int mmax, hipStream_t s);
// ---- noise.hip: spectral coefficients of a spherical Gaussian random field ----------------
// coeffs (n, lmax, mmax) complex interleaved, 8-byte aligned:
// coeffs = a prev + b sqrt_eig[(field0 + i) % K][l] xi(seed, draw, field0 + i, l, m); prev
// null (a ignored) or as coeffs (may be coeffs itself); draw_dev (device) overrides draw
int launch_noise_spectral(float* coeffs, const float* prev, const float* sqrt_eig, int K,
                          int64_t n, int64_t field0, int lmax, int mmax, float a, float b,
                          uint64_t seed, uint64_t draw, const uint64_t* draw_dev,
                          hipStream_t s);
// *draw_dev += by
int launch_noise_advance(uint64_t* draw_dev, uint64_t by, hipStream_t s);
// ---- vector.hip: the streams between the two scalar transforms of a vector transform ------
// A (2bc, lmax + 1, mmax), B (2bc, lmax, mmax) complex -> st (bc, 2, lmax, mmax):
// s = A_theta[l+1] - i B_phi[l], t = A_phi[l+1] + i B_theta[l]; zeros where l < m or l = 0
int launch_vsht_combine(const float2* A, const float2* B, float2* st, int bc, int lmax, int mmax,
                        hipStream_t s);
// st -> Cd (2bc, lmax + 1, mmax) = (s, t) at l + 1 under a zero row, Cq (2bc, lmax, mmax) =
// (-i t, i s); zeros where l < m
int launch_vsht_pack(const float2* st, float2* Cd, float2* Cq, int bc, int lmax, int mmax,
                     hipStream_t s);
// v[i] += q[i], i < n
int launch_vsht_add(float* v, const float* q, int64_t n, hipStream_t s);
// full block backward (block_bwd.cpp): per-row InstanceNorm moments and affine,
// InstanceNorm backward (with the FiLM factor 1 + gamma s and up to two addends),
// ComplexReLU(real) mask, complex conjugate transposes, tril <-> dense spectra, fill
int launch_row_moments(const float* x, int64_t rows, int C, int64_t P, const float* w,
                       const float* b, float eps, float* mean, float* rstd, float* scale,
                       float* shift, hipStream_t s);
int launch_inorm_backward(const float* x, const float* mean, const float* rstd, const float* w,
                          const float* gamma, float film_scale, const float* g, const float* add1,
                          const float* add2, float* dx, int64_t rows, int C, int64_t P,
                          hipStream_t s);
int launch_relu_real_mask(float* dh, const float* h, int64_t n, hipStream_t s);
int launch_conj_swap01(const float* w, int I, int K, int64_t T, float* wt, hipStream_t s);
int launch_tril_map(const float* src, float* dst, int64_t rows, int lmax, int mmax, int64_t T,
                    bool gather, hipStream_t s);
int launch_fill(float* p, int64_t n, float v, hipStream_t s);
// sc = (1 + gamma s) an, sh = (1 + gamma s) tn + beta s (n = B*C)
int launch_film_affine(const float* an, const float* tn, const float* gamma, const float* beta,
                       float film_scale, float* sc, float* sh, int64_t n, hipStream_t s);
// parameter gradients (param_bwd.hip): C[m * ldc + n * cs] = sum_b sum_k A_b[m][k] B'_b[n][k]
// (B' by mode: B, per-(b, n) affine sc B + sh, GELU(B), complex pairs (re, im) -> (im, -re))
enum { WGRAD_PLAIN = 0, WGRAD_AFFINE = 1, WGRAD_GELU = 2, WGRAD_CSWAP = 3 };
size_t wgrad_nt_workspace(int M, int N, int64_t K, int batch);
int launch_wgrad_nt(const float* A, int64_t lda, int64_t sA, const float* B, int64_t ldb,
                    int64_t sB, int M, int N, int64_t K, int batch, int mode, const float* bsc,
                    const float* bsh, float* C, int64_t ldc, int cs, void* ws, size_t ws_bytes,
                    hipStream_t s);
// dw[k][i][t] = sum_b g[b][k][t] conj(a[b][i][t]) (complex, the linear filter's weights)
int launch_lin_wgrad(const float* g, const float* a, float* dw, int B, int Co, int Ci, int64_t T,
                     hipStream_t s);
// InstanceNorm affine gradients (x null: the bias / row-sum gradient db only)
size_t norm_param_grad_workspace(int B, int C);
int launch_norm_param_grad(const float* g, const float* x, const float* mean, const float* rstd,
                           const float* gamma, float film_scale, int B, int C, int64_t P,
                           float* dw, float* db, void* ws, hipStream_t s);
// *d_flag |= 1 unless table[m][l][nlat-1-k] = (-1)^(l-m) table[m][l][k] (rel. 1e-5)
int launch_check_symmetry(const float* table, int mmax, int lmax, int nlat, int* d_flag,
                          hipStream_t s);
// symmetric plans: transposes that fold / unfold the hemispheres (common.h LatGeom)
int launch_transpose_fwd_sym(const float2* Xn, float* Xt, int B, int C, const LatGeom& g, int mmax,
                             const float* nscale, const float* nshift, hipStream_t s);
int launch_transpose_inv_sym(const float* Yt, float2* Yn, int B, int C, const LatGeom& g, int mmax,
                             int mact, hipStream_t s);
// x3h planes (legendre_x3f's A): the folded slab as fp16 pairs interleaved per 8 k
// ([m][R][ldk / 8][plane][8]), scaled per channel by lsig (chan_affine; 1 / sigma -> isr[R])
int launch_transpose_fwd_sym_h(const float2* Xn, unsigned short* Xp, int B, int C,
                               const LatGeom& g, int mmax, const float* nscale,
                               const float* nshift, const float* lsig, float* isr,
                               hipStream_t s);
int launch_band_pack_h(const float2* Xn, unsigned short* send, int B, int C, const LatGeom& g,
                       int mmax, const float* nscale, const float* nshift, const float* lsig,
                       float* isr, const int* perm, int W, hipStream_t s);
// S layout <-> reference (bc, lmax, mmax) complex dense
int launch_spec_to_ref(const msfno_sht_plan_s& p, const float* S, float2* out, int B, int C,
                       const int* d_off, hipStream_t s);
int launch_ref_to_spec(const msfno_sht_plan_s& p, const float2* in, float* S, int B, int C,
                       const int* d_off, hipStream_t s);
// S layout <-> tril (B,C,T,2) (torch.tril_indices(lmax,mmax) order, layers.py:368)
int launch_spec_to_tril(const msfno_sht_plan_s& p, const float* S, float* xt, int B, int C,
                        hipStream_t s);
int launch_tril_to_spec(const msfno_sht_plan_s& p, const float* yt, float* S, int B, int C,
                        hipStream_t s);
// compl_contract_fwd_c: a (B,Ci,T,2), w (Co,Ci,T,2) -> y (B,Co,T,2)
int launch_compl_contract(const float* a, const float* w, float* y, int B, int Ci, int Co,
                          int64_t T, hipStream_t s);
// compl_mul2d_fwd_c reference layout (standalone op)
int launch_compl_mul2d(const float* a, const float* w, float* y, int B, int Ci, int Co,
                       int64_t XY, int relu_real, hipStream_t s);

}  // namespace msfno
