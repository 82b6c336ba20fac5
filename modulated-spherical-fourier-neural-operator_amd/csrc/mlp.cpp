// Channel MLP of the network (encoder / decoder): forward, and the backward with
// respect to its inputs and its parameters.
#include <algorithm>

#include "block.h"

namespace msfno {
namespace {

// msfno_mlp_forward without the fused kernel
struct MlpBufs {
  float* h;  // hidden activation (B, Hid, P), fp32 or bf16x3 planes
  float* t;  // first half of fc1 (two-GEMM concatenation on the fp32 engine only), else null
  void *w1, *w12, *w2;  // split weights: fc1, fc1's x2 columns (Cin2 > 0, else null), fc2
  size_t w1_b, w12_b, w2_b;
};

void carve_mlp(Carve& cv, MlpBufs& b, const msfno_mlp_desc* d, int B, int64_t P) {
  const int64_t Hd = d->Hid;
  b.h = cv.take<float>(std::max<int64_t>((int64_t)B * Hd * P, mlp_h_floats(B, Hd, P)));
  b.t = (d->Cin2 > 0 && !gemm_use_x6()) ? cv.take<float>((int64_t)B * Hd * P) : nullptr;
  b.w1_b = gemm_dense_workspace(d->Hid, d->Cin + d->Cin2, 1);
  b.w1 = cv.take<char>(b.w1_b);
  b.w12_b = d->Cin2 > 0 ? gemm_dense_workspace(d->Hid, d->Cin2, 1) : 0;
  b.w12 = d->Cin2 > 0 ? cv.take<char>(b.w12_b) : nullptr;
  b.w2_b = gemm_dense_workspace(d->Cout, d->Hid, 1);
  b.w2 = cv.take<char>(b.w2_b);
}

// msfno_mlp_backward_input (params false) and msfno_mlp_backward_params
struct MlpBwdBufs {
  float *pre, *t;     // fc1's pre-activation; its first half, then dh
  float *W2T, *W1T;   // W2^T; W1[:, :Cin]^T (before it W1[:, Cin:]^T: Cin2 <= Cin)
  void *w1, *w12, *w2, *w3;  // split weights: W1[:, :Cin], W1[:, Cin:] (or null), W2^T, W1^T
  size_t w1_b, w12_b, w2_b, w3_b;
  void *wg, *nr;  // params: weight-gradient K-split partials, bias-gradient row sums
  size_t wg_b;
};

void carve_mlp_bwd(Carve& cv, MlpBwdBufs& b, const msfno_mlp_desc* d, int B, int64_t P,
                   bool params) {
  const int64_t Hd = d->Hid;
  b.pre = cv.take<float>((int64_t)B * Hd * P);
  b.t = cv.take<float>((int64_t)B * Hd * P);
  b.W2T = cv.take<float>(Hd * d->Cout);
  b.W1T = cv.take<float>((int64_t)d->Cin * Hd);
  b.w1_b = gemm_dense_workspace(d->Hid, d->Cin, 1);
  b.w1 = cv.take<char>(b.w1_b);
  b.w12_b = d->Cin2 > 0 ? gemm_dense_workspace(d->Hid, d->Cin2, 1) : 0;
  b.w12 = d->Cin2 > 0 ? cv.take<char>(b.w12_b) : nullptr;
  b.w2_b = gemm_dense_workspace(d->Hid, d->Cout, 1);
  b.w2 = cv.take<char>(b.w2_b);
  b.w3_b = gemm_dense_workspace(d->Cin, d->Hid, 1);
  b.w3 = cv.take<char>(b.w3_b);
  b.wg = b.nr = nullptr;
  b.wg_b = 0;
  if (!params) return;
  // the widest weight gradient and bias gradient of the two layers
  const int wide = std::max({d->Cin, d->Cin2, d->Hid, d->Cout});
  b.wg_b = wgrad_nt_workspace(wide, wide, P, B);
  b.wg = cv.take<char>(b.wg_b);
  b.nr = cv.take<char>(norm_param_grad_workspace(B, wide));
}

size_t mlp_bwd_workspace(const msfno_mlp_desc* d, int B, long long P, bool params) {
  if (!d || B <= 0 || P <= 0) return 0;
  Carve cv;
  MlpBwdBufs b;
  carve_mlp_bwd(cv, b, d, B, P, params);
  return cv.off;
}

}  // namespace
}  // namespace msfno

using namespace msfno;

// ---------------------------------------------------------------------------
// channel MLP (encoder / decoder of the network)
// ---------------------------------------------------------------------------
extern "C" {

size_t msfno_mlp_workspace_size(const msfno_mlp_desc* d, int B, long long P) {
  if (!d || B <= 0 || P <= 0) return 0;
  if (mlp_gen_h_supported(d->Cin + d->Cin2, d->Hid, d->Cout))
    return mlp_gen_h_workspace(d->Cin + d->Cin2, d->Hid, d->Cout);
  Carve cv;
  MlpBufs b;
  carve_mlp(cv, b, d, B, P);
  return cv.off;
}

int msfno_mlp_fused_supported(const msfno_mlp_desc* d) {
  return d && mlp_gen_h_supported(d->Cin + d->Cin2, d->Hid, d->Cout) ? 1 : 0;
}

size_t msfno_mlp_wcache_size(const msfno_mlp_desc* d) {
  return msfno_mlp_fused_supported(d) ? mlp_gen_h_workspace(d->Cin + d->Cin2, d->Hid, d->Cout) : 0;
}

int msfno_mlp_forward_affine(const msfno_mlp_desc* d, const float* x, const float* x_scale,
                             const float* x_shift, const float* x2, const float* addend,
                             long long add_bstride, float* out, int B, long long P, void* ws,
                             size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(d && x && x_scale && x_shift && out && d->fc1_w && d->fc1_b && d->fc2_w,
                MSFNO_EINVAL, "mlp_forward_affine: missing tensors");
  MSFNO_REQUIRE(msfno_mlp_fused_supported(d), MSFNO_EUNSUPPORTED,
                "mlp_forward_affine: widths without the fused x3h kernel");
  MSFNO_REQUIRE((d->Cin2 > 0) == (x2 != nullptr) && B > 0 && P > 0 &&
                    ws_bytes >= msfno_mlp_workspace_size(d, B, P),
                MSFNO_EINVAL, "mlp_forward_affine: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  prof(ST_MLP_GEN, s);
  MSFNO_TRY(launch_mlp_gen_h(x, x_scale, x_shift, x2, d->Cin, d->Cin2, d->fc1_w, d->fc1_b, d->fc2_w,
                             d->fc2_b, d->Hid, d->Cout, addend, add_bstride, out, B, P, ws,
                             ws_bytes, s, d->wcache, d->wcache_valid));
  prof(ST_END, s);
  return MSFNO_OK;
}

int msfno_mlp_forward(const msfno_mlp_desc* d, const float* x, const float* x2,
                      const float* addend, long long add_bstride, float* out, int B,
                      long long P, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(d && x && out && d->fc1_w && d->fc2_w && d->fc1_b, MSFNO_EINVAL,
                "mlp: missing tensors");
  MSFNO_REQUIRE(d->Cin > 0 && d->Hid > 0 && d->Cout > 0 && d->Cin2 >= 0 && B > 0 && P > 0,
                MSFNO_EINVAL, "mlp: bad sizes");
  MSFNO_REQUIRE((d->Cin2 > 0) == (x2 != nullptr), MSFNO_EINVAL,
                "mlp: x2 must be given exactly when Cin2 > 0");
  MSFNO_REQUIRE(P <= 0x7fffffff, MSFNO_EINVAL, "mlp: too many pixels");
  MSFNO_REQUIRE(ws_bytes >= msfno_mlp_workspace_size(d, B, P), MSFNO_EWORKSPACE,
                "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (mlp_gen_h_supported(d->Cin + d->Cin2, d->Hid, d->Cout)) {
    // one fused x3h launch, the hidden activation on-chip (mlp_gen_h.hip)
    prof(ST_MLP_GEN, s);
    MSFNO_TRY(launch_mlp_gen_h(x, nullptr, nullptr, x2, d->Cin, d->Cin2, d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b,
                               d->Hid, d->Cout, addend, add_bstride, out, B, P, ws, ws_bytes, s,
                               d->wcache, d->wcache_valid));
    prof(ST_END, s);
    return MSFNO_OK;
  }
  Carve cv;
  cv.base = (char*)ws;
  MlpBufs b;
  carve_mlp(cv, b, d, B, P);
  const int64_t Hd = d->Hid, Ct = d->Cin + d->Cin2;
  const int Pi = (int)P;
  // x6 engine: h travels as bf16x3 planes [B][3][Hd][ldh] (fc1's epilogue splits it
  // once); fc2 stages it by LDS-DMA (gemm_x6p) or, for Cout <= 128 (the decoder's
  // 256 -> 73), on the 128-row x6 tile with plane B
  const bool planes = mlp_h_planes(b.w1 != nullptr && b.w2 != nullptr);
  const int64_t ldh = planes ? round_up(P, 8) : P;
  unsigned short* hx = planes ? reinterpret_cast<unsigned short*>(b.h) : nullptr;
  prof(ST_FC1, s);
  if (d->Cin2 > 0 && gemm_use_x6()) {
    // fc1 over the concatenation [x ; x2] as one GEMM, K = Cin + Cin2: the B rows past
    // Cin are read from x2 in place (GemmEpi::b2)
    GemmEpi e1;
    e1.bias = d->fc1_b;
    e1.act = 1;
    e1.b2 = x2; e1.b2_k = d->Cin; e1.b2_ld = Pi; e1.b2_stride = (int64_t)d->Cin2 * P;
    if (planes) { e1.c_planes = hx; e1.c_plane_stride = Hd * ldh; }
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w, x, b.h, (int)Hd, Pi, (int)Ct, (int)Ct, Pi,
                         (int)ldh, 0, (int64_t)d->Cin * P, (planes ? 3 : 1) * Hd * ldh, B, e1,
                         b.w1, b.w1_b, s));
  } else if (d->Cin2 > 0) {
    // fc1 over the concatenation [x ; x2]: t = W1[:, :Cin]·x, then h = GELU(W1[:, Cin:]·x2 + b1 + t)
    GemmEpi e0;
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w, x, b.t, (int)Hd, Pi, d->Cin, (int)Ct, Pi,
                         Pi, 0, (int64_t)d->Cin * P, Hd * P, B, e0, b.w1, b.w1_b, s));
    GemmEpi e1;
    e1.bias = d->fc1_b;
    e1.addend = b.t; e1.sD = Hd * P; e1.ldd = Pi;
    e1.act = 1;
    if (planes) { e1.c_planes = hx; e1.c_plane_stride = Hd * ldh; }
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w + d->Cin, x2, b.h, (int)Hd, Pi, d->Cin2,
                         (int)Ct, Pi, (int)ldh, 0, (int64_t)d->Cin2 * P,
                         (planes ? 3 : 1) * Hd * ldh, B, e1, b.w12, b.w12_b, s));
  } else {
    GemmEpi e1;
    e1.bias = d->fc1_b;
    e1.act = 1;
    if (planes) { e1.c_planes = hx; e1.c_plane_stride = Hd * ldh; }
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w, x, b.h, (int)Hd, Pi, d->Cin, d->Cin, Pi,
                         (int)ldh, 0, (int64_t)d->Cin * P, (planes ? 3 : 1) * Hd * ldh, B, e1,
                         b.w1, b.w1_b, s));
  }
  prof(ST_FC2, s);
  GemmEpi e2;
  e2.bias = d->fc2_b;
  if (addend) { e2.addend = addend; e2.sD = add_bstride; e2.ldd = Pi; }
  if (planes) {
    e2.b_planes = hx;
    e2.b_plane_stride = Hd * ldh;
    if (d->Cout > 128) {
      MSFNO_TRY(gemm_x6p(d->fc2_w, out, d->Cout, Pi, (int)Hd, (int)Hd, (int)ldh, Pi, 0,
                         3 * Hd * ldh, (int64_t)d->Cout * P, B, e2, b.w2, b.w2_b, s));
      prof(ST_END, s);
      return MSFNO_OK;
    }
  }
  const GemmTile t2 = d->Cout <= 128 ? TILE_128x128 : TILE_256x128;
  MSFNO_TRY(gemm_dense(t2, d->fc2_w, b.h, out, d->Cout, Pi, (int)Hd, (int)Hd, (int)ldh, Pi,
                       0, (planes ? 3 : 1) * Hd * ldh, (int64_t)d->Cout * P, B, e2, b.w2, b.w2_b,
                       s));
  prof(ST_END, s);
  return MSFNO_OK;
}

}  // extern "C"

extern "C" {

size_t msfno_mlp_backward_input_workspace_size(const msfno_mlp_desc* d, int B, long long P) {
  return mlp_bwd_workspace(d, B, P, false);
}

size_t msfno_mlp_backward_params_workspace_size(const msfno_mlp_desc* d, int B, long long P) {
  return mlp_bwd_workspace(d, B, P, true);
}

int msfno_mlp_backward_input(const msfno_mlp_desc* d, const float* x, const float* x2,
                             const float* dy, float* dx, int B, long long P, void* ws,
                             size_t ws_bytes, void* stream) {
  MSFNO_REQUIRE(dx, MSFNO_EINVAL, "mlp backward: missing tensors");
  return msfno_mlp_backward_params(d, x, x2, dy, dx, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   B, P, ws, ws_bytes, stream);
}

int msfno_mlp_backward_params(const msfno_mlp_desc* d, const float* x, const float* x2,
                              const float* dy, float* dx, float* dx2, float* dfc1_w,
                              float* dfc1_b, float* dfc2_w, float* dfc2_b, int B, long long P,
                              void* ws, size_t ws_bytes, void* stream) {
  const bool params = dfc1_w || dfc1_b || dfc2_w || dfc2_b || dx2;
  MSFNO_REQUIRE(d && x && dy && d->fc1_w && d->fc2_w && d->fc1_b, MSFNO_EINVAL,
                "mlp backward: missing tensors");
  MSFNO_REQUIRE(d->Cin > 0 && d->Hid > 0 && d->Cout > 0 && d->Cin2 >= 0 && B > 0 && P > 0 &&
                    P <= 0x7fffffff,
                MSFNO_EINVAL, "mlp backward: bad sizes");
  MSFNO_REQUIRE((d->Cin2 > 0) == (x2 != nullptr), MSFNO_EINVAL,
                "mlp backward: x2 must be given exactly when Cin2 > 0");
  // (W1T and w3 are sized for dx: they hold dx2's Cin2 x Hid transpose first)
  MSFNO_REQUIRE(!dx2 || (x2 && d->Cin2 > 0 && d->Cin2 <= d->Cin), MSFNO_EINVAL,
                "mlp backward: dx2 needs x2 and Cin2 <= Cin");
  Carve cv;
  cv.base = (char*)ws;
  MlpBwdBufs b;
  carve_mlp_bwd(cv, b, d, B, P, params);
  MSFNO_REQUIRE(ws_bytes >= cv.off, MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t Hd = d->Hid, Ct = d->Cin + d->Cin2;
  const int Pi = (int)P;
  // pre = W1 [x ; x2] + b1 (fc1 without its GELU)
  if (d->Cin2 > 0) {
    GemmEpi e0;
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w, x, b.t, (int)Hd, Pi, d->Cin, (int)Ct, Pi,
                         Pi, 0, (int64_t)d->Cin * P, Hd * P, B, e0, b.w1, b.w1_b, s));
    GemmEpi e1;
    e1.bias = d->fc1_b;
    e1.addend = b.t; e1.sD = Hd * P; e1.ldd = Pi;
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w + d->Cin, x2, b.pre, (int)Hd, Pi, d->Cin2,
                         (int)Ct, Pi, Pi, 0, (int64_t)d->Cin2 * P, Hd * P, B, e1, b.w12, b.w12_b,
                         s));
  } else {
    GemmEpi e1;
    e1.bias = d->fc1_b;
    MSFNO_TRY(gemm_dense(TILE_128x256, d->fc1_w, x, b.pre, (int)Hd, Pi, d->Cin, d->Cin, Pi,
                         Pi, 0, (int64_t)d->Cin * P, Hd * P, B, e1, b.w1, b.w1_b, s));
  }
  // dh = GELU'(pre) * W2^T dy ;  dx = W1[:, :Cin]^T dh
  MSFNO_TRY(launch_transpose_mat(d->fc2_w, d->Cout, (int)Hd, (int)Hd, b.W2T, s));
  GemmEpi e0;
  float* dh = b.t;
  MSFNO_TRY(gemm_dense(TILE_256x128, b.W2T, dy, dh, (int)Hd, Pi, d->Cout, d->Cout, Pi, Pi,
                       0, (int64_t)d->Cout * P, Hd * P, B, e0, b.w2, b.w2_b, s));
  if (params) {
    // dW2 = dy GELU(pre)^T and db2 = sum dy, before dh overwrites pre's partner buffer
    if (dfc2_w)
      MSFNO_TRY(launch_wgrad_nt(dy, P, (int64_t)d->Cout * P, b.pre, P, Hd * P, d->Cout, (int)Hd, P,
                                B, WGRAD_GELU, nullptr, nullptr, dfc2_w, Hd, 1, b.wg, b.wg_b, s));
    if (dfc2_b)
      MSFNO_TRY(launch_norm_param_grad(dy, nullptr, nullptr, nullptr, nullptr, 0.f, B, d->Cout, P,
                                       nullptr, dfc2_b, b.nr, s));
    MSFNO_TRY(launch_gelu_grad_mul(dh, b.pre, (int64_t)B * Hd * P, s));
    // dW1 = dpre [x ; x2]^T (columns Cin.. from x2), db1 = sum dpre
    if (dfc1_w) {
      MSFNO_TRY(launch_wgrad_nt(dh, P, Hd * P, x, P, (int64_t)d->Cin * P, (int)Hd, d->Cin, P, B,
                                WGRAD_PLAIN, nullptr, nullptr, dfc1_w, Ct, 1, b.wg, b.wg_b, s));
      if (d->Cin2 > 0)
        MSFNO_TRY(launch_wgrad_nt(dh, P, Hd * P, x2, P, (int64_t)d->Cin2 * P, (int)Hd, d->Cin2, P, B,
                                  WGRAD_PLAIN, nullptr, nullptr, dfc1_w + d->Cin, Ct, 1, b.wg,
                                  b.wg_b, s));
    }
    if (dfc1_b)
      MSFNO_TRY(launch_norm_param_grad(dh, nullptr, nullptr, nullptr, nullptr, 0.f, B, (int)Hd, P,
                                       nullptr, dfc1_b, b.nr, s));
  } else {
    MSFNO_TRY(launch_gelu_grad_mul(dh, b.pre, (int64_t)B * Hd * P, s));
  }
  if (dx2) {
    // dx2 = W1[:, Cin:]^T dpre (W1T holds the Cin2 x Hd transpose first, then dx's)
    MSFNO_TRY(launch_transpose_mat(d->fc1_w + d->Cin, (int)Hd, d->Cin2, (int)Ct, b.W1T, s));
    MSFNO_TRY(gemm_dense(TILE_256x128, b.W1T, dh, dx2, d->Cin2, Pi, (int)Hd, (int)Hd, Pi,
                         Pi, 0, Hd * P, (int64_t)d->Cin2 * P, B, e0, b.w3, b.w3_b, s));
  }
  if (!dx) return MSFNO_OK;
  MSFNO_TRY(launch_transpose_mat(d->fc1_w, (int)Hd, d->Cin, (int)Ct, b.W1T, s));
  return gemm_dense(TILE_256x128, b.W1T, dh, dx, d->Cin, Pi, (int)Hd, (int)Hd, Pi, Pi, 0,
                    Hd * P, (int64_t)d->Cin * P, B, e0, b.w3, b.w3_b, s);
}

}  // extern "C"
