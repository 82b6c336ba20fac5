// Graph-convolution FiLM generator (sst -> gamma, beta): forward, and the backward with
// respect to every parameter and the input.  Per layer S = H W runs on gemm_dense (the
// activation is the split operand, the input-major weight the fp32 one) and the sparse
// kernel of graph.hip forms H + leaky(A S + b): A (h W), so that bias, LeakyReLU, residual
// and the pool ride on the aggregation and the shared GEMMs keep their epilogues.  The first
// layer is rank Fin: (A x) W0, the narrow input aggregated and then expanded.
#include <algorithm>

#include "block.h"

namespace msfno {
namespace {

constexpr int kGcnMaxFin = 16;
constexpr int64_t kGcnMaxRows = 1 << 21;  // B N: the transposes' grid (65535 x 32 rows)

struct GcnBufs {
  // written by a forward, read by the backward of a training forward
  float* ax;       // A x0 (B N, Fin)
  float* poolsum;  // (B, hid) node sums of the last activation
  float* P[MSFNO_GCN_MAX_DEPTH + 1];  // pre-activations of conv1, conv_layers[l - 1]
  float* H[MSFNO_GCN_MAX_DEPTH + 2];  // H[l]: input of conv_layers[l - 1]; H[depth + 1] the last
  float *ha, *hb;  // forward without train: the two activations in flight
  float* part;     // column partials (pool, bias gradients)
  // scratch of one call (the backward reuses the forward's S and gw, then its own)
  float* S;        // H W; backward: dS
  void* gw;        // gemm_dense's split operand
  size_t gw_b;
  float *dHa, *dHb, *dP, *T1, *T2, *Wt, *dpool, *dax, *axT;
  void* wg;
  size_t wg_b;
};

void carve_gcn(Carve& cv, GcnBufs& b, int B, int N, int Fin, int hid, int depth, int train) {
  const int64_t rows = (int64_t)B * N, act = rows * hid;
  b = GcnBufs{};
  b.ax = cv.take<float>(rows * Fin);
  b.poolsum = cv.take<float>((int64_t)B * hid);
  b.part = reinterpret_cast<float*>(cv.take<char>(gcn_partial_bytes(B, N, hid)));
  if (train) {
    for (int l = 0; l <= depth; ++l) b.P[l] = cv.take<float>(act);
    for (int l = 1; l <= depth + 1; ++l) b.H[l] = cv.take<float>(act);
  } else {
    b.ha = cv.take<float>(act);
    b.hb = cv.take<float>(act);
  }
  b.S = cv.take<float>(act);
  b.gw_b = gemm_dense_workspace((int)rows, hid, 1);
  b.gw = cv.take<char>(b.gw_b);
  if (!train) return;
  b.dHa = cv.take<float>(act);
  b.dHb = cv.take<float>(act);
  b.dP = cv.take<float>(act);
  b.T1 = cv.take<float>(act);
  b.T2 = cv.take<float>(act);
  b.Wt = cv.take<float>((int64_t)hid * hid);
  b.dpool = cv.take<float>((int64_t)B * hid);
  b.dax = cv.take<float>(rows * Fin);
  b.axT = cv.take<float>(rows * Fin);
  b.wg_b = wgrad_nt_workspace(std::max(hid, Fin), hid, rows, 1);
  b.wg = cv.take<char>(b.wg_b);
}

// 0: fine, else the status the entry points return
int gcn_sizes(int B, int N, int Fin, int hid, int depth, int out) {
  if (B < 1 || N < 1 || Fin < 1 || hid < 1 || depth < 0 || out < 1) return MSFNO_EINVAL;
  if (hid % 4 != 0 || Fin > kGcnMaxFin || depth > MSFNO_GCN_MAX_DEPTH ||
      (int64_t)B * N > kGcnMaxRows)
    return MSFNO_EUNSUPPORTED;
  return MSFNO_OK;
}

const char* kGcnSizes =
    "gcn: hidden % 4 == 0, in_features <= 16, depth <= 16 and B * N <= 2^21 only";

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace msfno

using namespace msfno;

extern "C" {

size_t msfno_gcn_workspace_size(int B, int N, int Fin, int hidden, int depth, int out,
                                int train) {
  if (gcn_sizes(B, N, Fin, hidden, depth, out) != MSFNO_OK) return 0;
  Carve cv;
  GcnBufs b;
  carve_gcn(cv, b, B, N, Fin, hidden, depth, train);
  return cv.off;
}

static int gcn_check(const msfno_gcn_graph* g, const msfno_gcn_desc* d, int B, bool transposed,
                     const char* what) {
  MSFNO_REQUIRE(g && d, MSFNO_EINVAL, std::string(what) + ": missing graph or descriptor");
  MSFNO_REQUIRE(g->N >= 1 && g->nnz >= 0 && B >= 1, MSFNO_EINVAL,
                std::string(what) + ": N, B below 1 or nnz below 0");
  MSFNO_REQUIRE(g->row_ptr && (g->nnz == 0 || (g->col && g->val)), MSFNO_EINVAL,
                std::string(what) + ": missing CSR arrays");
  MSFNO_REQUIRE(!transposed || (g->t_row_ptr && (g->nnz == 0 || (g->t_col && g->t_val))),
                MSFNO_EINVAL, std::string(what) + ": missing CSR arrays of the transpose");
  const int rc = gcn_sizes(B, g->N, d->Fin, d->hidden, d->depth, d->out);
  MSFNO_REQUIRE(rc != MSFNO_EINVAL, MSFNO_EINVAL, std::string(what) + ": bad sizes");
  MSFNO_REQUIRE(rc == MSFNO_OK, MSFNO_EUNSUPPORTED, kGcnSizes);
  bool ok = d->conv1_w && d->conv1_b && d->head_w && d->head_b;
  for (int l = 0; l < d->depth; ++l) ok = ok && d->conv_w[l] && d->conv_b[l];
  MSFNO_REQUIRE(ok, MSFNO_EINVAL, std::string(what) + ": missing parameters");
  ok = aligned16(d->conv1_w) && aligned16(d->conv1_b);
  for (int l = 0; l < d->depth; ++l) ok = ok && aligned16(d->conv_w[l]) && aligned16(d->conv_b[l]);
  MSFNO_REQUIRE(ok, MSFNO_EINVAL, std::string(what) + ": parameters off the 16-byte grid");
  return MSFNO_OK;
}

int msfno_gcn_forward(const msfno_gcn_graph* g, const msfno_gcn_desc* d, const float* x0, float* y,
                      int B, int train, void* ws, size_t ws_bytes, void* stream) {
  MSFNO_TRY(gcn_check(g, d, B, false, "gcn_forward"));
  MSFNO_REQUIRE(x0 && y && ws, MSFNO_EINVAL, "gcn_forward: missing tensors");
  MSFNO_REQUIRE(aligned16(ws), MSFNO_EINVAL, "gcn_forward: workspace off the 16-byte grid");
  const int N = g->N, Fin = d->Fin, hid = d->hidden, depth = d->depth;
  Carve cv;
  cv.base = (char*)ws;
  GcnBufs b;
  carve_gcn(cv, b, B, N, Fin, hid, depth, train);
  MSFNO_REQUIRE(ws_bytes >= cv.off, MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * N;
  MSFNO_TRY(launch_gcn_spmm_narrow(g->row_ptr, g->col, g->val, x0, b.ax, B, N, Fin, s));
  float* h = train ? b.H[1] : b.ha;
  MSFNO_TRY(launch_gcn_expand(b.ax, d->conv1_w, d->conv1_b, h, train ? b.P[0] : nullptr,
                              depth == 0 ? b.part : nullptr, B, N, Fin, hid, s));
  for (int l = 1; l <= depth; ++l) {
    GemmEpi e;
    MSFNO_TRY(gemm_dense(TILE_128x128, h, d->conv_w[l - 1], b.S, rows, hid, hid, hid, hid, hid, 0,
                         0, 0, 1, e, b.gw, b.gw_b, s));
    float* o = train ? b.H[l + 1] : (h == b.ha ? b.hb : b.ha);
    MSFNO_TRY(launch_gcn_aggregate(g->row_ptr, g->col, g->val, b.S, d->conv_b[l - 1], h, o,
                                   train ? b.P[l] : nullptr, l == depth ? b.part : nullptr, B, N,
                                   hid, s));
    h = o;
  }
  MSFNO_TRY(launch_gcn_colsum_combine(b.part, b.poolsum, B * hid, gcn_chunks(N), s));
  return launch_gcn_head(b.poolsum, d->head_w, d->head_b, y, B, hid, d->out, N, s);
}

int msfno_gcn_backward(const msfno_gcn_graph* g, const msfno_gcn_desc* d, const float* dy,
                       const msfno_gcn_grads* gr, float* dx0, int B, void* ws, size_t ws_bytes,
                       void* stream) {
  MSFNO_TRY(gcn_check(g, d, B, true, "gcn_backward"));
  MSFNO_REQUIRE(dy && gr && ws, MSFNO_EINVAL, "gcn_backward: missing tensors");
  bool ok = gr->conv1_w && gr->conv1_b && gr->head_w && gr->head_b;
  for (int l = 0; l < d->depth; ++l) ok = ok && gr->conv_w[l] && gr->conv_b[l];
  MSFNO_REQUIRE(ok, MSFNO_EINVAL, "gcn_backward: missing gradient tensors");
  MSFNO_REQUIRE(aligned16(ws), MSFNO_EINVAL, "gcn_backward: workspace off the 16-byte grid");
  const int N = g->N, Fin = d->Fin, hid = d->hidden, depth = d->depth;
  Carve cv;
  cv.base = (char*)ws;
  GcnBufs b;
  carve_gcn(cv, b, B, N, Fin, hid, depth, 1);
  MSFNO_REQUIRE(ws_bytes >= cv.off, MSFNO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * N, chunks = gcn_chunks(N);
  MSFNO_TRY(launch_gcn_head_bwd(dy, b.poolsum, d->head_w, b.dpool, gr->head_w, gr->head_b, B, hid,
                                d->out, N, s));
  float *dH = b.dHa, *dHn = b.dHb;
  MSFNO_TRY(launch_gcn_bcast(b.dpool, dH, B, N, hid, s));
  for (int l = depth; l >= 1; --l) {
    // dP = dH leaky'(P), db = sum dP;  dS = A^T dP;  dW = H^T dS;  dH_prev = dH + dS W^T
    MSFNO_TRY(launch_gcn_act_grad(dH, b.P[l], b.dP, b.part, B, N, hid, s));
    MSFNO_TRY(launch_gcn_colsum_combine(b.part, gr->conv_b[l - 1], hid, B * chunks, s));
    MSFNO_TRY(launch_gcn_aggregate(g->t_row_ptr, g->t_col, g->t_val, b.dP, nullptr, nullptr, b.S,
                                   nullptr, nullptr, B, N, hid, s));
    // launch_wgrad_nt contracts over the contiguous index: both operands feature-major
    MSFNO_TRY(launch_transpose_mat(b.H[l], rows, hid, hid, b.T1, s));
    MSFNO_TRY(launch_transpose_mat(b.S, rows, hid, hid, b.T2, s));
    MSFNO_TRY(launch_wgrad_nt(b.T1, rows, 0, b.T2, rows, 0, hid, hid, rows, 1, WGRAD_PLAIN, nullptr,
                              nullptr, gr->conv_w[l - 1], hid, 1, b.wg, b.wg_b, s));
    MSFNO_TRY(launch_transpose_mat(d->conv_w[l - 1], hid, hid, hid, b.Wt, s));
    GemmEpi e;
    e.addend = dH;
    e.ldd = hid;
    MSFNO_TRY(gemm_dense(TILE_128x128, b.S, b.Wt, dHn, rows, hid, hid, hid, hid, hid, 0, 0, 0, 1,
                         e, b.gw, b.gw_b, s));
    std::swap(dH, dHn);
  }
  // conv1: dW0 = (A x0)^T dP, and to the input dx0 = A^T (dP W0^T)
  MSFNO_TRY(launch_gcn_act_grad(dH, b.P[0], b.dP, b.part, B, N, hid, s));
  MSFNO_TRY(launch_gcn_colsum_combine(b.part, gr->conv1_b, hid, B * chunks, s));
  MSFNO_TRY(launch_transpose_mat(b.dP, rows, hid, hid, b.T2, s));
  MSFNO_TRY(launch_transpose_mat(b.ax, rows, Fin, Fin, b.axT, s));
  MSFNO_TRY(launch_wgrad_nt(b.axT, rows, 0, b.T2, rows, 0, Fin, hid, rows, 1, WGRAD_PLAIN, nullptr,
                            nullptr, gr->conv1_w, hid, 1, b.wg, b.wg_b, s));
  if (!dx0) return MSFNO_OK;
  MSFNO_TRY(launch_gcn_dax(b.dP, d->conv1_w, b.dax, rows, hid, Fin, s));
  return launch_gcn_spmm_narrow(g->t_row_ptr, g->t_col, g->t_val, b.dax, dx0, B, N, Fin, s);
}

}  // extern "C"
