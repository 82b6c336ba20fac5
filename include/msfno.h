/*
 * msfno.h — C-ABI of libmsfno.so, the MI355X (gfx950) implementation of the
 * SFNO-Block forward hot path of Slusny/Modulated-Spherical-Fourier-Neural-Operator.
 *
 * The reference path is pure Python/PyTorch (no FFI).  Every entry point below
 * replaces one stock-torch / torch-harmonics call of the reference; the
 * replaced interface is cited on each declaration (paths relative to the
 * reference repo).  The Python host layer (msfno_amd/, ctypes) mirrors the
 * reference module API on top of these functions.
 *
 * Conventions
 *   - Plain pointers + sizes; every device pointer is caller-owned (PyTorch
 *     tensors); the library owns only plans (tables, twiddles, descriptors).
 *   - All work is stream-ordered on the hipStream_t passed as `stream`
 *     (void*); no call synchronises the device, allocates device memory or
 *     copies to the host, except *_plan_create/_load_* (one-time setup).
 *   - Return value: 0 = ok, otherwise an MSFNO_E* code; msfno_last_error()
 *     returns a thread-local message.  The Python layer re-raises the
 *     reference's exception types (NotImplementedError / ValueError /
 *     AssertionError) from these codes.
 *   - fp32 arithmetic throughout (complex64 in spectral space), as the
 *     reference runs its transforms with autocast disabled
 *     (MSFNO/Models/sfno/layers.py:403-422, 627-637).
 */
#ifndef MSFNO_H
#define MSFNO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSFNO_OK 0
#define MSFNO_EINVAL 1         /* bad argument / shape   -> ValueError / AssertionError */
#define MSFNO_EUNSUPPORTED 2   /* unsupported config    -> NotImplementedError        */
#define MSFNO_EHIP 3           /* HIP runtime failure   -> RuntimeError               */
#define MSFNO_EWORKSPACE 4     /* workspace too small    -> ValueError                 */

#define MSFNO_GRID_EQUIANGULAR 0
#define MSFNO_GRID_LEGENDRE_GAUSS 1

typedef struct msfno_sht_plan_s* msfno_sht_plan_t;

const char* msfno_last_error(void);
int msfno_abi_version(void);

/* ---------------------------------------------------------------------------
 * Host-side plan math (fp64).  Replaces torch_harmonics.quadrature
 * (used at MSFNO/Models/losses.py:90,129) and torch_harmonics.legendre as
 * used by RealSHT/InverseRealSHT.__init__ (constructed at
 * MSFNO/Models/sfno/sfnonet.py:537-548).
 * ------------------------------------------------------------------------- */
/* nodes ascending in [-1,1] (cos of colatitude, before the north->south flip) */
int msfno_quadrature(int nlat, int grid, double* nodes, double* weights);
/* table (mmax, lmax, nlat) float64, colatitudes north->south:
 *   inverse == 0 : P̄_l^m(cos θ_k) · w_k   (RealSHT.weights)
 *   inverse == 1 : P̄_l^m(cos θ_k)         (InverseRealSHT.pct)
 * orthonormal ("ortho") normalisation, Condon–Shortley phase if csphase. */
int msfno_legendre_table(int mmax, int lmax, int nlat, int grid, int inverse, int csphase,
                         double* table);

/* ---------------------------------------------------------------------------
 * SHT plans.  One plan per transform object (RealSHT / InverseRealSHT).
 * ------------------------------------------------------------------------- */
int msfno_sht_plan_create(int nlat, int nlon, int lmax, int mmax, int inverse,
                          msfno_sht_plan_t* plan);
int msfno_sht_plan_destroy(msfno_sht_plan_t plan);
/* Copy + re-lay-out the module's table (mmax,lmax,nlat) fp32 device buffer
 * (RealSHT.weights incl. the ×1e5 of sfnonet.py:552/554, or
 * InverseRealSHT.pct incl. the ÷1e5 of :553/:555) into the plan's GEMM layout. */
int msfno_sht_plan_load_table(msfno_sht_plan_t plan, const float* table, void* stream);

/* RealSHT.forward  (torch_harmonics RealSHT; called at layers.py:405,629):
 *   x (bc, nlat, nlon) fp32  ->  out (bc, lmax, mmax) complex64 interleaved */
size_t msfno_sht_workspace_size(msfno_sht_plan_t plan, int bc);
int msfno_sht_forward(msfno_sht_plan_t plan, const float* x, float* out, int bc,
                      void* ws, size_t ws_bytes, void* stream);
/* InverseRealSHT.forward (called at layers.py:421,638):
 *   in (bc, lmax, mmax) complex64 -> x (bc, nlat, nlon) fp32 */
int msfno_sht_inverse(msfno_sht_plan_t plan, const float* in, float* x, int bc,
                      void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Vector spherical harmonic transforms (torch_harmonics RealVectorSHT /
 * InverseRealVectorSHT; the reference forecasts 30 wind components and never transforms
 * them; the Python mirror is msfno_amd/harmonics/vector.py).  A tangent field has the
 * components (v_θ, v_φ), southward and eastward; s is its spheroidal coefficient (of
 * ∇Y_lm) and t its toroidal one (of r̂ × ∇Y_lm).  With D_l^m = dP̄_l^m/dθ,
 * Q_l^m = m P̄_l^m / sin θ and the scalar transforms' longitude step, per m:
 *   synthesis  v_θ = Σ_l D s - i Q t,              v_φ = Σ_l i Q s + D t
 *   analysis   s = 1/(l(l+1)) Σ_k w_k [D v_θ - i Q v_φ],  t = 1/(l(l+1)) Σ_k w_k [i Q v_θ + D v_φ]
 * with s = t = 0 at l = 0 and where l < m.
 *
 * msfno_vector_legendre_table: table (2, mmax, lmax, nlat) float64, [0] = D, [1] = Q,
 * colatitudes north->south, normalisation and phase of msfno_legendre_table; inverse == 0
 * multiplies both by w_k / (l(l+1)) (the l = 0 row is zero), inverse == 1 leaves them bare.
 * Rows l < m are zero; no step divides by sin θ, so the pole columns are exact (zero but for
 * m = 1, where D = Q).
 *
 * A vector transform runs on two scalar plans of its direction, made and loaded by
 * msfno_sht_plan_create / msfno_sht_plan_load_table:
 *   plan_d  lmax + 1 degrees, table row l + 1 = D_l (row 0 zero): moved up one degree, D has
 *           the equatorial parity of a scalar table and takes the hemisphere-folded path;
 *   plan_q  lmax degrees, table Q.
 * v (bc, 2, nlat, nlon) fp32, st (bc, 2, lmax, mmax) complex64 interleaved, [.][0] = s and
 * [.][1] = t; every word of the output is written.  Nothing allocates, synchronises or
 * memsets, so the calls record into a graph (after one call outside it, as the scalar
 * transforms).  MSFNO_EINVAL for null pointers, bc < 1, plans that differ in grid, mmax or
 * direction, are of the wrong direction, or whose degree counts are not lmax + 1 and lmax;
 * MSFNO_EWORKSPACE for a short workspace; all before any launch.
 * msfno_vsht_workspace_size returns 0 for a pair of plans the transforms refuse.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
int msfno_vector_legendre_table(int mmax, int lmax, int nlat, int grid, int inverse,
                                int csphase, double* table);
size_t msfno_vsht_workspace_size(msfno_sht_plan_t plan_d, msfno_sht_plan_t plan_q, int bc);
int msfno_vsht_forward(msfno_sht_plan_t plan_d, msfno_sht_plan_t plan_q, const float* v,
                       float* st, int bc, void* ws, size_t ws_bytes, void* stream);
int msfno_vsht_inverse(msfno_sht_plan_t plan_d, msfno_sht_plan_t plan_q, const float* st,
                       float* v, int bc, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Contractions (MSFNO/Models/sfno/contractions.py)
 * ------------------------------------------------------------------------- */
/* compl_contract_fwd_c  (contractions.py:37-41, einsum "bin,kin->bkn"):
 *   a (B,Ci,T,2), w (Co,Ci,T,2) -> y (B,Co,T,2)   [linear filter, layers.py:410-413] */
int msfno_compl_contract_fwd_c(const float* a, const float* w, float* y, int B, int Ci,
                               int Co, int T, void* stream);
/* compl_mul2d_fwd_c (contractions.py:132-137, einsum "bixy,io->boxy"):
 *   a (B,Ci,XY,2), w (Ci,Co,2) -> y (B,Co,XY,2); relu_real != 0 fuses
 *   ComplexReLU(mode="real") (activations.py:42-46) */
int msfno_compl_mul2d_fwd_c(const float* a, const float* w, float* y, int B, int Ci, int Co,
                            long long XY, int relu_real, void* stream);

/* 1x1 convolution, the block's inner skip as a standalone op (nn.Conv2d(C, C, 1) at
 * sfnonet.py:304-307, applied at :366-371):  out[b] = W x[b] + bias (per pixel)
 *   w (Cout, Cin, 1, 1), bias (Cout) or NULL, x (B, Cin, P), out (B, Cout, P); fp32 in and
 *   out, computed on the x3h engine (fp32 as two fp16 terms, three MFMAs per product)
 *   under per-(b, channel) power-of-two scales from max |x| (as accurate as fp32). */
size_t msfno_conv1x1_workspace_size(int B, int Cin, int Cout);
int msfno_conv1x1(const float* w, const float* bias, const float* x, float* out, int B, int Cin,
                  int Cout, long long P, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Fused SFNO-Block forward.
 * Replaces FourierNeuralOperatorBlock.forward (sfnonet.py:221-251) and
 * FourierNeuralOperatorBlock_Filmed.forward (sfnonet.py:359-393) including
 * SpectralFilterLayer (:56-133), SpectralAttentionS2 (layers.py:536-639) /
 * SpectralConvS2 (layers.py:336-427), InstanceNorm2d ×2, FiLM (:689-697) and
 * MLP (layers.py:145-178).
 * ------------------------------------------------------------------------- */
#define MSFNO_FILTER_NONLINEAR 0
#define MSFNO_FILTER_LINEAR 1
#define MSFNO_SKIP_NONE 0
#define MSFNO_SKIP_LINEAR 1
#define MSFNO_SKIP_IDENTITY 2

typedef struct msfno_block_desc {
  int C;                    /* embed_dim_sfno                                       */
  int filter_type;          /* MSFNO_FILTER_*                                       */
  int inner_skip;           /* MSFNO_SKIP_*   (sfnonet.py:304-307)                  */
  int outer_skip;           /* MSFNO_SKIP_NONE / _IDENTITY (sfnonet.py:333-336)      */
  int has_mlp;              /* mlp_mode != "none" (sfnonet.py:323)                  */
  int mlp_hidden;           /* int(C*mlp_ratio)                                      */
  int spectral_layers;      /* non-linear: number of hidden complex layers (w.0..)  */
  int spec_hidden;          /* non-linear: int(hidden_size_factor*C)               */
  float norm_eps;           /* InstanceNorm2d eps (1e-6, sfnonet.py:494)            */
  const float* norm0_w; const float* norm0_b;       /* (C)                          */
  const float* norm1_w; const float* norm1_b;       /* (C)                          */
  const float* spec_w[8];   /* non-linear: w.l  (Cin_l, Cout_l, 2)                  */
  const float* spec_wout;   /* non-linear: wout (spec_hidden, C, 2)                 */
  const float* lin_w;       /* linear: w (C, C, T, 2), T = #tril(lmax,mmax)         */
  const float* skip_w; const float* skip_b;         /* inner_skip (C,C,1,1), (C)    */
  const float* fc1_w; const float* fc1_b;           /* mlp.fwd.0 (H,C,1,1), (H)     */
  const float* fc2_w; const float* fc2_b;           /* mlp.fwd.2 (C,H,1,1), (C)     */
  /* Prepared-weight cache (optional).  The kernels consume the weights as bf16x3
   * "images" (the spectral-MLP 3M A images, the fused block MLP's slice image).
   * wcache: device buffer of msfno_block_wcache_size(d) bytes owned by the caller
   * (one per module), or NULL: the images are rebuilt in the workspace on every
   * call.  wcache_valid = 1: wcache already holds the images of the current weight
   * values (the call skips the preparation); 0: the call rebuilds them into
   * wcache.  The caller tracks weight changes (the Python mirror keys it on the
   * parameters' (data_ptr, _version)). */
  void* wcache;
  int wcache_valid;
} msfno_block_desc;

size_t msfno_block_wcache_size(const msfno_block_desc* d);

size_t msfno_block_workspace_size(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                                  msfno_sht_plan_t inv, int B);
/* x (B,C,nlat_in,nlon_in) -> out (B,C,nlat_out,nlon_out).  gamma/beta (B,C) may
 * be NULL (unfilmed block); FiLM is (1+γ·scale)·x + β·scale after norm1. */
int msfno_block_forward(const msfno_block_desc* d, msfno_sht_plan_t fwd, msfno_sht_plan_t inv,
                        const float* x, const float* gamma, const float* beta, float film_scale,
                        float* out, int B, void* ws, size_t ws_bytes, void* stream);
/* The same block stopped before its output affine (blocks without MLP and outer skip:
 * the network's last block, sfnonet.py:838-846): x1_out (B,C,nlat_out,nlon_out) gets the
 * block's pre-norm1 state and affine_out (2*B*C) the per-(b,c) norm1 (+ FiLM) affine as
 * [scale (B*C)][shift (B*C)]; out = scale * x1 + shift.  The network hands both to
 * msfno_mlp_forward_affine (the decoder), so the affine pass over the full grid is
 * folded into the decoder's input loads.  Workspace: msfno_block_workspace_size. */
int msfno_block_forward_deferred(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                                 msfno_sht_plan_t inv, const float* x, const float* gamma,
                                 const float* beta, float film_scale, float* x1_out,
                                 float* affine_out, int B, void* ws, size_t ws_bytes,
                                 void* stream);
/* FourierNeuralOperatorBlock_Filmed.global_conv(x, residual) (sfnonet.py:341-356): the
 * block up to norm1 -- norm0(x) -> filter -> + inner_skip(residual) (+ GELU for the
 * linear filter) -> norm1 -- without FiLM, MLP or outer skip.  residual may be NULL
 * (= x).  x, residual (B,C,nlat_in,nlon_in) -> out (B,C,nlat_out,nlon_out).
 * Workspace: msfno_block_workspace_size. */
int msfno_block_global_conv(const msfno_block_desc* d, msfno_sht_plan_t fwd, msfno_sht_plan_t inv,
                            const float* x, const float* residual, float* out, int B, void* ws,
                            size_t ws_bytes, void* stream);
/* SpectralFilterLayer.forward alone (sfnonet.py:132-133): SHT -> filter -> ISHT,
 * no norms.  x (B,C,nlat_in,nlon_in) -> y (B,C,nlat_out,nlon_out). */
int msfno_filter_forward(const msfno_block_desc* d, msfno_sht_plan_t fwd, msfno_sht_plan_t inv,
                         const float* x, float* y, int B, void* ws, size_t ws_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------
 * Channel MLP (MSFNO/Models/sfno/layers.py:145-178, MLP.forward) as used by the
 * network encoder and decoder (sfnonet.py:513-523, 617-629, forward :667-686):
 *   out = W2 · GELU(W1 · [x ; x2] + b1) (+ b2) (+ addend)
 * x (B, Cin, P) and the optional second input x2 (B, Cin2, P) are the two halves
 * of the channel concatenation torch.cat((x, residual), dim=1) of the big skip
 * (sfnonet.py:680-681), consumed without materialising it; fc1_w is
 * (Hid, Cin + Cin2).  addend (optional) is added to the output with batch
 * stride add_bstride (0 broadcasts it: the encoder's pos_embed, :674).
 * ------------------------------------------------------------------------- */
typedef struct msfno_mlp_desc {
  int Cin, Cin2, Hid, Cout;
  const float* fc1_w; const float* fc1_b;   /* (Hid, Cin+Cin2, 1, 1), (Hid)  */
  const float* fc2_w; const float* fc2_b;   /* (Cout, Hid, 1, 1), (Cout) or NULL */
  /* Prepared-weight cache of the fused widths (as msfno_block_desc.wcache): NULL, or a
   * device buffer of msfno_mlp_wcache_size(d) bytes owned by the caller (one per
   * module) holding the x3h weight image; wcache_valid = 1 skips its preparation. */
  void* wcache;
  int wcache_valid;
} msfno_mlp_desc;

size_t msfno_mlp_wcache_size(const msfno_mlp_desc* d);
size_t msfno_mlp_workspace_size(const msfno_mlp_desc* d, int B, long long P);
/* 1 when the widths (Cin + Cin2, Hid, Cout) have the one-launch fused x3h kernel
 * (the encoder 73 -> 256 -> 256 and decoder 329 -> 256 -> 73 of the reference config). */
int msfno_mlp_fused_supported(const msfno_mlp_desc* d);
/* msfno_mlp_forward with x replaced by x_scale[b][c] * x + x_shift[b][c] (c < Cin; the
 * affine_out of msfno_block_forward_deferred); fused widths only (MSFNO_EUNSUPPORTED
 * otherwise).  Workspace: msfno_mlp_workspace_size. */
int msfno_mlp_forward_affine(const msfno_mlp_desc* d, const float* x, const float* x_scale,
                             const float* x_shift, const float* x2, const float* addend,
                             long long add_bstride, float* out, int B, long long P, void* ws,
                             size_t ws_bytes, void* stream);
int msfno_mlp_forward(const msfno_mlp_desc* d, const float* x, const float* x2,
                      const float* addend, long long add_bstride, float* out, int B,
                      long long P, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * FiLM backward.  MSFNO fine-tunes only its FiLM
 * generator: the filmed blocks and the decoder run with autograd, every SFNO
 * weight is frozen (MSFNO/Models/sfno/sfnonet.py:787-860, the training loop of
 * MSFNO/main.py).  These entry points give the gradients autograd would
 * compute there.
 *
 * msfno_block_film_backward replaces the backward of
 * FourierNeuralOperatorBlock_Filmed.forward(x, gamma, beta, scale)
 * (sfnonet.py:359-393) with respect to gamma and beta: given dout = dL/d(out),
 *   dgamma[b,c] = scale * sum_p du[b,c,p] * xhat[b,c,p],
 *   dbeta[b,c]  = scale * sum_p du[b,c,p],
 * with xhat = norm1(x1) (InstanceNorm-1 output), u = (1 + gamma scale) xhat +
 * beta scale, du = dL/du (through the channel MLP when the block has one; the
 * identity outer skip does not depend on u).  The forward up to x1 is recomputed
 * (as the reference's checkpoint(blk, ...)).  dL/dx is not produced: with the
 * reference default film_layers = 1 the filmed block is the last one and
 * nothing before it takes gradients.
 * ------------------------------------------------------------------------- */
size_t msfno_block_film_backward_workspace_size(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                                                msfno_sht_plan_t inv, int B);
int msfno_block_film_backward(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                              msfno_sht_plan_t inv, const float* x, const float* gamma,
                              const float* beta, float film_scale, const float* dout,
                              float* dgamma, float* dbeta, int B, void* ws, size_t ws_bytes,
                              void* stream);

/* Full backward of the block, SFNO weights frozen: dx = dL/dx (and dgamma / dbeta for a
 * filmed block) for dout = dL/d(out) of msfno_block_forward -- what --film-layers k
 * (main.py:1083-1087) and --repeat-film (main.py:1133-1136) need, whose filmed blocks
 * run back to back with autograd (sfnonet.py:838-844).  The forward is recomputed.  Two
 * adjoint transform plans (built once by the caller):
 *   fwd_adj: a FORWARD plan on inv's grid, table pct[m,l,k] c_m nlon_out / (2 pi) with
 *            c_m = 1 for m = 0 and m = nlon_out / 2, else 2   (the adjoint of inv);
 *   inv_adj: an INVERSE plan on fwd's grid, table weights[m,l,k] d_m (2 pi) / nlon_in with
 *            d_m = 1 for m = 0 and m = nlon_in / 2, else 1/2  (the adjoint of fwd).
 * dx (B,C,nlat_in,nlon_in), dgamma / dbeta (B,C) may each be NULL; gamma / beta NULL for an
 * unfilmed block. */
size_t msfno_block_backward_workspace_size(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                                           msfno_sht_plan_t inv, msfno_sht_plan_t fwd_adj,
                                           msfno_sht_plan_t inv_adj, int B);
int msfno_block_backward(const msfno_block_desc* d, msfno_sht_plan_t fwd, msfno_sht_plan_t inv,
                         msfno_sht_plan_t fwd_adj, msfno_sht_plan_t inv_adj, const float* x,
                         const float* gamma, const float* beta, float film_scale,
                         const float* dout, float* dx, float* dgamma, float* dbeta, int B,
                         void* ws, size_t ws_bytes, void* stream);
/* Parameter gradients of the block (the reference's --retrain-film, main.py:958-960: the
 * decoder and the last film_layers blocks train, MSFNO/Models/sfno/model.py:922-923,
 * 1016-1019).  Device fp32 outputs, each laid out as the parameter it is the gradient of;
 * NULL = not wanted.  Written (not accumulated). */
typedef struct msfno_block_param_grads {
  float* norm0_w;      /* (C)                     norm0.weight */
  float* norm0_b;      /* (C)                     norm0.bias */
  float* spec_w[8];    /* (Ci, Co, 2)             filter_layer.filter.w.l (non-linear) */
  float* spec_wout;    /* (spec_hidden, C, 2)     filter_layer.filter.wout */
  float* lin_w;        /* (C, C, T, 2)            filter_layer.filter.w (linear) */
  float* skip_w;       /* (C, C)                  inner_skip.weight */
  float* skip_b;       /* (C)                     inner_skip.bias */
  float* norm1_w;      /* (C)                     norm1.weight */
  float* norm1_b;      /* (C)                     norm1.bias */
  float* fc1_w;        /* (mlp_hidden, C)         mlp.fwd.0.weight */
  float* fc1_b;        /* (mlp_hidden)            mlp.fwd.0.bias */
  float* fc2_w;        /* (C, mlp_hidden)         mlp.fwd.2.weight */
  float* fc2_b;        /* (C)                     mlp.fwd.2.bias */
} msfno_block_param_grads;

/* msfno_block_backward plus the parameter gradients `pg` asks for (NULL pg: exactly
 * msfno_block_backward).  Weight gradients reduce over pixels or spectral modes in fp32
 * chunks combined in fp64. */
size_t msfno_block_backward_params_workspace_size(const msfno_block_desc* d,
                                                  msfno_sht_plan_t fwd, msfno_sht_plan_t inv,
                                                  msfno_sht_plan_t fwd_adj,
                                                  msfno_sht_plan_t inv_adj, int B);
int msfno_block_backward_params(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                                msfno_sht_plan_t inv, msfno_sht_plan_t fwd_adj,
                                msfno_sht_plan_t inv_adj, const float* x, const float* gamma,
                                const float* beta, float film_scale, const float* dout, float* dx,
                                float* dgamma, float* dbeta, const msfno_block_param_grads* pg,
                                int B, void* ws, size_t ws_bytes, void* stream);

/* Introspection of msfno_block_backward's workspace: the byte offsets of the recomputed
 * non-linear filter's hidden activations h_l = ComplexReLU(...) (B, spec_hidden, lmax,
 * mmax) complex, l < spectral_layers, whose ReLU(real) masks the backward applies.  Writes
 * at most n offsets and the number of hidden layers (0 for the linear filter) to *nlayers.
 * Lets a test compare the masks the GPU actually used with an oracle's. */
int msfno_block_backward_hidden_offsets(const msfno_block_desc* d, msfno_sht_plan_t fwd,
                                        msfno_sht_plan_t inv, msfno_sht_plan_t fwd_adj,
                                        msfno_sht_plan_t inv_adj, int B, size_t* offsets, int n,
                                        int* nlayers);

/* Backward of the channel MLP (layers.py:145-178) to its first input, weights
 * frozen: the decoder over cat(x, residual) (sfnonet.py:679-686) when the loss
 * gradient dy = dL/dy reaches it.
 *   dx = W1[:, :Cin]^T (GELU'(W1 [x ; x2] + b1) * (W2^T dy))
 * (dL/dx2 is not produced: x2 is the network input.) */
/* The same backward with the second input's and the parameter gradients (the decoder
 * under --retrain-film; a plain network in training, whose big skip x2 is the network
 * input):  dx2 = W1[:, Cin:]^T dpre,  dW1 = dpre [x ; x2]^T, db1 = sum dpre,
 * dW2 = dy GELU(pre)^T, db2 = sum dy (summed over the batch and the P pixels).  dx, dx2
 * and each gradient output may be NULL. */
size_t msfno_mlp_backward_params_workspace_size(const msfno_mlp_desc* d, int B, long long P);
int msfno_mlp_backward_params(const msfno_mlp_desc* d, const float* x, const float* x2,
                              const float* dy, float* dx, float* dx2, float* dfc1_w,
                              float* dfc1_b, float* dfc2_w, float* dfc2_b, int B, long long P,
                              void* ws, size_t ws_bytes, void* stream);
size_t msfno_mlp_backward_input_workspace_size(const msfno_mlp_desc* d, int B, long long P);
int msfno_mlp_backward_input(const msfno_mlp_desc* d, const float* x, const float* x2,
                             const float* dy, float* dx, int B, long long P, void* ws,
                             size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Sphere-weighted training losses (MSFNO/Models/losses.py:6-28, 80-155: CosineMSELoss,
 * L2Sphere, L2Sphere_noSine, built at MSFNO/Models/train.py:434-446 and called once per
 * training step at :162, :229, :283; the validation MSEs of :553-564).  All of them are
 * per (b, c)
 *   num = sum_h w_lat[h] sum_x (prd - tar)^2,    den = sum_h w_lat[h] sum_x tar^2
 * under different latitude weights, finished by a few ops on the (B, C) sums (the Python
 * mirror msfno_amd/losses.py).  prd, tar (BC, nlat, nlon) fp32, w_lat (nlat) fp32.  A
 * latitude band passes its own rows and their weights; the sums of the bands add up.
 * The reduction is deterministic (no atomics: fp32 partials per chunk of rows, combined
 * per (b, c) in fp64 in a fixed order).  The workspace may hold anything on entry.
 *   msfno_loss_sums:     sums (BC, 2) = {num, den}
 *   msfno_loss_backward: dprd = 2 gnum[bc] w_lat[h] (prd - tar), gnum (BC) = dL/d num
 *     (the target takes no gradient, as in the reference)
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
size_t msfno_loss_workspace_size(int BC, int nlat, int nlon);
int msfno_loss_sums(const float* prd, const float* tar, const float* w_lat, float* sums, int BC,
                    int nlat, int nlon, void* ws, size_t ws_bytes, void* stream);
int msfno_loss_backward(const float* prd, const float* tar, const float* w_lat,
                        const float* gnum, float* dprd, int BC, int nlat, int nlon,
                        void* stream);

/* ---------------------------------------------------------------------------
 * Forecast verification: the sums behind RMSE, bias, MAE, the climatology skill score and
 * the anomaly correlation of a rollout (MSFNO/Models/sfno/model.py:737-758 and
 * train.py:533-583 form them on the host after copying every scored output there; the
 * Python mirror is msfno_amd/verification.py).  One pass over prd, tar (BC, nlat, nlon)
 * fp32 and an optional climatology, all in one (real) space; per (b, c) under w_lat (nlat)
 *   sums[bc] = { se    = sum w (p - t)^2,   err   = sum w (p - t),   ae = sum w |p - t|,
 *                pa2   = sum w (p - c)^2,   ta2   = sum w (t - c)^2,
 *                cross = sum w (p - c)(t - c) }
 * clim is a stack of (nlat, nlon) fp32 slabs and clim_slab a device int32[BC]: the slab
 * index of bc (not range-checked), or -1 for none; both NULL for no climatology at all.
 * A slab without one gets pa2 = ta2 = cross = 0 exactly, and every word of sums is
 * written by every call.  A latitude band passes its own rows, their weights and the same
 * rows of clim; the sums of the bands add up.  Deterministic as msfno_loss_sums (no
 * atomics, fp32 partials combined per (b, c) in fp64 in a fixed order); the workspace may
 * hold anything on entry; nothing allocates, synchronises or memsets, so the call records
 * into a graph.  MSFNO_EINVAL for null required pointers, an extent below 1, or only one
 * of clim / clim_slab; MSFNO_EWORKSPACE for a short workspace; both before any launch.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
size_t msfno_verify_workspace_size(int BC, int nlat, int nlon);
int msfno_verify_sums(const float* prd, const float* tar, const float* w_lat, const float* clim,
                      const int* clim_slab, float* sums /* (BC, 6) */, int BC, int nlat,
                      int nlon, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Regional and masked verification: the sums of msfno_verify_sums per region, for
 * 1 <= nregions <= 32 regions of the grid in one call (the Python mirror is
 * msfno_amd/regions.py and verification.region_sums).  Bit r of three device uint32 tables
 * speaks for region r: pixel (h, x) is in region r iff bit r of
 *   row_bits[h] & col_bits[x] & pix_bits[h * nlon + x]
 * is set (row_bits (nlat), col_bits (nlon), pix_bits (nlat, nlon) or NULL for all ones;
 * bits at and above nregions are ignored).  Membership is binary.  A pixel is valid unless
 * skip_nan != 0 and tar is NaN there, or the slab has a climatology and clim is NaN there;
 * a NaN in prd is never skipped.  Per (bc, region), over the region's valid pixels,
 *   sums[bc][r] = { n = sum w, se, err, ae, pa2, ta2, cross }
 * with the last six as in msfno_verify_sums; the scores divide by n, not by nlon sum(w).
 * Out-of-region and skipped pixels are selected out, never multiplied by zero: a region's
 * sums depend only on the values at its own valid pixels (a NaN or Inf elsewhere leaves
 * them bit-identical); a region of all ones with skip_nan = 0 has bitwise the six sums of
 * msfno_verify_sums on the same inputs; a missing truth and a cleared pix_bits bit give
 * the same bits; an empty or all-missing region gives seven +0.  A latitude band passes its
 * own rows of every field, of w_lat, row_bits and pix_bits; the sums of the bands add up.
 * Deterministic as msfno_verify_sums (no atomics, fixed order); every word of sums is
 * written by every call; the workspace may hold anything on entry; nothing allocates,
 * synchronises or memsets, so the call records into a graph.  MSFNO_EINVAL for null
 * required pointers (pix_bits may be NULL), nregions outside 1..32, an extent below 1, or
 * only one of clim / clim_slab; MSFNO_EWORKSPACE for a short workspace; both before any
 * launch.  The workspace size is 0 for arguments the call refuses.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
size_t msfno_verify_regions_workspace_size(int BC, int nlat, int nlon, int nregions);
int msfno_verify_region_sums(const float* prd, const float* tar, const float* w_lat,
                             const float* clim, const int* clim_slab,
                             const uint32_t* row_bits, const uint32_t* col_bits,
                             const uint32_t* pix_bits /* or NULL */, int nregions, int skip_nan,
                             float* sums /* (BC, nregions, 7) */, int BC, int nlat, int nlon,
                             void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Ensemble verification and the (fair) CRPS: the sums behind the ensemble-mean RMSE and
 * bias, the MAE, the spread, the spread/skill ratio, the CRPS, the fair CRPS and the rank
 * histogram of M members against one truth (the reference has no ensemble score; the
 * Python mirror is msfno_amd/ensemble.py).  One pass over the members and tar, all fp32
 * in one (real) space.  Member i of slab s = (b, c) starts at
 *   ens + i * member_stride + s * nlat * nlon
 * (member_stride in floats, >= S * nlat * nlon, any 16-byte phase); tar is (S, nlat, nlon),
 * w_lat (nlat).  Per slab, summed over its pixels, with dbar = (1/M) sum_i (x_i - y):
 *   sums[s] = { se   = sum w dbar^2,   err = sum w dbar,
 *               abs  = sum w (1/M) sum_i |x_i - y|,
 *               gini = sum w sum_{i<j} |x_i - x_j|,
 *               sq   = sum w sum_{i<j} (x_i - x_j)^2 }
 *   hist[s][r] = sum w [#{i : x_i < y} == r],  r = 0..M  (strict <; hist may be NULL,
 *               the ranks are then not formed)
 * Every per-pixel quantity is formed from a difference x_i - y or x_i - x_j, never from
 * the raw values or a raw mean.  CRPS = (abs - gini / M^2) / n and the fair CRPS =
 * (abs - gini / (M (M - 1))) / n with n = nlon sum w; sq = M sum_i (x_i - xbar)^2.
 * 2 <= M <= 32.  A latitude band passes its own rows and their weights; the sums and the
 * histograms of the bands add up.  Deterministic as msfno_loss_sums (no atomics: integer
 * rank counts per row, fp32 partials combined per slab in fp64 in a fixed order); every
 * word of sums and hist is written by every call; the workspace may hold anything on
 * entry; nothing allocates, synchronises or memsets, so the calls record into a graph.
 *   msfno_ens_crps_backward: the gradient of L = sum_s g[s] (abs_s - kappa gini_s),
 *     dens_i = w_lat[h] g[s] (sign(x_i - y) / M - kappa sum_{j != i} sign(x_i - x_j)),
 *     sign(0) = 0 (what autograd gives for |.|), kappa = 1 / M^2 or 1 / (M (M - 1));
 *     member i of dens at dens + i * dens_member_stride + s * nlat * nlon.  g (S).  The
 *     truth takes no gradient.  No workspace.
 * MSFNO_EINVAL for null required pointers, an extent below 1, M < 2 or a member stride
 * shorter than a member; MSFNO_EUNSUPPORTED for M > 32; MSFNO_EWORKSPACE for a short
 * workspace; all before any launch.  msfno_ens_workspace_size returns 0 for arguments
 * that msfno_ens_sums refuses.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
size_t msfno_ens_workspace_size(int S, int M, int nlat, int nlon);
int msfno_ens_sums(const float* ens, long long member_stride, const float* tar,
                   const float* w_lat, float* sums /* (S, 5) */, float* hist /* (S, M + 1) */,
                   int M, int S, int nlat, int nlon, void* ws, size_t ws_bytes, void* stream);
int msfno_ens_crps_backward(const float* ens, long long member_stride, const float* tar,
                            const float* w_lat, const float* g, float kappa, float* dens,
                            long long dens_member_stride, int M, int S, int nlat, int nlon,
                            void* stream);

/* ---------------------------------------------------------------------------
 * Ensemble products and the counts behind the threshold scores (the Python mirror is
 * msfno_amd/ensemble.py: products, threshold_sums, finish_thresholds).  Members as
 * msfno_ens_sums takes them: member i of slab s at ens + i * member_stride + s * nlat * nlon,
 * 2 <= M <= 32, any member stride >= S * nlat * nlon, any 16-byte phase.  Inputs are finite:
 * the caller's contract, it is not checked.
 *   msfno_ens_products: per-pixel maps, one pass over the members, no workspace.  Every
 *   output of *out is optional (NULL: not wanted, its work is not done; at least one is):
 *     mean  (S, nlat, nlon)  x_0 + (1/M) sum_i d_i,  d_i = x_i - x_0
 *     std   (S, nlat, nlon)  sqrt(sum_i (d_i - dm)^2 / (M - 1)),  dm = (1/M) sum_i d_i: the
 *                            unbiased spread from differences, exactly 0 for equal members
 *     min, max (S, nlat, nlon)  members, bit for bit
 *     quant (nq, S, nlat, nlon)  level q_levels[l] of the sorted members x_(0) <= .. <=
 *                            x_(M-1), linear interpolation: with pos = q (M - 1),
 *                            lo = floor(pos), hi = min(lo + 1, M - 1), frac = pos - lo (formed
 *                            on the host in fp64), x_(lo) + frac (x_(hi) - x_(lo)); where
 *                            frac = 0 the member itself, bit for bit.  q_levels is a host
 *                            array of nq <= 8 levels in [0, 1], read before the call returns.
 *     prob  (nt, S, nlat, nlon)  #{i : x_i > thr[s][t]} (1/M), strict >; thr (S, nt) fp32 on
 *                            the device, in field units per slab, nt <= 8
 *   Every word of every wanted output is written.  A latitude band passes its own rows: the
 *   maps are row-local.
 *   msfno_ens_threshold_sums: per slab s and threshold t < nt <= 8, with
 *   k = #{i : x_i > thr[s][t]} and o = [y > thr[s][t]] (strict > on both sides),
 *     counts[s][t][0][k] = sum w_lat[h] [count == k],  k = 0..M
 *     counts[s][t][1][k] = sum w_lat[h] [count == k] [o == 1]
 *   counts (S, nt, 2, M + 1) fp32; tar (S, nlat, nlon), w_lat (nlat).  From them follow the
 *   Brier score and its decomposition, the reliability diagram and the ROC curve.  A latitude
 *   band passes its own rows and their weights; the counts of the bands add up.
 *   Deterministic as msfno_ens_sums (integer counts per row and wave, one weighted add per row
 *   and bin, waves in index order, chunks combined in fp64; no floating-point and no global
 *   atomics); every word of counts is written by every call; the workspace may hold anything
 *   on entry; nothing allocates, synchronises or memsets, so the calls record into a graph.
 * MSFNO_EINVAL for null required pointers, *out with no output wanted, an extent below 1,
 * M < 2, a member stride shorter than a member, a level outside [0, 1], quant wanted with
 * nq < 1, prob wanted with nt < 1 or thr NULL, nq or nt below 0 (nt < 1 for the sums);
 * MSFNO_EUNSUPPORTED for M > 32 or nq, nt > 8; MSFNO_EWORKSPACE for a short workspace; all
 * before any launch.  The workspace size is 0 for arguments that the sums refuse.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
#define MSFNO_ENS_MAX_LEVELS 8
typedef struct msfno_ens_products_out {
  float *mean, *std, *min, *max, *quant, *prob;
} msfno_ens_products_out;
int msfno_ens_products(const float* ens, long long member_stride, const double* q_levels,
                       int nq, const float* thr, int nt, const msfno_ens_products_out* out,
                       int M, int S, int nlat, int nlon, void* stream);
size_t msfno_ens_threshold_workspace_size(int S, int M, int nt, int nlat, int nlon);
int msfno_ens_threshold_sums(const float* ens, long long member_stride, const float* tar,
                             const float* w_lat, const float* thr, int nt,
                             float* counts /* (S, nt, 2, M + 1) */, int M, int S, int nlat,
                             int nlon, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Forecast export: 16-bit simple packing of selected fields on the device, and its decode
 * (the Python mirror is msfno_amd/export.py: pack, unpack, ForecastWriter).  x is (S_in,
 * nlat, nlon) fp32 at any 4-byte alignment.  Per output slab s, over the selected points
 * only, in fp32:
 *     lo = min x, hi = max x, d = hi - lo, ref[s] = lo
 *     exp2[s] = E = 0 where d == 0, else the smallest integer with d <= 65535 * 2^E, at
 *               least -126 (every 65535 * 2^E is exact in fp32: no logarithm is taken)
 *     q = (uint16) rint((x - ref) * 2^-E)   round to nearest even, clamped to [0, 65535];
 *                                           the product with a power of two is exact
 *     decode: xhat = ref + (float)q * 2^E   so |xhat - x| <= 2^(E-1) + ulp(d)/2 + ulp(xhat)/2
 *   The encoding is that of GRIB simple packing with a binary scale, and of a netCDF / zarr
 *   scale_factor = 2^E, add_offset = ref.  A numpy fp32 restatement gives the same bits.
 *   Inputs are finite and so is hi - lo: the caller's contract, it is not checked.
 *   Selection: slab (S_out) int32 on the device gives the source slab of each output slab
 *   (any order, repeats allowed; not range-checked on the device, as clim_slab is not;
 *   NULL: output slab s is slab s, S_out <= S_in); *win picks the rows lat0 + i lat_step,
 *   i < nlat_out, and the columns lon0 + j lon_step, j < nlon_out, of a slab (a host
 *   struct read before the call returns; NULL: the whole slab).  The range is that of the
 *   selected points: a subset gets the precision of its own range.
 *   msfno_pack16 writes ref (S_out), exp2 (S_out) and q (S_out, nlat_out, nlon_out), dense.
 *   msfno_unpack16 decodes S slabs of n_per_slab values into y at any 4-byte alignment.
 *   Deterministic (min and max do not depend on an order; no atomics); every word of ref,
 *   exp2, q and y is written by every call; the workspace may hold anything on entry;
 *   nothing allocates, synchronises or memsets, so the calls record into a graph.
 * MSFNO_EINVAL for null required pointers, an extent or a step below 1, S_out > S_in without
 * a slab list, a window that leaves the slab (lat0 + (nlat_out - 1) lat_step >= nlat,
 * likewise in longitude, or a negative origin); MSFNO_EWORKSPACE for a short workspace; all
 * before any launch.  The workspace size is 0 for arguments that the call refuses.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
typedef struct msfno_window {
  int lat0, lat_step, nlat_out, lon0, lon_step, nlon_out;
} msfno_window;
size_t msfno_pack16_workspace_size(int S_out, int nlat_out, int nlon_out);
int msfno_pack16(const float* x, int S_in, int nlat, int nlon, const int* slab, int S_out,
                 const msfno_window* win, float* ref /* (S_out) */, int* exp2 /* (S_out) */,
                 unsigned short* q /* (S_out, nlat_out, nlon_out), dense */, void* ws,
                 size_t ws_bytes, void* stream);
int msfno_unpack16(const unsigned short* q, const float* ref, const int* exp2, float* y,
                   long long n_per_slab, int S, void* stream);

/* ---------------------------------------------------------------------------
 * Regridding: a separable, banded linear map over (lat, lon), optionally normalised by the
 * valid weight: conservative remapping (WeatherBench's 1.5 degree scores and exports out of
 * 0.25 degree), bilinear sampling, block means (the reference's SST input of the FiLM
 * generator, coarsen(latitude=4, longitude=4, boundary='trim').mean() with NaN over land
 * skipped, MSFNO/Models/data.py:205-213) and their adjoints (the Python mirror is
 * msfno_amd/regrid.py: Grid, Regridder, sst_input).  x is (S_in, lat.n_in, lon.n_in) fp32 and
 * y (S_out, lat.n_out, lon.n_out) fp32, dense, both at any 4-byte alignment.  Each axis is an
 * ELL table on the device: start (n_out) int32, count (n_out) int32, w (n_out, taps) fp32.
 * With cl = count cut to [0, taps] (likewise co), per output point, in fp32:
 *     num[s][j][i] = sum_{a < cl[j]} sum_{b < co[i]} wlat[j][a] wlon[i][b] v
 *                        x[src(s)][clamp(lat.start[j] + a, 0, lat.n_in - 1)]
 *                                 [(lon.start[i] + b) mod lon.n_in]
 *   Linear mode (mask == NULL and skip_nan == 0): v = 1 and y = num; min_valid and fill are
 *   not read.  Only the taps below the count are read, padding never, so a NaN of x reaches
 *   exactly the outputs whose counted taps cover it.
 *   Normalised mode (a mask, skip_nan, or both): v = mask[row][col] (mask (lat.n_in,
 *   lon.n_in) fp32 >= 0, if given) * (x == x) (if skip_nan); den is the same sum over v
 *   alone; y = num / den where den > 0 and den >= min_valid, else fill.  Where v == 0 the
 *   value of x is not multiplied in, so a NaN that is skipped or masked never reaches num.
 *   The latitude index is clamped and the longitude index reduced mod lon.n_in on the device:
 *   a wrong table gives wrong values, never a read outside a slab.  `wrap` records whether
 *   the axis is periodic for the table's maker (the Python builders set it on the longitude);
 *   the device does not read it.  slab (S_out) int32 on the device gives the source slab
 *   src(s) of each output slab (any order, repeats allowed, S_out > S_in allowed; not
 *   range-checked on the device; NULL: src(s) = s, S_out <= S_in), as in msfno_pack16.
 *   Order of every sum: the latitude taps in index order per source column, then the
 *   longitude taps in index order, one fused multiply-add each, the first product of a linear
 *   chain not added to anything (one tap of weight 1 copies the bits).  No atomics and no
 *   workspace: results are bitwise reproducible and do not depend on S, on the launch
 *   geometry or on where a slab sits in a batch.  Every word of y is written by every call;
 *   nothing allocates, synchronises or memsets, so the call records into a graph.
 * MSFNO_EINVAL for null required pointers (x, y, an axis or one of its tables), an extent
 * below 1, taps outside 1..MSFNO_REGRID_MAX_TAPS, S_out > S_in without a slab list, or a
 * negative or non-finite min_valid; MSFNO_EUNSUPPORTED for lon.n_in > 8188 (a source row
 * and its valid weight are staged in 64 KiB of LDS); all before any launch.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
#define MSFNO_REGRID_MAX_TAPS 32
typedef struct msfno_regrid_axis {
  int n_in, n_out, taps, wrap;
  const int* start;   /* (n_out), device */
  const int* count;   /* (n_out), device */
  const float* w;     /* (n_out, taps), device */
} msfno_regrid_axis;
int msfno_regrid(const float* x, int S_in, const int* slab, int S_out,
                 const msfno_regrid_axis* lat, const msfno_regrid_axis* lon,
                 const float* mask /* (nlat_in, nlon_in) >= 0, or NULL */, int skip_nan,
                 float min_valid, float fill, float* y /* (S_out, nlat_out, nlon_out) dense */,
                 void* stream);

/* ---------------------------------------------------------------------------
 * Statistics over time at fixed pixel: climatologies, score maps, the time mean and the
 * variability of a long rollout (the reference forms its hour-of-year climatology on the
 * host, data_process/climatology.py: IterMean, mean += (x - mean) / n; the Python mirror is
 * msfno_amd/timestats.py).  A slab is a flat run of P = nlat * nlon fp32 elements: no
 * latitude weights here.  A state is a uint32 count (S, P) and K fp32 planes (K, S, P),
 * plane k at state + k * plane_stride (in floats, >= S * P); count, state and every input
 * sit at any 4-byte alignment.  K is what the planes call returns for (kind, flags):
 *
 *   kind                  flags                K   planes
 *   MSFNO_TSTATS_FIELD    0                    2   mean, m2
 *   MSFNO_TSTATS_FIELD    MSFNO_TSTATS_MINMAX  4   mean, m2, lo, hi
 *   MSFNO_TSTATS_ERROR    0                    3   mean_d, m2_d, mean_abs
 *   MSFNO_TSTATS_ERROR    MSFNO_TSTATS_ANOM    8   mean_d, m2_d, mean_abs, mean_pa, m2_pa,
 *                                                  mean_ta, m2_ta, c_pt
 *
 * FIELD takes x = in0 (in1 NULL) and the value a = x - c, or a = x without a climatology;
 * ERROR takes p = in0, t = in1 with d = p - t and, with a climatology, pa = p - c and
 * ta = t - c.  The anomaly planes are there iff the climatology is: an ERROR update has
 * MSFNO_TSTATS_ANOM set iff clim is given.  A fresh state is count 0, planes 0, lo = +inf,
 * hi = -inf.
 *   Update folds a batch into one state.  in0, in1 are (B, S, P), batch element b at
 *   in + b * batch_stride (in floats, any value: need not be a multiple of 4); clim is a
 *   stack of (P) slabs and clim_slab a device int32[B * S], the slab of (b, s), every entry
 *   >= 0 (the caller's contract; not range-checked), or both NULL.  Per pixel the B updates
 *   are applied in the order b = 0 .. B - 1, in fp32 with a true division:
 *     n += 1
 *     delta = a - mean;  mean += delta / (float)n;  m2 = fma(delta, a - mean, m2)  (new mean)
 *     mean_abs += (|d| - mean_abs) / n
 *     c_pt = fma(pa - mean_pa_old, ta - mean_ta_new, c_pt)
 *     lo = fminf(lo, a);  hi = fmaxf(hi, a)
 *   so a call of B elements leaves the bits of B calls of one.  Every quantity is formed
 *   from a difference, never from raw sums of squares.  With skip_nan != 0 an update
 *   (b, s, i) is selected out, never multiplied by zero, where x or c is NaN (FIELD) or t or
 *   c is NaN (ERROR; a NaN in p is never skipped, as in msfno_verify_region_sums): all of that
 *   pixel's words keep their bits.  Without skip_nan a NaN poisons the moment planes of that
 *   pixel and of no other (fminf and fmaxf pass it over: lo and hi stay numbers).
 *   Traffic is B times the inputs plus one read and one write of the state.
 *   Merge is dst <- dst (+) src over N = S * P elements, states of one kind and flags:
 *     n = na + nb;  delta = mean_b - mean_a;  f = nb / n
 *     mean = fma(delta, f, mean_a);  m2 = fma(delta^2, na f, m2_a + m2_b)
 *     c_pt = fma(delta_pa delta_ta, na f, c_pt_a + c_pt_b);  mean_abs as mean;  lo by
 *     fminf, hi by fmaxf
 *   where nb == 0 dst keeps its bits and where na == 0 it takes src's.  It combines the
 *   accumulators of processes or devices, and neighbouring climatology bins into a window.
 *   dst and src must not overlap.
 * No atomics and no workspace: results are bitwise reproducible and do not depend on the
 * alignment of any buffer or on the launch geometry.  Nothing allocates, synchronises or
 * memsets and the running count lives on the device, so both calls record into a graph and
 * replay.  All three return MSFNO_EINVAL (msfno_last_error names the argument), before any
 * launch, for a null required pointer, an extent below 1, an unknown kind or flag
 * (MSFNO_TSTATS_MINMAX on ERROR, MSFNO_TSTATS_ANOM on FIELD), in1 missing for ERROR or given
 * for FIELD, only one of clim / clim_slab, MSFNO_TSTATS_ANOM that disagrees with clim on an
 * ERROR update, or a plane stride below S * P (N for the merge).  No K equals MSFNO_EINVAL.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
#define MSFNO_TSTATS_FIELD 0
#define MSFNO_TSTATS_ERROR 1
#define MSFNO_TSTATS_MINMAX 1 /* flag of FIELD */
#define MSFNO_TSTATS_ANOM 2   /* flag of ERROR */
int msfno_tstats_planes(int kind, int flags);
int msfno_tstats_update(int kind, int flags, const float* in0, const float* in1 /* or NULL */,
                        long long batch_stride0, long long batch_stride1,
                        const float* clim /* or NULL */, const int* clim_slab /* or NULL */,
                        int B, int S, long long P, int skip_nan, uint32_t* count /* (S, P) */,
                        float* state /* (K, S, P) */, long long plane_stride, void* stream);
int msfno_tstats_merge(int kind, int flags, uint32_t* dst_count, float* dst_state,
                       long long dst_plane_stride, const uint32_t* src_count,
                       const float* src_state, long long src_plane_stride, long long N,
                       void* stream);

/* ---------------------------------------------------------------------------
 * Graph-convolution FiLM generator (MSFNO/Models/gcn/gcn.py:96-167 GCN_custom,
 * layers.py:8-43 GraphConvolution; the Python mirror is msfno_amd/filmgen.py): the network
 * that turns the ocean points of an SST field into the FiLM vector, and its backward.  Per
 * sample b, all fp32, with leaky the LeakyReLU of slope 0.01 and A any real N x N sparse
 * matrix (unsymmetric, unnormalised, empty rows allowed):
 *   h_1     = leaky(A (x0 W0) + b0)                       x0 (B, N, Fin), W0 (Fin, hidden)
 *   h_{l+1} = h_l + leaky(A (h_l W_l) + b_l), l = 1..depth   W_l (hidden, hidden), input-major
 *   y       = mean_nodes(h_last) Wh^T + bh                Wh (out, hidden), y (B, out)
 * the per-sample math the reference states in layers.py:37-39 (its executed code takes
 * sample 0 only and runs at depth 0 only).  A is CSR with values on the device (row_ptr
 * N + 1 int32, col and val nnz, every col in [0, N): the caller's contract, it is not
 * checked); t_* is the CSR of A^T, needed by msfno_gcn_backward only.  The K = hidden
 * products run on the split-precision MFMA engine, the conv1 layer as (A x0) W0.
 *   msfno_gcn_forward: y from x0.  With train != 0 it keeps every layer's input and
 *     pre-activation in the workspace, and msfno_gcn_backward on the same, untouched
 *     workspace (sized with train = 1, same B, graph and descriptor) gives the gradients
 *     of L for dy = dL/dy (B, out): every tensor of grads, and dx0 (B, N, Fin) unless NULL.
 * No atomics: every sum has a fixed order (a row's neighbours in CSR order; column sums
 * per lane, per workgroup, then in fp64 over the chunks), so results are bitwise
 * reproducible.  Every word of y, of every gradient and of dx0 is written by every call;
 * the workspace may hold anything on entry to the forward; nothing allocates, synchronises
 * or memsets, so the calls record into a graph.  MSFNO_EINVAL for null required pointers,
 * an extent below 1, parameters or a workspace off the 16-byte grid; MSFNO_EUNSUPPORTED for
 * hidden % 4 != 0, Fin > 16, depth > MSFNO_GCN_MAX_DEPTH or B * N > 2^21;
 * MSFNO_EWORKSPACE for a short workspace; all before any launch.
 * msfno_gcn_workspace_size returns 0 for sizes the calls refuse.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
#define MSFNO_GCN_MAX_DEPTH 16
typedef struct msfno_gcn_graph {
  int N;
  long long nnz;
  const int* row_ptr;
  const int* col;
  const float* val;
  const int* t_row_ptr; /* A^T; all three may be NULL for forward-only use */
  const int* t_col;
  const float* t_val;
} msfno_gcn_graph;
typedef struct msfno_gcn_desc {
  int Fin, hidden, depth, out;
  const float* conv1_w; /* (Fin, hidden) */
  const float* conv1_b; /* (hidden) */
  const float* conv_w[MSFNO_GCN_MAX_DEPTH]; /* (hidden, hidden) each */
  const float* conv_b[MSFNO_GCN_MAX_DEPTH];
  const float* head_w; /* (out, hidden) */
  const float* head_b; /* (out) */
} msfno_gcn_desc;
typedef struct msfno_gcn_grads { /* shapes as in msfno_gcn_desc; all required */
  float* conv1_w;
  float* conv1_b;
  float* conv_w[MSFNO_GCN_MAX_DEPTH];
  float* conv_b[MSFNO_GCN_MAX_DEPTH];
  float* head_w;
  float* head_b;
} msfno_gcn_grads;
size_t msfno_gcn_workspace_size(int B, int N, int Fin, int hidden, int depth, int out, int train);
int msfno_gcn_forward(const msfno_gcn_graph* g, const msfno_gcn_desc* d, const float* x0,
                      float* y /* (B, out) */, int B, int train, void* ws, size_t ws_bytes,
                      void* stream);
int msfno_gcn_backward(const msfno_gcn_graph* g, const msfno_gcn_desc* d, const float* dy,
                       const msfno_gcn_grads* grads, float* dx0 /* (B, N, Fin) or NULL */, int B,
                       void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Per-degree power spectrum of spherical-harmonic coefficients and its gradient: the
 * middle step of the reference's spectral losses (MSFNO/Models/losses.py:158-232,
 * spectral_l2loss_sphere, spectral_loss_sphere, h1loss_sphere; the Python mirror is
 * msfno_amd/losses.py) and a per-degree diagnostic of a rollout.  The weight 2 applies to
 * every m >= 1 (Nyquist included) and all m of a row are read: coeffs is any complex
 * tensor, not only a transform's output.  No workspace, no atomics: the result is bitwise
 * reproducible.  MSFNO_EINVAL for null pointers, an extent below 1, or coefficient
 * pointers off the 8-byte grid of a complex tensor.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
/* power[n][l] = |c[n][l][0]|^2 + 2 * sum_{m>=1} |c[n][l][m]|^2
 * coeffs (N, lmax, mmax) complex64 interleaved, power (N, lmax) fp32 */
int msfno_spectrum_power(const float* coeffs, float* power, long long N, int lmax, int mmax,
                         void* stream);
/* dcoeffs[n][l][m] = (2 e_m gpower[n][l]) * coeffs[n][l][m], e_0 = 1, e_m = 2 (m >= 1) */
int msfno_spectrum_power_backward(const float* coeffs, const float* gpower, float* dcoeffs,
                                  long long N, int lmax, int mmax, void* stream);

/* ---------------------------------------------------------------------------
 * Spherical Gaussian random fields: spectral coefficients of white or red-in-time (AR(1))
 * noise in the layout msfno_sht_inverse reads (the Python side is
 * msfno_amd/harmonics/random_fields.py).  The stream is a pure function of (seed, draw,
 * global field index, l, m) ("Spherical Gaussian random fields"): Philox4x32-10
 * with key (seed lo, seed hi) and counter (l * ceil(mmax / 2) + m / 2, field, draw lo,
 * draw hi), Box-Muller on u = ((w >> 9) + 0.5) * 2^-23; xi = (z0, 0) for m = 0,
 * (z0, z1) / sqrt(2) for 1 <= m <= l and exactly (0, 0) for m > l, where the output is
 * zero whatever prev holds.  Independent of the launch geometry and of how fields are
 * split over calls.  Neither call allocates or synchronises: both record into a graph.
 * MSFNO_EINVAL for null coeffs or sqrt_eig, coefficient pointers off the 8-byte grid,
 * an extent below 1, K < 1, lmax * ceil(mmax / 2) >= 2^32 or field0 + n > 2^32.
 * Added under ABI version 6: additions only, nothing existing changed.
 * ------------------------------------------------------------------------- */
/* coeffs (n, lmax, mmax) complex64 interleaved: the layout msfno_sht_inverse reads.
 * sqrt_eig (K, lmax) fp32; local field i uses row (field0 + i) % K.
 * out = a * prev + b * sqrt_eig[l] * xi(seed, draw, field0 + i, l, m)
 * prev: NULL (then a is ignored) or (n, lmax, mmax) complex64; prev == coeffs is allowed
 * (in place).  draw: the host value when draw_dev == NULL; otherwise the kernel reads
 * *draw_dev (device uint64). */
int msfno_noise_spectral(float* coeffs, const float* prev, const float* sqrt_eig, int K,
                         long long n, long long field0, int lmax, int mmax, float a, float b,
                         unsigned long long seed, unsigned long long draw,
                         const unsigned long long* draw_dev, void* stream);
/* *draw_dev += by, by one lane of one workgroup */
int msfno_noise_advance(unsigned long long* draw_dev, unsigned long long by, void* stream);

/* ---------------------------------------------------------------------------
 * Latitude-band sharded SFNO-Block (multi-GPU form of
 * msfno_block_forward).  The reference runs one block per process on the whole
 * field (DDP = replicas, MSFNO/main.py:1153); this splits ONE field batch over
 * `world` ranks.  row_start (world + 1 entries) partitions the northern half of
 * the grid, rows [0, nlat - nlat/2) (the equator row of an odd grid included):
 * rank r owns the band [row_start[r], row_start[r+1]) and the mirror rows
 * nlat-1-k of its band rows k < nlat/2, for every pointwise / FFT / 1x1-conv /
 * MLP stage (msfno_band_local_rows lists them: the band ascending, then the
 * mirrors ascending), and the zonal wavenumbers {m : m_owner[m] == r} for the
 * Legendre transforms and the spectral filter.  Owning mirror pairs keeps the
 * hemisphere fold of the symmetric Legendre transform local, and the exchange
 * buffers are the Legendre GEMMs' own operands (no re-layout pass).
 * The caller (Python, torch.distributed over RCCL) performs the collectives
 * between the stages; the library never communicates:
 *
 *   stage 0  x_local -> inner-skip GEMM (side stream), FFT rows    -> stats_local
 *   [all_gather stats_local -> stats_all]              (norm0, B*C*3 doubles)
 *   stage 1  norm0 affine, pack spectra by owner of m     -> send
 *   [all_to_all send -> recv, counts from msfno_band_exchange_counts(phase 0)]
 *   stage 2  recv -> Legendre fwd -> filter -> Legendre inv -> send
 *   [all_to_all send -> recv, phase 1]
 *   stage 3  recv -> inverse FFT rows + skip (+GELU)       -> stats_local
 *   [all_gather stats_local -> stats_all]              (norm1)
 *   stage 4  norm1 (+FiLM) -> MLP (+outer skip)            -> out_local
 *
 * Resampling blocks (different input and output grids, sfnonet.py:573-614: the
 * first block 721x1440 -> 120x240 and the last one back) take a second row
 * partition for the output grid (msfno_band_plan_create2); skips then must be
 * absent, as in the reference.  Both filters: the linear filter's per-mode
 * weight is sharded with the m-set (msfno_band_linear_modes), so each rank
 * streams only its modes' slice.  At most 64 ranks.
 *
 * Several sub-batches of one forward may be in flight between stage 0 and
 * stage 3 at once (their exchanges overlapping each other's compute): give each
 * a distinct io.slot (0..63), its own workspace and its own exchange buffers.
 * ------------------------------------------------------------------------- */
typedef struct msfno_band_plan_s* msfno_band_plan_t;

/* Default partition (host only, no GPU): balanced bands of the northern half and
 * a zig-zag (snake) assignment of m = 0..mact-1 that balances both the count of
 * m and the Legendre/filter work sum(lmax - m) per rank; m >= lmax -> -1. */
int msfno_band_partition(int world, int nlat, int lmax, int mmax, int* row_start, int* m_owner);
/* all-to-all element counts (floats) per peer for `rank` (host only):
 * phase 0 (spectra rows->m), phase 1 (m->rows); R = 2*B*C.  Every exchanged slab
 * row holds 2W floats, W = the widest band rounded up to 16. */
int msfno_band_exchange_counts(int world, int rank, int nlat, int mmax, const int* row_start,
                               const int* m_owner, int R, int phase, long long* send_counts,
                               long long* recv_counts);
/* The global latitude rows of `rank`'s local rows, in local order (rows may be
 * NULL to query *count = band rows + mirror rows). */
int msfno_band_local_rows(int world, int rank, int nlat, const int* row_start, int* rows,
                          int* count);
int msfno_band_plan_create(int nlat, int nlon, int lmax, int mmax, int world, int rank,
                           const int* row_start, const int* m_owner, msfno_band_plan_t* plan);
/* Resampling form: rows of the input grid (nlat_in x nlon_in, the forward
 * transform's) in row_in, of the output grid (the inverse transform's) in row_out. */
int msfno_band_plan_create2(int nlat_in, int nlon_in, int nlat_out, int nlon_out, int lmax,
                            int mmax, int world, int rank, const int* row_in, const int* row_out,
                            const int* m_owner, msfno_band_plan_t* plan);
/* all-to-all counts (floats per peer) of this plan's rank, phase 0 / 1, R = 2*B*C */
int msfno_band_plan_exchange_counts(msfno_band_plan_t plan, int R, int phase,
                                    long long* send_counts, long long* recv_counts);
/* Linear filter (SpectralConvS2, layers.py:336-427): the global tril indices
 * (torch.tril_indices(lmax, mmax) order, layers.py:368) of this rank's modes, in
 * ascending order; *count = their number T_r (modes may be NULL to query it).
 * The descriptor's lin_w for msfno_band_block_stage is then w[:, :, modes, :],
 * i.e. (C, C, T_r, 2) — the rank's share of the 34 GB weight at lmax 360. */
int msfno_band_linear_modes(msfno_band_plan_t plan, long long* modes, long long* count);
int msfno_band_plan_destroy(msfno_band_plan_t plan);
/* full reference tables (mmax,lmax,nlat) fp32 device buffers (RealSHT.weights,
 * InverseRealSHT.pct incl. the 1e5 rescale); only this rank's m-set is kept */
int msfno_band_plan_load_tables(msfno_band_plan_t plan, const float* fwd_table,
                                const float* inv_table, void* stream);

typedef struct msfno_band_io {
  const float* x;           /* (B, C, rows_local, nlon), msfno_band_local_rows  */
  const float* gamma;       /* (B, C) or NULL                                   */
  const float* beta;        /* (B, C) or NULL                                   */
  float film_scale;
  float* out;               /* (B, C, rows_local, nlon)                         */
  float* send;              /* exchange buffers, >= max over phases of the sum  */
  float* recv;              /*   of the send / recv counts (floats)             */
  double* stats_local;      /* (B*C, 3) {n, mean, M2}                           */
  const double* stats_all;  /* (world, B*C, 3), the all_gather of stats_local   */
  int slot;                 /* in-flight sub-batch index 0..63 (inner-skip join) */
} msfno_band_io;

size_t msfno_band_workspace_size(const msfno_block_desc* d, msfno_band_plan_t plan, int B);
/* Run one stage (0..4) on `stream`.  ws must be the same buffer for all five
 * stages of one forward. */
int msfno_band_block_stage(const msfno_block_desc* d, msfno_band_plan_t plan, int stage,
                           const msfno_band_io* io, int B, void* ws, size_t ws_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------
 * Instrumentation (not a reference interface): per-stage device time of the
 * fused block measured with hipEvents recorded on the caller's stream between
 * stages.  Used by bench.py to time the dominant kernel inside the timed region.
 * ------------------------------------------------------------------------- */
#define MSFNO_PROF_NSTAGES 32
int msfno_profile_enable(int on);
/* mark the start of `stage` on `stream` (bench: the wait on a collective) */
int msfno_profile_mark(int stage, void* stream);
/* synchronises on the recorded events, adds per-stage milliseconds / launch
 * counts since the last collect into total_ms[stage] / counts[stage] (arrays of
 * MSFNO_PROF_NSTAGES), and clears the recorded marks */
int msfno_profile_collect(double* total_ms, int* counts);
const char* msfno_profile_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* MSFNO_H */
