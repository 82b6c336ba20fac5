// Complex channel contraction of the non-linear spectral filter with the
// 3-multiplication (Gauss / "3M") scheme on fp32 MFMA:
//
//   y[o] = sum_i x[i] * w[i][o]          (compl_mul2d_fwd_c, contractions.py:132-137)
//   P1 = Wr.Xr,  P2 = Wi.Xi,  P3 = (Wr+Wi).(Xr+Xi)
//   Re y = P1 - P2,   Im y = P3 - P1 - P2  (then ComplexReLU(real) on Re y, activations.py:42-46)
//
// Three real products per complex one instead of the four of the real-ified
// [[Wr,-Wi],[Wi,Wr]] GEMM: 25 % fewer MFMAs for the 409 GFLOP spectral MLP.
// The sums Wr+Wi and Xr+Xi are formed from the staged fragments just before the
// MFMAs (one add per fragment), so LDS holds only the four real planes.
// Operands in the S layout: X rows [b][re|im][ci] x N columns (ld ldx), Y rows
// [b][re|im][co] (ld ldy); Ar/Ai are (co x ci) row-major: Ar[o][i] = Re w[i][o].
#include "kernels.h"

namespace msfno {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct C3MParams {
  const float* Ar;
  const float* Ai;
  const float* X;
  float* Y;
  int co, ci, N, ldx, ldy;
  int64_t sX, sY;  // batch strides
  int tiles_m, tiles_n;
  int relu;
};

__device__ __forceinline__ int xcd_remap_c(int orig, int nwg) {
  const int xcd = orig & 7;
  const int q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

template <int BM, int BN, bool RELU>
__global__ __launch_bounds__(256) void gemm_c3m_kernel(C3MParams p) {
  constexpr int BK = 16;
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int MT = WM / 32, NT = WN / 32;
  constexpr int LDA = BM + 2;  // k-major A staging (conflict-free transposed writes)
  constexpr int A_LD = BM * BK / 1024, B_LD = BN * BK / 1024;
  constexpr int SA = BK * LDA, SB = BK * BN;
  // [buf][plane] A tiles, then [buf][plane] B tiles
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * SA + 2 * 2 * SB];
  auto As = [&](int buf, int pl) { return lds + (buf * 2 + pl) * SA; };
  auto Bs = [&](int buf, int pl) { return lds + 4 * SA + (buf * 2 + pl) * SB; };

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5, l32 = lane & 31;
  const int lin = xcd_remap_c(blockIdx.x, gridDim.x);
  const int tm = lin % p.tiles_m, tn = lin / p.tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const int M = p.co, K = p.ci, N = p.N;
  const float* Xr = p.X + blockIdx.z * p.sX;
  const float* Xi = Xr + (int64_t)K * p.ldx;
  float* Yr = p.Y + blockIdx.z * p.sY;
  float* Yi = Yr + (int64_t)M * p.ldy;
  const int Mc = M - 1, Kc = K - 1, Nc = N - 1;

  float4 ra[2][A_LD], rb[2][B_LD];
  auto load = [&](int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int q = 0; q < A_LD; ++q) {
      const int idx = tid + 256 * q;
      const int row = min(m0 + idx / (BK / 4), Mc);
      const int k = min(k0 + (idx % (BK / 4)) * 4, Kc & ~3);
      ra[0][q] = *reinterpret_cast<const float4*>(p.Ar + (int64_t)row * K + k);
      ra[1][q] = *reinterpret_cast<const float4*>(p.Ai + (int64_t)row * K + k);
    }
#pragma unroll
    for (int q = 0; q < B_LD; ++q) {
      const int idx = tid + 256 * q;
      const int kr = min(k0 + idx / (BN / 4), Kc);
      const int col = min(n0 + (idx % (BN / 4)) * 4, Nc & ~3);
      rb[0][q] = *reinterpret_cast<const float4*>(Xr + (int64_t)kr * p.ldx + col);
      rb[1][q] = *reinterpret_cast<const float4*>(Xi + (int64_t)kr * p.ldx + col);
    }
  };
  auto store = [&](int buf, int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
      for (int q = 0; q < A_LD; ++q) {
        const int idx = tid + 256 * q;
        const int row = idx / (BK / 4), k = (idx % (BK / 4)) * 4;
        const bool rok = m0 + row < M;
        const int kg = k0 + k;
        float* d = As(buf, pl) + k * LDA + row;
        d[0] = (rok && kg + 0 < K) ? ra[pl][q].x : 0.f;
        d[LDA] = (rok && kg + 1 < K) ? ra[pl][q].y : 0.f;
        d[2 * LDA] = (rok && kg + 2 < K) ? ra[pl][q].z : 0.f;
        d[3 * LDA] = (rok && kg + 3 < K) ? ra[pl][q].w : 0.f;
      }
#pragma unroll
      for (int q = 0; q < B_LD; ++q) {
        const int idx = tid + 256 * q;
        const int kr = idx / (BN / 4), col = (idx % (BN / 4)) * 4;
        const bool kok = k0 + kr < K;
        const int cg = n0 + col;
        float4 v = rb[pl][q];
        v.x = (kok && cg + 0 < N) ? v.x : 0.f;
        v.y = (kok && cg + 1 < N) ? v.y : 0.f;
        v.z = (kok && cg + 2 < N) ? v.z : 0.f;
        v.w = (kok && cg + 3 < N) ? v.w : 0.f;
        *reinterpret_cast<float4*>(Bs(buf, pl) + kr * BN + col) = v;
      }
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

  const int nk = (K + BK - 1) / BK;
  if (nk > 0) {
    load(0);
    store(0, 0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
    const float* ar_s = As(cur, 0);
    const float* ai_s = As(cur, 1);
    const float* br_s = Bs(cur, 0);
    const float* bi_s = Bs(cur, 1);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const int k = 2 * kk + half;
      float ar[MT], ai[MT], as[MT], br[NT], bi[NT], bsum[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        ar[i] = ar_s[k * LDA + wm * WM + i * 32 + l32];
        ai[i] = ai_s[k * LDA + wm * WM + i * 32 + l32];
        as[i] = ar[i] + ai[i];
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        br[j] = br_s[k * BN + wn * WN + j * 32 + l32];
        bi[j] = bi_s[k * BN + wn * WN + j * 32 + l32];
        bsum[j] = br[j] + bi[j];
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[0][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[i], br[j], acc[0][i][j], 0, 0, 0);
          acc[1][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[i], bi[j], acc[1][i][j], 0, 0, 0);
          acc[2][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(as[i], bsum[j], acc[2][i][j], 0, 0, 0);
        }
    }
    if (kt + 1 < nk) store(cur ^ 1, kt + 1);
    __syncthreads();
  }

  // epilogue: Re = P1 - P2 (ReLU for hidden layers), Im = P3 - P1 - P2
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * WN + j * 32 + l32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float p1 = acc[0][i][j][r], p2 = acc[1][i][j][r], p3 = acc[2][i][j][r];
        float re = p1 - p2;
        const float im = p3 - p1 - p2;
        if (RELU) re = fmaxf(re, 0.f);
        if (row < M && col < N) {
          Yr[(int64_t)row * p.ldy + col] = re;
          Yi[(int64_t)row * p.ldy + col] = im;
        }
      }
    }
}

__global__ void split_complex_weight_kernel(const float* __restrict__ w, float* __restrict__ Ar,
                                            float* __restrict__ Ai, int Ci, int Co) {
  const int64_t n = (int64_t)Ci * Co;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(e / Ci), i = (int)(e - (int64_t)o * Ci);
    Ar[e] = w[((int64_t)i * Co + o) * 2 + 0];
    Ai[e] = w[((int64_t)i * Co + o) * 2 + 1];
  }
}

int launch_split_complex_weight(const float* w, float* Ar, float* Ai, int Ci, int Co,
                                hipStream_t s) {
  const int64_t n = (int64_t)Ci * Co;
  hipLaunchKernelGGL(split_complex_weight_kernel,
                     dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, s, w,
                     Ar, Ai, Ci, Co);
  return launch_check("split_complex_weight");
}

int gemm_c3m(const float* Ar, const float* Ai, const float* X, float* Y, int co, int ci, int N,
             int ldx, int ldy, int64_t sX, int64_t sY, int B, bool relu, hipStream_t s) {
  if (co <= 0 || N <= 0 || B <= 0) return MSFNO_OK;
  MSFNO_REQUIRE(ci % 4 == 0 && ldx % 4 == 0 && N % 4 == 0, MSFNO_EUNSUPPORTED,
                "3M spectral GEMM needs ci, ldx and N multiples of 4");
  MSFNO_REQUIRE(B <= 65535, MSFNO_EINVAL, "gemm_c3m: batch too large");
  constexpr int BM = 64, BN = 128;  // measured best of 128x64, 64x128, 128x128 (in-block A/B)
  C3MParams p{};
  p.Ar = Ar; p.Ai = Ai; p.X = X; p.Y = Y;
  p.co = co; p.ci = ci; p.N = N; p.ldx = ldx; p.ldy = ldy; p.sX = sX; p.sY = sY;
  p.tiles_m = (int)cdiv(p.co, BM);
  p.tiles_n = (int)cdiv(p.N, BN);
  dim3 grid((unsigned)(p.tiles_m * p.tiles_n), 1, (unsigned)B);
  if (relu)
    hipLaunchKernelGGL((gemm_c3m_kernel<BM, BN, true>), grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL((gemm_c3m_kernel<BM, BN, false>), grid, dim3(256), 0, s, p);
  return launch_check("gemm_c3m");
}

}  // namespace msfno
