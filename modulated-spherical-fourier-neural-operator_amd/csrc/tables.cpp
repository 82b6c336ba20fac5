// Host-side fp64 plan math: quadrature nodes and weights, the Legendre tables of the
// scalar and the vector transforms, and their C entry points.  No device code and no HIP
// runtime: this unit builds with a plain host compiler (tools/tables_check.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "error.h"

namespace msfno {

// ---------------------------------------------------------------------------
// host-side fp64 plan math ([TH] torch_harmonics.quadrature / .legendre)
// ---------------------------------------------------------------------------
static void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& w) {
  x.assign(n, 0.0);
  w.assign(n, 0.0);
  for (int i = 0; i < n; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5));
    double pp = 0.0;
    for (int it = 0; it < 100; ++it) {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 1; j <= n; ++j) {
        const double p3 = p2;
        p2 = p1;
        p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
      }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      const double z1 = z;
      z = z1 - p1 / pp;
      if (std::fabs(z - z1) < 1e-16) break;
    }
    // recompute derivative at the converged root
    double p1 = 1.0, p2 = 0.0;
    for (int j = 1; j <= n; ++j) {
      const double p3 = p2;
      p2 = p1;
      p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
    }
    pp = n * (z * p1 - p2) / (z * z - 1.0);
    x[n - 1 - i] = z;  // ascending
    w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
  }
}

static void clenshaw_curtis(int n, std::vector<double>& x, std::vector<double>& w) {
  x.assign(n, 0.0);
  w.assign(n, 0.0);
  if (n == 2) {
    x[0] = -1.0; x[1] = 1.0;
    w[0] = w[1] = 1.0;
    return;
  }
  const int N = n - 1;
  for (int j = 0; j < n; ++j) {
    const double th = M_PI - (double)j * M_PI / N;  // cos(linspace(pi, 0, n))
    x[j] = std::cos(th);
    const double tj = (double)j * M_PI / N;
    double s = 0.0;
    for (int k = 1; k <= N / 2; ++k) {
      const double bk = (2 * k == N) ? 1.0 : 2.0;
      s += bk / (4.0 * k * k - 1.0) * std::cos(2.0 * k * tj);
    }
    const double cj = (j == 0 || j == N) ? 1.0 : 2.0;
    w[j] = cj / N * (1.0 - s);
  }
}

static int quadrature(int nlat, int grid, std::vector<double>& x, std::vector<double>& w) {
  if (grid == MSFNO_GRID_LEGENDRE_GAUSS) {
    MSFNO_REQUIRE(nlat >= 1, MSFNO_EINVAL, "nlat must be >= 1");
    gauss_legendre(nlat, x, w);
  } else if (grid == MSFNO_GRID_EQUIANGULAR) {
    MSFNO_REQUIRE(nlat >= 2, MSFNO_EINVAL, "equiangular grid needs nlat >= 2");
    clenshaw_curtis(nlat, x, w);
  } else {
    set_error("Unknown quadrature mode");
    return MSFNO_EUNSUPPORTED;
  }
  return MSFNO_OK;
}

// (-1)^m c_l^m P_l^m at cos(theta_k), same recurrence and operation order as [TH] legpoly
static int legendre_table(int mmax, int lmax, int nlat, int grid, int inverse, int csphase,
                          double* out) {
  std::vector<double> x, w;
  MSFNO_TRY(quadrature(nlat, grid, x, w));
  const int nmax = std::max(mmax, lmax);
  // k-independent recurrence coefficients (same expressions as [TH] legpoly)
  std::vector<double> ca((size_t)nmax * nmax, 0.0), cb((size_t)nmax * nmax, 0.0);
  for (int l = 2; l < nmax; ++l)
    for (int m = 0; m < l - 1; ++m) {
      ca[(size_t)m * nmax + l] = std::sqrt((2.0 * l - 1) / (l - m) * (2.0 * l + 1) / (l + m));
      cb[(size_t)m * nmax + l] = std::sqrt((double)(l + m - 1) / (l - m) * (2.0 * l + 1) /
                                           (2.0 * l - 3) * (l - m - 1) / (l + m));
    }
  std::vector<double> vdm((size_t)nmax * nmax);
  for (int k = 0; k < nlat; ++k) {
    // theta = flip(arccos(nodes)): colatitude index k uses node nlat-1-k
    const double xk = std::cos(std::acos(x[nlat - 1 - k]));
    std::fill(vdm.begin(), vdm.end(), 0.0);
    auto V = [&](int m, int l) -> double& { return vdm[(size_t)m * nmax + l]; };
    V(0, 0) = 1.0 / std::sqrt(4.0 * M_PI);  // ortho norm; inverse factor is 1 as well
    for (int l = 1; l < nmax; ++l) {
      V(l - 1, l) = std::sqrt(2.0 * l + 1) * xk * V(l - 1, l - 1);
      V(l, l) = std::sqrt((2.0 * l + 1) * (1 + xk) * (1 - xk) / 2.0 / l) * V(l - 1, l - 1);
    }
    for (int m = 0; m < nmax; ++m) {
      const double* a = &ca[(size_t)m * nmax];
      const double* b = &cb[(size_t)m * nmax];
      double* v = &vdm[(size_t)m * nmax];
      for (int l = m + 2; l < nmax; ++l) v[l] = xk * a[l] * v[l - 1] - b[l] * v[l - 2];
    }
    const double wk = inverse ? 1.0 : w[k];  // weights are symmetric (unflipped in [TH])
    for (int m = 0; m < mmax; ++m) {
      const double sgn = (csphase && (m & 1)) ? -1.0 : 1.0;
      for (int l = 0; l < lmax; ++l)
        out[((size_t)m * lmax + l) * nlat + k] = sgn * V(m, l) * wk;
    }
  }
  return MSFNO_OK;
}

// The vector transform's tables D = dP̄_l^m/dθ and Q = m P̄_l^m / sin θ (out: (2, mmax,
// lmax, nlat)), from the recurrence of legendre_table run one order further.  With the
// Condon-Shortley phase in P̄ (p below) and l >= m:
//   D_l^m = -1/2 [ sqrt((l+m)(l-m+1)) P̄_l^{m-1} - sqrt((l-m)(l+m+1)) P̄_l^{m+1} ]   (m >= 1)
//   D_l^0 = sqrt(l(l+1)) P̄_l^1
//   Q_l^m = -1/2 sqrt((2l+1)/(2l-1)) [ sqrt((l-m)(l-m-1)) P̄_{l-1}^{m+1}
//                                     + sqrt((l+m)(l+m-1)) P̄_{l-1}^{m-1} ]       (m >= 1)
// Nothing divides by sin θ: at a pole x = ±1 exactly, every P̄ of order >= 1 is an exact
// zero, so only m = 1 survives there (through the order-0 terms) and D = Q.  Without the
// phase both tables carry (-1)^m, as P̄ does.  inverse == 0: times w_k / (l(l+1)), the
// l = 0 row zero.
static int vector_legendre_table(int mmax, int lmax, int nlat, int grid, int inverse, int csphase,
                                 double* out) {
  std::vector<double> x, w;
  MSFNO_TRY(quadrature(nlat, grid, x, w));
  const int nmax = std::max(mmax + 1, lmax) + 1;  // orders <= mmax, degrees < lmax
  std::vector<double> ca((size_t)nmax * nmax, 0.0), cb((size_t)nmax * nmax, 0.0);
  for (int l = 2; l < nmax; ++l)
    for (int m = 0; m < l - 1; ++m) {
      ca[(size_t)m * nmax + l] = std::sqrt((2.0 * l - 1) / (l - m) * (2.0 * l + 1) / (l + m));
      cb[(size_t)m * nmax + l] = std::sqrt((double)(l + m - 1) / (l - m) * (2.0 * l + 1) /
                                           (2.0 * l - 3) * (l - m - 1) / (l + m));
    }
  std::vector<double> vdm((size_t)nmax * nmax);
  const size_t plane = (size_t)mmax * lmax * nlat;
  for (int k = 0; k < nlat; ++k) {
    const double xk = std::cos(std::acos(x[nlat - 1 - k]));
    std::fill(vdm.begin(), vdm.end(), 0.0);
    auto V = [&](int m, int l) -> double& { return vdm[(size_t)m * nmax + l]; };
    V(0, 0) = 1.0 / std::sqrt(4.0 * M_PI);
    for (int l = 1; l < nmax; ++l) {
      V(l - 1, l) = std::sqrt(2.0 * l + 1) * xk * V(l - 1, l - 1);
      V(l, l) = std::sqrt((2.0 * l + 1) * (1 + xk) * (1 - xk) / 2.0 / l) * V(l - 1, l - 1);
    }
    for (int m = 0; m < nmax; ++m) {
      const double* a = &ca[(size_t)m * nmax];
      const double* b = &cb[(size_t)m * nmax];
      double* v = &vdm[(size_t)m * nmax];
      for (int l = m + 2; l < nmax; ++l) v[l] = xk * a[l] * v[l - 1] - b[l] * v[l - 2];
    }
    // p(m, l): P̄_l^m with the Condon-Shortley phase (0 for l < m)
    auto p = [&](int m, int l) { return (m & 1) ? -V(m, l) : V(m, l); };
    for (int m = 0; m < mmax; ++m) {
      const double sgn = (!csphase && (m & 1)) ? -1.0 : 1.0;
      for (int l = 0; l < lmax; ++l) {
        double d = 0.0, q = 0.0;
        if (l >= m && l >= 1) {
          const double dl = l, dm = m;
          if (m == 0) {
            d = std::sqrt(dl * (dl + 1)) * p(1, l);
          } else {
            d = -0.5 * (std::sqrt((dl + dm) * (dl - dm + 1)) * p(m - 1, l) -
                        std::sqrt((dl - dm) * (dl + dm + 1)) * p(m + 1, l));
            q = -0.5 * std::sqrt((2 * dl + 1) / (2 * dl - 1)) *
                (std::sqrt((dl - dm) * (dl - dm - 1)) * p(m + 1, l - 1) +
                 std::sqrt((dl + dm) * (dl + dm - 1)) * p(m - 1, l - 1));
          }
          const double f = sgn * (inverse ? 1.0 : w[k] / (dl * (dl + 1)));
          d *= f;
          q *= f;
        }
        const size_t at = ((size_t)m * lmax + l) * nlat + k;
        out[at] = d;
        out[plane + at] = q;
      }
    }
  }
  return MSFNO_OK;
}

}  // namespace msfno

using namespace msfno;

extern "C" {

int msfno_quadrature(int nlat, int grid, double* nodes, double* weights) {
  std::vector<double> x, w;
  MSFNO_TRY(quadrature(nlat, grid, x, w));
  std::memcpy(nodes, x.data(), nlat * sizeof(double));
  std::memcpy(weights, w.data(), nlat * sizeof(double));
  return MSFNO_OK;
}

int msfno_legendre_table(int mmax, int lmax, int nlat, int grid, int inverse, int csphase,
                         double* table) {
  MSFNO_REQUIRE(mmax > 0 && lmax > 0 && nlat > 0 && table, MSFNO_EINVAL, "bad table arguments");
  return legendre_table(mmax, lmax, nlat, grid, inverse, csphase, table);
}

int msfno_vector_legendre_table(int mmax, int lmax, int nlat, int grid, int inverse, int csphase,
                                double* table) {
  MSFNO_REQUIRE(mmax > 0 && lmax > 0 && nlat > 0 && table, MSFNO_EINVAL, "bad table arguments");
  return vector_legendre_table(mmax, lmax, nlat, grid, inverse, csphase, table);
}

}  // extern "C"
