// Host check of csrc/tables.cpp (the fp64 quadrature and Legendre-table math): built from
// this file and tables.cpp alone by the plain host compiler with
// -fsanitize=address,undefined (`make -C csrc tables_check`) and run as its own process.
// Every table lives in a heap buffer of exactly the documented size, so an index past it
// stops the run; beyond that the edge shapes are held to identities of the tables:
// Legendre-Gauss nlat 1, equiangular nlat 2 (both nodes on the poles), mmax > lmax,
// lmax > mmax, forward and inverse, both csphase values.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../include/msfno.h"

// tables.cpp reports through the library's last-error hook (csrc/error.h)
namespace msfno {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace msfno

static int g_failed = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                       \
      std::printf("\n");                              \
      ++g_failed;                                     \
    }                                                 \
  } while (0)

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static bool close(double a, double b, double tol) { return std::fabs(a - b) <= tol * (1.0 + std::fabs(b)); }

static void check_quadrature(int nlat, int grid) {
  std::vector<double> x(nlat, kNaN), w(nlat, kNaN);
  CHECK(msfno_quadrature(nlat, grid, x.data(), w.data()) == MSFNO_OK, "quadrature(%d, %d)", nlat, grid);
  double sum = 0.0;
  for (int k = 0; k < nlat; ++k) {
    CHECK(x[k] >= -1.0 && x[k] <= 1.0 && w[k] > 0.0, "node %d of (%d, %d): x %g w %g", k, nlat, grid, x[k], w[k]);
    CHECK(k == 0 || x[k] > x[k - 1], "nodes of (%d, %d) not ascending at %d", nlat, grid, k);
    CHECK(close(x[k], -x[nlat - 1 - k], 1e-14) && close(w[k], w[nlat - 1 - k], 1e-14),
          "nodes of (%d, %d) not symmetric at %d", nlat, grid, k);
    sum += w[k];
  }
  CHECK(close(sum, 2.0, 1e-14), "weights of (%d, %d) sum to %.17g", nlat, grid, sum);
}

struct Shape {
  int mmax, lmax, nlat, grid;
};

static std::vector<double> table(bool vector, const Shape& s, int inverse, int csphase) {
  std::vector<double> t((size_t)(vector ? 2 : 1) * s.mmax * s.lmax * s.nlat, kNaN);
  const int rc = vector ? msfno_vector_legendre_table(s.mmax, s.lmax, s.nlat, s.grid, inverse, csphase, t.data())
                        : msfno_legendre_table(s.mmax, s.lmax, s.nlat, s.grid, inverse, csphase, t.data());
  CHECK(rc == MSFNO_OK, "table(vector %d, %d %d %d %d): rc %d (%s)", (int)vector, s.mmax, s.lmax, s.nlat,
        s.grid, rc, msfno::g_error.c_str());
  for (size_t i = 0; i < t.size(); ++i)
    CHECK(std::isfinite(t[i]), "table(vector %d, %d %d %d %d)[%zu] not finite", (int)vector, s.mmax, s.lmax,
          s.nlat, s.grid, i);
  return t;
}

static void check_tables(const Shape& s) {
  std::vector<double> x(s.nlat), w(s.nlat);
  CHECK(msfno_quadrature(s.nlat, s.grid, x.data(), w.data()) == MSFNO_OK, "quadrature");
  const size_t plane = (size_t)s.mmax * s.lmax * s.nlat;
  auto at = [&](int m, int l, int k) { return ((size_t)m * s.lmax + l) * s.nlat + k; };
  for (int vec = 0; vec < 2; ++vec) {
    const auto inv = table(vec, s, 1, 1), fwd = table(vec, s, 0, 1);
    const auto inv0 = table(vec, s, 1, 0), fwd0 = table(vec, s, 0, 0);
    for (int pl = 0; pl <= vec; ++pl)
      for (int m = 0; m < s.mmax; ++m)
        for (int l = 0; l < s.lmax; ++l)
          for (int k = 0; k < s.nlat; ++k) {
            const size_t i = pl * plane + at(m, l, k);
            // the phase convention only flips the sign of the odd orders
            const double flip = (m & 1) ? -1.0 : 1.0;
            CHECK(inv0[i] == flip * inv[i] && fwd0[i] == flip * fwd[i], "csphase at %d %d %d", m, l, k);
            if (l < m || (vec && l == 0) || (vec && pl == 1 && m == 0))
              CHECK(inv[i] == 0.0 && fwd[i] == 0.0, "structural zero at %d %d %d", m, l, k);
            // forward = inverse times the quadrature weight (vector: over l (l + 1))
            const double f = vec ? (l ? w[k] / ((double)l * (l + 1)) : 0.0) : w[k];
            CHECK(close(fwd[i], inv[i] * f, 1e-14), "forward weight at %d %d %d", m, l, k);
          }
    for (int k = 0; k < s.nlat; ++k) {
      const double xk = x[s.nlat - 1 - k];  // colatitude index k: node nlat - 1 - k
      if (!vec) {
        CHECK(close(inv[at(0, 0, k)], 1.0 / std::sqrt(4.0 * M_PI), 1e-15), "P_0^0 at %d", k);
        if (s.lmax > 1)
          CHECK(close(inv[at(0, 1, k)], std::sqrt(3.0 / (4.0 * M_PI)) * xk, 1e-14), "P_1^0 at %d", k);
      } else if (s.lmax > 1) {
        // dP_1^0 / dtheta = -sqrt(3 / 4 pi) sin(theta)
        CHECK(close(inv[at(0, 1, k)], -std::sqrt(3.0 / (4.0 * M_PI)) * std::sqrt((1 + xk) * (1 - xk)), 1e-14),
              "dP_1^0 at %d", k);
      }
    }
    // Legendre-Gauss with 2 nlat > 2 lmax - 2 integrates the products exactly:
    // 2 pi sum_k fwd(m, l, k) inv(m, l', k) = delta(l, l')
    if (!vec && s.grid == MSFNO_GRID_LEGENDRE_GAUSS && s.nlat >= s.lmax)
      for (int m = 0; m < s.mmax; ++m)
        for (int l = m; l < s.lmax; ++l)
          for (int l2 = m; l2 < s.lmax; ++l2) {
            double dot = 0.0;
            for (int k = 0; k < s.nlat; ++k) dot += fwd[at(m, l, k)] * inv[at(m, l2, k)];
            CHECK(close(2.0 * M_PI * dot, l == l2 ? 1.0 : 0.0, 1e-12), "orthonormality at m %d l %d l' %d: %g",
                  m, l, l2, 2.0 * M_PI * dot);
          }
  }
}

int main() {
  const int LG = MSFNO_GRID_LEGENDRE_GAUSS, EQ = MSFNO_GRID_EQUIANGULAR;
  for (int nlat : {1, 2, 3, 8, 33}) check_quadrature(nlat, LG);
  for (int nlat : {2, 3, 4, 9, 32}) check_quadrature(nlat, EQ);

  double one[1] = {kNaN}, two[1] = {kNaN};
  msfno::g_error.clear();
  CHECK(msfno_quadrature(1, EQ, one, two) == MSFNO_EINVAL && !msfno::g_error.empty(), "equiangular nlat 1");
  CHECK(msfno_quadrature(0, LG, one, two) == MSFNO_EINVAL, "Legendre-Gauss nlat 0");
  CHECK(msfno_quadrature(4, 7, one, two) == MSFNO_EUNSUPPORTED, "unknown grid");
  CHECK(std::isnan(one[0]) && std::isnan(two[0]), "a refused quadrature wrote its outputs");
  CHECK(msfno_legendre_table(0, 1, 1, LG, 0, 1, one) == MSFNO_EINVAL, "mmax 0");
  CHECK(msfno_legendre_table(1, 1, 1, LG, 0, 1, nullptr) == MSFNO_EINVAL, "null table");
  CHECK(msfno_vector_legendre_table(1, 0, 1, LG, 0, 1, one) == MSFNO_EINVAL, "lmax 0");
  CHECK(msfno_vector_legendre_table(2, 2, 1, EQ, 0, 1, one) == MSFNO_EINVAL, "equiangular nlat 1 table");

  const Shape shapes[] = {
      {1, 1, 1, LG},  // one node on the equator, one mode
      {2, 3, 1, LG},  // ... and more modes than nodes
      {3, 2, 2, EQ},  // both nodes on the poles, mmax > lmax
      {2, 5, 2, EQ},  // ... lmax > mmax
      {6, 3, 5, LG},  // mmax > lmax
      {3, 7, 8, LG},  // lmax > mmax, exact quadrature
      {5, 5, 9, LG},  // square, exact quadrature
      {4, 6, 7, EQ},
  };
  for (const Shape& s : shapes) check_tables(s);
  if (g_failed) {
    std::printf("tables_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("tables_check: ok\n");
  return 0;
}
