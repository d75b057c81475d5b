// Host-side driver for the AddressSanitizer / UndefinedBehaviorSanitizer build of libgbm (tools/asan_host.sh),
// beside asan_driver.cpp: the host code of the principal-component entries. It runs the cyclic Jacobi
// (gbm_debug_sym_eig) on matrices of every size class the eigensolver's driver uses and checks the pairs, and it
// calls gbm_session_pcs, gbm_dev_grm_symmetrize and gbm_dev_rows_times_sym with bad arguments (return code and
// message; the pointers are never dereferenced). The 32x32 Cholesky inverse of the CholQR passes is internal to
// gbm_session_pcs and runs only with a device, so it is not reached here. Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/gbm.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                       \
    }                                                                   \
  } while (0)

// A symmetric m x m matrix from a small linear congruential sequence; kind 1: diagonal, kind 2: a repeated eigenvalue
static std::vector<double> matrix(int m, int kind, uint32_t seed) {
  std::vector<double> A((size_t)m * m, 0.0);
  uint32_t x = seed * 2654435761u + 12345u;
  for (int i = 0; i < m; i++)
    for (int j = i; j < m; j++) {
      x = x * 1664525u + 1013904223u;
      double v = (double)(x >> 8) / 16777216.0 - 0.5;
      if (kind == 1 && i != j) v = 0.0;
      if (kind == 2) v = (i == j) ? (i < m / 2 ? 2.0 : -1.0) : 0.0;
      A[(size_t)i * m + j] = A[(size_t)j * m + i] = v;
    }
  return A;
}

static void sym_eig_pairs(int m, int kind, uint32_t seed) {
  const std::vector<double> A = matrix(m, kind, seed);
  std::vector<double> w(m), V((size_t)m * m);
  CHECK(gbm_debug_sym_eig(A.data(), m, w.data(), V.data()) == GBM_OK);
  double norm = 0.0, worst = 0.0;
  for (double v : A) norm += v * v;
  norm = std::sqrt(norm);
  for (int i = 0; i < m; i++) {
    CHECK(i == 0 || w[i] <= w[i - 1]);
    for (int r = 0; r < m; r++) {  // (A v_i − w_i v_i)[r], v_i = row i of V
      double a = 0.0;
      for (int c = 0; c < m; c++) a += A[(size_t)r * m + c] * V[(size_t)i * m + c];
      worst = std::fmax(worst, std::fabs(a - w[i] * V[(size_t)i * m + r]));
    }
  }
  CHECK(worst <= 64.0 * std::numeric_limits<double>::epsilon() * std::fmax(norm, 1e-300));
}

static void bad_arguments() {
  double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, w[3], V[9];
  CHECK(gbm_debug_sym_eig(nullptr, 3, w, V) == GBM_E_ARG && std::strstr(gbm_last_error(), "gbm_debug_sym_eig"));
  CHECK(gbm_debug_sym_eig(A, 0, w, V) == GBM_E_ARG);
  CHECK(gbm_debug_sym_eig(A, 65, w, V) == GBM_E_ARG);
  A[5] = NAN;
  CHECK(gbm_debug_sym_eig(A, 3, w, V) == GBM_E_ARG && std::strstr(gbm_last_error(), "NaN"));

  std::vector<double> vec(100 * 16), val(16);
  auto pcs = [&](int64_t n_train, int kind, int64_t k, double tol, int64_t max_iter, bool v, bool l) {
    return gbm_session_pcs(nullptr, nullptr, n_train, kind, k, tol, max_iter, v ? vec.data() : nullptr,
                           l ? val.data() : nullptr, nullptr, nullptr, nullptr);
  };
  CHECK(pcs(100, 2, 2, 1e-10, 10, true, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "kind"));
  CHECK(pcs(100, 0, 0, 1e-10, 10, true, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "k must be"));
  CHECK(pcs(100, 0, 17, 1e-10, 10, true, true) == GBM_E_ARG);
  CHECK(pcs(63, 0, 2, 1e-10, 10, true, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "at least 64"));
  CHECK(pcs(100, 0, 2, 0.0, 10, true, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "tol"));
  CHECK(pcs(100, 0, 2, NAN, 10, true, true) == GBM_E_ARG);
  CHECK(pcs(100, 0, 2, INFINITY, 10, true, true) == GBM_E_ARG);
  CHECK(pcs(100, 0, 2, 1e-10, 0, true, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "max_iter"));
  CHECK(pcs(100, 0, 2, 1e-10, 10, false, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "NULL"));
  CHECK(pcs(100, 0, 2, 1e-10, 10, true, false) == GBM_E_ARG);
  CHECK(pcs(64, 1, 16, 1e-10, 1, true, true) == GBM_E_ARG && std::strstr(gbm_last_error(), "session is NULL"));

  const int64_t n = 300, npad = gbm_dev_npad(n), gdim = gbm_dev_gdim(n);
  double* G = (double*)(uintptr_t)(1 << 20);  // never dereferenced
  double* K = (double*)(uintptr_t)(1 << 24);
  double* Y = (double*)(uintptr_t)(1 << 26);
  void* ws = (void*)(uintptr_t)(1 << 28);
  CHECK(gbm_dev_grm_symmetrize(nullptr, gdim, n, 1.0, K, npad, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_grm_symmetrize(G, gdim, n, 1.0, nullptr, npad, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_grm_symmetrize(G, gdim, n, 1.0, G, gdim, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_grm_symmetrize(G, gdim, 0, 1.0, K, npad, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_grm_symmetrize(G, npad - 1, n, 1.0, K, npad, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_grm_symmetrize(G, gdim, n, 1.0, K, npad + 1, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_grm_symmetrize(G, gdim, n, NAN, K, npad, nullptr) == GBM_E_ARG);
  const int64_t wsb = gbm_dev_rows_times_sym_workspace(n, 32);
  CHECK(wsb >= 16 && gbm_dev_rows_times_sym_workspace(n, 64) >= wsb && gbm_dev_rows_times_sym_workspace(0, 32) == 0);
  CHECK(gbm_dev_rows_times_sym(K, npad, n, G, npad, 24, Y, npad, ws, wsb, nullptr) == GBM_E_ARG &&
        std::strstr(gbm_last_error(), "rows must be"));
  CHECK(gbm_dev_rows_times_sym(K, npad, n, G, npad, 80, Y, npad, ws, wsb, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_rows_times_sym(K, npad, 0, G, npad, 32, Y, npad, ws, wsb, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_rows_times_sym(nullptr, npad, n, G, npad, 32, Y, npad, ws, wsb, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_rows_times_sym(K, npad, n, G, npad, 32, G, npad, ws, wsb, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_rows_times_sym(K, npad - 2, n, G, npad, 32, Y, npad, ws, wsb, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_rows_times_sym(K, npad, n, G, npad + 1, 32, Y, npad, ws, wsb, nullptr) == GBM_E_ARG);
  CHECK(gbm_dev_rows_times_sym(K, npad, n, G, npad, 32, Y, npad, nullptr, wsb, nullptr) == GBM_E_ARG &&
        std::strstr(gbm_last_error(), "workspace"));
  CHECK(gbm_dev_rows_times_sym(K, npad, n, G, npad, 32, Y, npad, ws, wsb - 8, nullptr) == GBM_E_ARG);
}

int main() {
  const int sizes[] = {1, 2, 3, 31, 32, 33, 64};
  for (int m : sizes) {
    sym_eig_pairs(m, 0, (uint32_t)m);
    sym_eig_pairs(m, 1, (uint32_t)m + 100);
    sym_eig_pairs(m, 2, 0);
  }
  bad_arguments();
  std::printf("asan pcs driver: %d failures\n", failures);
  return failures ? 1 : 0;
}
