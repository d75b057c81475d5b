// Host-side driver for the AddressSanitizer / UndefinedBehaviorSanitizer build of libgbm (tools/asan_host.sh),
// beside asan_driver.cpp: the host code of gbm_bayes_fit_ordinal in front of its first device call. The class
// scan (sort, distinct values, class of every individual, start thresholds through AS241) runs on real arrays
// for K = 1, 2, 3, 32 and 33 and capacities below and at K; with no device the calls that pass every argument
// check end in GBM_E_NODEV, the others in GBM_E_ARG with the entry's name in the message. Then the host half of
// gbm_debug_ordinal_math (Φ, Φ⁻¹, TN of csrc/gibbs_common.h) and its argument checks. Test infrastructure only.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static int fit(int64_t n, int64_t p, int nclasses, int64_t max_classes, double bad_value = 0.0, int model = GBM_BAYES_B,
               int64_t n_iter = 10, int64_t ldprobs_less = 0) {
  std::vector<double> X((size_t)n * p), y(n), b(p + 1), yp(n), pip(p), probs((size_t)n * 33);
  for (size_t t = 0; t < X.size(); t++) X[t] = (double)((t * 7 + t / 3) % 3) * 0.5;
  for (int64_t i = 0; i < n; i++) y[i] = (double)((i * 5) % nclasses) - 1.0;  // unsorted, a negative class value
  if (bad_value != 0.0) y[n / 2] = bad_value;
  // capacities exactly as passed: the sanitizer sees any write past max_classes
  std::vector<double> classes(max_classes > 0 ? max_classes : 1), thresholds(max_classes > 1 ? max_classes - 1 : 1);
  double var[3];
  int64_t K = -1;
  return gbm_bayes_fit_ordinal(model, X.data(), n, p, n, y.data(), n_iter, 2, 1, 0.5, 5.0, 0.5, 10.0, 1, 0, b.data(),
                               yp.data(), var, pip.data(), max_classes, &K, classes.data(), thresholds.data(),
                               probs.data(), n - ldprobs_less);
}

int main() {
  const double inf = 1.0 / 0.0;
  // refused before any device work
  CHECK(fit(40, 30, 1, 32) == GBM_E_ARG && std::strstr(gbm_last_error(), "gbm_bayes_fit_ordinal"));
  CHECK(fit(40, 30, 33, 64) == GBM_E_ARG && std::strstr(gbm_last_error(), "distinct"));
  CHECK(fit(40, 30, 4, 3) == GBM_E_ARG);
  CHECK(fit(40, 30, 3, 0) == GBM_E_ARG);
  CHECK(fit(40, 30, 3, 32, inf) == GBM_E_ARG);
  CHECK(fit(40, 30, 3, 32, 0.0, 7) == GBM_E_ARG && std::strstr(gbm_last_error(), "model"));
  CHECK(fit(40, 30, 3, 32, 0.0, GBM_BAYES_B, 2) == GBM_E_ARG);  // no post-burn-in sample
  CHECK(fit(40, 30, 3, 32, 0.0, GBM_BAYES_B, 10, 1) == GBM_E_ARG);  // ldprobs < n
  // every argument check passed: the class scan ran; the device check answers
  for (int k : {2, 3, 32}) {
    const int rc = fit(70, 20, k, k);
    CHECK(rc == GBM_E_NODEV || rc == GBM_OK);
  }
  // gbm_debug_ordinal_math, host only (dev_out = NULL): buffers of exactly m (4 m for TN) values, the ends of
  // Φ⁻¹, a draw where u Φ(β) rounds to 0 and one where pa + u (1 − pa) rounds to 1: both finite, the interval's end
  {
    const std::vector<double> p = {0.0, 0.5, 1.0}, tn = {38.0, -inf, 0.0, 0x1p-54, 1.0, 0.0, inf, 1.0 - 0x1p-53};
    std::vector<double> out(3), draws(2);
    CHECK(gbm_debug_ordinal_math(1, p.data(), 3, 0, out.data(), nullptr) == GBM_OK);
    CHECK(out[0] == -inf && out[1] == 0.0 && out[2] == inf);
    CHECK(gbm_debug_ordinal_math(0, p.data(), 3, 0, out.data(), nullptr) == GBM_OK && out[0] == 0.5);
    CHECK(gbm_debug_ordinal_math(2, tn.data(), 2, 0, draws.data(), nullptr) == GBM_OK);
    CHECK(draws[0] == 0.0 && draws[1] == 0.0);
    CHECK(gbm_debug_ordinal_math(3, p.data(), 3, 0, out.data(), nullptr) == GBM_E_ARG &&
          std::strstr(gbm_last_error(), "gbm_debug_ordinal_math"));
    CHECK(gbm_debug_ordinal_math(1, nullptr, 3, 0, out.data(), nullptr) == GBM_E_ARG);
    CHECK(gbm_debug_ordinal_math(1, p.data(), 3, 0, nullptr, nullptr) == GBM_E_ARG);
    CHECK(gbm_debug_ordinal_math(1, p.data(), 0, 0, out.data(), nullptr) == GBM_E_ARG);
    CHECK(gbm_debug_ordinal_math(1, p.data(), ((int64_t)1 << 20) + 1, 0, out.data(), nullptr) == GBM_E_ARG);
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("asan_ordinal_driver ok\n");
  return 0;
}
