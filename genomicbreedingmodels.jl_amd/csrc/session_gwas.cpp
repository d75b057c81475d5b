// ---- GWAS scan on the cached factor (reference gwasreml / gwasols, src/gwas.jl:241-245, 591-599) ----
// Mixed model: V = σ²_u ZZᵀ/q + σ²_e I = σ²_u V_λ, λ = σ²_e/σ²_u. One bordered solve with [C, y] as right-hand
// sides leaves the factor U of V_λ, the whitened rows U⁻ᵀ[1, C, y] (lower-copy rows npad + s) and
// −[1, C, y]ᵀV_λ⁻¹[1, C, y] (the Schur block); the locus rows are whitened chunk by chunk (gbm_dev_whiten_rows)
// and each locus' statistic is the Schur complement of the bordered normal equations (gwas_stats_kernel).
// z = z_λ/√σ²_u, b = b_λ. OLS: the same statistics kernel on the unwhitened rows with V = I.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "session.h"

using namespace gbm;

// A⁻¹ of the K x K (K <= 8) symmetric positive definite A (row-major, pitch 8) by Cholesky, in place
static bool invert_spd8(double* A, int K) {
  double L[64] = {0.0};
  for (int j = 0; j < K; j++) {
    double d = A[j * 8 + j];
    for (int k = 0; k < j; k++) d -= L[j * 8 + k] * L[j * 8 + k];
    if (!(d > 1e-13 * A[j * 8 + j]) || !std::isfinite(d)) return false;
    L[j * 8 + j] = std::sqrt(d);
    for (int i = j + 1; i < K; i++) {
      double v = A[i * 8 + j];
      for (int k = 0; k < j; k++) v -= L[i * 8 + k] * L[j * 8 + k];
      L[i * 8 + j] = v / L[j * 8 + j];
    }
  }
  double Li[64] = {0.0};  // L⁻¹ (lower)
  for (int j = 0; j < K; j++) {
    Li[j * 8 + j] = 1.0 / L[j * 8 + j];
    for (int i = j + 1; i < K; i++) {
      double v = 0.0;
      for (int k = j; k < i; k++) v -= L[i * 8 + k] * Li[k * 8 + j];
      Li[i * 8 + j] = v / L[i * 8 + i];
    }
  }
  for (int a = 0; a < K; a++)
    for (int b = 0; b < K; b++) {
      double v = 0.0;
      for (int k = std::max(a, b); k < K; k++) v += Li[k * 8 + a] * Li[k * 8 + b];
      A[a * 8 + b] = v;
    }
  return true;
}

// Loci per chunk of the GWAS scan. One whitening workgroup owns a 64-row strip for the whole sweep, so a
// chunk's launch keeps at most chunk/64 compute units busy: the chunk is as many strips as the device has
// compute units (a multiple of that while the buffer stays under 768 MB, fewer when even one round does not
// fit), and the chunks are balanced so that no launch is left with a few strips. GBM_GWAS_CHUNK (loci)
// overrides. The statistics do not depend on the chunking.
static int64_t gwas_chunk(int64_t p, int64_t npadT, int dev) {
  const int64_t forced = knob_i64("GBM_GWAS_CHUNK", 0);
  if (forced > 0) return forced < p ? forced : p;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) {
    (void)hipGetLastError();
    ncu = 256;
  }
  const int64_t strips = (p + 63) / 64;
  int64_t cap = ((int64_t)768 << 20) / (npadT * 8 * 64);  // strips in 768 MB
  if (cap < 1) cap = 1;
  if (cap >= ncu) cap = cap / ncu * ncu;
  const int64_t nchunks = (strips + cap - 1) / cap;
  const int64_t c = (strips + nchunks - 1) / nchunks * 64;
  return c < p ? c : p;
}

extern "C" int gbm_session_gwas(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y, const double* C,
                                int64_t ldc, int64_t kc, int model, double sigma2_e, double sigma2_u, double* z_out,
                                double* b_out, double* sigma2_out, int64_t* tested_out) {
  RoctxRange r_("gbm_session_gwas");
  if (kc < 0 || kc > 7) return fail(GBM_E_ARG, "gbm_session_gwas: kc (extra covariates) must be in [0, 7]");
  if (model != 0 && model != 1) return fail(GBM_E_ARG, "gbm_session_gwas: model must be 0 (mixed model) or 1 (OLS)");
  const bool estimate = std::isnan(sigma2_e) || std::isnan(sigma2_u);
  if (model == 0 && !estimate &&
      (!(sigma2_e > 0.0) || !(sigma2_u > 0.0) || !std::isfinite(sigma2_e) || !std::isfinite(sigma2_u)))
    return fail(GBM_E_ARG, "gbm_session_gwas: sigma2_e and sigma2_u must be > 0 (or NaN: estimated by REML)");
  if (!s) return fail(GBM_E_ARG, "gbm_session_gwas: session is NULL");
  if (!y || !z_out || (kc > 0 && (!C || ldc < n_train)))
    return fail(GBM_E_ARG, "gbm_session_gwas: bad arguments (y, z_out, C with ldc >= n_train)");
  if (n_train < kc + 3) return fail(GBM_E_ARG, "gbm_session_gwas: n_train must be at least kc + 3");
  GBM_SESSION_ENTER(s);
  GBM_TRY(check_y(y, n_train, n_train, 1));
  for (int64_t c = 0; c < kc; c++)
    for (int64_t i = 0; i < n_train; i++)
      if (!std::isfinite(C[c * ldc + i]))
        return fail(GBM_E_ARG, "gbm_session_gwas: covariate " + std::to_string(c + 1) + " has a NaN/Inf value at entry " +
                                   std::to_string(i + 1));
  GBM_TRY(ensure_training(s, idx, n_train));
  hipStream_t st = s->stream.s;
  gbm_session::Gwas& gw = s->gw;
  const int64_t p = s->p, nT = s->nT, npadT = s->npadT, gdimT = s->gdimT;
  const int K = (int)kc + 1;  // covariate rows, the intercept first
  const std::vector<double> ys = standardise_y(y, n_train);
  GBM_TRY(ensure_rhs(s, kc + 2));
  for (DevBuf* b : {&gw.z, &gw.b}) GBM_TRY(ensure(*b, s->dev, p * 8));
  GBM_TRY(ensure(gw.cnt, s->dev, 8));
  GBM_HIP_TRY(hipMemsetAsync(gw.cnt.p, 0, 8, st));
  GwasCoef co;
  std::memset(&co, 0, sizeof(co));
  co.kcov = K;
  double u[8] = {0.0};
  double used[2] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN()};
  const double *Z = s->Z.as<const double>(), *Gw = s->Gw.as<const double>();
  if (model == 0) {
    if (estimate) {
      RemlResult res;
      GBM_TRY(reml_cached(s, ys, res));
      sigma2_e = res.s2e;
      sigma2_u = res.s2u;
    }
    used[0] = sigma2_e;
    used[1] = sigma2_u;
    // right-hand sides [C, y]: with the bordered 1 column, W = U⁻ᵀ[1, C, y]
    std::vector<double> rhs((size_t)(K * n_train));
    for (int64_t c = 0; c < kc; c++) std::memcpy(&rhs[(size_t)(c * n_train)], C + c * ldc, (size_t)n_train * 8);
    std::memcpy(&rhs[(size_t)(kc * n_train)], ys.data(), (size_t)n_train * 8);
    GBM_TRY(upload_y(s, rhs.data(), n_train, K));
    GBM_TRY(solve_cached(s, K, sigma2_e / sigma2_u, 1.0 / (double)s->q));
    // the Schur block −WᵀW (upper part): A = C̃ᵀC̃, u = C̃ᵀỹ
    double S[9 * 9];
    GBM_HIP_TRY(hipMemcpy2DAsync(S, (K + 1) * 8, Gw + npadT * gdimT + npadT, gdimT * 8, (K + 1) * 8, K + 1,
                                 hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    for (int a = 0; a < K; a++) {
      for (int b = 0; b < K; b++) co.Ainv[a * 8 + b] = -S[std::min(a, b) * (K + 1) + std::max(a, b)];
      u[a] = -S[a * (K + 1) + K];
    }
    co.zscale = 1.0 / std::sqrt(sigma2_u);
  } else {
    // rows [1, C, y] on the device (in the right-hand-side buffer); A = XᵀX, u = Xᵀy on the host
    std::vector<double> rowsb((size_t)((K + 1) * npadT), 0.0);
    for (int64_t i = 0; i < n_train; i++) rowsb[(size_t)i] = 1.0;
    for (int64_t c = 0; c < kc; c++)
      for (int64_t i = 0; i < n_train; i++) rowsb[(size_t)((c + 1) * npadT + i)] = C[c * ldc + i];
    for (int64_t i = 0; i < n_train; i++) rowsb[(size_t)(K * npadT + i)] = ys[(size_t)i];
    GBM_HIP_TRY(hipMemcpyAsync(s->Y.p, rowsb.data(), rowsb.size() * 8, hipMemcpyHostToDevice, st));
    for (int a = 0; a < K; a++) {
      for (int b = a; b < K; b++) {
        double v = 0.0;
        for (int64_t i = 0; i < n_train; i++) v += rowsb[(size_t)(a * npadT + i)] * rowsb[(size_t)(b * npadT + i)];
        co.Ainv[a * 8 + b] = co.Ainv[b * 8 + a] = v;
      }
      double v = 0.0;
      for (int64_t i = 0; i < n_train; i++) v += rowsb[(size_t)(a * npadT + i)] * rowsb[(size_t)(K * npadT + i)];
      u[a] = v;
    }
    GBM_HIP_TRY(hipStreamSynchronize(st));  // rowsb leaves scope below
    co.zscale = 1.0;
  }
  if (!invert_spd8(co.Ainv, K))
    return fail(GBM_E_DATA, "gbm_session_gwas: the covariates (with the intercept) are collinear");
  for (int a = 0; a < K; a++)
    for (int b = 0; b < K; b++) co.Au[a] += co.Ainv[a * 8 + b] * u[b];
  const int32_t* keep = s->keep.as<const int32_t>();
  double *zd = gw.z.as<double>(), *bd = gw.b.as<double>();
  unsigned long long* cnt = gw.cnt.as<unsigned long long>();
  if (model == 0) {
    const int64_t chunk = gwas_chunk(p, npadT, s->dev);
    GBM_TRY(ensure(gw.W, s->dev, chunk * npadT * 8));
    double* W = gw.W.as<double>();
    for (int64_t j0 = 0; j0 < p; j0 += chunk) {
      const int64_t rows = std::min(chunk, p - j0);
      // the cached Z is never written: whiten a copy of the chunk
      GBM_HIP_TRY(hipMemcpyAsync(W, Z + j0 * npadT, (size_t)(rows * npadT * 8), hipMemcpyDeviceToDevice, st));
      GBM_TRY(gbm_dev_whiten_rows(Gw, gdimT, nT, s->wss.p, W, npadT, rows, st));
      GBM_TRY(launch_gwas_stats(W, npadT, rows, nT, Gw + npadT * gdimT, gdimT, Gw + (npadT + K) * gdimT, co, keep + j0,
                                zd + j0, bd + j0, nullptr, cnt, st));
    }
  } else {
    const double* rows_d = s->Y.as<const double>();
    GBM_TRY(launch_gwas_stats(Z, npadT, p, nT, rows_d, npadT, rows_d + K * npadT, co, keep, zd, bd, nullptr, cnt, st));
  }
  unsigned long long tested = 0;
  GBM_HIP_TRY(hipMemcpyAsync(z_out, zd, p * 8, hipMemcpyDeviceToHost, st));
  if (b_out) GBM_HIP_TRY(hipMemcpyAsync(b_out, bd, p * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipMemcpyAsync(&tested, cnt, 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  if (sigma2_out) {
    sigma2_out[0] = used[0];
    sigma2_out[1] = used[1];
  }
  if (tested_out) *tested_out = (int64_t)tested;
  return GBM_OK;
}
