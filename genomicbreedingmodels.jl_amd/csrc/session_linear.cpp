// The glmnet paths of a session on the centred training genotypes (standardize = false): the ridge λ_max and the
// exact ridge path on the cached kernel, and the lasso / elastic-net path by coordinate descent (enet.hip).
#include <algorithm>
#include <cmath>

#include "session.h"

using namespace gbm;

// every λ finite and > 0; non_increasing: and none above the one before it (checked λ by λ, in that order)
static int check_lambdas(const std::string& entry, const double* lambdas, int64_t nl, bool non_increasing) {
  for (int64_t k = 0; k < nl; k++) {
    if (!(lambdas[k] > 0.0) || !std::isfinite(lambdas[k])) return fail(GBM_E_ARG, entry + ": lambdas must be finite and > 0");
    if (non_increasing && k > 0 && lambdas[k] > lambdas[k - 1])
      return fail(GBM_E_ARG, entry + ": lambdas must be non-increasing (the path is warm-started)");
  }
  return GBM_OK;
}

// ---- ridge path (glmnet alpha = 0, standardize = false; reference ridge, src/linear.jl:193-203) --
// glmnet minimises (1/2n)‖y − a0 − Xb‖² + (λ/2)‖b‖² on y scaled by its population sd σ_y, with the
// user λ divided by the same σ_y (elnet: vlam = ulam/ys). On the original scale that is
// (X_cᵀX_c + (nλ/σ_y)I) b = X_cᵀ(y − ȳ): the GBLUP system on the unscaled centred-X kernel
// K = X_cX_cᵀ with λ' = nλ/σ_y, whose GLS intercept is ȳ (K1 = 0) and whose marker effects are
// b = X_cᵀa. σ_y is taken over the training rows of each call (each CV fold has its own).

extern "C" int gbm_session_ridge_lambda_max(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                                            double* lambda_max) {
  if (!s || !y || !lambda_max) return fail(GBM_E_ARG, "gbm_session_ridge_lambda_max: bad arguments");
  GBM_SESSION_ENTER(s);
  GBM_TRY(check_y(y, n_train, n_train, 1));
  GBM_TRY(ensure_training(s, idx, n_train, 1));
  GBM_TRY(ensure_rhs(s, 1));
  // glmnet's first λ for alpha < 1e-3: max_j |x_cjᵀ(y − ȳ)|/n / 1e-3
  const double m = centre_y(y, n_train).mean;
  std::vector<double> r(s->npadT, 0.0);
  for (int64_t i = 0; i < n_train; i++) r[i] = y[i] - m;
  hipStream_t st = s->stream.s;
  GBM_HIP_TRY(hipMemcpyAsync(s->A.p, r.data(), s->npadT * 8, hipMemcpyHostToDevice, st));
  GBM_TRY(effects_cached(s, s->A.as<const double>(), s->npadT, 1, 1.0));
  std::vector<double> g(s->p);
  GBM_HIP_TRY(hipMemcpyAsync(g.data(), s->B.p, s->p * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  double gmax = 0.0;
  for (double v : g) gmax = std::max(gmax, std::fabs(v));
  *lambda_max = gmax / (double)n_train / 1e-3;
  return GBM_OK;
}

extern "C" int gbm_session_ridge_path(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                                      const double* lambdas, int64_t nl, double* b_path_out, const int64_t* idx_eval,
                                      int64_t n_eval, double* pred_out) {
  RoctxRange r_("gbm_session_ridge_path");
  if (!s || !y || !lambdas || nl < 1 || !b_path_out || (n_eval > 0 && (!idx_eval || !pred_out)))
    return fail(GBM_E_ARG, "gbm_session_ridge_path: bad arguments");
  GBM_TRY(check_lambdas("gbm_session_ridge_path", lambdas, nl, false));
  GBM_SESSION_ENTER(s);
  GBM_TRY(check_y(y, n_train, n_train, 1));
  if (n_eval > 0) GBM_TRY(check_idx(s, idx_eval, n_eval, "gbm_session_ridge_path (eval)"));
  GBM_TRY(ensure_training(s, idx, n_train, 1));
  GBM_TRY(ensure_rhs(s, 1));
  GBM_TRY(upload_y(s, y, n_train, 1));
  const double ys = centre_y(y, n_train).sd;
  if (!(ys > 0.0)) return fail(GBM_E_ARG, "gbm_session_ridge_path: y has zero variance");
  hipStream_t st = s->stream.s;
  const int64_t p = s->p;
  for (int64_t k = 0; k < nl; k++) {
    GBM_TRY(solve_cached(s, 1, (double)n_train * lambdas[k] / ys, 1.0));
    GBM_TRY(effects_cached(s, s->A.as<const double>(), s->npadT, 1, 1.0));
    double mu = 0.0, msum = 0.0;
    double* bk = b_path_out + k * (p + 1);
    GBM_HIP_TRY(hipMemcpyAsync(bk + 1, s->B.p, p * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipMemcpyAsync(&mu, s->mu_d.p, 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipMemcpyAsync(&msum, s->msum.p, 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    bk[0] = mu - msum;
    if (n_eval > 0)
      GBM_TRY(predict_at(s, bk, p + 1, s->B.as<const double>(), 1, idx_eval, n_eval, pred_out + k * n_eval, n_eval));
  }
  return GBM_OK;
}

// ---- lasso / elastic-net path (glmnet alpha in (0, 1], standardize = false; reference lasso, src/linear.jl:333-343) --
// Cyclic coordinate descent on an active set (include/gbm.h states the model and the schedule). Per λ: passes over
// the packed active rows (one enet_chain_kernel launch per 64-marker block, one host synchronisation per pass for
// the convergence scalar), then a screen g = Zᵀe over all p loci (gbm_dev_marker_effects) whose violators are
// appended to the active list; b, e and the active list are carried from λ to λ on the device.
extern "C" int gbm_session_enet_path(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y, double alpha,
                                     const double* lambdas, int64_t nl, double tol, int64_t max_passes, double dev_max,
                                     double fdev, double* b_path_out, const int64_t* idx_eval, int64_t n_eval,
                                     double* pred_out, int64_t* nl_done_out, double* dev_ratio_out, int64_t* passes_out,
                                     int64_t* nnz_out) {
  RoctxRange r_("gbm_session_enet_path");
  set_error("");
  if (!s || !y || !lambdas || nl < 1 || !b_path_out || (n_eval > 0 && (!idx_eval || !pred_out)))
    return fail(GBM_E_ARG, "gbm_session_enet_path: bad arguments");
  if (!(alpha > 0.0 && alpha <= 1.0))
    return fail(GBM_E_ARG, "gbm_session_enet_path: alpha must be in (0, 1] (alpha = 0 is gbm_session_ridge_path, "
                           "which solves that case exactly)");
  GBM_TRY(check_lambdas("gbm_session_enet_path", lambdas, nl, true));
  if (!(tol > 0.0) || !std::isfinite(tol) || max_passes < 1)
    return fail(GBM_E_ARG, "gbm_session_enet_path: tol must be > 0 and max_passes >= 1");
  if (std::isnan(dev_max) || !(fdev >= 0.0) || !std::isfinite(fdev))
    return fail(GBM_E_ARG, "gbm_session_enet_path: dev_max must not be NaN and fdev must be finite and >= 0");
  GBM_SESSION_ENTER(s);
  GBM_TRY(check_y(y, n_train, n_train, 1));
  if (n_eval > 0) GBM_TRY(check_idx(s, idx_eval, n_eval, "gbm_session_enet_path (eval)"));
  GBM_TRY(ensure_training(s, idx, n_train, 1));
  GBM_TRY(ensure_rhs(s, 1));
  const YStats yst = centre_y(y, n_train);
  const double ym = yst.mean, yss = yst.ss, ys = yst.sd;
  if (!(ys > 0.0)) return fail(GBM_E_ARG, "gbm_session_enet_path: y has zero variance");
  hipStream_t st = s->stream.s;
  gbm_session::Enet& en = s->en;
  const int dev_id = s->dev;
  const int64_t p = s->p, nT = s->nT;
  const int64_t lda = enet_lda(nT), cap = std::min(p, 2 * s->npadT), cappad = round_up(cap, 64);
  const int64_t C = (nT + 255) / 256;
  GBM_TRY(ensure(en.Za, dev_id, cap * lda * 8));
  GBM_TRY(ensure(en.W, dev_id, cappad * 64 * 8));
  for (DevBuf* b : {&en.x2a, &en.inv}) GBM_TRY(ensure(*b, dev_id, cappad * 8));
  GBM_TRY(ensure(en.b, dev_id, 2 * cappad * 8));
  GBM_TRY(ensure(en.e, dev_id, lda * 8));
  GBM_TRY(ensure(en.x2, dev_id, p * 8));
  GBM_TRY(ensure(en.part, dev_id, 2 * C * 64 * 8));
  GBM_TRY(ensure(en.blk, dev_id, (cappad / 64) * 8));
  GBM_TRY(ensure(en.red, dev_id, 2 * 8));
  GBM_TRY(ensure(en.rows, dev_id, cap * 4));
  GBM_TRY(ensure(en.gws, dev_id, enet_gram_workspace(nT)));
  const double* const Z = s->Z.as<const double>();
  double *const Za = en.Za.as<double>(), *const W = en.W.as<double>(), *const x2a = en.x2a.as<double>();
  double *const inv = en.inv.as<double>(), *const bdev = en.b.as<double>(), *const e = en.e.as<double>();
  double* const red = en.red.as<double>();
  std::vector<double> e0(lda, 0.0), x2h(p), meanh(p), g(p), bh(cap);
  for (int64_t i = 0; i < nT; i++) e0[i] = y[i] - ym;
  GBM_HIP_TRY(hipMemcpyAsync(e, e0.data(), lda * 8, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemsetAsync(x2a, 0, cappad * 8, st));
  GBM_HIP_TRY(hipMemsetAsync(bdev, 0, 2 * cappad * 8, st));
  GBM_TRY(launch_enet_x2(Z, s->npadT, p, nT, en.x2.as<double>(), st));
  GBM_HIP_TRY(hipMemcpyAsync(x2h.data(), en.x2.p, p * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipMemcpyAsync(meanh.data(), s->mean.p, p * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  std::vector<char> active(p, 0);
  std::vector<int64_t> act;
  std::vector<int32_t> fresh;
  int par = 0;  // the copy of b that holds the current coefficients
  int64_t done = 0, first_unconverged = -1;
  double dev_prev = 0.0;
  const int64_t mnl = std::min<int64_t>(5, nl);
  for (int64_t k = 0; k < nl; k++) {
    const double thr = (double)nT * lambdas[k] * alpha, l2 = (double)nT * lambdas[k] * (1.0 - alpha) / ys;
    int64_t A = (int64_t)act.size(), passes = 0;
    bool hit = false;
    GBM_TRY(launch_enet_prep(A, x2a, l2, inv, st));
    for (;;) {
      while (A > 0) {
        if (passes >= max_passes) {
          hit = true;
          break;
        }
        double r2[2] = {0.0, 0.0};
        GBM_TRY(launch_enet_pass(Za, lda, nT, A, W, x2a, inv, bdev + par * cappad, bdev + (par ^ 1) * cappad, thr,
                                 en.part.as<double>(), en.blk.as<double>(), e, red, st));
        par ^= 1;
        GBM_HIP_TRY(hipMemcpyAsync(r2, red, 16, hipMemcpyDeviceToHost, st));
        GBM_HIP_TRY(hipStreamSynchronize(st));
        passes++;
        if (r2[0] < tol * ys * ys) break;
      }
      if (hit) break;
      // screen: g = Zᵀe over all p loci; every inactive locus past the threshold joins the list (ascending j)
      GBM_TRY(effects_cached(s, e, lda, 1, 1.0));
      GBM_HIP_TRY(hipMemcpyAsync(g.data(), s->B.p, p * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));
      fresh.clear();
      for (int64_t j = 0; j < p; j++)
        if (!active[j] && std::fabs(g[j]) > thr && x2h[j] > 0.0) fresh.push_back((int32_t)j);
      if (fresh.empty()) break;
      const int64_t cnt = (int64_t)fresh.size();
      if (A + cnt > cap)
        return fail(GBM_E_ARG, "gbm_session_enet_path: the active set needs " + std::to_string(A + cnt) +
                                   " markers at lambda number " + std::to_string(k + 1) + ", over the cap of min(p, 2 npad) = " +
                                   std::to_string(cap) + " packed rows (use a larger lambda or alpha)");
      GBM_HIP_TRY(hipMemcpyAsync(en.rows.p, fresh.data(), cnt * 4, hipMemcpyHostToDevice, st));
      GBM_TRY(launch_enet_gather(Z, s->npadT, nT, en.rows.as<const int32_t>(), A, cnt, en.x2.as<const double>(), Za, lda,
                                 x2a, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));  // `fresh` is pageable: the copy has read it before it changes
      for (int32_t j : fresh) {
        active[j] = 1;
        act.push_back(j);
      }
      const int64_t blk0 = A / 64;  // the partly filled last block and the new ones
      A += cnt;
      GBM_TRY(launch_enet_gram(Za, lda, A, nT, blk0, W, en.gws.as<double>(), st));
      GBM_TRY(launch_enet_prep(A, x2a, l2, inv, st));
    }
    if (hit && first_unconverged < 0) first_unconverged = k;
    double r2[2] = {0.0, 0.0};
    GBM_TRY(launch_enet_norm(e, nT, red, st));
    GBM_HIP_TRY(hipMemcpyAsync(r2, red, 16, hipMemcpyDeviceToHost, st));
    if (A > 0) GBM_HIP_TRY(hipMemcpyAsync(bh.data(), bdev + par * cappad, A * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    double* bk = b_path_out + k * (p + 1);
    std::fill(bk, bk + p + 1, 0.0);
    double msum = 0.0;
    int64_t nnz = 0;
    for (int64_t a = 0; a < A; a++) {
      bk[1 + act[a]] = bh[a];
      msum += meanh[act[a]] * bh[a];
      nnz += bh[a] != 0.0;
    }
    bk[0] = ym - msum;
    const double dev = 1.0 - r2[1] / yss;
    if (dev_ratio_out) dev_ratio_out[k] = dev;
    if (passes_out) passes_out[k] = passes;
    if (nnz_out) nnz_out[k] = nnz;
    if (n_eval > 0) GBM_TRY(predict_at(s, bk, p + 1, nullptr, 1, idx_eval, n_eval, pred_out + k * n_eval, n_eval));
    done = k + 1;
    // glmnet's early stop: the λ that trips it is the last one kept
    if (done >= mnl && (dev > dev_max || (fdev > 0.0 && dev - dev_prev < fdev * dev))) break;
    dev_prev = dev;
  }
  if (nl_done_out) *nl_done_out = done;
  if (first_unconverged >= 0)
    set_error("warning: gbm_session_enet_path: max_passes = " + std::to_string(max_passes) +
              " reached before convergence, first at lambda number " + std::to_string(first_unconverged + 1) +
              " (the coefficients returned there are the last pass's)");
  return GBM_OK;
}
