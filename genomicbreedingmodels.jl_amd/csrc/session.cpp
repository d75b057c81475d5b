// Device-resident genotype sessions: fold farming for cross-validation (SURVEY.md §8f row 1,
// config C5) and REML choice of λ (§8f row 2).
//
// A session uploads X once to one device (locus-major, individuals contiguous) and then fits
// GBLUP on entry subsets: the training columns are gathered on the device inside the
// standardisation pass, and the standardised training genotypes + their GRM are cached, keyed by
// the training set, so further traits, λ values or REML evaluations on the same set skip the
// SYRK. This replaces the per-fold `model(genomes=..., idx_entries=idx_training, ...)` calls of
// reference src/cross_validation.jl:159-186 (cvmultithread!), which re-extract X and rebuild
// everything per fold. One session per device; a session serialises its own calls (mutex),
// sessions on different devices run concurrently (one host thread each).
//
// This file: the life cycle, the training-set cache and the steps on it that the analyses share (session.h),
// the GBLUP fit and predict.
#include <cmath>
#include <cstring>
#include <memory>

#include "session.h"

namespace gbm {
namespace {

int session_alloc_x(gbm_session* s) {
  GBM_HIP_TRY(hipSetDevice(s->dev));
  s->stream.dev = s->dev;
  GBM_HIP_TRY(hipStreamCreateWithFlags(&s->stream.s, hipStreamNonBlocking));
  s->npad = npad_of(s->n);
  GBM_TRY(ensure(s->Xt, s->dev, s->p * s->npad * 8));
  GBM_HIP_TRY(hipMemsetAsync(s->Xt.p, 0, (size_t)(s->p * s->npad * 8), s->stream.s));
  return GBM_OK;
}

// The frame of the three create entries: a session on `device` with X allocated and zeroed, then filled by
// fill(s); a failure of either frees the session and is the entry's error.
template <class Fill>
int session_create(int64_t n, int64_t p, int device, gbm_session** out, Fill&& fill) {
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  auto s = std::make_unique<gbm_session>();
  s->dev = devs[0];
  s->n = n;
  s->p = p;
  GBM_TRY(session_alloc_x(s.get()));
  GBM_TRY(fill(s.get()));
  *out = s.release();
  return GBM_OK;
}

// Whether the session's genotypes are diploid dosages/2 (one device pass over X, the first time it is asked).
int session_dosage2(gbm_session* s, bool& out) {
  if (!s->dosage_checked) {
    GBM_TRY(ensure(s->q2, s->dev, 8));
    GBM_HIP_TRY(hipMemsetAsync(s->q2.p, 0, 4, s->stream.s));
    GBM_TRY(launch_dosage_from_f64(s->Xt.as<const double>(), s->npad, s->n, s->p, nullptr, 0, s->q2.as<int32_t>(),
                                   s->stream.s));
    int32_t bad = 0;
    GBM_HIP_TRY(hipMemcpyAsync(&bad, s->q2.p, 4, hipMemcpyDeviceToHost, s->stream.s));
    GBM_HIP_TRY(hipStreamSynchronize(s->stream.s));
    s->dosage2 = bad == 0;
    s->dosage_checked = true;
  }
  out = s->dosage2;
  return GBM_OK;
}

}  // namespace

int check_idx(const gbm_session* s, const int64_t* idx, int64_t m, const char* what) {
  if (!idx || m < 1) return fail(GBM_E_ARG, std::string(what) + ": empty entry index");
  for (int64_t i = 0; i < m; i++) {
    if (idx[i] < 0 || idx[i] >= s->n)
      return fail(GBM_E_ARG, std::string(what) + ": entry index " + std::to_string(idx[i]) + " out of range [0, " +
                                 std::to_string(s->n) + ")");
    if (i > 0 && idx[i] <= idx[i - 1])
      return fail(GBM_E_ARG, std::string(what) + ": entry indices must be strictly increasing");
  }
  return GBM_OK;
}

int ensure_training(gbm_session* s, const int64_t* idx, int64_t nT, int mode) {
  GBM_TRY(check_idx(s, idx, nT, "gbm_session"));
  if (nT < 2) return fail(GBM_E_DATA, "there are less than 2 entries (reference src/prediction.jl:117-123)");
  bool exact = false;
  const int gm = resolve_grm_mode(s->grm_mode);
  if (mode == 0 && gm != GBM_GRM_FP64) {
    GBM_TRY(session_dosage2(s, exact));
    if (!exact && gm == GBM_GRM_EXACT)
      return fail(GBM_E_ARG, "grm_mode exact: the session's genotypes are not diploid dosages (2x must be exactly 0, "
                             "1 or 2 in every cell; use grm_mode auto or fp64)");
  }
  if (s->mode == mode && s->exact_cached == exact && (int64_t)s->key.size() == nT &&
      std::memcmp(s->key.data(), idx, (size_t)nT * 8) == 0) {
    s->hits++;
    return GBM_OK;
  }
  s->key.clear();
  hipStream_t st = s->stream.s;
  const int dev = s->dev;
  const int64_t p = s->p, npadT = npad_of(nT), gdimT = gdim_of(nT), wsb = gbm_dev_grm_workspace(nT, p);
  s->npadT = npadT;
  s->gdimT = gdimT;
  GBM_TRY(ensure(s->Z, dev, p * npadT * 8));
  for (DevBuf* g : {&s->Gc, &s->Gw}) GBM_TRY(ensure(*g, dev, gdimT * gdimT * 8));
  GBM_TRY(ensure(s->wss, dev, gbm_dev_solve_workspace(nT, 63)));
  for (DevBuf* b : {&s->mean, &s->sd}) GBM_TRY(ensure(*b, dev, p * 8));
  GBM_TRY(ensure(s->keep, dev, p * 4));
  GBM_TRY(ensure(s->qd, dev, 8));
  GBM_TRY(ensure(s->idx32, dev, nT * 4));
  GBM_TRY(ensure(s->wsg, dev, wsb));
  std::vector<int32_t> i32(idx, idx + nT);
  GBM_HIP_TRY(hipMemcpyAsync(s->idx32.p, i32.data(), nT * 4, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemsetAsync(s->qd.p, 0, 8, st));
  GBM_TRY(gbm_dev_standardize_gather(s->Xt.as<const double>(), s->npad, p, s->idx32.as<const int32_t>(), nT,
                                     s->Z.as<double>(), npadT, s->mean.as<double>(), s->sd.as<double>(),
                                     s->keep.as<int32_t>(), s->qd.as<int64_t>(), mode, st));
  int64_t q = 0;
  GBM_HIP_TRY(hipMemcpyAsync(&q, s->qd.p, 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  if (q == 0) return fail(GBM_E_DATA, "no polymorphic locus-allele in the training set (src/gwas.jl:112-115)");
  if (exact) {
    // exact-integer GRM of the training dosages; its per-locus statistics go to scratch (Z, mean and sd
    // above are what the marker effects and predictions use; q is the same count)
    const int64_t wsx = gbm_dev_grm_exact_workspace(nT, p);
    GBM_TRY(ensure(s->D8T, dev, p * nT));
    GBM_TRY(ensure(s->wsx, dev, wsx));
    for (DevBuf* b : {&s->mean2, &s->sd2}) GBM_TRY(ensure(*b, dev, p * 8));
    GBM_TRY(ensure(s->keep2, dev, p * 4));
    GBM_TRY(ensure(s->q2, dev, 8));
    GBM_TRY(launch_gather_dosage(s->Xt.as<const double>(), s->npad, p, s->idx32.as<const int32_t>(), nT,
                                 s->D8T.as<int8_t>(), st));
    GBM_HIP_TRY(hipMemsetAsync(s->q2.p, 0, 8, st));
    GBM_TRY(launch_grm_exact(s->D8T.as<const int8_t>(), nT, p, nT, 2, s->Gc.as<double>(), gdimT, s->mean2.as<double>(),
                             s->sd2.as<double>(), s->keep2.as<int32_t>(), s->q2.as<int64_t>(), 0, s->wsx.p, wsx, nullptr,
                             st));
    GBM_TRY(grm_exact_status(s->wsx.p, nT, p, st));
  } else {
    GBM_TRY(gbm_dev_grm(s->Z.as<const double>(), npadT, p, nT, s->Gc.as<double>(), gdimT, s->wsg.p, wsb, st));
  }
  s->nT = nT;
  s->q = q;
  s->key.assign(idx, idx + nT);
  s->mode = mode;
  s->exact_cached = exact;
  s->builds++;
  return GBM_OK;
}

int ensure_rhs(gbm_session* s, int64_t nrhs) {
  for (DevBuf* b : {&s->Y, &s->A, &s->gebv}) GBM_TRY(ensure(*b, s->dev, nrhs * s->npadT * 8));
  for (DevBuf* b : {&s->mu_d, &s->msum}) GBM_TRY(ensure(*b, s->dev, nrhs * 8));
  GBM_TRY(ensure(s->info, s->dev, 4));
  GBM_TRY(ensure(s->B, s->dev, nrhs * s->p * 8));
  GBM_TRY(ensure(s->terms, s->dev, (2 + 2 * nrhs) * 8));
  return GBM_OK;
}

int upload_y(gbm_session* s, const double* Y, int64_t ldy, int64_t nrhs) {
  GBM_HIP_TRY(hipMemsetAsync(s->Y.p, 0, (size_t)(nrhs * s->npadT * 8), s->stream.s));
  GBM_HIP_TRY(hipMemcpy2DAsync(s->Y.p, s->npadT * 8, Y, ldy * 8, s->nT * 8, nrhs, hipMemcpyHostToDevice, s->stream.s));
  return GBM_OK;
}

int solve_cached(gbm_session* s, int64_t nrhs, double lambda, double inv_q) {
  hipStream_t st = s->stream.s;
  // the solve factors in place: work on a copy of the cached GRM (rows [0, npad) are read)
  GBM_HIP_TRY(hipMemcpyAsync(s->Gw.p, s->Gc.p, (size_t)(s->npadT * s->gdimT * 8), hipMemcpyDeviceToDevice, st));
  GBM_TRY(gbm_dev_gblup_solve(s->Gw.as<double>(), s->gdimT, s->nT, inv_q, nullptr, lambda, s->Y.as<const double>(),
                              s->npadT, nrhs, s->A.as<double>(), s->gebv.as<double>(), s->npadT, s->mu_d.as<double>(),
                              s->info.as<int32_t>(), s->wss.p, gbm_dev_solve_workspace(s->nT, 63), st));
  int32_t info = 0;
  GBM_HIP_TRY(hipMemcpyAsync(&info, s->info.p, 4, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  if (info < 0) return fail(GBM_E_HIP, "solve: a wait between workgroups timed out (dataflow Cholesky or back substitution; the result is invalid)");
  if (info != 0)
    return fail(GBM_E_NOTPD, "G/q + lambda*I is not positive definite (pivot " + std::to_string(info) + ")");
  return GBM_OK;
}

int effects_cached(gbm_session* s, const double* A, int64_t lda, int64_t nrhs, double inv_q) {
  return gbm_dev_marker_effects(s->Z.as<const double>(), s->npadT, s->p, s->nT, A, lda, nrhs, inv_q, nullptr,
                                s->mean.as<const double>(), s->sd.as<const double>(), s->keep.as<const int32_t>(),
                                s->B.as<double>(), s->p, s->msum.as<double>(), s->stream.s);
}

int predict_at(gbm_session* s, const double* b, int64_t ldb, const double* b_dev, int64_t nrhs, const int64_t* idx,
               int64_t m, double* out, int64_t ldo) {
  hipStream_t st = s->stream.s;
  const int64_t p = s->p, n = s->n, npad = s->npad, nchunks = predict_chunks(n, p);
  GBM_TRY(ensure(s->bvec, s->dev, nrhs * (p + 1) * 8));
  GBM_TRY(ensure(s->part, s->dev, nchunks * nrhs * npad * 8));
  GBM_TRY(ensure(s->pout, s->dev, nrhs * npad * 8));
  if (b_dev) {
    GBM_HIP_TRY(hipMemcpyAsync(s->bvec.p, b, 8, hipMemcpyHostToDevice, st));
    GBM_HIP_TRY(hipMemcpyAsync(s->bvec.as<double>() + 1, b_dev, p * 8, hipMemcpyDeviceToDevice, st));
  } else {
    GBM_HIP_TRY(hipMemcpy2DAsync(s->bvec.p, (p + 1) * 8, b, ldb * 8, (p + 1) * 8, nrhs, hipMemcpyHostToDevice, st));
  }
  GBM_TRY(launch_predict(s->Xt.as<const double>(), npad, p, n, s->bvec.as<const double>(), p + 1, nrhs,
                         s->part.as<double>(), nchunks, s->pout.as<double>(), npad, st));
  std::vector<double> all(nrhs * npad);
  GBM_HIP_TRY(hipMemcpyAsync(all.data(), s->pout.p, nrhs * npad * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  for (int64_t t = 0; t < nrhs; t++)
    for (int64_t i = 0; i < m; i++) out[t * ldo + i] = all[t * npad + idx[i]];
  return GBM_OK;
}

YStats centre_y(const double* y, int64_t n) {
  double m = 0.0, ss = 0.0;
  for (int64_t i = 0; i < n; i++) m += y[i];
  m /= (double)n;
  for (int64_t i = 0; i < n; i++) ss += (y[i] - m) * (y[i] - m);
  return {m, ss, std::sqrt(ss / (double)n)};
}

}  // namespace gbm

using namespace gbm;

extern "C" int gbm_session_create(const double* X, int64_t n, int64_t p, int64_t ldx, int device, gbm_session** out) {
  RoctxRange r_("gbm_session_create");
  if (!out) return fail(GBM_E_ARG, "gbm_session_create: out is NULL");
  *out = nullptr;
  if (!X || n < 1 || p < 1 || ldx < n) return fail(GBM_E_ARG, "gbm_session_create: bad arguments");
  return session_create(n, p, device, out, [&](gbm_session* s) {
    if (hipMemcpy2DAsync(s->Xt.p, s->npad * 8, X, ldx * 8, n * 8, p, hipMemcpyHostToDevice, s->stream.s) !=
            hipSuccess ||
        hipStreamSynchronize(s->stream.s) != hipSuccess)
      return fail(GBM_E_HIP, "gbm_session_create: upload failed");
    return GBM_OK;
  });
}

extern "C" int gbm_session_create_synthetic(uint64_t seed, int64_t n, int64_t p, int device, gbm_session** out) {
  RoctxRange r_("gbm_session_create_synthetic");
  if (!out) return fail(GBM_E_ARG, "gbm_session_create_synthetic: out is NULL");
  *out = nullptr;
  if (n < 1 || p < 1) return fail(GBM_E_ARG, "gbm_session_create_synthetic: bad arguments");
  return session_create(n, p, device, out, [&](gbm_session* s) {
    GBM_TRY(gbm_dev_synth_genotypes(s->Xt.as<double>(), s->npad, p, n, seed, 0, s->stream.s));
    s->dosage2 = s->dosage_checked = true;  // X = dosage/2 (SURVEY.md §8d generator)
    if (hipStreamSynchronize(s->stream.s) != hipSuccess)
      return fail(GBM_E_HIP, "gbm_session_create_synthetic: generation failed");
    return GBM_OK;
  });
}

extern "C" int gbm_session_create_dosage_i8(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy,
                                            int device, gbm_session** out) {
  RoctxRange r_("gbm_session_create_dosage_i8");
  if (!out) return fail(GBM_E_ARG, "gbm_session_create_dosage_i8: out is NULL");
  *out = nullptr;
  if (!D || n < 1 || p < 1 || ldd < n || ploidy < 1)
    return fail(GBM_E_ARG, "gbm_session_create_dosage_i8: bad arguments");
  return session_create(n, p, device, out, [&](gbm_session* s) {
    DevMem d8;
    GBM_TRY(dalloc(d8, s->dev, n * p));
    if (hipMemcpy2DAsync(d8.p, n, D, ldd, n, p, hipMemcpyHostToDevice, s->stream.s) != hipSuccess)
      return fail(GBM_E_HIP, "gbm_session_create_dosage_i8: upload failed");
    GBM_TRY(gbm_dev_expand_dosage_i8(d8.as<const int8_t>(), n, n, p, ploidy, s->Xt.as<double>(), s->npad, s->stream.s));
    if (hipStreamSynchronize(s->stream.s) != hipSuccess) return fail(GBM_E_HIP, "stream sync");
    return GBM_OK;
  });
}

extern "C" int gbm_session_set_grm_mode(gbm_session* s, int grm_mode) {
  if (!s) return fail(GBM_E_ARG, "gbm_session_set_grm_mode: session is NULL");
  if (grm_mode < GBM_GRM_DEFAULT || grm_mode > GBM_GRM_DROPIN)
    return fail(GBM_E_ARG, "gbm_session_set_grm_mode: grm_mode must be GBM_GRM_DEFAULT, _FP64, _EXACT, _AUTO or _DROPIN");
  std::lock_guard<std::mutex> lock(s->mu);
  s->grm_mode = grm_mode;
  return GBM_OK;
}

extern "C" int gbm_session_grm_used(gbm_session* s, int* grm_used) {
  if (!s || !grm_used) return fail(GBM_E_ARG, "gbm_session_grm_used: NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  *grm_used = s->key.empty() ? -1 : s->exact_cached ? GBM_GRM_EXACT : GBM_GRM_FP64;
  return GBM_OK;
}

extern "C" void gbm_session_destroy(gbm_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->dev);
  delete s;
}

extern "C" int gbm_session_stats(gbm_session* s, int64_t* grm_builds, int64_t* grm_hits) {
  if (!s) return fail(GBM_E_ARG, "gbm_session_stats: session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  if (grm_builds) *grm_builds = s->builds;
  if (grm_hits) *grm_hits = s->hits;
  return GBM_OK;
}

extern "C" int gbm_session_gblup_fit(gbm_session* s, const int64_t* idx, int64_t n_train, const double* Y, int64_t ldy,
                                     int64_t nrhs, double lambda, double* b_hat_out, double* y_pred_out, double* mu_out,
                                     int64_t* q_out) {
  RoctxRange r_("gbm_session_gblup_fit");
  if (!s) return fail(GBM_E_ARG, "gbm_session_gblup_fit: session is NULL");
  if (!Y || ldy < n_train || nrhs < 1 || nrhs > 63 || !b_hat_out || !y_pred_out)
    return fail(GBM_E_ARG, "gbm_session_gblup_fit: bad arguments (ldy >= n_train, 1 <= nrhs <= 63, outputs)");
  if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(GBM_E_ARG, "gbm_session_gblup_fit: lambda must be > 0");
  GBM_SESSION_ENTER(s);
  GBM_TRY(check_y(Y, n_train, ldy, nrhs));
  GBM_TRY(ensure_training(s, idx, n_train));
  GBM_TRY(ensure_rhs(s, nrhs));
  GBM_TRY(upload_y(s, Y, ldy, nrhs));
  GBM_TRY(solve_cached(s, nrhs, lambda, 1.0 / (double)s->q));
  hipStream_t st = s->stream.s;
  const int64_t p = s->p;
  GBM_TRY(effects_cached(s, s->A.as<const double>(), s->npadT, nrhs, 1.0 / (double)s->q));
  std::vector<double> mu(nrhs), msum(nrhs);
  GBM_HIP_TRY(hipMemcpy2DAsync(b_hat_out + 1, (p + 1) * 8, s->B.p, p * 8, p * 8, nrhs, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipMemcpy2DAsync(y_pred_out, n_train * 8, s->gebv.p, s->npadT * 8, n_train * 8, nrhs,
                               hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipMemcpyAsync(mu.data(), s->mu_d.p, nrhs * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipMemcpyAsync(msum.data(), s->msum.p, nrhs * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  for (int64_t t = 0; t < nrhs; t++) {
    b_hat_out[t * (p + 1)] = mu[t] - msum[t];
    if (mu_out) mu_out[t] = mu[t];
  }
  if (q_out) *q_out = s->q;
  return GBM_OK;
}

extern "C" int gbm_session_predict(gbm_session* s, const int64_t* idx, int64_t n_val, const double* b_hat, int64_t ldb,
                                   int64_t nrhs, double* out, int64_t ldo) {
  RoctxRange r_("gbm_session_predict");
  if (!s) return fail(GBM_E_ARG, "gbm_session_predict: session is NULL");
  if (!b_hat || ldb < s->p + 1 || nrhs < 1 || !out || ldo < n_val)
    return fail(GBM_E_ARG, "gbm_session_predict: bad arguments");
  GBM_SESSION_ENTER(s);
  GBM_TRY(check_idx(s, idx, n_val, "gbm_session_predict"));
  return predict_at(s, b_hat, ldb, nullptr, nrhs, idx, n_val, out, ldo);
}
