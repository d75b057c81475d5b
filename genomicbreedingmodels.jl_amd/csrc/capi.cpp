// Host entry points of libgbm.so (include/gbm.h): the thread-local error state, argument checks,
// H2D/D2H and run_fit, which shards the SNP columns over the devices' pooled fit contexts
// (fit_ctx.h), builds each shard's partial GRM (shard_grm.cpp), sums them and solves
// (dist_solve.cpp) and downloads the marker effects.
#include <cmath>

#include "fit_ctx.h"

namespace gbm {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
const std::string& last_error() { return g_last_error; }

int resolve_grm_mode(int grm_mode) {
  if (grm_mode != GBM_GRM_DEFAULT && grm_mode != GBM_GRM_DROPIN) return grm_mode;
  const char* e = ::gbm::knob("GBM_GRM");
  if (e && strcmp(e, "exact") == 0) return GBM_GRM_EXACT;
  if (e && strcmp(e, "auto") == 0) return GBM_GRM_AUTO;
  if (e && strcmp(e, "fp64") == 0) return GBM_GRM_FP64;
  return grm_mode == GBM_GRM_DROPIN ? GBM_GRM_AUTO : GBM_GRM_FP64;
}

namespace {

// Solve + marker effects for the traits [t0, t0 + nt) of Y at one λ on the summed G of every device
// leader (factored in place), into the caller's output columns of those traits.
int solve_effects(const Problem& pr, Shards& shards, const std::vector<int>& leaders,
                  const std::vector<int>& ldevs, int64_t q, const double* Y, int64_t ldy, int64_t t0, int64_t nt,
                  double lambda, double* b_hat_out, double* y_pred_out, double* mu_out) {
  const int64_t n = pr.n, p = pr.p, npad = npad_of(n), gdim = gdim_of(n);
  const double inv_q = 1.0 / (double)q;
  // Below GBM_DIST_SOLVE_MIN_N individuals (default 16384, re-read per call; the knob of
  // gbm.sharded.dist_solve_min_n) each device leader solves the (identical) n x n system, all
  // devices at once; from there the leaders factor it together (solve_distributed). Either way a
  // ends up on every leader for the marker back-solve (same-device shards copy it from theirs).
  const bool distributed = (leaders.size() > 1 || force_rccl()) && n >= knob_i64("GBM_DIST_SOLVE_MIN_N", 16384);
  std::vector<int32_t> infos(shards.size(), 0);
  {
    RoctxRange rsolve(distributed ? "gbm: distributed solve" : "gbm: solve");
    for (size_t k = 0; k < shards.size(); k++) {
      Shard& sh = *shards[k];
      FitCtx& c = sh.x();
      GBM_HIP_TRY(hipSetDevice(c.dev));
      hipStream_t s = c.stream.s;
      GBM_TRY(ensure(c.A, c.dev, nt * npad * 8));
      GBM_TRY(ensure(c.B, c.dev, nt * sh.p * 8));
      GBM_TRY(ensure(c.msum, c.dev, nt * 8));
      if (sh.leader != (int)k) continue;
      GBM_TRY(ensure(c.Y, c.dev, nt * npad * 8));
      GBM_TRY(ensure(c.gebv, c.dev, nt * npad * 8));
      GBM_TRY(ensure(c.mu, c.dev, nt * 8));
      GBM_TRY(ensure(c.info, c.dev, 4));
      const int64_t wss = gbm_dev_solve_workspace(n, nt);
      GBM_TRY(ensure(c.wss, c.dev, wss));
      GBM_HIP_TRY(hipMemcpy2DAsync(c.Y.p, npad * 8, Y + t0 * ldy, ldy * 8, n * 8, nt, hipMemcpyHostToDevice, s));
      if (!distributed)
        GBM_TRY(gbm_dev_gblup_solve((double*)c.G.p, gdim, n, inv_q, nullptr, lambda, (const double*)c.Y.p, npad, nt,
                                    (double*)c.A.p, (double*)c.gebv.p, npad, (double*)c.mu.p, (int32_t*)c.info.p,
                                    c.wss.p, wss, s));
    }
    if (distributed) GBM_TRY(solve_distributed(shards, leaders, ldevs, n, inv_q, lambda, nt));
    for (int k : leaders) {
      FitCtx& c = shards[k]->x();
      GBM_HIP_TRY(hipSetDevice(c.dev));
      GBM_HIP_TRY(hipMemcpyAsync(&infos[k], c.info.p, 4, hipMemcpyDeviceToHost, c.stream.s));
    }
    for (int k : leaders) {
      FitCtx& c = shards[k]->x();
      GBM_HIP_TRY(hipSetDevice(c.dev));
      GBM_HIP_TRY(hipStreamSynchronize(c.stream.s));
      const int32_t info = infos[k];
      if (info < 0) return fail(GBM_E_HIP, "solve: a wait between workgroups timed out (dataflow Cholesky or back substitution; the result is invalid)");
      if (info != 0)
        return fail(GBM_E_NOTPD, "G/q + lambda*I is not positive definite (pivot " + std::to_string(info) +
                                     "); check for non-finite genotypes");
    }
  }
  RoctxRange reff("gbm: marker effects + download");
  std::vector<std::vector<double>> msums(shards.size(), std::vector<double>(nt, 0.0));
  std::vector<double> mu(nt, 0.0);
  double* bo = b_hat_out + t0 * (p + 1);
  for (size_t k = 0; k < shards.size(); k++) {
    Shard& sh = *shards[k];
    FitCtx& c = sh.x();
    GBM_HIP_TRY(hipSetDevice(c.dev));
    hipStream_t s = c.stream.s;
    if (sh.leader != (int)k)
      GBM_HIP_TRY(hipMemcpyAsync(c.A.p, shards[sh.leader]->x().A.p, nt * npad * 8, hipMemcpyDeviceToDevice, s));
    if (sh.stream || sh.exact)
      GBM_TRY(stream_effects_shard(pr, sh, nt, inv_q));
    else
      GBM_TRY(gbm_dev_marker_effects((const double*)c.Xt.p, npad, sh.p, n, (const double*)c.A.p, npad, nt, inv_q,
                                     nullptr, (const double*)c.mean.p, (const double*)c.sd.p, (const int32_t*)c.keep.p,
                                     (double*)c.B.p, sh.p, (double*)c.msum.p, s));
    GBM_HIP_TRY(hipMemcpy2DAsync(bo + 1 + sh.j0, (p + 1) * 8, c.B.p, sh.p * 8, sh.p * 8, nt, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipMemcpyAsync(msums[k].data(), c.msum.p, nt * 8, hipMemcpyDeviceToHost, s));
    if (k == 0) {
      GBM_HIP_TRY(hipMemcpy2DAsync(y_pred_out + t0 * n, n * 8, c.gebv.p, npad * 8, n * 8, nt, hipMemcpyDeviceToHost, s));
      GBM_HIP_TRY(hipMemcpyAsync(mu.data(), c.mu.p, nt * 8, hipMemcpyDeviceToHost, s));
    }
  }
  std::vector<double> msum_total(nt, 0.0);
  for (size_t k = 0; k < shards.size(); k++) {
    GBM_HIP_TRY(hipSetDevice(shards[k]->x().dev));
    GBM_HIP_TRY(hipStreamSynchronize(shards[k]->x().stream.s));
    for (int64_t t = 0; t < nt; t++) msum_total[t] += msums[k][t];  // shard order: deterministic
  }
  for (int64_t t = 0; t < nt; t++) {
    bo[t * (p + 1)] = mu[t] - msum_total[t];
    if (mu_out) mu_out[t0 + t] = mu[t];
  }
  return GBM_OK;
}

// REML outputs of gbm_gblup_fit_reml (per trait; any may be NULL)
struct RemlOut {
  double* lambda;
  double* s2e;
  double* s2u;
};

// REML λ of trait column y on device leader `c`: each evaluation restores the summed G from its
// pristine copy Gc, solves at λ for the standardised y (one right-hand side) and reads the
// loglikreml terms off the bordered factorisation (as gbm_session_reml does on its cached GRM).
int reml_lambda(FitCtx& c, int64_t n, int64_t q, const double* y, RemlResult& res) {
  const int64_t npad = npad_of(n), gdim = gdim_of(n);
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  const int64_t wss = gbm_dev_solve_workspace(n, 1);
  GBM_TRY(ensure(c.Y, c.dev, npad * 8));
  GBM_TRY(ensure(c.A, c.dev, npad * 8));
  GBM_TRY(ensure(c.gebv, c.dev, npad * 8));
  GBM_TRY(ensure(c.mu, c.dev, 8));
  GBM_TRY(ensure(c.info, c.dev, 4));
  GBM_TRY(ensure(c.wss, c.dev, wss));
  GBM_TRY(ensure(c.tmp, c.dev, 4 * 8));
  const std::vector<double> ys = standardise_y(y, n);
  GBM_HIP_TRY(hipMemsetAsync(c.Y.p, 0, (size_t)(npad * 8), s));
  GBM_HIP_TRY(hipMemcpyAsync(c.Y.p, ys.data(), n * 8, hipMemcpyHostToDevice, s));
  auto eval = [&](double lambda, RemlEval& e) -> int {
    GBM_HIP_TRY(hipMemcpyAsync(c.G.p, c.Gc.p, (size_t)(npad * gdim * 8), hipMemcpyDeviceToDevice, s));
    GBM_TRY(gbm_dev_gblup_solve((double*)c.G.p, gdim, n, 1.0 / (double)q, nullptr, lambda, (const double*)c.Y.p, npad,
                                1, (double*)c.A.p, (double*)c.gebv.p, npad, (double*)c.mu.p, (int32_t*)c.info.p, c.wss.p,
                                wss, s));
    GBM_TRY(gbm_dev_gblup_terms((const double*)c.G.p, gdim, n, 1, c.wss.p, (double*)c.tmp.p, s));
    double t[4];
    int32_t info = 0;
    GBM_HIP_TRY(hipMemcpyAsync(t, c.tmp.p, 4 * 8, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipMemcpyAsync(&info, c.info.p, 4, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
    if (info < 0) return fail(GBM_E_HIP, "solve: a wait between workgroups timed out (dataflow Cholesky or back substitution; the result is invalid)");
    if (info != 0) return fail(GBM_E_NOTPD, "REML: G/q + lambda*I is not positive definite (pivot " + std::to_string(info) + ")");
    e = reml_profile(n, lambda, t);
    return GBM_OK;
  };
  return reml_search(eval, res);
}

int run_fit(const Problem& pr, const double* Y, int64_t ldy, int64_t nrhs, double lambda, const int* devices, int ndev,
            double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out, const RemlOut* reml = nullptr,
            int grm_mode = GBM_GRM_DEFAULT, int* grm_used_out = nullptr) {
  const int64_t n = pr.n, p = pr.p;
  if (n < 2) return fail(GBM_E_DATA, "there are less than 2 entries (reference src/prediction.jl:117-123)");
  if (p < 1 || pr.ld < n || !Y || ldy < n || nrhs < 1 || nrhs > 63 || !b_hat_out || !y_pred_out)
    return fail(GBM_E_ARG, "gbm_gblup_fit: bad arguments (need p >= 1, ldx >= n, ldy >= n, 1 <= nrhs <= 63, outputs)");
  if (!reml && (!(lambda > 0.0) || !std::isfinite(lambda)))
    return fail(GBM_E_ARG, "gbm_gblup_fit: lambda must be finite and > 0");
  if (reml && n < 3) return fail(GBM_E_DATA, "REML needs at least 3 entries");
  GBM_TRY(check_y(Y, n, ldy, nrhs));
  const int mode = resolve_grm_mode(grm_mode);
  if (mode != GBM_GRM_FP64 && mode != GBM_GRM_EXACT && mode != GBM_GRM_AUTO)
    return fail(GBM_E_ARG, "grm_mode must be GBM_GRM_DEFAULT, GBM_GRM_FP64, GBM_GRM_EXACT or GBM_GRM_AUTO (GBM_GRM: fp64 | exact | auto)");
  if (mode == GBM_GRM_EXACT && pr.src == Source::I8 && pr.ploidy != 2)
    return fail(GBM_E_ARG, "grm_mode exact: the exact-integer GRM needs diploid dosages (ploidy 2)");
  std::vector<int> devs;
  GBM_TRY(check_devices(devices, ndev, devs));
  const int64_t npad = npad_of(n), gdim = gdim_of(n);
  Shards shards;
  GBM_TRY(make_shards(devs, p, shards));
  int64_t q = 0, pmax = 0;
  for (auto& sh : shards) pmax = std::max(pmax, sh->p);
  const int64_t chunk = pr.src == Source::SYNTH ? 0 : host_chunk(pmax);
  // exact: every shard's dosages resident as bytes, nothing to stream; auto: the same unless the genotypes
  // turn out not to be diploid dosages (2x outside {0, 1, 2}, int8 ploidy != 2), then the fp64 path
  bool exact = mode != GBM_GRM_FP64 && !(pr.src == Source::I8 && pr.ploidy != 2);
  // GBM_HOST_PACK (default 1): fp64 host X crosses PCIe as dosage bytes packed on the host, the threads shared by the shards
  const bool host_pack = knob_i64("GBM_HOST_PACK", 1) != 0;
  const int pack_threads = std::max(1, host_pack_threads() / (int)shards.size());
  auto fp64_grm = [&]() -> int {
    GBM_TRY(plan_streaming(pr, shards, reml != nullptr));
    // each shard's GRM is launched behind its own standardisation (a shard without polymorphic
    // loci contributes a zero partial; q == 0 over all shards fails below): streamed when its
    // rows do not fit, else resident (host chunks pipelined with the GRM, or in one piece)
    // fp64 host X with grm_mode fp64: tried as dosages packed on the host first; X that is not dosage-valued
    // falls back to the fp64 upload at its first non-dosage chunk
    const bool pack = mode == GBM_GRM_FP64 && pr.src == Source::F64 && host_pack;
    return parallel_shards(shards, [&](size_t, Shard& sh) {
      if (sh.stream) return stream_grm_shard(pr, sh);
      if (chunk > 0) {
        if (pack) {
          const int rc = upload_grm_pipelined_packed(pr, sh, chunk, pack_threads);
          if (rc != kNotDosage) return rc;
        }
        return upload_grm_pipelined(pr, sh, chunk);
      }
      return prepare_grm_shard(pr, sh);
    });
  };
  {
    RoctxRange r("gbm: upload + standardise + GRM");
    if (exact) {
      for (auto& sh : shards) sh->exact = true;
      // fp64 host X: packed to dosage bytes on the host, or (GBM_HOST_PACK=0) converted on the device from
      // uploaded fp64 chunks
      const int rc = parallel_shards(shards, [&](size_t, Shard& sh) {
        if (pr.src == Source::F64) {
          if (host_pack)
            GBM_TRY(host_pack_upload_shard(pr, sh, pack_threads));
          else
            GBM_TRY(dosage_upload_shard(pr, sh, mode == GBM_GRM_AUTO));
        }
        return exact_grm_shard(pr, sh, mode == GBM_GRM_AUTO && pr.src == Source::I8);
      });
      if (rc == kNotDosage && mode == GBM_GRM_EXACT)
        return fail(GBM_E_ARG, "grm_mode exact: the genotypes are not diploid dosages (2x must be exactly 0, 1 or 2 "
                               "in every cell; use grm_mode auto or fp64)");
      // auto: data that is not dosage-valued, and the exact path's own limits (out of memory for the resident
      // bytes and staging, the 128-bit bracket's range: GBM_E_OOM / GBM_E_ARG), fall back to the fp64 path
      const bool fallback = mode == GBM_GRM_AUTO && (rc == kNotDosage || rc == GBM_E_OOM || rc == GBM_E_ARG);
      if (fallback) {
        exact = false;
        for (auto& sh : shards) {
          sh->exact = sh->d8_ready = false;
          // the fp64 path of fp64 genotypes never reads D8: free it, so plan_streaming sees the memory (a
          // dosage source keeps it: its fp64 path refills D8)
          FitCtx& c = sh->x();
          if (pr.src == Source::F64 && c.D8.p) {
            (void)hipSetDevice(c.dev);
            c.D8.reset();
            c.D8.cap = 0;
          }
        }
        set_error("");
      } else {
        GBM_TRY(rc);
      }
    }
    if (!exact) GBM_TRY(fp64_grm());
  }
  if (grm_used_out) *grm_used_out = exact ? GBM_GRM_EXACT : GBM_GRM_FP64;
  for (auto& sh : shards) q += sh->q_host;
  if (q_out) *q_out = q;
  if (q == 0) return fail(GBM_E_DATA, "no polymorphic locus-allele (all standard deviations <= eps, src/gwas.jl:112-115)");
  {
    RoctxRange r("gbm: partial-GRM all-reduce");
    GBM_TRY(allreduce_grm(shards, n));
  }
  std::vector<int> leaders, ldevs;
  shard_leaders(shards, leaders, ldevs);
  if (!reml) return solve_effects(pr, shards, leaders, ldevs, q, Y, ldy, 0, nrhs, lambda, b_hat_out, y_pred_out, mu_out);
  // REML (gbm_gblup_fit_reml): λ per trait chosen on the first leader's summed G, kept pristine in
  // that leader's Gc only (each solve factors G in place; every leader restores its G from it:
  // one extra n x n buffer per call, not per leader — 20 GB per device at C3); then one solve +
  // effects per trait at its λ.
  const int64_t vbytes = npad * gdim * 8;  // rows [0, npad) of G: everything a solve reads of it
  FitCtx& c0 = shards[leaders[0]]->x();
  GBM_HIP_TRY(hipSetDevice(c0.dev));
  GBM_TRY(ensure(c0.Gc, c0.dev, gdim * gdim * 8));
  GBM_HIP_TRY(hipMemcpyAsync(c0.Gc.p, c0.G.p, (size_t)vbytes, hipMemcpyDeviceToDevice, c0.stream.s));
  std::vector<double> lam(nrhs);
  {
    RoctxRange r("gbm: REML lambda");
    for (int64_t t = 0; t < nrhs; t++) {
      RemlResult res;
      GBM_TRY(reml_lambda(shards[leaders[0]]->x(), n, q, Y + t * ldy, res));
      lam[t] = res.lambda;
      if (reml->lambda) reml->lambda[t] = res.lambda;
      if (reml->s2e) reml->s2e[t] = res.s2e;
      if (reml->s2u) reml->s2u[t] = res.s2u;
    }
  }
  GBM_HIP_TRY(hipSetDevice(c0.dev));
  GBM_HIP_TRY(hipStreamSynchronize(c0.stream.s));  // Gc complete before other leaders' streams read it
  for (int64_t t = 0; t < nrhs; t++) {
    for (int k : leaders) {
      FitCtx& c = shards[k]->x();
      GBM_TRY(copy_dd(c, c.G.p, c0, c0.Gc.p, vbytes));
    }
    GBM_TRY(solve_effects(pr, shards, leaders, ldevs, q, Y, ldy, t, 1, lam[t], b_hat_out, y_pred_out, mu_out));
  }
  return GBM_OK;
}

// scale · (the summed G of context c) into the caller's n x n G_out
int export_grm(FitCtx& c, int64_t n, double scale, double* G_out, int64_t ldg) {
  GBM_HIP_TRY(hipSetDevice(c.dev));
  GBM_TRY(ensure(c.out, c.dev, n * n * 8));
  GBM_TRY(launch_grm_export((const double*)c.G.p, gdim_of(n), n, scale, (double*)c.out.p, n, c.stream.s));
  GBM_HIP_TRY(hipMemcpy2DAsync(G_out, ldg * 8, c.out.p, n * 8, n * 8, n, hipMemcpyDeviceToHost, c.stream.s));
  GBM_HIP_TRY(hipStreamSynchronize(c.stream.s));
  return GBM_OK;
}

}  // namespace
}  // namespace gbm

using namespace gbm;

extern "C" int gbm_version(void) { return GBM_VERSION; }

extern "C" const char* gbm_last_error(void) { return g_last_error.c_str(); }

extern "C" int gbm_device_count(int* count) {
  if (!count) return fail(GBM_E_ARG, "gbm_device_count: NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *count = 0;
    return e == hipErrorNoDevice ? GBM_OK : fail(GBM_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return GBM_OK;
}

extern "C" int64_t gbm_device_allocations(void) { return alloc_counter().load(std::memory_order_relaxed); }

extern "C" int gbm_debug_oom_retries(int64_t* retries, int64_t* contexts_freed) {
  if (retries) *retries = oom_trim().retries.load();
  if (contexts_freed) *contexts_freed = oom_trim().freed.load();
  return GBM_OK;
}

extern "C" int gbm_release_device_cache(void) {
  pool().clear();
  brr_release_cache();
  return GBM_OK;
}

extern "C" int gbm_gblup_fit_ex(const double* X, int64_t n, int64_t p, int64_t ldx, const double* Y, int64_t ldy,
                                int64_t nrhs, double lambda, const int* devices, int ndev, int grm_mode,
                                double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out,
                                int* grm_used_out) {
  RoctxRange r_("gbm_gblup_fit");
  if (!X) return fail(GBM_E_ARG, "gbm_gblup_fit: X is NULL");
  Problem pr{Source::F64, X, nullptr, 1, n, p, ldx};
  return run_fit(pr, Y, ldy, nrhs, lambda, devices, ndev, b_hat_out, y_pred_out, mu_out, q_out, nullptr, grm_mode,
                 grm_used_out);
}

extern "C" int gbm_gblup_fit(const double* X, int64_t n, int64_t p, int64_t ldx, const double* Y, int64_t ldy,
                             int64_t nrhs, double lambda, const int* devices, int ndev, double* b_hat_out,
                             double* y_pred_out, double* mu_out, int64_t* q_out) {
  return gbm_gblup_fit_ex(X, n, p, ldx, Y, ldy, nrhs, lambda, devices, ndev, GBM_GRM_DEFAULT, b_hat_out, y_pred_out,
                          mu_out, q_out, nullptr);
}

extern "C" int gbm_gblup_fit_reml_ex(const double* X, int64_t n, int64_t p, int64_t ldx, const double* Y, int64_t ldy,
                                     int64_t nrhs, const int* devices, int ndev, int grm_mode, double* b_hat_out,
                                     double* y_pred_out, double* mu_out, int64_t* q_out, double* lambda_out,
                                     double* sigma2_e_out, double* sigma2_u_out, int* grm_used_out) {
  RoctxRange r_("gbm_gblup_fit_reml");
  if (!X) return fail(GBM_E_ARG, "gbm_gblup_fit_reml: X is NULL");
  Problem pr{Source::F64, X, nullptr, 1, n, p, ldx};
  const RemlOut ro{lambda_out, sigma2_e_out, sigma2_u_out};
  return run_fit(pr, Y, ldy, nrhs, 0.0, devices, ndev, b_hat_out, y_pred_out, mu_out, q_out, &ro, grm_mode,
                 grm_used_out);
}

extern "C" int gbm_gblup_fit_reml(const double* X, int64_t n, int64_t p, int64_t ldx, const double* Y, int64_t ldy,
                                  int64_t nrhs, const int* devices, int ndev, double* b_hat_out, double* y_pred_out,
                                  double* mu_out, int64_t* q_out, double* lambda_out, double* sigma2_e_out,
                                  double* sigma2_u_out) {
  return gbm_gblup_fit_reml_ex(X, n, p, ldx, Y, ldy, nrhs, devices, ndev, GBM_GRM_DEFAULT, b_hat_out, y_pred_out,
                               mu_out, q_out, lambda_out, sigma2_e_out, sigma2_u_out, nullptr);
}

extern "C" int gbm_gblup_fit_synthetic_ex(uint64_t seed, int64_t n, int64_t p, const double* Y, int64_t ldy,
                                          int64_t nrhs, double lambda, const int* devices, int ndev, int grm_mode,
                                          double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out,
                                          int* grm_used_out) {
  RoctxRange r_("gbm_gblup_fit_synthetic");
  if (n < 1 || p < 1) return fail(GBM_E_ARG, "gbm_gblup_fit_synthetic: bad arguments (n, p >= 1)");
  Problem pr{Source::SYNTH, nullptr, nullptr, 1, n, p, n};
  pr.seed = seed;
  return run_fit(pr, Y, ldy, nrhs, lambda, devices, ndev, b_hat_out, y_pred_out, mu_out, q_out, nullptr, grm_mode,
                 grm_used_out);
}

extern "C" int gbm_gblup_fit_synthetic(uint64_t seed, int64_t n, int64_t p, const double* Y, int64_t ldy, int64_t nrhs,
                                       double lambda, const int* devices, int ndev, double* b_hat_out,
                                       double* y_pred_out, double* mu_out, int64_t* q_out) {
  return gbm_gblup_fit_synthetic_ex(seed, n, p, Y, ldy, nrhs, lambda, devices, ndev, GBM_GRM_DEFAULT, b_hat_out,
                                    y_pred_out, mu_out, q_out, nullptr);
}

extern "C" int gbm_gblup_fit_dosage_i8_ex(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy,
                                          const double* Y, int64_t ldy, int64_t nrhs, double lambda, const int* devices,
                                          int ndev, int grm_mode, double* b_hat_out, double* y_pred_out,
                                          double* mu_out, int64_t* q_out, int* grm_used_out) {
  RoctxRange r_("gbm_gblup_fit_dosage_i8");
  if (!D || ploidy < 1) return fail(GBM_E_ARG, "gbm_gblup_fit_dosage_i8: D is NULL or ploidy < 1");
  Problem pr{Source::I8, nullptr, D, ploidy, n, p, ldd};
  return run_fit(pr, Y, ldy, nrhs, lambda, devices, ndev, b_hat_out, y_pred_out, mu_out, q_out, nullptr, grm_mode,
                 grm_used_out);
}

extern "C" int gbm_gblup_fit_dosage_i8(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy, const double* Y,
                                       int64_t ldy, int64_t nrhs, double lambda, const int* devices, int ndev,
                                       double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out) {
  return gbm_gblup_fit_dosage_i8_ex(D, n, p, ldd, ploidy, Y, ldy, nrhs, lambda, devices, ndev, GBM_GRM_DEFAULT,
                                    b_hat_out, y_pred_out, mu_out, q_out, nullptr);
}

extern "C" int gbm_debug_rccl_calls(int64_t* allreduce, int64_t* allgather) {
  rccl_call_counts(allreduce, allgather);
  return GBM_OK;
}

extern "C" int gbm_grm(const double* X, int64_t n, int64_t p, int64_t ldx, const int* devices, int ndev, double* G_out,
                       int64_t ldg, int64_t* q_out) {
  RoctxRange r_("gbm_grm");
  if (!X || !G_out || n < 1 || p < 1 || ldx < n || ldg < n) return fail(GBM_E_ARG, "gbm_grm: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(devices, ndev, devs));
  Problem pr{Source::F64, X, nullptr, 1, n, p, ldx};
  Shards shards;
  GBM_TRY(make_shards(devs, p, shards));
  int64_t q = 0;
  {
    RoctxRange r("gbm: upload + standardise + GRM");
    GBM_TRY(parallel_shards(shards, [&](size_t, Shard& sh) { return prepare_grm_shard(pr, sh); }));
  }
  for (auto& sh : shards) q += sh->q_host;
  if (q_out) *q_out = q;
  if (q == 0) return fail(GBM_E_DATA, "no polymorphic locus-allele");
  {
    RoctxRange r("gbm: partial-GRM all-reduce");
    GBM_TRY(allreduce_grm(shards, n));
  }
  return export_grm(shards[0]->x(), n, 1.0 / (double)q, G_out, ldg);
}

extern "C" int gbm_grm_ploidy_aware(const double* X, int64_t n, int64_t p, int64_t ldx, int ploidy, const int* devices,
                                    int ndev, double* G_out, int64_t ldg, double* denom_out) {
  RoctxRange r_("gbm_grm_ploidy_aware");
  if (!X || !G_out || n < 1 || p < 1 || ldx < n || ldg < n || ploidy < 1)
    return fail(GBM_E_ARG, "gbm_grm_ploidy_aware: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(devices, ndev, devs));
  Problem pr{Source::F64, X, nullptr, 1, n, p, ldx};
  Shards shards;
  GBM_TRY(make_shards(devs, p, shards));
  // X_c = X − 1 fᵀ (f_j = column mean = allele frequency); denominator Σ_j f_j (1 − f_j) in locus
  // order over the shards (host, from the device means)
  double den = 0.0;
  {
    RoctxRange r("gbm: upload + centre + GRM");
    std::vector<std::vector<double>> f(shards.size());
    GBM_TRY(parallel_shards(shards, [&](size_t k, Shard& sh) {
      GBM_TRY(prepare_shard(pr, sh, true, false));
      FitCtx& c = sh.x();
      f[k].resize(sh.p);
      GBM_HIP_TRY(hipMemcpyAsync(f[k].data(), c.mean.p, sh.p * 8, hipMemcpyDeviceToHost, c.stream.s));
      GBM_TRY(grm_shard(pr, sh));
      GBM_HIP_TRY(hipStreamSynchronize(c.stream.s));
      return GBM_OK;
    }));
    for (const auto& fk : f)
      for (double v : fk) den += v * (1.0 - v);  // locus order over the shards, as before
  }
  if (denom_out) *denom_out = den;
  if (!(den > 0.0) || !std::isfinite(den)) return fail(GBM_E_DATA, "gbm_grm_ploidy_aware: no polymorphic locus-allele");
  {
    RoctxRange r("gbm: partial-GRM all-reduce");
    GBM_TRY(allreduce_grm(shards, n));
  }
  return export_grm(shards[0]->x(), n, (double)ploidy / den, G_out, ldg);
}

extern "C" int gbm_colstats(const double* X, int64_t n, int64_t p, int64_t ldx, int device, double* mean_out,
                            double* sd_out, uint8_t* keep_out, int64_t* q_out) {
  if (!X || n < 1 || p < 1 || ldx < n) return fail(GBM_E_ARG, "gbm_colstats: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  Problem pr{Source::F64, X, nullptr, 1, n, p, ldx};
  Shards shards;
  GBM_TRY(make_shards(devs, p, shards));
  Shard& sh = *shards[0];
  GBM_TRY(prepare_shard(pr, sh));
  if (q_out) *q_out = sh.q_host;
  FitCtx& c = sh.x();
  hipStream_t s = c.stream.s;
  if (mean_out) GBM_HIP_TRY(hipMemcpyAsync(mean_out, c.mean.p, p * 8, hipMemcpyDeviceToHost, s));
  if (sd_out) GBM_HIP_TRY(hipMemcpyAsync(sd_out, c.sd.p, p * 8, hipMemcpyDeviceToHost, s));
  std::vector<int32_t> k32;
  if (keep_out) {
    k32.resize(p);
    GBM_HIP_TRY(hipMemcpyAsync(k32.data(), c.keep.p, p * 4, hipMemcpyDeviceToHost, s));
  }
  GBM_HIP_TRY(hipStreamSynchronize(s));
  if (keep_out)
    for (int64_t j = 0; j < p; j++) keep_out[j] = (uint8_t)(k32[j] != 0);
  return GBM_OK;
}

extern "C" int gbm_predict(const double* X, int64_t n, int64_t p, int64_t ldx, const double* b_hat, int64_t ldb,
                           int64_t nrhs, int device, double* out, int64_t ldo) {
  RoctxRange r_("gbm_predict");
  if (!X || !b_hat || !out || n < 1 || p < 1 || ldx < n || ldb < p + 1 || nrhs < 1 || ldo < n)
    return fail(GBM_E_ARG, "gbm_predict: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  std::unique_ptr<FitCtx> lease;
  GBM_TRY(pool().acquire(devs[0], lease));
  struct Release {
    std::unique_ptr<FitCtx>& c;
    ~Release() { pool().release(std::move(c)); }
  } release{lease};
  FitCtx& c = *lease;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  const int64_t nchunks = predict_chunks(n, p);
  GBM_TRY(ensure(c.Xt, c.dev, p * n * 8));
  GBM_TRY(ensure(c.B, c.dev, nrhs * (p + 1) * 8));
  GBM_TRY(ensure(c.part, c.dev, nchunks * nrhs * n * 8));
  GBM_TRY(ensure(c.out, c.dev, nrhs * n * 8));
  GBM_HIP_TRY(hipMemcpy2DAsync(c.Xt.p, n * 8, X, ldx * 8, n * 8, p, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpy2DAsync(c.B.p, (p + 1) * 8, b_hat, ldb * 8, (p + 1) * 8, nrhs, hipMemcpyHostToDevice, s));
  GBM_TRY(launch_predict((const double*)c.Xt.p, n, p, n, (const double*)c.B.p, p + 1, nrhs, (double*)c.part.p, nchunks,
                         (double*)c.out.p, n, s));
  GBM_HIP_TRY(hipMemcpy2DAsync(out, ldo * 8, c.out.p, n * 8, n * 8, nrhs, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  return GBM_OK;
}
