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
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <vector>

#include "gbm_internal.h"
#include "host_util.h"

struct gbm_session {
  std::mutex mu;
  int dev = 0;
  gbm::Stream stream;
  int64_t n = 0, p = 0, npad = 0;
  gbm::DevMem Xt;  // p x npad raw genotypes
  // training-set cache (key: the entry set and the standardisation mode)
  std::vector<int64_t> key;
  int mode = -1;  // 0: GBLUP standardisation, 1: centre only (glmnet standardize=false)
  int64_t nT = 0, npadT = 0, gdimT = 0, q = 0;
  gbm::DevMem idx32, Z, mean, sd, keep, qd, Gc, wsg;
  // per-fit buffers (sized for the cached training set)
  int64_t nrhs_cap = 0;
  gbm::DevMem Gw, wss, Y, A, gebv, mu_d, info, B, msum, terms;
  // predict buffers
  gbm::DevMem bvec, part, pout;
  int64_t builds = 0, hits = 0;
  // genotypes that are diploid dosages/2 (2x ∈ {0, 1, 2} in every cell: synthetic sessions by construction,
  // others checked on the device once, when a fit first asks for it): grm_mode exact / auto
  // (gbm_session_set_grm_mode, else GBM_GRM) builds the training GRM with the exact-integer kernels
  // (grm_exact.hip) from the gathered training dosages
  bool dosage2 = false, dosage_checked = false;
  int grm_mode = GBM_GRM_DEFAULT;
  bool exact_cached = false;  // the cached training GRM is the exact one (part of the cache key)
  gbm::DevMem D8T, wsx, mean2, sd2, keep2, q2;
  int64_t d8t_bytes = 0, wsx_bytes = 0;
  // GWAS scan (gbm_session_gwas): the chunk of locus rows being whitened, the statistics of all p loci and
  // the count of tested loci
  gbm::DevMem gwW, gwz, gwb, gwcnt;
  int64_t gww_bytes = 0;
  // elastic-net path (gbm_session_enet_path): the packed active rows and their Gram blocks, the per-slot
  // constants and coefficients (two copies, by pass parity), the residual, the per-locus x2, the chain's
  // partial dots and block maxima, the pass scalars and the rows of one admission
  gbm::DevBuf enZa, enW, enx2a, eninv, enb, ene, enx2, enpart, enblk, enred, enrows, engws;
  // principal components (gbm_session_pcs): the vector blocks Q, Y, W and the rotated output rows, the block
  // product's partials, the Gram partials, the small matrices exchanged with the host, and K's column statistics
  gbm::DevBuf pcQ, pcY, pcW, pcV, pcws, pcgram, pcsmall, pcm, pcsd, pcrt;
  // epistasis scan (gbm_session_pair_scan): the gathered work matrix, the row and locus indices, y and yc, the
  // loci's variances and skip flags, one panel of slopes, the counters, the selection's state and block counts,
  // and the candidates
  gbm::DevBuf psW, psidx, psloci, psy, psyc, psvar, psskip, psbeta, pscnt, pssel, psblk, pscidx, pscbeta;
};

namespace gbm {

// Reference loglikreml (src/gwas.jl:450-483) with X = 1 and V = σ²_u GRM + σ²_e I, from the
// terms of one solve at λ = σ²_e/σ²_u: logdet V = n log σ²_u + logdet V_λ, yᵀPy = Q_λ/σ²_u,
// logdet XᵀV⁻¹X = log c11_λ − log σ²_u.
double reml_objective(int64_t n, double logdet, double c11, double Q, double s2u) {
  return 0.5 * ((double)n * std::log(s2u) + logdet) + Q / s2u + std::log(c11) - std::log(s2u);
}

// g(λ): the objective minimised over σ²_u inside the reference's box (σ²_e, σ²_u ∈ [eps, 1]),
// σ²_e = λσ²_u. For fixed λ the objective is a log σ + Q/σ with a = n/2 − 1 > 0: unimodal, its
// minimiser Q/a clamped to the box. t = {logdet V_λ, 1ᵀV_λ⁻¹1, 1ᵀV_λ⁻¹y, yᵀV_λ⁻¹y}.
RemlEval reml_profile(int64_t n, double lambda, const double t[4]) {
  const double logdet = t[0], c11 = t[1], c1y = t[2], yy = t[3];
  const double Q = yy - c1y * c1y / c11;
  const double eps = std::numeric_limits<double>::epsilon();
  const double lo = std::max(eps, eps / lambda), hi = std::min(1.0, 1.0 / lambda);
  const double a = 0.5 * (double)n - 1.0;
  double s2u = Q / a;
  if (!(s2u >= lo)) s2u = lo;
  if (s2u > hi) s2u = hi;
  return {reml_objective(n, logdet, c11, Q, s2u), s2u, lambda * s2u};
}

// The search of gbm_session_reml and gbm_gblup_fit_reml: a scan of log10 λ over [-6, 6] in steps of
// 0.5, then golden-section refinement on [best − 0.5, best + 0.5] (to 1e-7 in log10 λ).
int reml_search(const std::function<int(double, RemlEval&)>& eval, RemlResult& out) {
  auto g = [&](double loglam, RemlEval& e) { return eval(std::pow(10.0, loglam), e); };
  double best_x = 0.0;
  RemlEval best{std::numeric_limits<double>::infinity(), 0.0, 0.0};
  for (int k = -12; k <= 12; k++) {
    RemlEval e;
    GBM_TRY(g(0.5 * k, e));
    if (e.g < best.g) {
      best = e;
      best_x = 0.5 * k;
    }
  }
  double a = best_x - 0.5, b = best_x + 0.5;
  const double r = 0.5 * (std::sqrt(5.0) - 1.0);
  double c = b - r * (b - a), d = a + r * (b - a);
  RemlEval ec, ed;
  GBM_TRY(g(c, ec));
  GBM_TRY(g(d, ed));
  for (int it = 0; it < 60 && (b - a) > 1e-7; it++) {
    if (ec.g < ed.g) {
      b = d;
      d = c;
      ed = ec;
      c = b - r * (b - a);
      GBM_TRY(g(c, ec));
    } else {
      a = c;
      c = d;
      ec = ed;
      d = a + r * (b - a);
      GBM_TRY(g(d, ed));
    }
  }
  const RemlEval& fin = ec.g < ed.g ? ec : ed;
  const double fin_x = ec.g < ed.g ? c : d;
  if (fin.g < best.g) {
    best = fin;
    best_x = fin_x;
  }
  out = {std::pow(10.0, best_x), best.s2e, best.s2u, best.g};
  return GBM_OK;
}

// y standardised as the reference's gwasprep does before REML (src/gwas.jl:127-128; sd ddof = 1)
std::vector<double> standardise_y(const double* y, int64_t n) {
  std::vector<double> ys(y, y + n);
  double m = 0.0;
  for (double v : ys) m += v;
  m /= (double)n;
  double ss = 0.0;
  for (double v : ys) ss += (v - m) * (v - m);
  const double sdv = std::sqrt(ss / (double)(n - 1));
  for (double& v : ys) v = (v - m) / sdv;
  return ys;
}

namespace {

int session_alloc_x(gbm_session* s) {
  GBM_HIP_TRY(hipSetDevice(s->dev));
  s->stream.dev = s->dev;
  GBM_HIP_TRY(hipStreamCreateWithFlags(&s->stream.s, hipStreamNonBlocking));
  s->npad = npad_of(s->n);
  GBM_TRY(dalloc(s->Xt, s->dev, s->p * s->npad * 8));
  GBM_HIP_TRY(hipMemsetAsync(s->Xt.p, 0, (size_t)(s->p * s->npad * 8), s->stream.s));
  return GBM_OK;
}

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

// Whether the session's genotypes are diploid dosages/2 (one device pass over X, the first time it is asked).
int session_dosage2(gbm_session* s, bool& out) {
  if (!s->dosage_checked) {
    GBM_TRY(dalloc(s->q2, s->dev, 8));
    GBM_HIP_TRY(hipMemsetAsync(s->q2.p, 0, 4, s->stream.s));
    GBM_TRY(launch_dosage_from_f64((const double*)s->Xt.p, s->npad, s->n, s->p, nullptr, 0, (int32_t*)s->q2.p,
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

// Standardise (mode 0) or centre (mode 1) the training set idx and build its GRM (cached).
int ensure_training(gbm_session* s, const int64_t* idx, int64_t nT, int mode = 0) {
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
  const int64_t npadT = npad_of(nT), gdimT = gdim_of(nT);
  if (npadT != s->npadT) {
    GBM_TRY(dalloc(s->Z, s->dev, s->p * npadT * 8));
    GBM_TRY(dalloc(s->Gc, s->dev, gdimT * gdimT * 8));
    GBM_TRY(dalloc(s->Gw, s->dev, gdimT * gdimT * 8));
    GBM_TRY(dalloc(s->wss, s->dev, gbm_dev_solve_workspace(nT, 63)));
    s->nrhs_cap = 0;
    s->npadT = npadT;
    s->gdimT = gdimT;
  }
  if (!s->mean.p) {
    GBM_TRY(dalloc(s->mean, s->dev, s->p * 8));
    GBM_TRY(dalloc(s->sd, s->dev, s->p * 8));
    GBM_TRY(dalloc(s->keep, s->dev, s->p * 4));
    GBM_TRY(dalloc(s->qd, s->dev, 8));
  }
  GBM_TRY(dalloc(s->idx32, s->dev, nT * 4));
  const int64_t wsb = gbm_dev_grm_workspace(nT, s->p);
  GBM_TRY(dalloc(s->wsg, s->dev, wsb));
  std::vector<int32_t> i32(idx, idx + nT);
  GBM_HIP_TRY(hipMemcpyAsync(s->idx32.p, i32.data(), nT * 4, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemsetAsync(s->qd.p, 0, 8, st));
  GBM_TRY(gbm_dev_standardize_gather((const double*)s->Xt.p, s->npad, s->p, (const int32_t*)s->idx32.p, nT,
                                     (double*)s->Z.p, npadT, (double*)s->mean.p, (double*)s->sd.p,
                                     (int32_t*)s->keep.p, (int64_t*)s->qd.p, mode, st));
  int64_t q = 0;
  GBM_HIP_TRY(hipMemcpyAsync(&q, s->qd.p, 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  if (q == 0) return fail(GBM_E_DATA, "no polymorphic locus-allele in the training set (src/gwas.jl:112-115)");
  if (exact) {
    // exact-integer GRM of the training dosages; its per-locus statistics go to scratch (Z, mean and sd
    // above are what the marker effects and predictions use; q is the same count)
    if (s->d8t_bytes < s->p * nT) {
      GBM_TRY(dalloc(s->D8T, s->dev, s->p * nT));
      s->d8t_bytes = s->p * nT;
    }
    const int64_t wsx = gbm_dev_grm_exact_workspace(nT, s->p);
    if (s->wsx_bytes < wsx) {
      GBM_TRY(dalloc(s->wsx, s->dev, wsx));
      s->wsx_bytes = wsx;
    }
    if (!s->mean2.p) {
      GBM_TRY(dalloc(s->mean2, s->dev, s->p * 8));
      GBM_TRY(dalloc(s->sd2, s->dev, s->p * 8));
      GBM_TRY(dalloc(s->keep2, s->dev, s->p * 4));
      GBM_TRY(dalloc(s->q2, s->dev, 8));
    }
    GBM_TRY(launch_gather_dosage((const double*)s->Xt.p, s->npad, s->p, (const int32_t*)s->idx32.p, nT,
                                 (int8_t*)s->D8T.p, st));
    GBM_HIP_TRY(hipMemsetAsync(s->q2.p, 0, 8, st));
    GBM_TRY(launch_grm_exact((const int8_t*)s->D8T.p, nT, s->p, nT, 2, (double*)s->Gc.p, gdimT, (double*)s->mean2.p,
                             (double*)s->sd2.p, (int32_t*)s->keep2.p, (int64_t*)s->q2.p, 0, s->wsx.p, wsx, nullptr, st));
    GBM_TRY(grm_exact_status(s->wsx.p, nT, s->p, st));
  } else {
    GBM_TRY(gbm_dev_grm((const double*)s->Z.p, npadT, s->p, nT, (double*)s->Gc.p, gdimT, s->wsg.p, wsb, st));
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
  if (nrhs <= s->nrhs_cap) return GBM_OK;
  const int64_t npadT = s->npadT;
  GBM_TRY(dalloc(s->Y, s->dev, nrhs * npadT * 8));
  GBM_TRY(dalloc(s->A, s->dev, nrhs * npadT * 8));
  GBM_TRY(dalloc(s->gebv, s->dev, nrhs * npadT * 8));
  GBM_TRY(dalloc(s->mu_d, s->dev, nrhs * 8));
  GBM_TRY(dalloc(s->info, s->dev, 4));
  GBM_TRY(dalloc(s->B, s->dev, nrhs * s->p * 8));
  GBM_TRY(dalloc(s->msum, s->dev, nrhs * 8));
  GBM_TRY(dalloc(s->terms, s->dev, (2 + 2 * nrhs) * 8));
  s->nrhs_cap = nrhs;
  return GBM_OK;
}

// Solve (G·inv_q + λI) on the cached GRM for the nrhs phenotype columns already in s->Y
// (inv_q = 1/q for GBLUP, 1 for the unscaled ridge kernel).
int solve_cached(gbm_session* s, int64_t nrhs, double lambda, double inv_q) {
  hipStream_t st = s->stream.s;
  // the solve factors in place: work on a copy of the cached GRM (rows [0, npad) are read)
  GBM_HIP_TRY(hipMemcpyAsync(s->Gw.p, s->Gc.p, (size_t)(s->npadT * s->gdimT * 8), hipMemcpyDeviceToDevice, st));
  GBM_TRY(gbm_dev_gblup_solve((double*)s->Gw.p, s->gdimT, s->nT, inv_q, nullptr, lambda,
                              (const double*)s->Y.p, s->npadT, nrhs, (double*)s->A.p, (double*)s->gebv.p, s->npadT,
                              (double*)s->mu_d.p, (int32_t*)s->info.p, s->wss.p,
                              gbm_dev_solve_workspace(s->nT, 63), st));
  int32_t info = 0;
  GBM_HIP_TRY(hipMemcpyAsync(&info, s->info.p, 4, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  if (info < 0) return fail(GBM_E_HIP, "solve: a wait between workgroups timed out (dataflow Cholesky or back substitution; the result is invalid)");
  if (info != 0)
    return fail(GBM_E_NOTPD, "G/q + lambda*I is not positive definite (pivot " + std::to_string(info) + ")");
  return GBM_OK;
}

int upload_y(gbm_session* s, const double* Y, int64_t ldy, int64_t nrhs) {
  GBM_HIP_TRY(hipMemsetAsync(s->Y.p, 0, (size_t)(nrhs * s->npadT * 8), s->stream.s));
  GBM_HIP_TRY(hipMemcpy2DAsync(s->Y.p, s->npadT * 8, Y, ldy * 8, s->nT * 8, nrhs, hipMemcpyHostToDevice, s->stream.s));
  return GBM_OK;
}

int reml_eval(gbm_session* s, double lambda, RemlEval& out) {
  GBM_TRY(solve_cached(s, 1, lambda, 1.0 / (double)s->q));
  double t[4];
  GBM_TRY(gbm_dev_gblup_terms((const double*)s->Gw.p, s->gdimT, s->nT, 1, s->wss.p, (double*)s->terms.p,
                              s->stream.s));
  GBM_HIP_TRY(hipMemcpyAsync(t, s->terms.p, 4 * 8, hipMemcpyDeviceToHost, s->stream.s));
  GBM_HIP_TRY(hipStreamSynchronize(s->stream.s));
  out = reml_profile(s->nT, lambda, t);
  return GBM_OK;
}

// The null-model REML search of gbm_session_reml on the cached training set (ys: the standardised y)
int reml_cached(gbm_session* s, const std::vector<double>& ys, RemlResult& res) {
  GBM_TRY(ensure_rhs(s, 1));
  GBM_TRY(upload_y(s, ys.data(), s->nT, 1));
  return reml_search([&](double lambda, RemlEval& e) { return reml_eval(s, lambda, e); }, res);
}

// A⁻¹ of the K x K (K <= 8) symmetric positive definite A (row-major, pitch 8) by Cholesky, in place
bool invert_spd8(double* A, int K) {
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
int64_t gwas_chunk(int64_t p, int64_t npadT, int dev) {
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

}  // namespace
}  // namespace gbm

using namespace gbm;

extern "C" int gbm_session_create(const double* X, int64_t n, int64_t p, int64_t ldx, int device, gbm_session** out) {
  RoctxRange r_("gbm_session_create");
  if (!out) return fail(GBM_E_ARG, "gbm_session_create: out is NULL");
  *out = nullptr;
  if (!X || n < 1 || p < 1 || ldx < n) return fail(GBM_E_ARG, "gbm_session_create: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  auto s = new gbm_session();
  s->dev = devs[0];
  s->n = n;
  s->p = p;
  int rc = session_alloc_x(s);
  if (rc == GBM_OK) {
    if (hipMemcpy2DAsync(s->Xt.p, s->npad * 8, X, ldx * 8, n * 8, p, hipMemcpyHostToDevice, s->stream.s) !=
            hipSuccess ||
        hipStreamSynchronize(s->stream.s) != hipSuccess)
      rc = fail(GBM_E_HIP, "gbm_session_create: upload failed");
  }
  if (rc != GBM_OK) {
    delete s;
    return rc;
  }
  *out = s;
  return GBM_OK;
}

extern "C" int gbm_session_create_synthetic(uint64_t seed, int64_t n, int64_t p, int device, gbm_session** out) {
  RoctxRange r_("gbm_session_create_synthetic");
  if (!out) return fail(GBM_E_ARG, "gbm_session_create_synthetic: out is NULL");
  *out = nullptr;
  if (n < 1 || p < 1) return fail(GBM_E_ARG, "gbm_session_create_synthetic: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  auto s = new gbm_session();
  s->dev = devs[0];
  s->n = n;
  s->p = p;
  int rc = session_alloc_x(s);
  if (rc == GBM_OK) rc = gbm_dev_synth_genotypes((double*)s->Xt.p, s->npad, p, n, seed, 0, s->stream.s);
  s->dosage2 = s->dosage_checked = true;  // X = dosage/2 (SURVEY.md §8d generator)
  if (rc == GBM_OK && hipStreamSynchronize(s->stream.s) != hipSuccess)
    rc = fail(GBM_E_HIP, "gbm_session_create_synthetic: generation failed");
  if (rc != GBM_OK) {
    delete s;
    return rc;
  }
  *out = s;
  return GBM_OK;
}

extern "C" int gbm_session_create_dosage_i8(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy,
                                            int device, gbm_session** out) {
  RoctxRange r_("gbm_session_create_dosage_i8");
  if (!out) return fail(GBM_E_ARG, "gbm_session_create_dosage_i8: out is NULL");
  *out = nullptr;
  if (!D || n < 1 || p < 1 || ldd < n || ploidy < 1)
    return fail(GBM_E_ARG, "gbm_session_create_dosage_i8: bad arguments");
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  auto s = new gbm_session();
  s->dev = devs[0];
  s->n = n;
  s->p = p;
  int rc = session_alloc_x(s);
  DevMem d8;
  if (rc == GBM_OK) rc = dalloc(d8, s->dev, n * p);
  if (rc == GBM_OK && (hipMemcpy2DAsync(d8.p, n, D, ldd, n, p, hipMemcpyHostToDevice, s->stream.s) != hipSuccess))
    rc = fail(GBM_E_HIP, "gbm_session_create_dosage_i8: upload failed");
  if (rc == GBM_OK) rc = gbm_dev_expand_dosage_i8((const int8_t*)d8.p, n, n, p, ploidy, (double*)s->Xt.p, s->npad,
                                                  s->stream.s);
  if (rc == GBM_OK && hipStreamSynchronize(s->stream.s) != hipSuccess) rc = fail(GBM_E_HIP, "stream sync");
  if (rc != GBM_OK) {
    delete s;
    return rc;
  }
  *out = s;
  return GBM_OK;
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

extern "C" int gbm_session_gblup_fit(gbm_session* s, const int64_t* idx, int64_t n_train, const double* Y, int64_t ldy,
                                     int64_t nrhs, double lambda, double* b_hat_out, double* y_pred_out, double* mu_out,
                                     int64_t* q_out) {
  RoctxRange r_("gbm_session_gblup_fit");
  if (!s) return fail(GBM_E_ARG, "gbm_session_gblup_fit: session is NULL");
  if (!Y || ldy < n_train || nrhs < 1 || nrhs > 63 || !b_hat_out || !y_pred_out)
    return fail(GBM_E_ARG, "gbm_session_gblup_fit: bad arguments (ldy >= n_train, 1 <= nrhs <= 63, outputs)");
  if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(GBM_E_ARG, "gbm_session_gblup_fit: lambda must be > 0");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(Y, n_train, ldy, nrhs));
  GBM_TRY(ensure_training(s, idx, n_train));
  GBM_TRY(ensure_rhs(s, nrhs));
  GBM_TRY(upload_y(s, Y, ldy, nrhs));
  GBM_TRY(solve_cached(s, nrhs, lambda, 1.0 / (double)s->q));
  hipStream_t st = s->stream.s;
  const int64_t p = s->p;
  GBM_TRY(gbm_dev_marker_effects((const double*)s->Z.p, s->npadT, p, s->nT, (const double*)s->A.p, s->npadT, nrhs,
                                 1.0 / (double)s->q, nullptr, (const double*)s->mean.p, (const double*)s->sd.p,
                                 (const int32_t*)s->keep.p, (double*)s->B.p, p, (double*)s->msum.p, st));
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
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_idx(s, idx, n_val, "gbm_session_predict"));
  hipStream_t st = s->stream.s;
  const int64_t p = s->p, n = s->n, npad = s->npad;
  const int64_t nchunks = predict_chunks(n, p);
  GBM_TRY(dalloc(s->bvec, s->dev, nrhs * (p + 1) * 8));
  GBM_TRY(dalloc(s->part, s->dev, nchunks * nrhs * npad * 8));
  GBM_TRY(dalloc(s->pout, s->dev, nrhs * npad * 8));
  GBM_HIP_TRY(hipMemcpy2DAsync(s->bvec.p, (p + 1) * 8, b_hat, ldb * 8, (p + 1) * 8, nrhs, hipMemcpyHostToDevice, st));
  GBM_TRY(launch_predict((const double*)s->Xt.p, npad, p, n, (const double*)s->bvec.p, p + 1, nrhs,
                         (double*)s->part.p, nchunks, (double*)s->pout.p, npad, st));
  std::vector<double> all(nrhs * npad);
  GBM_HIP_TRY(hipMemcpyAsync(all.data(), s->pout.p, nrhs * npad * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  for (int64_t t = 0; t < nrhs; t++)
    for (int64_t i = 0; i < n_val; i++) out[t * ldo + i] = all[t * npad + idx[i]];
  return GBM_OK;
}

extern "C" int gbm_session_reml_objective(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                                          const double* sigma2_e, const double* sigma2_u, int64_t m, double* out) {
  if (!s) return fail(GBM_E_ARG, "gbm_session_reml_objective: session is NULL");
  if (!y || !sigma2_e || !sigma2_u || m < 1 || !out) return fail(GBM_E_ARG, "gbm_session_reml_objective: bad arguments");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(y, n_train, n_train, 1));
  GBM_TRY(ensure_training(s, idx, n_train));
  GBM_TRY(ensure_rhs(s, 1));
  GBM_TRY(upload_y(s, y, n_train, 1));
  for (int64_t k = 0; k < m; k++) {
    if (!(sigma2_e[k] > 0.0) || !(sigma2_u[k] > 0.0))
      return fail(GBM_E_ARG, "gbm_session_reml_objective: variance components must be > 0");
    GBM_TRY(solve_cached(s, 1, sigma2_e[k] / sigma2_u[k], 1.0 / (double)s->q));
    double t[4];
    GBM_TRY(gbm_dev_gblup_terms((const double*)s->Gw.p, s->gdimT, s->nT, 1, s->wss.p, (double*)s->terms.p,
                                s->stream.s));
    GBM_HIP_TRY(hipMemcpyAsync(t, s->terms.p, 4 * 8, hipMemcpyDeviceToHost, s->stream.s));
    GBM_HIP_TRY(hipStreamSynchronize(s->stream.s));
    const double Q = t[3] - t[2] * t[2] / t[1];
    out[k] = reml_objective(n_train, t[0], t[1], Q, sigma2_u[k]);
  }
  return GBM_OK;
}

extern "C" int gbm_session_reml(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                                double* lambda_out, double* sigma2_e_out, double* sigma2_u_out, double* objective_out) {
  RoctxRange r_("gbm_session_reml");
  if (!s) return fail(GBM_E_ARG, "gbm_session_reml: session is NULL");
  if (!y) return fail(GBM_E_ARG, "gbm_session_reml: y is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(y, n_train, n_train, 1));
  if (n_train < 3) return fail(GBM_E_DATA, "REML needs at least 3 entries");
  GBM_TRY(ensure_training(s, idx, n_train));
  const std::vector<double> ys = standardise_y(y, n_train);
  RemlResult res;
  GBM_TRY(reml_cached(s, ys, res));
  if (lambda_out) *lambda_out = res.lambda;
  if (sigma2_e_out) *sigma2_e_out = res.s2e;
  if (sigma2_u_out) *sigma2_u_out = res.s2u;
  if (objective_out) *objective_out = res.objective;
  return GBM_OK;
}

extern "C" int gbm_session_stats(gbm_session* s, int64_t* grm_builds, int64_t* grm_hits) {
  if (!s) return fail(GBM_E_ARG, "gbm_session_stats: session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  if (grm_builds) *grm_builds = s->builds;
  if (grm_hits) *grm_hits = s->hits;
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
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(y, n_train, n_train, 1));
  GBM_TRY(ensure_training(s, idx, n_train, 1));
  GBM_TRY(ensure_rhs(s, 1));
  // glmnet's first λ for alpha < 1e-3: max_j |x_cjᵀ(y − ȳ)|/n / 1e-3
  double m = 0.0;
  for (int64_t i = 0; i < n_train; i++) m += y[i];
  m /= (double)n_train;
  std::vector<double> r(s->npadT, 0.0);
  for (int64_t i = 0; i < n_train; i++) r[i] = y[i] - m;
  hipStream_t st = s->stream.s;
  GBM_HIP_TRY(hipMemcpyAsync(s->A.p, r.data(), s->npadT * 8, hipMemcpyHostToDevice, st));
  GBM_TRY(gbm_dev_marker_effects((const double*)s->Z.p, s->npadT, s->p, s->nT, (const double*)s->A.p, s->npadT, 1,
                                 1.0, nullptr, (const double*)s->mean.p, (const double*)s->sd.p,
                                 (const int32_t*)s->keep.p, (double*)s->B.p, s->p, (double*)s->msum.p, st));
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
  for (int64_t k = 0; k < nl; k++)
    if (!(lambdas[k] > 0.0) || !std::isfinite(lambdas[k]))
      return fail(GBM_E_ARG, "gbm_session_ridge_path: lambdas must be finite and > 0");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(y, n_train, n_train, 1));
  if (n_eval > 0) GBM_TRY(check_idx(s, idx_eval, n_eval, "gbm_session_ridge_path (eval)"));
  GBM_TRY(ensure_training(s, idx, n_train, 1));
  GBM_TRY(ensure_rhs(s, 1));
  GBM_TRY(upload_y(s, y, n_train, 1));
  double ym = 0.0, yss = 0.0;
  for (int64_t i = 0; i < n_train; i++) ym += y[i];
  ym /= (double)n_train;
  for (int64_t i = 0; i < n_train; i++) yss += (y[i] - ym) * (y[i] - ym);
  const double ys = std::sqrt(yss / (double)n_train);
  if (!(ys > 0.0)) return fail(GBM_E_ARG, "gbm_session_ridge_path: y has zero variance");
  hipStream_t st = s->stream.s;
  const int64_t p = s->p, n = s->n, npad = s->npad;
  const int64_t nchunks = predict_chunks(n, p);
  if (n_eval > 0) {
    GBM_TRY(dalloc(s->bvec, s->dev, (p + 1) * 8));
    GBM_TRY(dalloc(s->part, s->dev, nchunks * npad * 8));
    GBM_TRY(dalloc(s->pout, s->dev, npad * 8));
  }
  std::vector<double> all(n_eval > 0 ? npad : 0);
  for (int64_t k = 0; k < nl; k++) {
    GBM_TRY(solve_cached(s, 1, (double)n_train * lambdas[k] / ys, 1.0));
    GBM_TRY(gbm_dev_marker_effects((const double*)s->Z.p, s->npadT, p, s->nT, (const double*)s->A.p, s->npadT, 1,
                                   1.0, nullptr, (const double*)s->mean.p, (const double*)s->sd.p,
                                   (const int32_t*)s->keep.p, (double*)s->B.p, p, (double*)s->msum.p, st));
    double mu = 0.0, msum = 0.0;
    double* bk = b_path_out + k * (p + 1);
    GBM_HIP_TRY(hipMemcpyAsync(bk + 1, s->B.p, p * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipMemcpyAsync(&mu, s->mu_d.p, 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipMemcpyAsync(&msum, s->msum.p, 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    bk[0] = mu - msum;
    if (n_eval > 0) {
      GBM_HIP_TRY(hipMemcpyAsync(s->bvec.p, bk, 8, hipMemcpyHostToDevice, st));
      GBM_HIP_TRY(hipMemcpyAsync((double*)s->bvec.p + 1, s->B.p, p * 8, hipMemcpyDeviceToDevice, st));
      GBM_TRY(launch_predict((const double*)s->Xt.p, npad, p, n, (const double*)s->bvec.p, p + 1, 1,
                             (double*)s->part.p, nchunks, (double*)s->pout.p, npad, st));
      GBM_HIP_TRY(hipMemcpyAsync(all.data(), s->pout.p, npad * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));
      for (int64_t i = 0; i < n_eval; i++) pred_out[k * n_eval + i] = all[idx_eval[i]];
    }
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
  for (int64_t k = 0; k < nl; k++) {
    if (!(lambdas[k] > 0.0) || !std::isfinite(lambdas[k]))
      return fail(GBM_E_ARG, "gbm_session_enet_path: lambdas must be finite and > 0");
    if (k > 0 && lambdas[k] > lambdas[k - 1])
      return fail(GBM_E_ARG, "gbm_session_enet_path: lambdas must be non-increasing (the path is warm-started)");
  }
  if (!(tol > 0.0) || !std::isfinite(tol) || max_passes < 1)
    return fail(GBM_E_ARG, "gbm_session_enet_path: tol must be > 0 and max_passes >= 1");
  if (std::isnan(dev_max) || !(fdev >= 0.0) || !std::isfinite(fdev))
    return fail(GBM_E_ARG, "gbm_session_enet_path: dev_max must not be NaN and fdev must be finite and >= 0");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(y, n_train, n_train, 1));
  if (n_eval > 0) GBM_TRY(check_idx(s, idx_eval, n_eval, "gbm_session_enet_path (eval)"));
  GBM_TRY(ensure_training(s, idx, n_train, 1));
  GBM_TRY(ensure_rhs(s, 1));
  double ym = 0.0, yss = 0.0;
  for (int64_t i = 0; i < n_train; i++) ym += y[i];
  ym /= (double)n_train;
  for (int64_t i = 0; i < n_train; i++) yss += (y[i] - ym) * (y[i] - ym);
  const double ys = std::sqrt(yss / (double)n_train);
  if (!(ys > 0.0)) return fail(GBM_E_ARG, "gbm_session_enet_path: y has zero variance");
  hipStream_t st = s->stream.s;
  const int64_t p = s->p, n = s->n, npad = s->npad, nT = s->nT;
  const int64_t lda = enet_lda(nT), cap = std::min(p, 2 * s->npadT), cappad = round_up(cap, 64);
  const int64_t C = (nT + 255) / 256;
  GBM_TRY(ensure(s->enZa, s->dev, cap * lda * 8));
  GBM_TRY(ensure(s->enW, s->dev, cappad * 64 * 8));
  GBM_TRY(ensure(s->enx2a, s->dev, cappad * 8));
  GBM_TRY(ensure(s->eninv, s->dev, cappad * 8));
  GBM_TRY(ensure(s->enb, s->dev, 2 * cappad * 8));
  GBM_TRY(ensure(s->ene, s->dev, lda * 8));
  GBM_TRY(ensure(s->enx2, s->dev, p * 8));
  GBM_TRY(ensure(s->enpart, s->dev, 2 * C * 64 * 8));
  GBM_TRY(ensure(s->enblk, s->dev, (cappad / 64) * 8));
  GBM_TRY(ensure(s->enred, s->dev, 2 * 8));
  GBM_TRY(ensure(s->enrows, s->dev, cap * 4));
  GBM_TRY(ensure(s->engws, s->dev, enet_gram_workspace(nT)));
  const int64_t nchunks = predict_chunks(n, p);
  if (n_eval > 0) {
    GBM_TRY(dalloc(s->bvec, s->dev, (p + 1) * 8));
    GBM_TRY(dalloc(s->part, s->dev, nchunks * npad * 8));
    GBM_TRY(dalloc(s->pout, s->dev, npad * 8));
  }
  double* const Za = (double*)s->enZa.p;
  double* const x2a = (double*)s->enx2a.p;
  double* const bdev = (double*)s->enb.p;
  double* const e = (double*)s->ene.p;
  double* const red = (double*)s->enred.p;
  std::vector<double> e0(lda, 0.0), x2h(p), meanh(p), g(p), bh(cap), all(n_eval > 0 ? npad : 0);
  for (int64_t i = 0; i < nT; i++) e0[i] = y[i] - ym;
  GBM_HIP_TRY(hipMemcpyAsync(e, e0.data(), lda * 8, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemsetAsync(x2a, 0, cappad * 8, st));
  GBM_HIP_TRY(hipMemsetAsync(bdev, 0, 2 * cappad * 8, st));
  GBM_TRY(launch_enet_x2((const double*)s->Z.p, s->npadT, p, nT, (double*)s->enx2.p, st));
  GBM_HIP_TRY(hipMemcpyAsync(x2h.data(), s->enx2.p, p * 8, hipMemcpyDeviceToHost, st));
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
    GBM_TRY(launch_enet_prep(A, x2a, l2, (double*)s->eninv.p, st));
    for (;;) {
      while (A > 0) {
        if (passes >= max_passes) {
          hit = true;
          break;
        }
        double r2[2] = {0.0, 0.0};
        GBM_TRY(launch_enet_pass(Za, lda, nT, A, (const double*)s->enW.p, x2a, (const double*)s->eninv.p,
                                 bdev + par * cappad, bdev + (par ^ 1) * cappad, thr, (double*)s->enpart.p,
                                 (double*)s->enblk.p, e, red, st));
        par ^= 1;
        GBM_HIP_TRY(hipMemcpyAsync(r2, red, 16, hipMemcpyDeviceToHost, st));
        GBM_HIP_TRY(hipStreamSynchronize(st));
        passes++;
        if (r2[0] < tol * ys * ys) break;
      }
      if (hit) break;
      // screen: g = Zᵀe over all p loci; every inactive locus past the threshold joins the list (ascending j)
      GBM_TRY(gbm_dev_marker_effects((const double*)s->Z.p, s->npadT, p, nT, e, lda, 1, 1.0, nullptr,
                                     (const double*)s->mean.p, (const double*)s->sd.p, (const int32_t*)s->keep.p,
                                     (double*)s->B.p, p, (double*)s->msum.p, st));
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
      GBM_HIP_TRY(hipMemcpyAsync(s->enrows.p, fresh.data(), cnt * 4, hipMemcpyHostToDevice, st));
      GBM_TRY(launch_enet_gather((const double*)s->Z.p, s->npadT, nT, (const int32_t*)s->enrows.p, A, cnt,
                                 (const double*)s->enx2.p, Za, lda, x2a, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));  // `fresh` is pageable: the copy has read it before it changes
      for (int32_t j : fresh) {
        active[j] = 1;
        act.push_back(j);
      }
      const int64_t blk0 = A / 64;  // the partly filled last block and the new ones
      A += cnt;
      GBM_TRY(launch_enet_gram(Za, lda, A, nT, blk0, (double*)s->enW.p, (double*)s->engws.p, st));
      GBM_TRY(launch_enet_prep(A, x2a, l2, (double*)s->eninv.p, st));
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
    if (n_eval > 0) {
      GBM_HIP_TRY(hipMemcpyAsync(s->bvec.p, bk, (p + 1) * 8, hipMemcpyHostToDevice, st));
      GBM_TRY(launch_predict((const double*)s->Xt.p, npad, p, n, (const double*)s->bvec.p, p + 1, 1,
                             (double*)s->part.p, nchunks, (double*)s->pout.p, npad, st));
      GBM_HIP_TRY(hipMemcpyAsync(all.data(), s->pout.p, npad * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));
      for (int64_t i = 0; i < n_eval; i++) pred_out[k * n_eval + i] = all[idx_eval[i]];
    }
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

// ---- GWAS scan on the cached factor (reference gwasreml / gwasols, src/gwas.jl:241-245, 591-599) ----
// Mixed model: V = σ²_u ZZᵀ/q + σ²_e I = σ²_u V_λ, λ = σ²_e/σ²_u. One bordered solve with [C, y] as right-hand
// sides leaves the factor U of V_λ, the whitened rows U⁻ᵀ[1, C, y] (lower-copy rows npad + s) and
// −[1, C, y]ᵀV_λ⁻¹[1, C, y] (the Schur block); the locus rows are whitened chunk by chunk (gbm_dev_whiten_rows)
// and each locus' statistic is the Schur complement of the bordered normal equations (gwas_stats_kernel).
// z = z_λ/√σ²_u, b = b_λ. OLS: the same statistics kernel on the unwhitened rows with V = I.
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
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_y(y, n_train, n_train, 1));
  for (int64_t c = 0; c < kc; c++)
    for (int64_t i = 0; i < n_train; i++)
      if (!std::isfinite(C[c * ldc + i]))
        return fail(GBM_E_ARG, "gbm_session_gwas: covariate " + std::to_string(c + 1) + " has a NaN/Inf value at entry " +
                                   std::to_string(i + 1));
  GBM_TRY(ensure_training(s, idx, n_train));
  hipStream_t st = s->stream.s;
  const int64_t p = s->p, nT = s->nT, npadT = s->npadT, gdimT = s->gdimT;
  const int K = (int)kc + 1;  // covariate rows, the intercept first
  const std::vector<double> ys = standardise_y(y, n_train);
  GBM_TRY(ensure_rhs(s, kc + 2));
  if (!s->gwz.p) {
    GBM_TRY(dalloc(s->gwz, s->dev, p * 8));
    GBM_TRY(dalloc(s->gwb, s->dev, p * 8));
    GBM_TRY(dalloc(s->gwcnt, s->dev, 8));
  }
  GBM_HIP_TRY(hipMemsetAsync(s->gwcnt.p, 0, 8, st));
  GwasCoef co;
  std::memset(&co, 0, sizeof(co));
  co.kcov = K;
  double u[8] = {0.0};
  double used[2] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN()};
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
    const double* Gw = (const double*)s->Gw.p;
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
  const int32_t* keep = (const int32_t*)s->keep.p;
  double *zd = (double*)s->gwz.p, *bd = (double*)s->gwb.p;
  unsigned long long* cnt = (unsigned long long*)s->gwcnt.p;
  if (model == 0) {
    const int64_t chunk = gwas_chunk(p, npadT, s->dev);
    if (s->gww_bytes < chunk * npadT * 8) {
      s->gww_bytes = 0;
      GBM_TRY(dalloc(s->gwW, s->dev, chunk * npadT * 8));
      s->gww_bytes = chunk * npadT * 8;
    }
    double* W = (double*)s->gwW.p;
    const double* Gw = (const double*)s->Gw.p;
    for (int64_t j0 = 0; j0 < p; j0 += chunk) {
      const int64_t rows = std::min(chunk, p - j0);
      // the cached Z is never written: whiten a copy of the chunk
      GBM_HIP_TRY(hipMemcpyAsync(W, (const double*)s->Z.p + j0 * npadT, (size_t)(rows * npadT * 8),
                                 hipMemcpyDeviceToDevice, st));
      GBM_TRY(gbm_dev_whiten_rows(Gw, gdimT, nT, s->wss.p, W, npadT, rows, st));
      GBM_TRY(launch_gwas_stats(W, npadT, rows, nT, Gw + npadT * gdimT, gdimT, Gw + (npadT + K) * gdimT, co, keep + j0,
                                zd + j0, bd + j0, nullptr, cnt, st));
    }
  } else {
    const double* rows_d = (const double*)s->Y.p;
    GBM_TRY(launch_gwas_stats((const double*)s->Z.p, npadT, p, nT, rows_d, npadT, rows_d + K * npadT, co, keep, zd, bd,
                              nullptr, cnt, st));
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

// ---- leading principal components of the cached GRM (reference gwasols' PC1, src/gwas.jl:130,234) ----
// Block subspace iteration with a Rayleigh–Ritz step every iteration (include/gbm.h states the operators, the stop
// rule and the sign rule; DESIGN.md §4.11 the schedule). Per iteration the device applies the operator to the
// orthonormal block Q (one or two gbm_dev_rows_times_sym), forms T = QYᵀ and YYᵀ, and the host answers with the
// Ritz vectors of T (cyclic Jacobi) and the inverse Cholesky factor of YYᵀ; the residuals and the first CholQR
// pass run behind that, the second pass behind one more 8 KB exchange: two host synchronisations per iteration.

namespace gbm {
namespace {

// Eigen-decomposition of the symmetric m x m A (m <= 64) by cyclic Jacobi rotations: w descending, V[i·m + r] =
// component r of eigenvector i. Only the upper triangle's values matter (A is symmetrised from both).
void sym_eig(const double* A, int m, double* w, double* V) {
  std::vector<double> a((size_t)m * m), v((size_t)m * m, 0.0);
  double fro2 = 0.0;
  for (int i = 0; i < m; i++) {
    v[(size_t)i * m + i] = 1.0;
    for (int j = 0; j < m; j++) {
      a[(size_t)i * m + j] = 0.5 * (A[i * m + j] + A[j * m + i]);
      fro2 += a[(size_t)i * m + j] * a[(size_t)i * m + j];
    }
  }
  for (int sweep = 0; sweep < 64; sweep++) {
    double off2 = 0.0;
    for (int p = 0; p < m; p++)
      for (int q = p + 1; q < m; q++) off2 += a[(size_t)p * m + q] * a[(size_t)p * m + q];
    if (!(off2 > 1e-40 * fro2)) break;
    for (int p = 0; p < m; p++)
      for (int q = p + 1; q < m; q++) {
        const double apq = a[(size_t)p * m + q];
        if (apq == 0.0) continue;
        const double app = a[(size_t)p * m + p], aqq = a[(size_t)q * m + q];
        if (std::fabs(apq) <= 1e-20 * (std::fabs(app) + std::fabs(aqq))) {
          a[(size_t)p * m + q] = a[(size_t)q * m + p] = 0.0;
          continue;
        }
        const double th = (aqq - app) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c, tau = sn / (1.0 + c);
        // Rutishauser's update: the diagonal moves by t·a_pq, every other entry by a multiple of s
        a[(size_t)p * m + p] = app - t * apq;
        a[(size_t)q * m + q] = aqq + t * apq;
        a[(size_t)p * m + q] = a[(size_t)q * m + p] = 0.0;
        for (int k = 0; k < m; k++) {
          if (k != p && k != q) {
            const double akp = a[(size_t)k * m + p], akq = a[(size_t)k * m + q];
            a[(size_t)k * m + p] = a[(size_t)p * m + k] = akp - sn * (akq + tau * akp);
            a[(size_t)k * m + q] = a[(size_t)q * m + k] = akq + sn * (akp - tau * akq);
          }
          const double vp = v[(size_t)p * m + k], vq = v[(size_t)q * m + k];  // eigenvector rows p, q
          v[(size_t)p * m + k] = vp - sn * (vq + tau * vp);
          v[(size_t)q * m + k] = vq + sn * (vp - tau * vq);
        }
      }
  }
  std::vector<int> ord(m);
  for (int i = 0; i < m; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(),
                   [&](int x, int y) { return a[(size_t)x * m + x] > a[(size_t)y * m + y]; });
  for (int i = 0; i < m; i++) {
    w[i] = a[(size_t)ord[i] * m + ord[i]];
    std::memcpy(V + (size_t)i * m, &v[(size_t)ord[i] * m], (size_t)m * 8);
  }
}

// L⁻¹ (32 x 32 row-major, lower) of the Cholesky factor G = LLᵀ; false when a pivot is not safely positive
bool inv_chol32(const double* G, double* Linv) {
  constexpr int B = kPcsBlock;
  double L[B * B] = {0.0};
  for (int j = 0; j < B; j++) {
    double d = G[j * B + j];
    for (int k = 0; k < j; k++) d -= L[j * B + k] * L[j * B + k];
    if (!(d > 1e-13 * G[j * B + j]) || !std::isfinite(d)) return false;
    L[j * B + j] = std::sqrt(d);
    for (int i = j + 1; i < B; i++) {
      double v = 0.5 * (G[i * B + j] + G[j * B + i]);
      for (int k = 0; k < j; k++) v -= L[i * B + k] * L[j * B + k];
      L[i * B + j] = v / L[j * B + j];
    }
  }
  std::fill(Linv, Linv + B * B, 0.0);
  for (int j = 0; j < B; j++) {
    Linv[j * B + j] = 1.0 / L[j * B + j];
    for (int i = j + 1; i < B; i++) {
      double v = 0.0;
      for (int k = j; k < i; k++) v -= L[i * B + k] * Linv[k * B + j];
      Linv[i * B + j] = v / L[i * B + i];
    }
  }
  return true;
}

}  // namespace
}  // namespace gbm

extern "C" int gbm_debug_sym_eig(const double* A, int m, double* w, double* V) {
  if (!A || !w || !V || m < 1 || m > 64) return fail(GBM_E_ARG, "gbm_debug_sym_eig: A, w, V non-NULL and 1 <= m <= 64");
  for (int e = 0; e < m * m; e++)
    if (!std::isfinite(A[e])) return fail(GBM_E_ARG, "gbm_debug_sym_eig: A has a NaN/Inf entry");
  sym_eig(A, m, w, V);
  return GBM_OK;
}

extern "C" int gbm_session_pcs(gbm_session* s, const int64_t* idx, int64_t n_train, int kind, int64_t k, double tol,
                               int64_t max_iter, double* vecs_out, double* vals_out, double* trace_out,
                               double* resid_out, int64_t* iters_out) {
  RoctxRange r_("gbm_session_pcs");
  set_error("");
  constexpr int B = kPcsBlock;
  if (kind != GBM_PCS_GRM && kind != GBM_PCS_REFERENCE)
    return fail(GBM_E_ARG, "gbm_session_pcs: kind must be 0 (GBM_PCS_GRM) or 1 (GBM_PCS_REFERENCE)");
  if (k < 1 || k > 16) return fail(GBM_E_ARG, "gbm_session_pcs: k must be in [1, 16]");
  if (n_train < 2 * B)
    return fail(GBM_E_ARG, "gbm_session_pcs: n_train must be at least 64 (twice the block width of 32)");
  if (!(tol > 0.0) || !std::isfinite(tol)) return fail(GBM_E_ARG, "gbm_session_pcs: tol must be finite and > 0");
  if (max_iter < 1) return fail(GBM_E_ARG, "gbm_session_pcs: max_iter must be >= 1");
  if (!vecs_out || !vals_out) return fail(GBM_E_ARG, "gbm_session_pcs: vecs_out and vals_out must not be NULL");
  if (!s) return fail(GBM_E_ARG, "gbm_session_pcs: session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(ensure_training(s, idx, n_train, 0));
  hipStream_t st = s->stream.s;
  const int64_t nT = s->nT, npadT = s->npadT, gdimT = s->gdimT, ld = npadT;
  const int64_t wsb = gbm_dev_rows_times_sym_workspace(nT, B), rchunks = pcs_resid_chunks(nT);
  // the small exchange area (doubles): Gram results, Ritz rows + θ, the two inverse factors, residual partials, trace
  const int64_t oG = 0, oS = 2048, oL = oS + 1088, oL2 = oL + 1024, oR = oL2 + 1024, oT = oR + rchunks * 16;
  for (gbm::DevBuf* b : {&s->pcQ, &s->pcY, &s->pcW}) GBM_TRY(ensure(*b, s->dev, B * ld * 8));
  GBM_TRY(ensure(s->pcV, s->dev, 16 * ld * 8));
  GBM_TRY(ensure(s->pcws, s->dev, wsb));
  GBM_TRY(ensure(s->pcgram, s->dev, pcs_gram_workspace(nT)));
  GBM_TRY(ensure(s->pcsmall, s->dev, (oT + 2) * 8));
  double *Q = (double*)s->pcQ.p, *Y = (double*)s->pcY.p, *W = (double*)s->pcW.p, *V = (double*)s->pcV.p;
  double* sm = (double*)s->pcsmall.p;
  double* gpart = (double*)s->pcgram.p;
  // K = Gc/q, both triangles, into the solve's scratch copy (Gc itself is never written)
  double* K = (double*)s->Gw.p;
  GBM_TRY(gbm_dev_grm_symmetrize((const double*)s->Gc.p, gdimT, nT, 1.0 / (double)s->q, K, gdimT, st));
  const double *m = nullptr, *sd = nullptr;
  if (kind == GBM_PCS_REFERENCE) {
    GBM_TRY(ensure(s->pcm, s->dev, npadT * 8));
    GBM_TRY(ensure(s->pcsd, s->dev, npadT * 8));
    GBM_TRY(ensure(s->pcrt, s->dev, nT * 8));
    GBM_TRY(launch_pcs_colstats(K, gdimT, nT, (double*)s->pcm.p, (double*)s->pcsd.p, st));
    std::vector<double> sh((size_t)nT);
    GBM_HIP_TRY(hipMemcpyAsync(sh.data(), s->pcsd.p, nT * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    double smax = 0.0;
    for (double v : sh) smax = std::isfinite(v) ? std::max(smax, v) : std::numeric_limits<double>::infinity();
    for (int64_t j = 0; j < nT; j++)
      if (!(sh[(size_t)j] > std::numeric_limits<double>::epsilon() * smax) || !std::isfinite(smax))
        return fail(GBM_E_DATA, "gbm_session_pcs: column " + std::to_string(j + 1) +
                                    " of the relationship matrix has no variance (the reference operator "
                                    "standardises the columns, src/gwas.jl:130)");
    m = (const double*)s->pcm.p;
    sd = (const double*)s->pcsd.p;
    GBM_TRY(launch_pcs_rowtrace(K, gdimT, nT, m, sd, (double*)s->pcrt.p, st));
    GBM_TRY(launch_pcs_sum((const double*)s->pcrt.p, 1, nT, sm + oT, st));
  } else {
    GBM_TRY(launch_pcs_sum(K, gdimT + 1, nT, sm + oT, st));
  }
  auto apply = [&](const double* Qin, double* Yout) -> int {  // Yout = M Qin (W is scratch)
    GBM_TRY(gbm_dev_rows_times_sym(K, gdimT, nT, Qin, ld, B, Yout, ld, s->pcws.p, wsb, st));
    if (kind == GBM_PCS_REFERENCE) {
      GBM_TRY(launch_pcs_ref_mid(Qin, ld, Yout, ld, nT, m, sd, W, ld, st));
      GBM_TRY(gbm_dev_rows_times_sym(K, gdimT, nT, W, ld, B, Yout, ld, s->pcws.p, wsb, st));
      GBM_TRY(launch_pcs_ref_post(W, ld, nT, m, Yout, ld, st));
    }
    return GBM_OK;
  };
  std::vector<double> hG(2 * B * B), hS(B * B + B), hL(B * B), hL2(B * B), hR((size_t)(rchunks * 16));
  // Out = L⁻¹ In for the Gram matrix G = In Inᵀ already on the host
  auto ortho_pass = [&](const double* Gh, std::vector<double>& Lh, int64_t off, const double* In, double* Out,
                        bool& ok) -> int {
    ok = inv_chol32(Gh, Lh.data());
    if (!ok) return GBM_OK;
    GBM_HIP_TRY(hipMemcpyAsync(sm + off, Lh.data(), B * B * 8, hipMemcpyHostToDevice, st));
    return launch_pcs_transform(sm + off, In, ld, nT, B, Out, ld, st);
  };
  const char* rankmsg = "gbm_session_pcs: the block lost rank (the operator has fewer than 32 eigenvalues that "
                        "are distinguishable from zero)";
  // start block: hashed, then CholQR twice (W → Y → Q)
  bool ok = true;
  GBM_TRY(launch_pcs_start(W, ld, nT, 0x9C5ull, st));
  GBM_TRY(launch_pcs_gram(W, ld, W, ld, nT, 1, gpart, sm + oG, st));
  GBM_HIP_TRY(hipMemcpyAsync(hG.data(), sm + oG, B * B * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  GBM_TRY(ortho_pass(hG.data(), hL, oL, W, Y, ok));
  if (!ok) return fail(GBM_E_DATA, rankmsg);
  GBM_TRY(launch_pcs_gram(Y, ld, Y, ld, nT, 1, gpart, sm + oG, st));
  GBM_HIP_TRY(hipMemcpyAsync(hG.data(), sm + oG, B * B * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  GBM_TRY(ortho_pass(hG.data(), hL2, oL2, Y, Q, ok));
  if (!ok) return fail(GBM_E_DATA, rankmsg);

  double theta[B], res[16] = {0.0};
  int64_t it = 0;
  bool converged = false;
  for (;;) {
    it++;
    GBM_TRY(apply(Q, Y));
    GBM_TRY(launch_pcs_gram(Q, ld, Y, ld, nT, 2, gpart, sm + oG, st));
    GBM_HIP_TRY(hipMemcpyAsync(hG.data(), sm + oG, 2 * B * B * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    for (double v : hG)
      if (!std::isfinite(v)) return fail(GBM_E_DATA, "gbm_session_pcs: the iteration produced a NaN/Inf value");
    sym_eig(hG.data(), B, theta, hS.data());  // T = QYᵀ (symmetrised inside); rows of hS are the Ritz vectors
    if (!(theta[0] > 0.0)) return fail(GBM_E_DATA, "gbm_session_pcs: the relationship matrix has no positive eigenvalue");
    std::memcpy(hS.data() + B * B, theta, B * 8);
    GBM_HIP_TRY(hipMemcpyAsync(sm + oS, hS.data(), (B * B + B) * 8, hipMemcpyHostToDevice, st));
    GBM_TRY(launch_pcs_resid(sm + oS, Q, ld, Y, ld, nT, (int)k, sm + oR, st));
    GBM_HIP_TRY(hipMemcpyAsync(hR.data(), sm + oR, rchunks * 16 * 8, hipMemcpyDeviceToHost, st));
    // first CholQR pass of the next block behind the residuals: W = L⁻¹Y, then its Gram matrix
    GBM_TRY(ortho_pass(hG.data() + B * B, hL, oL, Y, W, ok));
    if (ok) {
      GBM_TRY(launch_pcs_gram(W, ld, W, ld, nT, 1, gpart, sm + oG, st));
      GBM_HIP_TRY(hipMemcpyAsync(hG.data(), sm + oG, B * B * 8, hipMemcpyDeviceToHost, st));
    }
    GBM_HIP_TRY(hipStreamSynchronize(st));
    double rmax = 0.0;
    for (int64_t i = 0; i < k; i++) {
      double r2 = 0.0;
      for (int64_t c = 0; c < rchunks; c++) r2 += hR[(size_t)(c * 16 + i)];
      res[i] = std::sqrt(r2) / theta[0];
      rmax = std::max(rmax, res[i]);
    }
    if (rmax < tol) {
      converged = true;
      break;
    }
    if (it >= max_iter) break;
    if (!ok) return fail(GBM_E_DATA, rankmsg);
    GBM_TRY(ortho_pass(hG.data(), hL2, oL2, W, Q, ok));
    if (!ok) return fail(GBM_E_DATA, rankmsg);
  }
  // v_i = Qᵀs_i (rows of V), renormalised and sign-fixed on the host
  GBM_TRY(launch_pcs_transform(sm + oS, Q, ld, nT, (int)k, V, ld, st));
  std::vector<double> hv((size_t)(k * nT));
  double tr = 0.0;
  GBM_HIP_TRY(hipMemcpy2DAsync(hv.data(), nT * 8, V, ld * 8, nT * 8, k, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipMemcpyAsync(&tr, sm + oT, 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  for (int64_t i = 0; i < k; i++) {
    double* v = &hv[(size_t)(i * nT)];
    double nn = 0.0, big = 0.0;
    int64_t at = 0;
    for (int64_t r = 0; r < nT; r++) {
      nn += v[r] * v[r];
      if (std::fabs(v[r]) > big) {
        big = std::fabs(v[r]);
        at = r;
      }
    }
    const double sc = (v[at] < 0.0 ? -1.0 : 1.0) / std::sqrt(nn);
    for (int64_t r = 0; r < nT; r++) vecs_out[i * nT + r] = v[r] * sc;
    vals_out[i] = theta[i];
    if (resid_out) resid_out[i] = res[i];
  }
  if (trace_out) *trace_out = tr;
  if (iters_out) *iters_out = it;
  if (!converged) {
    char num[64];
    snprintf(num, sizeof(num), "%.3g against tol %.3g", *std::max_element(res, res + k), tol);
    set_error("warning: gbm_session_pcs: max_iter = " + std::to_string(max_iter) +
              " reached before convergence (largest relative residual " + num +
              "; the pairs returned are the last iteration's)");
  }
  return GBM_OK;
}

// ---- epistasis feature scan (reference transform1 / transform2, src/transformation.jl:130-468) ----------------
// include/gbm.h states the model and the rules. Per call: one gather (launch_pair_prep), then per panel of i-rows
// one scan launch and one selection; only the panels' candidates (<= k each) and the three counters come back.
extern "C" int gbm_session_pair_scan(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                                     const int64_t* loci, int64_t l, int op, double eps, int use_abs,
                                     double var_threshold, int commutative, int64_t panel_rows, int64_t k,
                                     int64_t* top_index_out, double* top_beta_out, int64_t* n_top_out,
                                     double* beta_out, int64_t* tested_out, int64_t* degenerate_out) {
  RoctxRange r_("gbm_session_pair_scan");
  set_error("");
  if (!s) return fail(GBM_E_ARG, "gbm_session_pair_scan: session is NULL");
  if (!y || !top_index_out || !top_beta_out || !n_top_out)
    return fail(GBM_E_ARG, "gbm_session_pair_scan: y, top_index_out, top_beta_out and n_top_out must not be NULL");
  if (op < GBM_PAIR_OP_MULT || op > GBM_PAIR_OP_LOG10EPS)
    return fail(GBM_E_ARG, "gbm_session_pair_scan: op must be one of GBM_PAIR_OP_* (0 to 5)");
  const bool unary = op >= GBM_PAIR_OP_SQUARE;
  if (unary && commutative) return fail(GBM_E_ARG, "gbm_session_pair_scan: commutative applies to the binary operations only");
  if (n_train < 3) return fail(GBM_E_ARG, "gbm_session_pair_scan: n_train must be at least 3");
  if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(GBM_E_ARG, "gbm_session_pair_scan: eps must be finite and >= 0");
  if (std::isnan(var_threshold)) return fail(GBM_E_ARG, "gbm_session_pair_scan: var_threshold is NaN");
  if (panel_rows < 0 || panel_rows % 64 != 0)
    return fail(GBM_E_ARG, "gbm_session_pair_scan: panel_rows must be 0 or a positive multiple of 64");
  std::lock_guard<std::mutex> lock(s->mu);
  GBM_HIP_TRY(hipSetDevice(s->dev));
  GBM_TRY(check_idx(s, idx, n_train, "gbm_session_pair_scan"));
  if (!loci) {
    if (l != s->p) return fail(GBM_E_ARG, "gbm_session_pair_scan: l must equal p when loci is NULL");
  } else {
    if (l < 1 || l > s->p) return fail(GBM_E_ARG, "gbm_session_pair_scan: l must be in [1, p]");
    std::vector<char> seen((size_t)s->p, 0);
    for (int64_t j = 0; j < l; j++) {
      if (loci[j] < 0 || loci[j] >= s->p)
        return fail(GBM_E_ARG, "gbm_session_pair_scan: locus index " + std::to_string(loci[j]) + " out of range [0, " +
                                   std::to_string(s->p) + ")");
      if (seen[(size_t)loci[j]]) return fail(GBM_E_ARG, "gbm_session_pair_scan: locus indices must be distinct");
      seen[(size_t)loci[j]] = 1;
    }
  }
  const int64_t li = unary ? 1 : l;  // i-rows
  const int64_t slopes = li * l;
  if (l > ((int64_t)1 << 30)) return fail(GBM_E_ARG, "gbm_session_pair_scan: too many loci");
  if (k < 1 || k > 65536 || k > slopes)
    return fail(GBM_E_ARG, "gbm_session_pair_scan: k must be in [1, 65536] and at most the number of slopes (" +
                               std::to_string(slopes) + ")");
  double ybar = 0.0;
  for (int64_t i = 0; i < n_train; i++) {
    if (!std::isfinite(y[i])) return fail(GBM_E_ARG, "gbm_session_pair_scan: y has a NaN/Inf value");
    ybar += y[i];
  }
  ybar /= (double)n_train;
  int64_t prow = panel_rows;
  if (prow == 0) {
    prow = ((int64_t)256 << 20) / (8 * l) / 64 * 64;
    if (prow < 64) prow = 64;
  }
  if (unary || prow > li) prow = li;
  const int64_t npanels = (li + prow - 1) / prow;
  if (beta_out && npanels > 1)
    return fail(GBM_E_ARG, "gbm_session_pair_scan: beta_out needs every slope in one panel (" +
                               std::to_string(npanels) + " panels of " + std::to_string(prow) + " rows here)");
  hipStream_t st = s->stream.s;
  const int64_t ldw = pair_scan_ldw(n_train), mmax = prow * l;
  GBM_TRY(ensure(s->psW, s->dev, l * ldw * 8));
  GBM_TRY(ensure(s->psidx, s->dev, n_train * 8));
  GBM_TRY(ensure(s->psloci, s->dev, l * 8));
  GBM_TRY(ensure(s->psy, s->dev, n_train * 8));
  GBM_TRY(ensure(s->psyc, s->dev, ldw * 8));
  GBM_TRY(ensure(s->psvar, s->dev, l * 8));
  GBM_TRY(ensure(s->psskip, s->dev, l * 4));
  GBM_TRY(ensure(s->psbeta, s->dev, mmax * 8));
  GBM_TRY(ensure(s->pscnt, s->dev, 3 * 8));
  GBM_TRY(ensure(s->pssel, s->dev, pair_sel_state_bytes()));
  GBM_TRY(ensure(s->psblk, s->dev, 2 * pair_sel_blocks(mmax) * 8));
  GBM_TRY(ensure(s->pscidx, s->dev, k * 8));
  GBM_TRY(ensure(s->pscbeta, s->dev, k * 8));
  GBM_HIP_TRY(hipMemcpyAsync(s->psidx.p, idx, n_train * 8, hipMemcpyHostToDevice, st));
  if (loci) GBM_HIP_TRY(hipMemcpyAsync(s->psloci.p, loci, l * 8, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemcpyAsync(s->psy.p, y, n_train * 8, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemsetAsync(s->pscnt.p, 0, 3 * 8, st));
  GBM_TRY(launch_pair_prep((const double*)s->Xt.p, s->npad, (const int64_t*)s->psidx.p, n_train,
                           loci ? (const int64_t*)s->psloci.p : nullptr, l, eps, use_abs ? 1 : 0, var_threshold,
                           (const double*)s->psy.p, ybar, (double*)s->psW.p, ldw, (double*)s->psvar.p,
                           (int32_t*)s->psskip.p, (double*)s->psyc.p, st));
  struct Cand {
    int64_t index;
    double beta;
  };
  std::vector<Cand> cands;
  std::vector<int64_t> hidx((size_t)k);
  std::vector<double> hbeta((size_t)k);
  const int64_t tot_off = pair_sel_state_bytes() - 16;
  for (int64_t pn = 0; pn < npanels; pn++) {
    const int64_t i0 = pn * prow, rows = std::min(prow, li - i0), m = rows * l;
    GBM_TRY(launch_pair_scan(op, (const double*)s->psW.p, ldw, n_train, l, li, i0, rows, (const double*)s->psyc.p,
                             (const int32_t*)s->psskip.p, commutative ? 1 : 0, (double*)s->psbeta.p,
                             (unsigned long long*)s->pscnt.p, st));
    GBM_TRY(launch_pair_select((const double*)s->psbeta.p, m, i0 * l, eps, k, s->pssel.p, (int64_t*)s->psblk.p,
                               (int64_t*)s->pscidx.p, (double*)s->pscbeta.p, st));
    int64_t tot[2] = {0, 0};
    GBM_HIP_TRY(hipMemcpyAsync(tot, (const char*)s->pssel.p + tot_off, 16, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    const int64_t got = std::min(k, tot[0] + tot[1]);
    if (got > 0) {
      GBM_HIP_TRY(hipMemcpyAsync(hidx.data(), s->pscidx.p, got * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipMemcpyAsync(hbeta.data(), s->pscbeta.p, got * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));
      for (int64_t c = 0; c < got; c++) cands.push_back({hidx[(size_t)c], hbeta[(size_t)c]});
    }
  }
  unsigned long long cnt[3] = {0, 0, 0};
  GBM_HIP_TRY(hipMemcpyAsync(cnt, s->pscnt.p, 3 * 8, hipMemcpyDeviceToHost, st));
  GBM_HIP_TRY(hipStreamSynchronize(st));
  if (cnt[2] > 0)
    return fail(GBM_E_DATA, "gbm_session_pair_scan: the operation gave a non-finite value (or sums that overflow) in " +
                                std::to_string(cnt[2]) + " of the tested " + (unary ? "loci" : "pairs") +
                                " (reference src/transformation.jl:391-405: a larger eps and/or use_abs)");
  std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) {
    const double fa = std::fabs(a.beta), fb = std::fabs(b.beta);
    return fa > fb || (fa == fb && a.index < b.index);
  });
  const int64_t ntop = std::min<int64_t>(k, (int64_t)cands.size());
  for (int64_t c = 0; c < ntop; c++) {
    top_index_out[c] = cands[(size_t)c].index;
    top_beta_out[c] = cands[(size_t)c].beta;
  }
  *n_top_out = ntop;
  if (beta_out) {
    GBM_HIP_TRY(hipMemcpyAsync(beta_out, s->psbeta.p, slopes * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
  }
  if (tested_out) *tested_out = (int64_t)cnt[0];
  if (degenerate_out) *degenerate_out = (int64_t)cnt[1];
  return GBM_OK;
}
