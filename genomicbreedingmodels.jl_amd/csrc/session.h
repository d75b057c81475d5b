// The device-resident genotype session and the steps its translation units share (session.cpp: life cycle,
// training-set cache, GBLUP fit and predict; session_reml.cpp, session_linear.cpp, session_gwas.cpp,
// session_pcs.cpp, session_pairscan.cpp: one analysis each). Not part of the ABI.
//
// Every device buffer is a DevBuf sized with ensure(): a session's buffers only grow, so a call on a training set
// no larger than an earlier one allocates nothing. Pitches and sizes (npadT, gdimT) are those of the current
// training set, whatever the capacity, and a call reads only what it has written.
#pragma once
#include <mutex>
#include <vector>

#include "gbm_internal.h"
#include "host_util.h"

struct gbm_session {
  std::mutex mu;
  int dev = 0;
  gbm::Stream stream;
  int64_t n = 0, p = 0, npad = 0;
  gbm::DevBuf Xt;  // p x npad raw genotypes
  // training-set cache (key: the entry set and the standardisation mode)
  std::vector<int64_t> key;
  int mode = -1;  // 0: GBLUP standardisation, 1: centre only (glmnet standardize=false)
  int64_t nT = 0, npadT = 0, gdimT = 0, q = 0;
  gbm::DevBuf idx32, Z, mean, sd, keep, qd, Gc, wsg;
  // per-fit buffers (sized for the cached training set)
  gbm::DevBuf Gw, wss, Y, A, gebv, mu_d, info, B, msum, terms;
  // predict buffers
  gbm::DevBuf bvec, part, pout;
  int64_t builds = 0, hits = 0;
  // genotypes that are diploid dosages/2 (2x ∈ {0, 1, 2} in every cell: synthetic sessions by construction,
  // others checked on the device once, when a fit first asks for it): grm_mode exact / auto
  // (gbm_session_set_grm_mode, else GBM_GRM) builds the training GRM with the exact-integer kernels
  // (grm_exact.hip) from the gathered training dosages
  bool dosage2 = false, dosage_checked = false;
  int grm_mode = GBM_GRM_DEFAULT;
  bool exact_cached = false;  // the cached training GRM is the exact one (part of the cache key)
  gbm::DevBuf D8T, wsx, mean2, sd2, keep2, q2;
  // GWAS scan (gbm_session_gwas): the chunk of locus rows being whitened, the statistics of all p loci and
  // the count of tested loci
  struct Gwas { gbm::DevBuf W, z, b, cnt; } gw;
  // elastic-net path (gbm_session_enet_path): the packed active rows and their Gram blocks, the per-slot
  // constants and coefficients (two copies, by pass parity), the residual, the per-locus x2, the chain's
  // partial dots and block maxima, the pass scalars and the rows of one admission
  struct Enet { gbm::DevBuf Za, W, x2a, inv, b, e, x2, part, blk, red, rows, gws; } en;
  // principal components (gbm_session_pcs): the vector blocks Q, Y, W and the rotated output rows, the block
  // product's partials, the Gram partials, the small matrices exchanged with the host, and K's column statistics
  struct Pcs { gbm::DevBuf Q, Y, W, V, ws, gram, small, m, sd, rt; } pc;
  // epistasis scan (gbm_session_pair_scan): the gathered work matrix, the row and locus indices, y and yc, the
  // loci's variances and skip flags, one panel of slopes, the counters, the selection's state and block counts,
  // and the candidates
  struct PairScan { gbm::DevBuf W, idx, loci, y, yc, var, skip, beta, cnt, sel, blk, cidx, cbeta; } ps;
};

// A session serialises its own calls and runs them on its device: the first statement after an entry's argument
// checks (the session is named s in every entry)
#define GBM_SESSION_ENTER(s)                 \
  std::lock_guard<std::mutex> lock_(s->mu); \
  GBM_HIP_TRY(hipSetDevice(s->dev))

namespace gbm {

// ---- session.cpp: the training-set cache and the steps on it ----
int check_idx(const gbm_session* s, const int64_t* idx, int64_t m, const char* what);
// Standardise (mode 0) or centre (mode 1) the training set idx and build its GRM (cached).
int ensure_training(gbm_session* s, const int64_t* idx, int64_t nT, int mode = 0);
int ensure_rhs(gbm_session* s, int64_t nrhs);
int upload_y(gbm_session* s, const double* Y, int64_t ldy, int64_t nrhs);
// Solve (G·inv_q + λI) on the cached GRM for the nrhs phenotype columns already in s->Y
// (inv_q = 1/q for GBLUP, 1 for the unscaled ridge kernel).
int solve_cached(gbm_session* s, int64_t nrhs, double lambda, double inv_q);
// The marker effects of the nrhs device columns A (pitch lda) on the cached training set: g = Zᵀa scaled by inv_q
// into s->B[t, :], and s->msum[t] = Σ_j mean_j B[t, j] (gbm_dev_marker_effects on the cached Z, mean, sd and keep)
int effects_cached(gbm_session* s, const double* A, int64_t lda, int64_t nrhs, double inv_q);
// out[t·ldo + i] = b0_t + X[idx[i], :] b_t for nrhs coefficient rows (intercept first): the host rows b (pitch
// ldb), or with b_dev (nrhs = 1) the host intercept b[0] and the p effects on the device
int predict_at(gbm_session* s, const double* b, int64_t ldb, const double* b_dev, int64_t nrhs, const int64_t* idx,
               int64_t m, double* out, int64_t ldo);
struct YStats {
  double mean, ss, sd;  // ȳ, Σ(y − ȳ)², the population sd
};
YStats centre_y(const double* y, int64_t n);

// ---- session_reml.cpp ----
// t = {logdet V_λ, 1ᵀV_λ⁻¹1, 1ᵀV_λ⁻¹y, yᵀV_λ⁻¹y} of the factor that solve_cached(s, 1, λ, ·) left
int solve_terms(gbm_session* s, double t[4]);
// The null-model REML search of gbm_session_reml on the cached training set (ys: the standardised y)
int reml_cached(gbm_session* s, const std::vector<double>& ys, RemlResult& res);

}  // namespace gbm
