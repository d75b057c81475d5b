// ---- leading principal components of the cached GRM (reference gwasols' PC1, src/gwas.jl:130,234) ----
// Block subspace iteration with a Rayleigh–Ritz step every iteration (include/gbm.h states the operators, the stop
// rule and the sign rule; DESIGN.md §4.11 the schedule). Per iteration the device applies the operator to the
// orthonormal block Q (one or two gbm_dev_rows_times_sym), forms T = QYᵀ and YYᵀ, and the host answers with the
// Ritz vectors of T (cyclic Jacobi) and the inverse Cholesky factor of YYᵀ; the residuals and the first CholQR
// pass run behind that, the second pass behind one more 8 KB exchange: two host synchronisations per iteration.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "session.h"

using namespace gbm;

// Eigen-decomposition of the symmetric m x m A (m <= 64) by cyclic Jacobi rotations: w descending, V[i·m + r] =
// component r of eigenvector i. Only the upper triangle's values matter (A is symmetrised from both).
static void sym_eig(const double* A, int m, double* w, double* V) {
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
static bool inv_chol32(const double* G, double* Linv) {
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
  GBM_SESSION_ENTER(s);
  GBM_TRY(ensure_training(s, idx, n_train, 0));
  hipStream_t st = s->stream.s;
  gbm_session::Pcs& pc = s->pc;
  const int64_t nT = s->nT, npadT = s->npadT, gdimT = s->gdimT, ld = npadT;
  const int64_t wsb = gbm_dev_rows_times_sym_workspace(nT, B), rchunks = pcs_resid_chunks(nT);
  // the small exchange area (doubles): Gram results, Ritz rows + θ, the two inverse factors, residual partials, trace
  const int64_t oG = 0, oS = 2048, oL = oS + 1088, oL2 = oL + 1024, oR = oL2 + 1024, oT = oR + rchunks * 16;
  for (DevBuf* b : {&pc.Q, &pc.Y, &pc.W}) GBM_TRY(ensure(*b, s->dev, B * ld * 8));
  GBM_TRY(ensure(pc.V, s->dev, 16 * ld * 8));
  GBM_TRY(ensure(pc.ws, s->dev, wsb));
  GBM_TRY(ensure(pc.gram, s->dev, pcs_gram_workspace(nT)));
  GBM_TRY(ensure(pc.small, s->dev, (oT + 2) * 8));
  double *Q = pc.Q.as<double>(), *Y = pc.Y.as<double>(), *W = pc.W.as<double>(), *V = pc.V.as<double>();
  double *sm = pc.small.as<double>(), *gpart = pc.gram.as<double>();
  // K = Gc/q, both triangles, into the solve's scratch copy (Gc itself is never written)
  double* K = s->Gw.as<double>();
  GBM_TRY(gbm_dev_grm_symmetrize(s->Gc.as<const double>(), gdimT, nT, 1.0 / (double)s->q, K, gdimT, st));
  const double *m = nullptr, *sd = nullptr;
  if (kind == GBM_PCS_REFERENCE) {
    for (DevBuf* b : {&pc.m, &pc.sd}) GBM_TRY(ensure(*b, s->dev, npadT * 8));
    GBM_TRY(ensure(pc.rt, s->dev, nT * 8));
    GBM_TRY(launch_pcs_colstats(K, gdimT, nT, pc.m.as<double>(), pc.sd.as<double>(), st));
    std::vector<double> sh((size_t)nT);
    GBM_HIP_TRY(hipMemcpyAsync(sh.data(), pc.sd.p, nT * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    double smax = 0.0;
    for (double v : sh) smax = std::isfinite(v) ? std::max(smax, v) : std::numeric_limits<double>::infinity();
    for (int64_t j = 0; j < nT; j++)
      if (!(sh[(size_t)j] > std::numeric_limits<double>::epsilon() * smax) || !std::isfinite(smax))
        return fail(GBM_E_DATA, "gbm_session_pcs: column " + std::to_string(j + 1) +
                                    " of the relationship matrix has no variance (the reference operator "
                                    "standardises the columns, src/gwas.jl:130)");
    m = pc.m.as<const double>();
    sd = pc.sd.as<const double>();
    GBM_TRY(launch_pcs_rowtrace(K, gdimT, nT, m, sd, pc.rt.as<double>(), st));
    GBM_TRY(launch_pcs_sum(pc.rt.as<const double>(), 1, nT, sm + oT, st));
  } else {
    GBM_TRY(launch_pcs_sum(K, gdimT + 1, nT, sm + oT, st));
  }
  auto apply = [&](const double* Qin, double* Yout) -> int {  // Yout = M Qin (W is scratch)
    GBM_TRY(gbm_dev_rows_times_sym(K, gdimT, nT, Qin, ld, B, Yout, ld, pc.ws.p, wsb, st));
    if (kind == GBM_PCS_REFERENCE) {
      GBM_TRY(launch_pcs_ref_mid(Qin, ld, Yout, ld, nT, m, sd, W, ld, st));
      GBM_TRY(gbm_dev_rows_times_sym(K, gdimT, nT, W, ld, B, Yout, ld, pc.ws.p, wsb, st));
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
