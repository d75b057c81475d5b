// ---- epistasis feature scan (reference transform1 / transform2, src/transformation.jl:130-468) ----------------
// include/gbm.h states the model and the rules. Per call: one gather (launch_pair_prep), then per panel of i-rows
// one scan launch and one selection; only the panels' candidates (<= k each) and the three counters come back.
#include <algorithm>
#include <cmath>

#include "session.h"

using namespace gbm;

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
  GBM_SESSION_ENTER(s);
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
  for (int64_t i = 0; i < n_train; i++)
    if (!std::isfinite(y[i])) return fail(GBM_E_ARG, "gbm_session_pair_scan: y has a NaN/Inf value");
  const double ybar = centre_y(y, n_train).mean;
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
  gbm_session::PairScan& ps = s->ps;
  const int64_t ldw = pair_scan_ldw(n_train), mmax = prow * l;
  GBM_TRY(ensure(ps.W, s->dev, l * ldw * 8));
  for (DevBuf* b : {&ps.idx, &ps.y}) GBM_TRY(ensure(*b, s->dev, n_train * 8));
  for (DevBuf* b : {&ps.loci, &ps.var}) GBM_TRY(ensure(*b, s->dev, l * 8));
  GBM_TRY(ensure(ps.yc, s->dev, ldw * 8));
  GBM_TRY(ensure(ps.skip, s->dev, l * 4));
  GBM_TRY(ensure(ps.beta, s->dev, mmax * 8));
  GBM_TRY(ensure(ps.cnt, s->dev, 3 * 8));
  GBM_TRY(ensure(ps.sel, s->dev, pair_sel_state_bytes()));
  GBM_TRY(ensure(ps.blk, s->dev, 2 * pair_sel_blocks(mmax) * 8));
  for (DevBuf* b : {&ps.cidx, &ps.cbeta}) GBM_TRY(ensure(*b, s->dev, k * 8));
  GBM_HIP_TRY(hipMemcpyAsync(ps.idx.p, idx, n_train * 8, hipMemcpyHostToDevice, st));
  if (loci) GBM_HIP_TRY(hipMemcpyAsync(ps.loci.p, loci, l * 8, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemcpyAsync(ps.y.p, y, n_train * 8, hipMemcpyHostToDevice, st));
  GBM_HIP_TRY(hipMemsetAsync(ps.cnt.p, 0, 3 * 8, st));
  GBM_TRY(launch_pair_prep(s->Xt.as<const double>(), s->npad, ps.idx.as<const int64_t>(), n_train,
                           loci ? ps.loci.as<const int64_t>() : nullptr, l, eps, use_abs ? 1 : 0, var_threshold,
                           ps.y.as<const double>(), ybar, ps.W.as<double>(), ldw, ps.var.as<double>(),
                           ps.skip.as<int32_t>(), ps.yc.as<double>(), st));
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
    GBM_TRY(launch_pair_scan(op, ps.W.as<const double>(), ldw, n_train, l, li, i0, rows, ps.yc.as<const double>(),
                             ps.skip.as<const int32_t>(), commutative ? 1 : 0, ps.beta.as<double>(),
                             ps.cnt.as<unsigned long long>(), st));
    GBM_TRY(launch_pair_select(ps.beta.as<const double>(), m, i0 * l, eps, k, ps.sel.p, ps.blk.as<int64_t>(),
                               ps.cidx.as<int64_t>(), ps.cbeta.as<double>(), st));
    int64_t tot[2] = {0, 0};
    GBM_HIP_TRY(hipMemcpyAsync(tot, ps.sel.as<const char>() + tot_off, 16, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
    const int64_t got = std::min(k, tot[0] + tot[1]);
    if (got > 0) {
      GBM_HIP_TRY(hipMemcpyAsync(hidx.data(), ps.cidx.p, got * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipMemcpyAsync(hbeta.data(), ps.cbeta.p, got * 8, hipMemcpyDeviceToHost, st));
      GBM_HIP_TRY(hipStreamSynchronize(st));
      for (int64_t c = 0; c < got; c++) cands.push_back({hidx[(size_t)c], hbeta[(size_t)c]});
    }
  }
  unsigned long long cnt[3] = {0, 0, 0};
  GBM_HIP_TRY(hipMemcpyAsync(cnt, ps.cnt.p, 3 * 8, hipMemcpyDeviceToHost, st));
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
    GBM_HIP_TRY(hipMemcpyAsync(beta_out, ps.beta.p, slopes * 8, hipMemcpyDeviceToHost, st));
    GBM_HIP_TRY(hipStreamSynchronize(st));
  }
  if (tested_out) *tested_out = (int64_t)cnt[0];
  if (degenerate_out) *degenerate_out = (int64_t)cnt[1];
  return GBM_OK;
}
