// BayesA, BayesB and BayesC with an ordinal response (gbm_bayes_fit_ordinal; the reference's
// bayesian(...; response_type = "ordinal"), src/bayes.jl:28-36, 161-172; include/gbm.h states the
// sampler). The threshold (probit) model is gbm_bayes_fit's chain on a latent liability y* with the
// residual variance fixed at 1: an iteration replays bayes_abc.hip's steps 1 and 2 unchanged
// (bayes_enqueue_chain), then redraws y* from its truncated normals (ordinal_latent_kernel), moves
// the thresholds between the classes' extremes (ordinal_threshold_kernel), accumulates the class
// probabilities (ordinal_probs_kernel), and ends with gbm_bayes_fit's variance draws less varE's.
// The three kernels touch O(n K) bytes per iteration beside the chain's O(n p).
#include <algorithm>
#include <cmath>

#include "gibbs_common.h"

namespace gbm {
namespace {

constexpr int OSL = 2 * ORD_MAXK;  // min/max slots of a chunk: [2k] = min, [2k + 1] = max of y* in class k

// Step (a) for one chunk of IW individuals (the chain kernels' chunks): ŷ = y* − e, y* ~ TN(ŷ; t_z,
// t_{z+1}) from u01(A + 7, i), e = y* − ŷ; then the chunk's per-class min and max of y*: a wave
// reduction per class, the four waves' results through LDS, part[chunk][2k], [2k + 1] (+∞ / −∞ for
// a class with nobody in the chunk). yh (may be NULL) keeps ŷ for ordinal_probs_kernel.
__global__ void __launch_bounds__(IW) ordinal_latent_kernel(double* __restrict__ ys, double* __restrict__ e,
                                                            double* __restrict__ yh, const uint8_t* __restrict__ cls,
                                                            int64_t n, const OrdinalState* __restrict__ os,
                                                            double* __restrict__ part) {
  __shared__ double ts[ORD_MAXK + 1];
  __shared__ double red[IW / 64][OSL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = (int)os->K;
  if (tid <= K) ts[tid] = os->t[tid];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * IW + tid;
  int z = -1;
  double v = 0.0;
  if (i < n) {
    z = cls[i];
    const double yhat = ys[i] - e[i];
    const uint64_t A = 8 * (uint64_t)os->s.it;
    v = gibbs_truncnorm(yhat, ts[z], ts[z + 1], brr_u01(os->s.seed, A + 7, (uint64_t)i));
    ys[i] = v;
    e[i] = v - yhat;
    if (yh) yh[i] = yhat;
  }
  for (int k = 0; k < K; k++) {
    double mn = z == k ? v : INFINITY, mx = z == k ? v : -INFINITY;
    for (int o = 32; o > 0; o >>= 1) {
      mn = fmin(mn, __shfl_xor(mn, o));
      mx = fmax(mx, __shfl_xor(mx, o));
    }
    if (lane == 0) {
      red[wave][2 * k] = mn;
      red[wave][2 * k + 1] = mx;
    }
  }
  __syncthreads();
  if (tid < 2 * K) {
    const double a = red[0][tid], b = red[1][tid], c = red[2][tid], d = red[3][tid];
    part[(int64_t)blockIdx.x * OSL + tid] = (tid & 1) ? fmax(fmax(a, b), fmax(c, d)) : fmin(fmin(a, b), fmin(c, d));
  }
}

// Step (b) and the thresholds' share of (c), one workgroup: the C chunks' partials reduced per slot (thread
// = slot + 64 q takes the chunks q, q + 4, …; min and max do not depend on the order), then thread 0 moves
// t_2 … t_{K−1} in order and updates the running means of t_1 … t_{K−1}. K = 2: nothing moves.
__global__ void __launch_bounds__(256) ordinal_threshold_kernel(const double* __restrict__ part, int64_t C,
                                                                OrdinalState* __restrict__ os) {
  __shared__ double red[4][OSL];
  const int tid = threadIdx.x, slot = tid & 63, q = tid >> 6;
  const int K = (int)os->K;
  double a = (slot & 1) ? -INFINITY : INFINITY;
  if (slot < 2 * K)
    for (int64_t c = q; c < C; c += 4) {
      const double v = part[c * OSL + slot];
      a = (slot & 1) ? fmax(a, v) : fmin(a, v);
    }
  red[q][slot] = a;
  __syncthreads();
  if (tid != 0) return;
  const uint64_t A = 8 * (uint64_t)os->s.it;
  for (int m = 2; m < K; m++) {
    const int sx = 2 * (m - 1) + 1, sn = 2 * m;
    const double mx = fmax(fmax(red[0][sx], red[1][sx]), fmax(red[2][sx], red[3][sx]));
    const double mn = fmin(fmin(red[0][sn], red[1][sn]), fmin(red[2][sn], red[3][sn]));
    const double lo = fmax(mx, os->t[m - 1]), hi = fmin(mn, os->t[m + 1]);
    os->t[m] = lo + (hi - lo) * brr_u01(os->s.seed, A + 7, 0xFFFFFFFF00000000ull + (uint64_t)m);
  }
  if (brr_accumulate(&os->s)) {
    const double k = (double)(os->s.nsum + 1);
    for (int m = 1; m < K; m++) os->tbar[m] = os->tbar[m] * ((k - 1.0) / k) + os->t[m] / k;
  }
}

// The probabilities' share of (c), one thread per individual: the running means of
// P(class k | i) = Φ(t_{k+1} − ŷ_i) − Φ(t_k − ŷ_i) with the thresholds just updated (pbar n x K,
// column-major, pitch ldp). Nothing to do when the iteration is not gated or no probabilities were asked for.
__global__ void __launch_bounds__(256) ordinal_probs_kernel(const double* __restrict__ yh, int64_t n, int64_t ldp,
                                                            const OrdinalState* __restrict__ os,
                                                            double* __restrict__ pbar) {
  if (!pbar || !brr_accumulate(&os->s)) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int K = (int)os->K;
  const double kk = (double)(os->s.nsum + 1), w0 = (kk - 1.0) / kk;
  const double m = yh[i];
  double prev = 0.0;
  for (int k = 0; k < K; k++) {
    const double next = k + 1 < K ? gibbs_phi(os->t[k + 1] - m) : 1.0;
    pbar[k * ldp + i] = pbar[k * ldp + i] * w0 + (next - prev) / kk;
    prev = next;
  }
}

// bayes_final_kernel (bayes_abc.hip) without the draw of varE, which stays 1: S, BayesC's common varB, π; the
// running means of μ, mean_j varB_j and π; next iteration. The stream A + 2 stays unused.
__global__ void __launch_bounds__(256) ordinal_final_kernel(const double* __restrict__ vpart, int64_t nvb, int64_t p,
                                                            BayesState* __restrict__ st) {
  __shared__ double red[4];
  double sum[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    double a = 0.0;
    for (int64_t k = threadIdx.x; k < nvb; k += 256) a += vpart[5 * k + u];
    sum[u] = brr_block_sum<256>(a, red);
  }
  if (threadIdx.x != 0) return;
  const uint64_t A = 8 * (uint64_t)st->it, seed = st->seed;
  const double df0 = st->df0, shape0 = st->shape0, rate0 = st->rate0;
  double vbmean;
  if (st->model == GBM_BAYES_C) {
    const double vb = (sum[2] + st->S) / brr_chisq(seed, A + 1, df0 + (double)p);
    st->varBc = vb;
    st->S = brr_chisq(seed, A + 4, 2.0 * (0.5 * df0 + shape0)) / (2.0 * (1.0 / (2.0 * vb) + rate0));
    vbmean = vb;
  } else {
    st->S = brr_chisq(seed, A + 4, 2.0 * (0.5 * (double)p * df0 + shape0)) / (2.0 * (0.5 * sum[0] + rate0));
    vbmean = sum[3] / (double)p;
  }
  if (st->model != GBM_BAYES_A) {
    const double m = sum[1];
    const double g1 = 0.5 * brr_chisq(seed, A + 5, 2.0 * (m + st->cIn));
    const double g2 = 0.5 * brr_chisq(seed, A + 6, 2.0 * (((double)p - m) + st->cOut));
    st->pi = g1 / (g1 + g2);
  }
  if (brr_accumulate(st)) {
    const double k = (double)(st->nsum + 1);
    st->mubar = st->mubar * ((k - 1.0) / k) + st->mu / k;
    st->varBbar = st->varBbar * ((k - 1.0) / k) + vbmean / k;
    st->pibar = st->pibar * ((k - 1.0) / k) + st->pi / k;
    st->nsum += 1;
  }
  st->it += 1;
}

// gbm_debug_ordinal_math: gibbs_common.h's Φ (what 0), Φ⁻¹ (1) and TN (2; four inputs per item), one item each
__host__ __device__ inline double ordinal_math(int what, const double* in, int64_t i) {
  if (what == 0) return gibbs_phi(in[i]);
  if (what == 1) return gibbs_ppnd16(in[i]);
  return gibbs_truncnorm(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]);
}
__global__ void __launch_bounds__(256) ordinal_math_kernel(int what, const double* __restrict__ in, int64_t m,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) out[i] = ordinal_math(what, in, i);
}

// the classes of y (sorted distinct values), every individual's class and the start thresholds
// t_k = Φ⁻¹(cum_k / n); host only
struct OrdinalClasses {
  std::vector<double> values;
  std::vector<uint8_t> z;
  double t[ORD_MAXK + 1];
};
int ordinal_classes(const double* y, int64_t n, int64_t max_classes, OrdinalClasses& oc) {
  oc.values.assign(y, y + n);
  std::sort(oc.values.begin(), oc.values.end());
  oc.values.erase(std::unique(oc.values.begin(), oc.values.end()), oc.values.end());
  const int64_t K = (int64_t)oc.values.size();
  if (K < 2 || K > ORD_MAXK || K > max_classes)
    return fail(GBM_E_ARG, "gbm_bayes_fit_ordinal: y has " + std::to_string(K) +
                               " distinct values (need 2 <= K <= 32 classes and K <= max_classes)");
  std::vector<int64_t> count(K, 0);
  oc.z.resize(n);
  for (int64_t i = 0; i < n; i++) {
    const int64_t k = std::lower_bound(oc.values.begin(), oc.values.end(), y[i]) - oc.values.begin();
    oc.z[i] = (uint8_t)k;
    count[k] += 1;
  }
  oc.t[0] = -INFINITY;
  oc.t[K] = INFINITY;
  int64_t cum = 0;
  for (int64_t k = 1; k < K; k++) {
    cum += count[k - 1];
    oc.t[k] = gibbs_ppnd16((double)cum / (double)n);
  }
  return GBM_OK;
}

}  // namespace
}  // namespace gbm

using namespace gbm;

// One ordinal fit on a leased context: the start liabilities on the host (n draws), gbm_bayes_fit's
// setup on them, then the iteration captured as the context's ordinal graph and replayed.
static int ordinal_fit_impl(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const OrdinalClasses& oc,
                            int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                            double counts, uint64_t seed, int dev, double* b_hat_out, double* y_pred_out,
                            double* var_out, double* pip_out, double* thresholds_out, double* probs_out,
                            int64_t ldprobs) {
  const int64_t K = (int64_t)oc.values.size();
  BrrLease lease;
  GBM_TRY(CtxPool<BrrCtx>::instance().acquire(dev, lease.c));
  BrrCtx& cx = *lease.c;
  GBM_HIP_TRY(hipSetDevice(dev));
  hipStream_t s = cx.stream.s;
  const int64_t npad = round_up(n, IW), C = (n + IW - 1) / IW, nvb = bayes_var_blocks(n, p);
  std::vector<double> ystar(npad, 0.0);
  for (int64_t i = 0; i < n; i++)
    ystar[i] = gibbs_truncnorm(0.0, oc.t[oc.z[i]], oc.t[oc.z[i] + 1], brr_u01(seed, ~0ull, (uint64_t)i));
  std::vector<uint8_t> zpad(npad, 0);
  std::copy(oc.z.begin(), oc.z.end(), zpad.begin());
  GBM_TRY(ensure(cx.ost, dev, sizeof(OrdinalState)));
  GBM_TRY(ensure(cx.oys, dev, npad * 8));
  GBM_TRY(ensure(cx.oyh, dev, npad * 8));
  GBM_TRY(ensure(cx.ocls, dev, npad));
  GBM_TRY(ensure(cx.opart, dev, C * OSL * 8));
  if (probs_out) GBM_TRY(ensure(cx.oprob, dev, npad * K * 8));
  GibbsData g;
  OrdinalState os0{};
  GBM_TRY(bayes_setup("gbm_bayes_fit_ordinal", cx, model, X, n, p, ldx, ystar.data(), n_burnin, thin, r2, df0, prob_in,
                      counts, seed, g, os0.s));
  os0.s.varE = 1.0;  // fixed: the liability's scale
  os0.K = K;
  for (int64_t k = 0; k <= K; k++) os0.t[k] = oc.t[k];
  const double xs = g.xs;
  GBM_HIP_TRY(hipMemcpyAsync(cx.oys.p, ystar.data(), npad * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.ocls.p, zpad.data(), npad, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.ost.p, &os0, sizeof(OrdinalState), hipMemcpyHostToDevice, s));
  if (probs_out) GBM_HIP_TRY(hipMemsetAsync(cx.oprob.p, 0, (size_t)(npad * K * 8), s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  auto* osp = (OrdinalState*)cx.ost.p;
  double* pbar = probs_out ? (double*)cx.oprob.p : nullptr;
  auto enqueue_iteration = [&]() -> int {
    bayes_enqueue_chain(cx, n, p, g, &osp->s);
    ordinal_latent_kernel<<<(unsigned)C, IW, 0, s>>>((double*)cx.oys.p, (double*)cx.e.p, pbar ? (double*)cx.oyh.p : nullptr,
                                                     (const uint8_t*)cx.ocls.p, n, osp, (double*)cx.opart.p);
    ordinal_threshold_kernel<<<1, 256, 0, s>>>((const double*)cx.opart.p, C, osp);
    ordinal_probs_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((const double*)cx.oyh.p, n, npad, osp, pbar);
    bayes_enqueue_var(cx, n, p, &osp->s);
    ordinal_final_kernel<<<1, 256, 0, s>>>((const double*)cx.vpart.p, nvb, p, &osp->s);
    return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, "gbm_bayes_fit_ordinal: launch failed");
  };
  cx.ordinal_graph.ensure({model, n, p, npad, (int64_t)(xs * 64.0), K, key_of(cx.Xt), key_of(cx.D), key_of(cx.W),
                           key_of(cx.r), key_of(cx.e), key_of(cx.b), key_of(cx.dind), key_of(cx.bbar), key_of(cx.dbar),
                           key_of(cx.varBj), key_of(cx.pk), key_of(cx.vpart), key_of(cx.x2), key_of(cx.ost),
                           key_of(cx.oys), key_of(cx.oyh), key_of(cx.ocls), key_of(cx.opart),
                           (int64_t)(uintptr_t)pbar},
                          s, enqueue_iteration);
  GBM_TRY(cx.ordinal_graph.run(n_iter, s, "gbm_bayes_fit_ordinal", enqueue_iteration));
  OrdinalState fin{};
  GBM_TRY(gibbs_outputs(cx, n, p, npad, cx.ost, &fin, sizeof(fin), &fin.s.mubar, b_hat_out, pip_out, y_pred_out));
  if (var_out) {
    var_out[0] = 1.0;
    var_out[1] = fin.s.varBbar;
    var_out[2] = fin.s.pibar;
  }
  if (thresholds_out)
    for (int64_t k = 1; k < K; k++) thresholds_out[k - 1] = fin.tbar[k];
  if (probs_out) {
    GBM_HIP_TRY(hipMemcpy2DAsync(probs_out, ldprobs * 8, cx.oprob.p, npad * 8, n * 8, K, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
  }
  return GBM_OK;
}

extern "C" int gbm_bayes_fit_ordinal(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                                     int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0,
                                     double prob_in, double counts, uint64_t seed, int device, double* b_hat_out,
                                     double* y_pred_out, double* var_out, double* pip_out, int64_t max_classes,
                                     int64_t* nclass_out, double* classes_out, double* thresholds_out,
                                     double* probs_out, int64_t ldprobs) {
  RoctxRange r_("gbm_bayes_fit_ordinal");
  set_error("");
  GBM_TRY(bayes_check_args("gbm_bayes_fit_ordinal", model, X, y, b_hat_out, n, p, ldx, n_iter, n_burnin, thin, r2, df0,
                           prob_in, counts));
  if (max_classes < 1 || !nclass_out || !classes_out || (probs_out && ldprobs < n))
    return fail(GBM_E_ARG, "gbm_bayes_fit_ordinal: bad arguments (max_classes >= 1, nclass_out and classes_out given, "
                           "ldprobs >= n)");
  // n < 2^32: the counters of the stream A + 7 above it belong to the thresholds
  if (n >= ((int64_t)1 << 32)) return fail(GBM_E_ARG, "gbm_bayes_fit_ordinal: n < 2^32");
  for (int64_t i = 0; i < n; i++)
    if (!std::isfinite(y[i]))
      return fail(GBM_E_ARG, "gbm_bayes_fit_ordinal: y has a missing/NaN/Inf value at entry " + std::to_string(i + 1));
  OrdinalClasses oc;
  GBM_TRY(ordinal_classes(y, n, max_classes, oc));
  int dev = 0;
  GBM_TRY(gibbs_check_run("gbm_bayes_fit_ordinal", y, n, n_iter, n_burnin, thin, device, dev));
  GBM_TRY(ordinal_fit_impl(model, X, n, p, ldx, oc, n_iter, n_burnin, thin, r2, df0, prob_in, counts, seed, dev,
                           b_hat_out, y_pred_out, var_out, pip_out, thresholds_out, probs_out, ldprobs));
  *nclass_out = (int64_t)oc.values.size();
  std::copy(oc.values.begin(), oc.values.end(), classes_out);
  return GBM_OK;
}

extern "C" int gbm_debug_ordinal_math(int what, const double* in, int64_t m, int device, double* host_out,
                                      double* dev_out) {
  set_error("");
  if (!in || !host_out || m < 1 || m > ((int64_t)1 << 20) || what < 0 || what > 2)
    return fail(GBM_E_ARG, "gbm_debug_ordinal_math: in and host_out non-NULL, 1 <= m <= 2^20, what in 0, 1, 2");
  for (int64_t i = 0; i < m; i++) host_out[i] = ordinal_math(what, in, i);
  if (!dev_out) return GBM_OK;  // host only: no device work
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  const int dev = devs[0];
  GBM_HIP_TRY(hipSetDevice(dev));
  const int64_t nin = what == 2 ? 4 * m : m;
  DevBuf din, dout;
  GBM_TRY(ensure(din, dev, nin * 8));
  GBM_TRY(ensure(dout, dev, m * 8));
  GBM_HIP_TRY(hipMemcpy(din.p, in, (size_t)(nin * 8), hipMemcpyHostToDevice));
  ordinal_math_kernel<<<(unsigned)((m + 255) / 256), 256>>>(what, (const double*)din.p, m, (double*)dout.p);
  GBM_LAUNCH_CHECK();
  GBM_HIP_TRY(hipMemcpy(dev_out, dout.p, (size_t)(m * 8), hipMemcpyDeviceToHost));
  return GBM_OK;
}
