// What the pieces of the Gibbs samplers share (not part of the ABI; include from .hip files only):
//   gibbs_setup.hip  the kernels, pooled context and host steps both samplers use;
//   brr.hip          Bayesian ridge regression: the per-launch kernels, gbm_brr_fit, the debug exports;
//   brr_sweep.hip    its persistent super-block sweep, behind brr_sweep_plan / _setup / _enqueue;
//   bayes_abc.hip    BayesA, BayesB, BayesC: gbm_bayes_fit, gbm_bayes_fit_multi (several chains over one X),
//                    gbm_bayes_fit_multi_rows (each chain on its own rows of X), and the steps the ordinal fit
//                    replays;
//   bayes_ordinal.hip  their ordinal (threshold-model) response: gbm_bayes_fit_ordinal.
//
// Random numbers: a counter-based hash of (seed, stream, counter) (no sampler state), Box-Muller
// normals and Marsaglia-Tsang gammas, restated bit-for-bit in oracle/oracle.py (brr_*), so the
// device chains and the oracle's un-blocked BGLR loops follow the same sample path.
#pragma once
#include <functional>
#include <mutex>
#include <type_traits>
#include <vector>

#include "counter_hash.h"
#include "gbm_internal.h"
#include "host_util.h"

namespace gbm {

constexpr int BB = 64;  // markers per block (one wave)
constexpr int IW = 256;  // individuals per workgroup in the block kernels
constexpr int BK2 = 2 * BB;  // markers per launch of the byte per-launch path
constexpr int SBK = 512;  // markers per super-block (brr_sweep.hip)
constexpr int SBN = SBK / (2 * BB);  // 128-marker sub-blocks per super-block

__host__ __device__ __forceinline__ double brr_u01(uint64_t seed, uint64_t a, uint64_t b) {
  const uint64_t h = mix64(mix64(seed ^ (a * 0xD1B54A32D192ED03ull)) ^ (b * 0x8CB92BA72F3D8DD7ull));
  return ((double)(h >> 11) + 0.5) * 0x1.0p-53;
}
__device__ __forceinline__ double brr_normal(uint64_t seed, uint64_t a, uint64_t b) {
  const double u1 = brr_u01(seed, a, 2 * b), u2 = brr_u01(seed, a, 2 * b + 1);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
// χ²(df) = 2 Gamma(df/2) by Marsaglia-Tsang (df/2 >= 1); attempt t uses normal (a, 2t) and
// uniform (a, 4t + 2)
__device__ inline double brr_chisq(uint64_t seed, uint64_t a, double df) {
  const double d = 0.5 * df - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  for (uint64_t t = 0; t < 1000; t++) {
    const double x = brr_normal(seed, a, 2 * t);
    double v = 1.0 + c * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double u = brr_u01(seed, a, 4 * t + 2);
    if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) return 2.0 * d * v;
  }
  return df;  // unreachable in practice (acceptance ≈ 0.98 per attempt)
}

// ---- the ordinal response's truncated normal (bayes_ordinal.hip; include/gbm.h gbm_bayes_fit_ordinal) ----
// Φ(x) = ½ erfc(−x/√2): 0 at −∞, 1 at +∞
__host__ __device__ inline double gibbs_phi(double x) { return 0.5 * erfc(-x * 0.7071067811865476); }
// Φ⁻¹(p) in fp64: Wichura's algorithm AS241, routine PPND16 (Applied Statistics 37 (1988) 477-484),
// written out here so that the host's start draws, the device's and tests/ordinal_ref.py's restatement
// run the same operations. p = 0 gives −∞, p = 1 gives +∞.
__host__ __device__ inline double gibbs_ppnd16(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num =
        ((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r +
            45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r +
         133.14166789178437745) * r + 3.387132872796366608;
    const double den =
        ((((((r * 5226.495278852854561 + 28729.085735721942674) * r + 39307.89580009271061) * r +
            21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r +
         42.313330701600911252) * r + 1.0;
    return q * num / den;
  }
  const double tail = q < 0.0 ? p : 1.0 - p;
  if (tail <= 0.0) return q < 0.0 ? -INFINITY : INFINITY;  // sqrt(−log 0) = ∞ would end as ∞/∞ below
  double r = sqrt(-log(tail));
  double val;
  if (r <= 5.0) {
    r -= 1.6;
    const double num =
        ((((((r * 7.7454501427834140764e-4 + 0.0227238449892691845833) * r + 0.24178072517745061177) * r +
            1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r +
         4.6303378461565452959) * r + 1.42343711074968357734;
    const double den =
        ((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r +
            0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r +
         2.05319162663775882187) * r + 1.0;
    val = num / den;
  } else {
    r -= 5.0;
    const double num =
        ((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r +
            0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r +
         5.4637849111641143699) * r + 6.6579046435011037772;
    const double den =
        ((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r +
            7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r +
         0.59983220655588793769) * r + 1.0;
    val = num / den;
  }
  return q < 0.0 ? -val : val;
}
// TN(m; a, b; u): the N(m, 1) variate truncated to [a, b] (a < b, at most one of them infinite) by inverse CDF
// from one uniform u, worked in the tail below the mean (an interval above it is reflected), where Φ keeps
// its relative precision. The draw is always finite: pa + u·w can round to 0 (a half-open class 37.6 to 38.5
// below its mean: w is subnormal, u small) or to 1 (a half-open interval around the mean, u → 1), where Φ⁻¹
// is infinite; then, as when the interval has no mass in fp64, the draw is the finite end nearer the mean.
__host__ __device__ inline double gibbs_truncnorm(double m, double a, double b, double u) {
  double al = a - m, be = b - m;
  const bool refl = al >= 0.0;
  if (refl) {
    const double t = al;
    al = -be;
    be = -t;
  }
  const double pa = gibbs_phi(al), w = gibbs_phi(be) - pa;
  double x = INFINITY;
  if (w > 0.0) {
    x = gibbs_ppnd16(pa + u * w);
    x = x < al ? al : x;
    x = x > be ? be : x;
  }
  if (!(fabs(x) < INFINITY)) x = fabs(be) <= fabs(al) ? be : al;  // at most one end is infinite
  return refl ? m - x : m + x;
}

struct BrrState {
  double mu, varE, varB, S0e, S0b, df0e, df0b;
  double mubar, varEbar, varBbar;
  int64_t it, burnin, thin, nsum;
  uint64_t seed;
  uint64_t epoch;  // distinct per fit: part of the super-block sweep's hand-off tags (pooled buffers)
};
struct BayesState {
  double mu, varE, varBc, S, pi;  // varBc: BayesC's common σ²_b
  double S0e, df0, rate0, shape0, cIn, cOut;
  double mubar, varEbar, varBbar, pibar;
  int64_t it, burnin, thin, nsum;
  uint64_t seed;
  int model;  // GBM_BAYES_A, _B or _C
};
// gbm_bayes_fit_ordinal: the chain's state (varE stays 1) and the thresholds of K classes
constexpr int ORD_MAXK = 32;
struct OrdinalState {
  BayesState s;
  double t[ORD_MAXK + 1];     // t_0 = −∞ < t_1 < … < t_{K−1} < t_K = +∞
  double tbar[ORD_MAXK + 1];  // running means of t_1 … t_{K−1} (entry k)
  int64_t K;
};
// gbm_bayes_fit_multi_rows: what the chains' training rows add to a kernel's arguments (SETS instantiations only;
// the others take the empty NoRowSets and compile as before)
struct RowSets {
  const uint32_t* mask;  // npad words: bit c set when the individual trains chain c (0 past n)
  const int* set_of;     // nchains: the chain's set
  const int64_t* nrows;  // nchains: n_c, the size of the chain's set
  int64_t wstride;       // doubles between two sets' Gram blocks
};
struct NoRowSets {};
template <bool SETS>
using RowSetsArg = std::conditional_t<SETS, RowSets, NoRowSets>;
// the sample gate: does this iteration enter the running posterior means?
template <typename State>
__device__ __forceinline__ bool brr_accumulate(const State* st) {
  const int64_t i = st->it + 1;  // BGLR's 1-based iteration
  return (i % st->thin == 0) && (i > st->burnin);
}

template <int BS>
__device__ __forceinline__ double brr_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < BS / 64; k++) s += red[k];
  return s;
}
// Workgroup barrier that waits for this wave's LDS operations only (__syncthreads also waits for
// every outstanding global load, e.g. the next block's rows that are needed much later).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)u, l);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32));
}

// Genotype storage of the block kernels: fp64 (any allele frequencies), or bytes d with
// x = d·xs when every x/xs is an integer in [0, 255] (xs = 1/2 for diploid dosages: exact, so
// both storages run the identical chain with 8× fewer bytes per block for the bytes).
// 64 byte-genotypes (4 × 16 B) times 64 values of es, accumulated in the fp64 path's order:
// even individuals into s, odd ones into s1. The bytes are summed unscaled and the caller scales
// both sums by xs: xs is a power of two, so (Σ d e)·xs has the bits of Σ (d·xs) e.
__device__ __forceinline__ void brr_dot64_u8(const uint4 (&v)[4], const double* es, double& s, double& s1) {
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const uint32_t wd[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int b = 0; b < 4; b += 2) {
        const int idx = 16 * u + 4 * w + b;
        s = fma((double)((wd[w] >> (8 * b)) & 0xFFu), es[idx], s);
        s1 = fma((double)((wd[w] >> (8 * b + 8)) & 0xFFu), es[idx + 1], s1);
      }
  }
}
template <typename T>
__device__ __forceinline__ double gval(T v, double xs) {
  if constexpr (sizeof(T) == 8) return (double)v;
  else return (double)v * xs;
}

// partial[c][k] = Σ_{i in chunk c} x_{j0+k, i} e_i over this workgroup's IW individuals, from es
// (the chunk of e in LDS): thread (k = tid/4, quarter) sums 64 contiguous individuals
template <typename T>
__device__ __forceinline__ void brr_partials(const T* __restrict__ Xt, int64_t ldx, int64_t n, int64_t i0,
                                             int64_t j0, int nb, double xs, const double* es,
                                             double* __restrict__ out) {
  const int tid = threadIdx.x, k = tid >> 2, qt = tid & 3;
  double s = 0.0;
  if (k < nb) {
    // 64 contiguous individuals per thread, all loads in flight (rows are zero-padded to ldx, a
    // multiple of IW, and es is 0 past n)
    const T* row = Xt + (j0 + k) * ldx + i0 + qt * 64;
    double s1 = 0.0;
    if constexpr (sizeof(T) == 8) {
      double2 v[32];
#pragma unroll
      for (int u = 0; u < 32; u++) v[u] = *reinterpret_cast<const double2*>(row + 2 * u);
#pragma unroll
      for (int u = 0; u < 32; u++) {
        s = fma(v[u].x, es[qt * 64 + 2 * u], s);
        s1 = fma(v[u].y, es[qt * 64 + 2 * u + 1], s1);
      }
    } else {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const uint4*>(row + 16 * u);
      brr_dot64_u8(v, es + qt * 64, s, s1);
      s *= xs;
      s1 *= xs;
    }
    s += s1;
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  if (qt == 0) out[blockIdx.x * BB + k] = s;  // k >= nb writes 0
}

// One 64x64 tile X_RᵀX_C of a Gram matrix for the marker rows R = [r0, r0 + 64), C = [c0, c0 + 64) of
// Xt (rows past p are zero), by one 256-thread workgroup: individuals in chunks of 64 staged through
// LDS, thread (a, b0) sums out[a][b0 .. b0 + 15]. out: the tile's first element, row pitch ldo.
// SETS: over a set of individuals, rows[i] != 0 (n of them readable); the others enter as 0.0 in the same order.
template <bool SETS = false>
__device__ __forceinline__ void brr_gram_tile(const double* __restrict__ Xt, int64_t ldx, int64_t p, int64_t n,
                                              int64_t r0, int64_t c0, double* __restrict__ out, int64_t ldo,
                                              const uint8_t* __restrict__ rows = nullptr) {
  __shared__ double TR[BB][BB + 1];
  __shared__ double TC[BB][BB + 1];
  const int tid = threadIdx.x, a = tid >> 2, b0 = (tid & 3) * 16;
  double acc[16];
#pragma unroll
  for (int u = 0; u < 16; u++) acc[u] = 0.0;
  for (int64_t k0 = 0; k0 < n; k0 += BB) {
    for (int e = tid; e < BB * BB; e += 256) {
      const int r = e / BB, c = e % BB;
      bool in = k0 + c < n;
      if constexpr (SETS) in = in && rows[k0 + c] != 0;
      TR[r][c] = (r0 + r < p && in) ? Xt[(r0 + r) * ldx + k0 + c] : 0.0;
      TC[r][c] = (c0 + r < p && in) ? Xt[(c0 + r) * ldx + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < BB; k++) {
      const double xa = TR[a][k];
#pragma unroll
      for (int u = 0; u < 16; u++) acc[u] += xa * TC[b0 + u][k];
    }
    __syncthreads();
  }
  out += a * ldo + b0;
#pragma unroll
  for (int u = 0; u < 16; u++) out[u] = acc[u];
}

// ---- host side ---------------------------------------------------------------------------------

// One Gibbs iteration captured as a hipGraph and replayed, kept while `key` (the call's shape and
// buffers) is unchanged; without a graph (capture or instantiation failed) run() launches directly.
struct IterGraph {
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  std::vector<int64_t> key;  // what the captured graph was built for
  void drop();
  void ensure(const std::vector<int64_t>& k, hipStream_t s, const std::function<int()>& enqueue);
  // n_iter iterations, then the stream synchronised; `entry` names the caller in the error text
  int run(int64_t n_iter, hipStream_t s, const char* entry, const std::function<int()>& enqueue);
};
inline int64_t key_of(const DevBuf& b) { return (int64_t)(uintptr_t)b.p; }  // a buffer's entry in a graph key

// Pooled per-device sampler contexts (as fit_ctx.h pools the GBLUP fit contexts): a fit leases one,
// its buffers only grow, so repeated fits of one shape allocate no device memory after the first
// (cvmultithread! runs bayesian("BRR") once per fold). BRR and BayesA/B/C fits that alternate on
// one context keep both captured graphs; the ordinal fits have a third, the multi-chain fits a fourth, the
// multi-chain fits with training sets a fifth.
struct BrrCtx {
  int dev = 0;
  Stream stream;
  DevBuf Xt, colmean, x2, e, b, bbar, r, stm, D, badm, W, Mb, alph, gamm, Dt, pb, part, pout;
  DevBuf Wsb, MS, Ssc, Pb, Rt, Dl, sbcnt;  // the super-block sweep
  DevBuf CS, CS2;                          // its cross-Grams C_s = X_sᵀ X_{s−1}, C2_s = X_sᵀ X_{s−2}
  DevBuf trace;                            // GBM_BRR_TRACE timestamps of this context's last sweep
  DevBuf dind, dbar, varBj, pk, vpart, bst;  // gbm_bayes_fit: indicators, PIP, varB_j, step constants, partial sums, state
  DevBuf oys, oyh, ocls, opart, oprob, ost;  // gbm_bayes_fit_ordinal: y*, ŷ, classes, min/max partials, P(class), state
  DevBuf srows, smask, sof, snrows;  // gbm_bayes_fit_multi_rows: the sets' row bytes, the chain-bit words, set_of, n_c
  IterGraph brr_graph, bayes_graph, ordinal_graph, multi_graph;  // multi_graph: gbm_bayes_fit_multi
  IterGraph rows_graph;                                          // gbm_bayes_fit_multi_rows
  ~BrrCtx() {
    (void)hipSetDevice(dev);
    brr_graph.drop();
    bayes_graph.drop();
    ordinal_graph.drop();
    multi_graph.drop();
    rows_graph.drop();
  }
};
struct BrrLease {
  std::unique_ptr<BrrCtx> c;
  ~BrrLease() {
    if (c) CtxPool<BrrCtx>::instance().release(std::move(c));
  }
};

// The checks gbm_brr_fit and gbm_bayes_fit share (`entry` opens the error text): the arguments, then
// (after a caller's own checks) the sampling schedule, the phenotypes (y = nullptr: the caller has checked
// them) and the device.
int gibbs_check_args(const char* entry, const double* X, const double* y, const double* b_hat_out, int64_t n, int64_t p,
                     int64_t ldx, int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0);
int gibbs_check_run(const char* entry, const double* y, int64_t n, int64_t n_iter, int64_t n_burnin, int64_t thin,
                    int device, int& dev_out);

// The genotypes of a fit on its context: X into Xt (rows padded with zeros to npad individuals),
// column means and Σx² (cm, xx: filled once the stream has been synchronised), and byte storage D
// where X = D·xs exactly (xs = 0: fp64 storage). Also sizes e, b, bbar and the partial dots r.
struct GibbsData {
  int64_t npad = 0, C64 = 0;  // individuals padded to whole IW chunks; the chunks
  double xs = 0.0;
  std::vector<double> cm, xx;
};
int gibbs_upload(BrrCtx& cx, const double* X, int64_t n, int64_t p, int64_t ldx, GibbsData& g);
// W = the Gram blocks of brr_gram_kernel (nw = 1 or 3) for nblk launches; sizes W
int gibbs_gram(BrrCtx& cx, int64_t n, int64_t p, int64_t npad, int64_t nblk, int nw);
// block 0's partial dots into r, from the fp64 rows or (bytes) from D as 64-marker blocks; for each of
// nchains chains (chain c: e at c·npad, its ping-pong partials at c·2·C64·BB)
void gibbs_dots0(BrrCtx& cx, int64_t n, int64_t p, const GibbsData& g, bool bytes, int64_t nchains = 1);
// BGLR's prior moments: ȳ, var(y) with ddof 1, MSx = Σ_j var(x_j), and the start residual y − ȳ
struct GibbsPrior {
  double ym = 0.0, vy = 0.0, msx = 0.0;
  std::vector<double> e0;  // npad values
};
int gibbs_prior(const char* entry, const double* y, int64_t n, int64_t p, const GibbsData& g, GibbsPrior& pr);
// the same over a set of individuals (rows[i] != 0, nc of them, in increasing order; cm and xx the set's column
// means and Σx²): e0 is 0 at the others and y is not read there. rows = nullptr: all n (nc = n).
int gibbs_prior_rows(const char* entry, const double* y, int64_t n, int64_t p, int64_t npad, const uint8_t* rows,
                     int64_t nc, const double* cm, const double* xx, GibbsPrior& pr);

// The training sets of gbm_bayes_fit_multi_rows on the host: nsets rows of n bytes (pitch ldrows), the chains' sets
// and, filled by the checks and by gibbs_sets, the sets' sizes and their column means and Σx² (nsets x p each).
struct RowSetsHost {
  int64_t nsets = 0;
  const uint8_t* rows = nullptr;
  int64_t ldrows = 0;
  const int* set_of = nullptr;
  std::vector<int64_t> nrows;
  std::vector<double> cm, xx;
};
// Per-set statistics on a context whose genotypes are uploaded: colmean and x2 at s·p, the Gram blocks W at
// s·nblk·64·64, each over the set's individuals (a held-out one enters as 0.0); the chain-bit words, set_of and
// n_c of nchains chains for the iteration's kernels. Fills rs.cm and rs.xx; the stream is synchronised.
int gibbs_sets(BrrCtx& cx, int64_t n, int64_t p, int64_t npad, int64_t nblk, int64_t nchains, RowSetsHost& rs);
// The tail of a fit: the final state (fin_bytes from `state` into fin) and the posterior means to
// the host, b_hat_out[0] = *mubar (a field of fin), then the optional y_pred = μ̄ + X b̄. `chain`: which
// chain of a multi-chain fit (entry `chain` of the state array, the means at chain·p).
int gibbs_outputs(BrrCtx& cx, int64_t n, int64_t p, int64_t npad, const DevBuf& state, void* fin, size_t fin_bytes,
                  const double* mubar, double* b_hat_out, double* pip_out, double* y_pred_out, int64_t chain = 0);

// ---- what gbm_bayes_fit shares with gbm_bayes_fit_ordinal (bayes_abc.hip) -------------------------
// gbm_bayes_fit's argument checks in front of gibbs_check_run (`entry` opens the error text)
int bayes_check_args(const char* entry, int model, const double* X, const double* y, const double* b_hat_out, int64_t n,
                     int64_t p, int64_t ldx, int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0,
                     double prob_in, double counts);
// A fit's setup on its context: genotypes, Gram blocks, the prior moments of y, the start state st0 (not
// uploaded: the caller owns the state's buffer) and the start values of e, b, d, varB_j and the running means.
int bayes_setup(const char* entry, BrrCtx& cx, int model, const double* X, int64_t n, int64_t p, int64_t ldx,
                const double* y, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in, double counts,
                uint64_t seed, GibbsData& g, BayesState& st0);
// The two halves of bayes_setup, which gbm_bayes_fit_multi calls once and once per chain. Shared: the buffers
// sized for nchains chains, the genotypes and the Gram blocks (stream synchronised). Per chain: y's prior
// moments, the start state st0 and the start values of the chain's e, b, d, varB_j and running means
// (chain c's arrays lie at c times the one-chain size in the context's buffers).
// rs (gbm_bayes_fit_multi_rows): per-set statistics and Gram blocks (gibbs_sets) in place of the common ones.
int bayes_setup_shared(BrrCtx& cx, const double* X, int64_t n, int64_t p, int64_t ldx, int64_t nchains, GibbsData& g,
                       RowSetsHost* rs = nullptr);
int bayes_start(const char* entry, BrrCtx& cx, int64_t chain, int model, int64_t n, int64_t p, const double* y,
                int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in, double counts, uint64_t seed,
                const GibbsData& g, BayesState& st0);
// bayes_start after the prior moments: the start state and start values from pr (e0 of npad values)
int bayes_start_from(BrrCtx& cx, int64_t chain, int model, int64_t p, int64_t npad, const GibbsPrior& pr,
                     int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in, double counts,
                     uint64_t seed, BayesState& st0);
// steps 1 and 2 of an iteration on the states st[0 .. nchains): the step constants, μ, block 0's partial dots,
// one chain launch per 64-marker block with per_wg (1 or 4) chains in a workgroup row; rs: the chains' training
// sets (the SETS instantiations of the kernels)
void bayes_enqueue_chain(BrrCtx& cx, int64_t n, int64_t p, const GibbsData& g, BayesState* st, int64_t nchains = 1,
                         int per_wg = 1, const RowSets* rs = nullptr);
// step 3's per-marker variances and the partial sums of the scalar draws (vpart)
void bayes_enqueue_var(BrrCtx& cx, int64_t n, int64_t p, BayesState* st, int64_t nchains = 1);
inline int64_t bayes_var_blocks(int64_t n, int64_t p) { return (std::max(n, p) + 255) / 256; }

// ---- the super-block sweep's host interface (brr_sweep.hip) -----------------------------------------
// The chunk shape of a sweep over n individuals on a device of `cus` CUs, per the knobs
// GBM_BRR_SWEEP, GBM_BRR_SB_K and GBM_BRR_OWN_R (read per call): uniform chunks of K individuals on C
// workgroups owning R rows of a super-block each, or (GBM_BRR_OWN_R) O owners of Ko and the rest Kn.
struct SweepPlan {
  bool on = false;  // the sweep can run: all its workgroups resident, one per CU
  int K = 0, Cu = 0, Ru = 0;  // the uniform split
  int Ko = 0, Kn = 0, R = 0, O = 0, C = 0;
};
int brr_sweep_plan(int64_t n, int cus, SweepPlan& pl);
// one-time setup after W, Mb, α, γ are sized: the sweep's buffers, cross-Grams and super-block Gram
// blocks (trace_n > 0: the trace buffer of a traced fit)
int brr_sweep_setup(BrrCtx& cx, const SweepPlan& pl, int64_t n, int64_t p, int64_t npad, int64_t nsb, int64_t trace_n);
// the sweep's share of an iteration: M_S of every super-block (three levels), then the sweep
void brr_sweep_enqueue(BrrCtx& cx, const SweepPlan& pl, int64_t n, int64_t p, int64_t npad, int64_t nsb, double xs,
                       int64_t* trace_dev);
inline int32_t* brr_sweep_error_cell(BrrCtx& cx) { return (int32_t*)cx.sbcnt.p + 24; }  // zeroed at setup; < 0: timed out
// sweeps of concurrent fits on one device take turns (held for a whole fit)
std::mutex& brr_sweep_lock(int dev);

}  // namespace gbm
