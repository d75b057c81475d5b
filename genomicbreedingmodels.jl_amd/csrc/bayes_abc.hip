// BayesA, BayesB and BayesC by Gibbs sampling (gbm_bayes_fit, the models behind reference
// src/linear.jl:440-626; include/gbm.h states the sampler). They reuse the per-launch skeleton of
// BRR (brr.hip) and its setup, pooled context and graph replay (gibbs_setup.hip, gibbs_common.h),
// but their indicator draw is not affine in x_kᵀe: a block's 64 steps run as a serial chain on the
// block's Gram matrix (bayes_chain_kernel).
//
// Marker j has an effect b_j, an inclusion indicator d_j (BayesA: always 1) and (A, B) its own
// variance varB_j. The indicator's probability is a non-linear function of x_jᵀe at the marker's
// turn, so a block's 64 single-site steps are no triangular solve (no δ = M r̃): they run as a
// serial chain on wave 0 of every chunk workgroup, lane k holding r_k = x_kᵀe + x2_k d_k b_k and
// column k of the block's Gram matrix. bayes_prep_kernel forms, for every marker and in parallel,
// everything of its step that does not depend on the chain (the normal, logit(u), 1/C, the square
// roots), so that a chain step is FMAs, one compare, selects and one lane broadcast.
//
// gbm_bayes_fit_multi runs up to 32 such chains (a model, phenotype column, priors and seed each) over one X
// in one pass: the same kernels with a chain index, each chain's bits those of gbm_bayes_fit.
// gbm_bayes_fit_multi_rows gives each chain a set of training rows of that X (the folds of a cross-validation):
// the SETS instantiations of the kernels, per-set column statistics and Gram blocks.
#include "gibbs_common.h"

namespace gbm {
namespace {

// the intercept step of brr_mu_kernel on the stream A = 8 it; workgroup c is chain c (e at c·lde, state c).
// SETS (gbm_bayes_fit_multi_rows): over the chain's n_c training rows; a held-out row adds 0.0 to the sum in its
// place and its e stays 0.0.
template <bool SETS>
__global__ void __launch_bounds__(1024) bayes_mu_kernel(double* __restrict__ e, int64_t lde, int64_t n,
                                                        BayesState* __restrict__ st, RowSetsArg<SETS> rs) {
  __shared__ double red[16];
  e += (int64_t)blockIdx.x * lde;
  st += blockIdx.x;
  const double mu_old = st->mu;
  double s = 0.0;
  int64_t nc = n;  // the individuals in the mean
  if constexpr (SETS) {
    nc = rs.nrows[blockIdx.x];
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (rs.mask[i] >> blockIdx.x) & 1u ? e[i] + mu_old : 0.0;
  } else {
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += e[i] + mu_old;
  }
  s = brr_block_sum<1024>(s, red);
  const double varE = st->varE;
  const double mu = s / (double)nc + sqrt(varE / (double)nc) * brr_normal(st->seed, 8 * (uint64_t)st->it, 0xFFFFFFFFull);
  if constexpr (SETS) {
    for (int64_t i = threadIdx.x; i < n; i += 1024)
      if ((rs.mask[i] >> blockIdx.x) & 1u) e[i] = (e[i] + mu_old) - mu;
  } else {
    for (int64_t i = threadIdx.x; i < n; i += 1024) e[i] = (e[i] + mu_old) - mu;
  }
  __syncthreads();
  if (threadIdx.x == 0) st->mu = mu;
}

// Per marker j (one thread each, padded to whole blocks with zeros), the step constants pk[8 j ..]:
//   0: x2 eff   1: eff = d b (old)   2: a = 1/(varE C)   3: c = sqrt(1/C) ξ   4: sqrt(varB) ξ
//   5: b/(2 varE)   6: −b x2   7: log(π/(1−π)) − logit(u)
// so that with r = x_jᵀe + x2 eff:  logOdds − logit(u) = pk5 (2 r + pk6) + pk7,  b_in = a r + c.
// BayesA: pk5 = pk6 = 0, pk7 = 1 (always included). blockIdx.y is the chain (x2 is common; b and d at
// c·2p, varB at c·p, pk at c·8·ppad, state c). SETS: x2 of the chain's set, at set·p.
template <bool SETS>
__global__ void __launch_bounds__(256) bayes_prep_kernel(int64_t p, int64_t ppad, const double* __restrict__ x2,
                                                         const double* __restrict__ b, const double* __restrict__ d,
                                                         const double* __restrict__ varB,
                                                         const BayesState* __restrict__ st, double* __restrict__ pk,
                                                         RowSetsArg<SETS> rs) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ppad) return;
  const int64_t ch = blockIdx.y;
  if constexpr (SETS) x2 += rs.set_of[ch] * p;
  b += ch * 2 * p;
  d += ch * 2 * p;
  varB += ch * p;
  st += ch;
  pk += ch * 8 * ppad;
  double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (j < p) {
    const int64_t par = st->it & 1;
    const uint64_t A = 8 * (uint64_t)st->it;
    const double varE = st->varE, iv = 1.0 / varE;
    const double vb = st->model == GBM_BAYES_C ? st->varBc : varB[j];
    const double bo = b[par * p + j], eff = d[par * p + j] * bo, xx = x2[j];
    const double xi = brr_normal(st->seed, A, (uint64_t)j);
    const double ic = 1.0 / (xx / varE + 1.0 / vb);
    q[0] = xx * eff;
    q[1] = eff;
    q[2] = iv * ic;
    q[3] = sqrt(ic) * xi;
    q[4] = sqrt(vb) * xi;
    if (st->model == GBM_BAYES_A) {
      q[7] = 1.0;
    } else {
      const double u = brr_u01(st->seed, A + 3, (uint64_t)j), pi = st->pi;
      q[5] = bo * (0.5 * iv);
      q[6] = -bo * xx;
      q[7] = log(pi / (1.0 - pi)) - log(u / (1.0 - u));
    }
  }
  double2* out = reinterpret_cast<double2*>(pk + 8 * j);
#pragma unroll
  for (int u = 0; u < 4; u++) out[u] = make_double2(q[2 * u], q[2 * u + 1]);
}

// One block of 64 markers, brr_step_kernel's skeleton with the GEMV δ = M r̃ replaced by the serial
// chain: d⁰ = Σ_c partial_in[c] (fixed order), r_k = d⁰_k + x2_k eff_k; step s broadcasts lane s's
// δ_s = eff_s − d_new b_new and the lanes k > s do r_k += δ_s W[s][k] (lane k holds W[·][k] with
// the entries s >= k zeroed, so a lane's r stops changing at its own step and its draw can be
// formed again from it after the chain: same operands, same bits as the value it broadcast). Wave 0
// of every workgroup runs the chain from identical inputs; then e += X_B δ and the next block's
// partials as in brr_step_kernel. Workgroup 0 stores b, d and the running means of d b and d.
//
// Several chains over one X (gbm_bayes_fit_multi): the grid is (chunks, ⌈nch/CH⌉) and workgroup row y
// holds the chains CH·y … CH·y + CH − 1 (those below nch). CH = 1 is the kernel above, one chain per
// row. With CH = 4 wave w runs the 64 steps of the row's chain w, where wave 0 alone runs them for
// CH = 1; the block's rows in LDS, the thread's 64 genotypes and W are read once for the four chains,
// and d⁰, e += X_B δ and the next block's partials are formed per chain by all four waves with the
// operations and the order of CH = 1, so a chain's bits do not depend on CH, on its slot or on its
// neighbours. Chain c's buffers: e at c·ldx, b and d at c·2p, the running means at c·p, pk at
// c·8·64·nblk, its ping-pong partials at c·2·64·chunks, state c. ROWS = false (CH = 1, one chain: the
// launch of gbm_bayes_fit) compiles the chain index out.
//
// SETS (gbm_bayes_fit_multi_rows): chain c trains on the individuals whose mask word has bit c. Its e is exactly
// 0.0 on the others (the start value is, and e += X_B δ is skipped there by a select), so every dot x_jᵀe (d⁰, the
// next block's partials, Σe²) runs unchanged: a held-out individual adds an exact zero in its place of the fixed
// order. The running wave loads its W column from its chain's set (W at set·wstride). One mask load per thread
// serves the row's chains.
template <typename T, int CH, bool ROWS, bool SETS = false>
__global__ void __launch_bounds__(256) bayes_chain_kernel(const T* __restrict__ Xt, int64_t ldx, int64_t n,
                                                          int64_t p, double xs, const double* __restrict__ W,
                                                          int64_t blk, int64_t nblk, int nch,
                                                          const double* __restrict__ partial_in,
                                                          double* __restrict__ partial_out,
                                                          const double* __restrict__ pk, double* __restrict__ b,
                                                          double* __restrict__ d, double* __restrict__ bbar,
                                                          double* __restrict__ dbar, double* __restrict__ e,
                                                          const BayesState* __restrict__ st,
                                                          RowSetsArg<SETS> rs) {
  constexpr int RP = IW + 2;  // doubles (row pitch 2064 B, as brr_step_kernel)
  __shared__ __attribute__((aligned(16))) double Xn[BB * RP];
  __shared__ double delta[CH][BB];
  __shared__ double es[CH][IW];
  __shared__ double part4[CH][4][BB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  static_assert(ROWS || CH == 1, "a launch without chain rows runs one chain");
  static_assert(ROWS || !SETS, "training sets come with chain rows");
  const int ch0 = ROWS ? (int)blockIdx.y * CH : 0;                 // the row's first chain
  const int nc = ROWS ? (nch - ch0 < CH ? nch - ch0 : CH) : 1;     // its chains (>= 1)
  const int mine = CH == 1 ? 0 : wave;                     // the slot whose chain this wave runs
  const bool runner = CH == 1 ? tid < 64 : wave < nc;      // this wave runs a chain
  const int64_t ch = ch0 + (runner ? mine : 0);            // that chain
  const int64_t pstride = 2 * (int64_t)gridDim.x * BB;     // a chain's ping-pong partials
  const int64_t j0 = blk * BB;
  const int nb = (int)((p - j0) < BB ? (p - j0) : BB);
  const int C = (int)gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  const int64_t i = i0 + tid;
  const bool more = blk + 1 < nblk;
  const int64_t j1 = j0 + BB;
  const int nb1 = more ? (int)((p - j1) < BB ? (p - j1) : BB) : 0;
  // (1) the next block's rows into LDS
  uint8_t* Xb = reinterpret_cast<uint8_t*>(Xn);  // byte storage: rows of IW bytes, unpadded
  if constexpr (sizeof(T) == 8) {
    for (int q = wave; q < 2 * nb1; q += 4) {
      const int k = q >> 1, h = q & 1;
      const T* src = Xt + (j1 + k) * ldx + i0 + h * 128 + lane * 2;
      __builtin_amdgcn_global_load_lds((const void*)src, (void*)(Xn + k * RP + h * 128), 16, 0, 0);
    }
  } else {
    // 4 rows per wave instruction: lane = 16 (row within the four) + c writes LDS chunk c of its
    // row, loaded from the row's 16-byte chunk c ^ (r & 15) (so chunk g of row r sits at position
    // g ^ (r & 15) and the partials loop's lanes, one row each, read distinct banks). Rows past the
    // block re-read row nb1 − 1: valid memory, never summed.
    for (int q = wave; q < (nb1 + 3) / 4; q += 4) {
      const int r = 4 * q + (lane >> 4), c = lane & 15;
      const T* src = Xt + (j1 + (r < nb1 ? r : nb1 - 1)) * ldx + i0 + ((c ^ (r & 15)) * 16);
      __builtin_amdgcn_global_load_lds((const void*)src, (void*)(Xb + q * 4 * IW), 16, 0, 0);
    }
  }
  // (2) this thread's 64 genotypes of the block (rows past p clamped; their δ = 0)
  double xv[BB];
#pragma unroll
  for (int s2 = 0; s2 < BB; s2++) xv[s2] = gval<T>(Xt[(j0 + (s2 < nb ? s2 : 0)) * ldx + i], xs);
  double e_old[CH];
#pragma unroll
  for (int c = 0; c < CH; c++) e_old[c] = c < nc ? e[(ch0 + c) * ldx + i] : 0.0;
  [[maybe_unused]] uint32_t trains = 0;  // bit c: this thread's individual trains chain ch0 + c
  if constexpr (SETS) trains = rs.mask[i] >> ch0;
  // (3) a running wave's operands: column `lane` of W (= its row: W is symmetric) and the step constants
  double w[BB];
  double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool on = lane < nb;
  const int64_t j = j0 + lane;
  if (runner) {
    const double* wr = W + (blk * BB + lane) * BB;
    if constexpr (SETS) wr += rs.set_of[ch] * rs.wstride;
#pragma unroll
    for (int s = 0; s < BB; s += 2) {
      const double2 v = *reinterpret_cast<const double2*>(wr + s);
      w[s] = v.x;
      w[s + 1] = v.y;
    }
    const double2* pq = reinterpret_cast<const double2*>(pk + (ch * nblk * BB + j) * 8);  // padded to whole blocks
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double2 v = pq[u];
      q[2 * u] = v.x;
      q[2 * u + 1] = v.y;
    }
  }
  const bool keeper = blockIdx.x == 0 && runner && on;
  const double bb_old = keeper ? bbar[ch * p + j] : 0.0, db_old = keeper ? dbar[ch * p + j] : 0.0;
#pragma unroll
  for (int c = 0; c < CH; c++) {
    if (c >= nc) break;
    const double* pin = partial_in + (ch0 + c) * pstride;
    double a = 0.0;
    for (int c0 = wave; c0 < C; c0 += 64) {
      double v[16];
#pragma unroll
      for (int m = 0; m < 16; m++) v[m] = pin[min(c0 + 4 * m, C - 1) * BB + lane];  // unconditional loads
#pragma unroll
      for (int m = 0; m < 16; m++) a += c0 + 4 * m < C ? v[m] : 0.0;
    }
    part4[c][wave][lane] = a;
  }
  __syncthreads();
  if (runner) {
    const double d0 = ((part4[mine][0][lane] + part4[mine][1][lane]) + part4[mine][2][lane]) + part4[mine][3][lane];
#pragma unroll
    for (int s = 0; s < BB; s++) w[s] = lane > s ? w[s] : 0.0;
    const double eff = q[1], qa = q[2], qc = q[3], bout = q[4], qbh = q[5], qm = q[6], qthr = q[7];
    double r = d0 + q[0];
#pragma unroll
    for (int s = 0; s < BB; s++) {
      const double lo = fma(qbh, fma(2.0, r, qm), qthr);
      const double bin = fma(r, qa, qc);
      const double cand = lo > 0.0 ? eff - bin : eff;
      r = fma(readlane_f64(cand, s), w[s], r);
    }
    const double lo = fma(qbh, fma(2.0, r, qm), qthr);
    const double bin = fma(r, qa, qc);
    const bool inc = lo > 0.0;
    delta[mine][lane] = inc ? eff - bin : eff;
    if (keeper) {
      const BayesState* sc = st + ch;
      const double bfin = inc ? bin : bout, dfin = inc ? 1.0 : 0.0;
      const int64_t o = ch * 2 * p + ((sc->it & 1) ^ 1) * p + j;
      b[o] = bfin;
      d[o] = dfin;
      if (brr_accumulate(sc)) {
        const double k = (double)(sc->nsum + 1);
        bbar[ch * p + j] = bb_old * ((k - 1.0) / k) + (inc ? bfin : 0.0) / k;
        dbar[ch * p + j] = db_old * ((k - 1.0) / k) + dfin / k;
      }
    }
  }
  __syncthreads();
  double ei[CH];
#pragma unroll
  for (int c = 0; c < CH; c++) {
    ei[c] = 0.0;
    if (c < nc && i < n) {
      double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < BB; s2 += 2) {
        acc0 = fma(delta[c][s2], xv[s2], acc0);
        acc1 = fma(delta[c][s2 + 1], xv[s2 + 1], acc1);
      }
      ei[c] = e_old[c] + (acc0 + acc1);
      if constexpr (SETS) ei[c] = (trains >> c) & 1u ? ei[c] : 0.0;
      e[(ch0 + c) * ldx + i] = ei[c];
    }
  }
  if (more) {
#pragma unroll
    for (int c = 0; c < CH; c++)
      if (c < nc) es[c][tid] = ei[c];
    __syncthreads();  // also completes the global_load_lds of Xn
    // byte storage: this lane's row, the wave's quarter (one read for the row's chains)
    [[maybe_unused]] uint4 v[4] = {};
    if constexpr (sizeof(T) != 8) {
      if (lane < nb1) {
        const uint8_t* xr = Xb + lane * IW;
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = *reinterpret_cast<const uint4*>(xr + (((4 * wave + t) ^ (lane & 15)) * 16));
      }
    }
#pragma unroll
    for (int c = 0; c < CH; c++) {
      if (c >= nc) break;
      double s0 = 0.0, s1 = 0.0;
      if (lane < nb1) {
        const double* er = es[c] + wave * 64;
        if constexpr (sizeof(T) == 8) {
          const double* xr = Xn + lane * RP + wave * 64;
#pragma unroll
          for (int u = 0; u < 64; u += 2) {
            const double2 xv2 = *reinterpret_cast<const double2*>(xr + u);
            s0 = fma(xv2.x, er[u], s0);
            s1 = fma(xv2.y, er[u + 1], s1);
          }
        } else {
          brr_dot64_u8(v, er, s0, s1);
          s0 *= xs;
          s1 *= xs;
        }
      }
      part4[c][wave][lane] = s0 + s1;
    }
    __syncthreads();
    if (runner)
      partial_out[ch * pstride + blockIdx.x * BB + lane] =
          ((part4[mine][0][lane] + part4[mine][1][lane]) + part4[mine][2][lane]) + part4[mine][3][lane];
  }
}

// Per-marker variances (BayesA, BayesB: varB_j = (S + b_j²)/χ²(df0 + 1) on the stream PM(it, j))
// and, per workgroup, the partial sums vpart[5 blk ..] = Σ 1/varB_j, Σ d_j, Σ b_j², Σ varB_j over
// its 256 markers and Σ e_i² over its 256 individuals (no atomics: bayes_final_kernel adds the
// workgroups' partials in index order). blockIdx.y is the chain (e at c·lde, vpart at c·5·gridDim.x).
__global__ void __launch_bounds__(256) bayes_var_kernel(const double* __restrict__ b, const double* __restrict__ d,
                                                        double* __restrict__ varB, int64_t p,
                                                        const double* __restrict__ e, int64_t lde, int64_t n,
                                                        const BayesState* __restrict__ st,
                                                        double* __restrict__ vpart) {
  __shared__ double red[4];
  const int64_t ch = blockIdx.y;
  b += ch * 2 * p;
  d += ch * 2 * p;
  varB += ch * p;
  e += ch * lde;
  st += ch;
  vpart += ch * 5 * (int64_t)gridDim.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t par = (st->it & 1) ^ 1;  // this iteration's samples
  double v[5] = {0, 0, 0, 0, 0};
  if (j < p) {
    const double bj = b[par * p + j];
    v[1] = d[par * p + j];
    v[2] = bj * bj;
    if (st->model != GBM_BAYES_C) {
      const uint64_t pm = (1ull << 63) | ((uint64_t)st->it << 40) | (uint64_t)j;
      const double vb = (st->S + v[2]) / brr_chisq(st->seed, pm, st->df0 + 1.0);
      varB[j] = vb;
      v[0] = 1.0 / vb;
      v[3] = vb;
    }
  }
  if (j < n) v[4] = e[j] * e[j];
#pragma unroll
  for (int u = 0; u < 5; u++) {
    const double s = brr_block_sum<256>(v[u], red);
    if (threadIdx.x == 0) vpart[5 * (int64_t)blockIdx.x + u] = s;
  }
}

// The scalar draws of an iteration (one workgroup): S, BayesC's common varB, π, varE; the running
// means of μ, varE, mean_j varB_j and π; next iteration. Workgroup c is chain c. SETS: n is the chain's n_c.
template <bool SETS>
__global__ void __launch_bounds__(256) bayes_final_kernel(const double* __restrict__ vpart, int64_t nvb, int64_t p,
                                                          int64_t n, BayesState* __restrict__ st,
                                                          RowSetsArg<SETS> rs) {
  __shared__ double red[4];
  vpart += (int64_t)blockIdx.x * 5 * nvb;
  st += blockIdx.x;
  if constexpr (SETS) n = rs.nrows[blockIdx.x];
  double sum[5];
#pragma unroll
  for (int u = 0; u < 5; u++) {
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
  st->varE = (sum[4] + st->S0e) / brr_chisq(seed, A + 2, df0 + (double)n);
  if (brr_accumulate(st)) {
    const double k = (double)(st->nsum + 1);
    st->mubar = st->mubar * ((k - 1.0) / k) + st->mu / k;
    st->varEbar = st->varEbar * ((k - 1.0) / k) + st->varE / k;
    st->varBbar = st->varBbar * ((k - 1.0) / k) + vbmean / k;
    st->pibar = st->pibar * ((k - 1.0) / k) + st->pi / k;
    st->nsum += 1;
  }
  st->it += 1;
}

}  // namespace

int bayes_check_args(const char* entry, int model, const double* X, const double* y, const double* b_hat_out, int64_t n,
                     int64_t p, int64_t ldx, int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0,
                     double prob_in, double counts) {
  const std::string who(entry);
  if (model != GBM_BAYES_A && model != GBM_BAYES_B && model != GBM_BAYES_C)
    return fail(GBM_E_ARG, who + ": model must be GBM_BAYES_A, GBM_BAYES_B or GBM_BAYES_C");
  GBM_TRY(gibbs_check_args(entry, X, y, b_hat_out, n, p, ldx, n_iter, n_burnin, thin, r2, df0));
  // the gamma sampler (Marsaglia-Tsang) needs shapes >= 1: (df0 + 1)/2 of the per-marker variances
  // and counts·prob_in, counts·(1 − prob_in) of π's Beta draw
  if (!(df0 >= 1.0) || !(prob_in > 0.0 && prob_in < 1.0) || !(counts * prob_in >= 1.0) ||
      !(counts * (1.0 - prob_in) >= 1.0))
    return fail(GBM_E_ARG, who + ": bad prior (df0 >= 1, 0 < prob_in < 1, counts*prob_in >= 1, "
                                 "counts*(1 - prob_in) >= 1)");
  // the per-marker random streams are (iteration, marker) packed into 23 + 40 bits
  if (n_iter > ((int64_t)1 << 23) || p >= ((int64_t)1 << 40))
    return fail(GBM_E_ARG, who + ": n_iter <= 2^23 and p < 2^40");
  return GBM_OK;
}

int bayes_setup_shared(BrrCtx& cx, const double* X, int64_t n, int64_t p, int64_t ldx, int64_t nchains, GibbsData& g,
                       RowSetsHost* rs) {
  const int dev = cx.dev;
  const int64_t nblk = (p + BB - 1) / BB, ppad = nblk * BB, T = nchains;
  const int64_t npad = round_up(n, IW), C = (n + IW - 1) / IW;
  GBM_TRY(ensure(cx.dind, dev, T * 2 * p * 8));  // two copies (iteration parity), as b
  GBM_TRY(ensure(cx.dbar, dev, T * p * 8));
  GBM_TRY(ensure(cx.varBj, dev, T * p * 8));
  GBM_TRY(ensure(cx.pk, dev, T * ppad * 8 * 8));
  GBM_TRY(ensure(cx.vpart, dev, T * bayes_var_blocks(n, p) * 5 * 8));
  if (T > 1) {  // the per-chain copies of what gibbs_upload sizes for one chain
    GBM_TRY(ensure(cx.e, dev, T * npad * 8));
    GBM_TRY(ensure(cx.b, dev, T * 2 * p * 8));
    GBM_TRY(ensure(cx.bbar, dev, T * p * 8));
    GBM_TRY(ensure(cx.r, dev, std::max<int64_t>(T * 2 * C * BB, 2 * C * BK2) * 8));
  }
  if (rs) {  // the per-set sizes first, so that gibbs_upload's own ensure finds them
    GBM_TRY(ensure(cx.colmean, dev, rs->nsets * p * 8));
    GBM_TRY(ensure(cx.x2, dev, rs->nsets * p * 8));
  }
  GBM_TRY(gibbs_upload(cx, X, n, p, ldx, g));
  if (rs) return gibbs_sets(cx, n, p, g.npad, nblk, nchains, *rs);
  GBM_TRY(gibbs_gram(cx, n, p, g.npad, nblk, 1));
  GBM_HIP_TRY(hipStreamSynchronize(cx.stream.s));
  return GBM_OK;
}

int bayes_start(const char* entry, BrrCtx& cx, int64_t chain, int model, int64_t n, int64_t p, const double* y,
                int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in, double counts, uint64_t seed,
                const GibbsData& g, BayesState& st0) {
  GibbsPrior pr;
  GBM_TRY(gibbs_prior(entry, y, n, p, g, pr));
  return bayes_start_from(cx, chain, model, p, g.npad, pr, n_burnin, thin, r2, df0, prob_in, counts, seed, st0);
}

int bayes_start_from(BrrCtx& cx, int64_t chain, int model, int64_t p, int64_t npad, const GibbsPrior& pr,
                     int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in, double counts,
                     uint64_t seed, BayesState& st0) {
  hipStream_t s = cx.stream.s;
  const double shape0 = 1.1;
  double S0 = pr.vy * r2 / pr.msx * (df0 + 2.0);
  if (model != GBM_BAYES_A) S0 /= prob_in;
  st0 = BayesState{};
  st0.mu = pr.ym;
  st0.S0e = pr.vy * (1.0 - r2) * (df0 + 2.0);
  st0.varE = st0.S0e / (df0 + 2.0);
  st0.S = S0;
  st0.varBc = S0 / (df0 + 2.0);
  st0.rate0 = (shape0 - 1.0) / S0;
  st0.shape0 = shape0;
  st0.df0 = df0;
  st0.pi = prob_in;
  st0.cIn = counts * prob_in;
  st0.cOut = counts * (1.0 - prob_in);
  st0.burnin = n_burnin;
  st0.thin = thin;
  st0.seed = seed;
  st0.model = model;
  double* e = (double*)cx.e.p + chain * npad;
  double* b = (double*)cx.b.p + chain * 2 * p;
  double* d = (double*)cx.dind.p + chain * 2 * p;
  std::vector<double> init(2 * p, 1.0);  // d = 1; then varB_j = S0/(df0 + 2)
  GBM_HIP_TRY(hipMemcpyAsync(e, pr.e0.data(), npad * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(d, init.data(), 2 * p * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  std::fill(init.begin(), init.begin() + p, st0.varBc);
  GBM_HIP_TRY(hipMemcpyAsync((double*)cx.varBj.p + chain * p, init.data(), p * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemsetAsync(b, 0, 2 * p * 8, s));
  GBM_HIP_TRY(hipMemsetAsync((double*)cx.bbar.p + chain * p, 0, p * 8, s));
  GBM_HIP_TRY(hipMemsetAsync((double*)cx.dbar.p + chain * p, 0, p * 8, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));  // init leaves scope
  return GBM_OK;
}

int bayes_setup(const char* entry, BrrCtx& cx, int model, const double* X, int64_t n, int64_t p, int64_t ldx,
                const double* y, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in, double counts,
                uint64_t seed, GibbsData& g, BayesState& st0) {
  GBM_TRY(bayes_setup_shared(cx, X, n, p, ldx, 1, g));
  return bayes_start(entry, cx, 0, model, n, p, y, n_burnin, thin, r2, df0, prob_in, counts, seed, g, st0);
}

namespace {
template <typename T, int CH, bool ROWS, bool SETS = false>
void launch_chain(BrrCtx& cx, int64_t n, int64_t p, const GibbsData& g, int64_t k, int64_t nblk, int64_t nchains,
                  BayesState* stp, RowSetsArg<SETS> rs = {}) {
  const int64_t C = g.C64;
  const T* X = sizeof(T) == 8 ? (const T*)cx.Xt.p : (const T*)cx.D.p;
  const double* pin = (const double*)cx.r.p + (k & 1) * C * BB;
  double* pout = (double*)cx.r.p + ((k + 1) & 1) * C * BB;
  bayes_chain_kernel<T, CH, ROWS, SETS><<<dim3((unsigned)C, (unsigned)((nchains + CH - 1) / CH)), 256, 0, cx.stream.s>>>(
      X, g.npad, n, p, sizeof(T) == 8 ? 1.0 : g.xs, (const double*)cx.W.p, k, nblk, (int)nchains, pin, pout,
      (const double*)cx.pk.p, (double*)cx.b.p, (double*)cx.dind.p, (double*)cx.bbar.p, (double*)cx.dbar.p,
      (double*)cx.e.p, stp, rs);
}
}  // namespace

void bayes_enqueue_chain(BrrCtx& cx, int64_t n, int64_t p, const GibbsData& g, BayesState* stp, int64_t nchains,
                         int per_wg, const RowSets* rs) {
  hipStream_t s = cx.stream.s;
  const int64_t nblk = (p + BB - 1) / BB, ppad = nblk * BB;
  const bool bytes = g.xs > 0.0;
  const dim3 pgrid((unsigned)(ppad / 256 + 1), (unsigned)nchains);
  if (rs) {
    bayes_prep_kernel<true><<<pgrid, 256, 0, s>>>(p, ppad, (const double*)cx.x2.p, (const double*)cx.b.p,
                                                  (const double*)cx.dind.p, (const double*)cx.varBj.p, stp,
                                                  (double*)cx.pk.p, *rs);
    bayes_mu_kernel<true><<<(unsigned)nchains, 1024, 0, s>>>((double*)cx.e.p, g.npad, n, stp, *rs);
  } else {
    bayes_prep_kernel<false><<<pgrid, 256, 0, s>>>(p, ppad, (const double*)cx.x2.p, (const double*)cx.b.p,
                                                   (const double*)cx.dind.p, (const double*)cx.varBj.p, stp,
                                                   (double*)cx.pk.p, NoRowSets{});
    bayes_mu_kernel<false><<<(unsigned)nchains, 1024, 0, s>>>((double*)cx.e.p, g.npad, n, stp, NoRowSets{});
  }
  gibbs_dots0(cx, n, p, g, bytes, nchains);
  for (int64_t k = 0; k < nblk; k++) {
    if (rs) {  // held-out rows: e stays 0.0 there (one chain per row also when there is one chain)
      if (per_wg == 4) {
        if (bytes) launch_chain<uint8_t, 4, true, true>(cx, n, p, g, k, nblk, nchains, stp, *rs);
        else launch_chain<double, 4, true, true>(cx, n, p, g, k, nblk, nchains, stp, *rs);
      } else {
        if (bytes) launch_chain<uint8_t, 1, true, true>(cx, n, p, g, k, nblk, nchains, stp, *rs);
        else launch_chain<double, 1, true, true>(cx, n, p, g, k, nblk, nchains, stp, *rs);
      }
    } else if (per_wg == 4) {
      if (bytes) launch_chain<uint8_t, 4, true>(cx, n, p, g, k, nblk, nchains, stp);
      else launch_chain<double, 4, true>(cx, n, p, g, k, nblk, nchains, stp);
    } else if (nchains > 1) {
      if (bytes) launch_chain<uint8_t, 1, true>(cx, n, p, g, k, nblk, nchains, stp);
      else launch_chain<double, 1, true>(cx, n, p, g, k, nblk, nchains, stp);
    } else {
      if (bytes) launch_chain<uint8_t, 1, false>(cx, n, p, g, k, nblk, 1, stp);
      else launch_chain<double, 1, false>(cx, n, p, g, k, nblk, 1, stp);
    }
  }
}

void bayes_enqueue_var(BrrCtx& cx, int64_t n, int64_t p, BayesState* stp, int64_t nchains) {
  const int64_t npad = round_up(n, IW);
  bayes_var_kernel<<<dim3((unsigned)bayes_var_blocks(n, p), (unsigned)nchains), 256, 0, cx.stream.s>>>(
      (const double*)cx.b.p, (const double*)cx.dind.p, (double*)cx.varBj.p, p, (const double*)cx.e.p, npad, n, stp,
      (double*)cx.vpart.p);
}

}  // namespace gbm

using namespace gbm;

// One BayesA / BayesB / BayesC fit on a leased context (include/gbm.h gbm_bayes_fit): the shared
// setup (genotypes, column statistics, byte quantisation, Gram blocks), then per iteration the
// linear chain prep, μ, block 0's partial dots, one chain launch per 64-marker block, the
// variances — captured once as a graph and replayed. Never the super-block sweep or its lock; the
// BRR path statistics are not written.
static int bayes_fit_impl(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                          int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                          double counts, uint64_t seed, int dev, double* b_hat_out, double* y_pred_out,
                          double* var_out, double* pip_out) {
  BrrLease lease;
  GBM_TRY(CtxPool<BrrCtx>::instance().acquire(dev, lease.c));
  BrrCtx& cx = *lease.c;
  GBM_HIP_TRY(hipSetDevice(dev));
  hipStream_t s = cx.stream.s;
  GBM_TRY(ensure(cx.bst, dev, sizeof(BayesState)));
  GibbsData g;
  BayesState st0{};
  GBM_TRY(bayes_setup("gbm_bayes_fit", cx, model, X, n, p, ldx, y, n_burnin, thin, r2, df0, prob_in, counts, seed, g,
                      st0));
  const int64_t npad = g.npad, nvb = bayes_var_blocks(n, p);
  const double xs = g.xs;
  GBM_HIP_TRY(hipMemcpyAsync(cx.bst.p, &st0, sizeof(BayesState), hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  auto* stp = (BayesState*)cx.bst.p;
  auto enqueue_iteration = [&]() -> int {
    bayes_enqueue_chain(cx, n, p, g, stp);
    bayes_enqueue_var(cx, n, p, stp);
    bayes_final_kernel<false><<<1, 256, 0, s>>>((const double*)cx.vpart.p, nvb, p, n, stp, NoRowSets{});
    return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, "gbm_bayes_fit: launch failed");
  };
  cx.bayes_graph.ensure({model, n, p, npad, (int64_t)(xs * 64.0), key_of(cx.Xt), key_of(cx.D), key_of(cx.W),
                         key_of(cx.r), key_of(cx.e), key_of(cx.b), key_of(cx.dind), key_of(cx.bbar), key_of(cx.dbar),
                         key_of(cx.varBj), key_of(cx.pk), key_of(cx.vpart), key_of(cx.x2), key_of(cx.bst)},
                        s, enqueue_iteration);
  GBM_TRY(cx.bayes_graph.run(n_iter, s, "gbm_bayes_fit", enqueue_iteration));
  BayesState fin{};
  GBM_TRY(gibbs_outputs(cx, n, p, npad, cx.bst, &fin, sizeof(fin), &fin.mubar, b_hat_out, pip_out, y_pred_out));
  if (var_out) {
    var_out[0] = fin.varEbar;
    var_out[1] = fin.varBbar;
    var_out[2] = fin.pibar;
  }
  return GBM_OK;
}

extern "C" int gbm_bayes_fit(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                             int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                             double counts, uint64_t seed, int device, double* b_hat_out, double* y_pred_out,
                             double* var_out, double* pip_out) {
  RoctxRange r_("gbm_bayes_fit");
  set_error("");
  GBM_TRY(bayes_check_args("gbm_bayes_fit", model, X, y, b_hat_out, n, p, ldx, n_iter, n_burnin, thin, r2, df0, prob_in,
                           counts));
  int dev = 0;
  GBM_TRY(gibbs_check_run("gbm_bayes_fit", y, n, n_iter, n_burnin, thin, device, dev));
  return bayes_fit_impl(model, X, n, p, ldx, y, n_iter, n_burnin, thin, r2, df0, prob_in, counts, seed, dev, b_hat_out,
                        y_pred_out, var_out, pip_out);
}


// gbm_bayes_fit_multi on a leased context: gbm_bayes_fit's setup once (genotypes, column statistics, byte
// quantisation, Gram blocks), a start state per chain, then the iteration of all chains (the kernels of
// gbm_bayes_fit with a chain index) captured as the context's multi graph and replayed; outputs per chain.
// rsh (gbm_bayes_fit_multi_rows): chain c trains on the rows of its set. The statistics and Gram blocks are built
// per set, the prior moments and the start residual are taken over the set, and the iteration is that of the SETS
// kernels, captured in a graph slot of its own (the key holds nsets and the mask buffers).
static std::atomic<int64_t> g_multi_calls{0}, g_multi_chains{0}, g_rows_calls{0}, g_rows_chains{0};

static int bayes_fit_multi_impl(int64_t T, const int* models, const double* X, int64_t n, int64_t p, int64_t ldx,
                                const double* Y, int64_t ldy, int64_t n_iter, int64_t n_burnin, int64_t thin,
                                const double* r2, const double* df0, const double* prob_in, const double* counts,
                                const uint64_t* seeds, int dev, double* b_hat_out, int64_t ldb, double* y_pred_out,
                                int64_t ldp, double* var_out, double* pip_out, int64_t ldpip,
                                RowSetsHost* rsh = nullptr) {
  const char* entry = rsh ? "gbm_bayes_fit_multi_rows" : "gbm_bayes_fit_multi";
  BrrLease lease;
  GBM_TRY(CtxPool<BrrCtx>::instance().acquire(dev, lease.c));
  BrrCtx& cx = *lease.c;
  GBM_HIP_TRY(hipSetDevice(dev));
  hipStream_t s = cx.stream.s;
  GBM_TRY(ensure(cx.bst, dev, T * (int64_t)sizeof(BayesState)));
  GibbsData g;
  GBM_TRY(bayes_setup_shared(cx, X, n, p, ldx, T, g, rsh));
  const int64_t npad = g.npad, nvb = bayes_var_blocks(n, p);
  std::vector<BayesState> st0((size_t)T);
  if (rsh) {
    GibbsPrior pr;
    for (int64_t t = 0; t < rsh->nsets; t++) {  // MSx of every set, named by set
      double msx = 0.0, smsq = 0.0;
      for (int64_t j = 0; j < p; j++) {
        msx += rsh->xx[(size_t)(t * p + j)];
        smsq += rsh->cm[(size_t)(t * p + j)] * rsh->cm[(size_t)(t * p + j)];
      }
      if (!(msx / (double)rsh->nrows[(size_t)t] - smsq > 0.0))
        return fail(GBM_E_DATA, std::string(entry) + ": set " + std::to_string(t) +
                                    ": the markers have no variance on its rows");
    }
    for (int64_t c = 0; c < T; c++) {
      const std::string who = std::string(entry) + ": chain " + std::to_string(c);
      const int64_t t = rsh->set_of[c];
      GBM_TRY(gibbs_prior_rows(who.c_str(), Y + c * ldy, n, p, npad, rsh->rows + t * rsh->ldrows,
                               rsh->nrows[(size_t)t], rsh->cm.data() + t * p, rsh->xx.data() + t * p, pr));
      GBM_TRY(bayes_start_from(cx, c, models[c], p, npad, pr, n_burnin, thin, r2[c], df0[c], prob_in[c], counts[c],
                               seeds[c], st0[(size_t)c]));
    }
  } else {
    for (int64_t c = 0; c < T; c++) {
      const std::string who = "gbm_bayes_fit_multi: chain " + std::to_string(c);
      GBM_TRY(bayes_start(who.c_str(), cx, c, models[c], n, p, Y + c * ldy, n_burnin, thin, r2[c], df0[c], prob_in[c],
                          counts[c], seeds[c], g, st0[(size_t)c]));
    }
  }
  GBM_HIP_TRY(hipMemcpyAsync(cx.bst.p, st0.data(), (size_t)T * sizeof(BayesState), hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  auto* stp = (BayesState*)cx.bst.p;
  // Chains per workgroup row of the chain launch (the results have the same bits): one (the one-chain kernel on
  // nchains rows) or four (a chain per wave). A workgroup holds a CU (LDS), so a launch runs in
  // ⌈workgroups / CUs⌉ rounds; a round of four-chain workgroups takes twice a round of one-chain workgroups (each
  // wave sums, updates and forms partials for four chains) and there are a quarter of the workgroups. The mapping
  // with the shorter launch by that count is taken, one chain per row at a tie (measured at C4: DESIGN.md
  // §4.6.3). GBM_BAYES_MULTI_WG = 1 or 4 forces the mapping (read per call).
  int cus = 0;
  GBM_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  cus = std::max(cus, 1);
  const int64_t rounds1 = (g.C64 * T + cus - 1) / cus, rounds4 = (g.C64 * ((T + 3) / 4) + cus - 1) / cus;
  const int64_t forced = knob_i64("GBM_BAYES_MULTI_WG", 0);
  const int per_wg = forced == 1 ? 1 : forced == 4 ? 4 : (rounds1 <= 2 * rounds4 ? 1 : 4);
  const RowSets rs{(const uint32_t*)cx.smask.p, (const int*)cx.sof.p, (const int64_t*)cx.snrows.p,
                   ((p + BB - 1) / BB) * BB * BB};  // read by the SETS launches only
  auto enqueue_iteration = [&]() -> int {
    bayes_enqueue_chain(cx, n, p, g, stp, T, per_wg, rsh ? &rs : nullptr);
    bayes_enqueue_var(cx, n, p, stp, T);
    if (rsh)
      bayes_final_kernel<true><<<(unsigned)T, 256, 0, s>>>((const double*)cx.vpart.p, nvb, p, n, stp, rs);
    else
      bayes_final_kernel<false><<<(unsigned)T, 256, 0, s>>>((const double*)cx.vpart.p, nvb, p, n, stp, NoRowSets{});
    return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, std::string(entry) + ": launch failed");
  };
  std::vector<int64_t> key{T, per_wg, n, p, npad, (int64_t)(g.xs * 64.0), key_of(cx.Xt), key_of(cx.D), key_of(cx.W),
                           key_of(cx.r), key_of(cx.e), key_of(cx.b), key_of(cx.dind), key_of(cx.bbar), key_of(cx.dbar),
                           key_of(cx.varBj), key_of(cx.pk), key_of(cx.vpart), key_of(cx.x2), key_of(cx.bst)};
  if (rsh) key.insert(key.end(), {rsh->nsets, key_of(cx.smask), key_of(cx.sof), key_of(cx.snrows)});
  IterGraph& graph = rsh ? cx.rows_graph : cx.multi_graph;
  graph.ensure(key, s, enqueue_iteration);
  GBM_TRY(graph.run(n_iter, s, entry, enqueue_iteration));
  for (int64_t c = 0; c < T; c++) {
    BayesState fin{};
    GBM_TRY(gibbs_outputs(cx, n, p, npad, cx.bst, &fin, sizeof(fin), &fin.mubar, b_hat_out + c * ldb,
                          pip_out ? pip_out + c * ldpip : nullptr, y_pred_out ? y_pred_out + c * ldp : nullptr, c));
    if (var_out) {
      var_out[3 * c] = fin.varEbar;
      var_out[3 * c + 1] = fin.varBbar;
      var_out[3 * c + 2] = fin.pibar;
    }
  }
  (rsh ? g_rows_calls : g_multi_calls).fetch_add(1, std::memory_order_relaxed);
  (rsh ? g_rows_chains : g_multi_chains).fetch_add(T, std::memory_order_relaxed);
  return GBM_OK;
}

// the checks of the chain count, the required pointers and the pitches that both multi-chain entries make first
static int multi_check_shape(const char* entry, int64_t nchains, const int* models, const double* X, const double* Y,
                             const double* r2, const double* df0, const double* prob_in, const double* counts,
                             const uint64_t* seeds, const double* b_hat_out, int64_t n, int64_t p, int64_t ldy,
                             int64_t ldb, const double* y_pred_out, int64_t ldp, const double* pip_out, int64_t ldpip) {
  const std::string who(entry);
  if (nchains < 1 || nchains > GBM_BAYES_MAX_CHAINS)
    return fail(GBM_E_ARG, who + ": 1 <= nchains <= " + std::to_string(GBM_BAYES_MAX_CHAINS));
  if (!models || !X || !Y || !r2 || !df0 || !prob_in || !counts || !seeds || !b_hat_out)
    return fail(GBM_E_ARG, who + ": models, X, Y, r2, df0, prob_in, counts, seeds and b_hat_out are required");
  if (ldy < n || ldb < p + 1 || (y_pred_out && ldp < n) || (pip_out && ldpip < p))
    return fail(GBM_E_ARG, who + ": bad pitch (ldy >= n, ldb >= p + 1, ldp >= n, ldpip >= p)");
  return GBM_OK;
}

extern "C" int gbm_bayes_fit_multi(int64_t nchains, const int* models, const double* X, int64_t n, int64_t p,
                                   int64_t ldx, const double* Y, int64_t ldy, int64_t n_iter, int64_t n_burnin,
                                   int64_t thin, const double* r2, const double* df0, const double* prob_in,
                                   const double* counts, const uint64_t* seeds, int device, double* b_hat_out,
                                   int64_t ldb, double* y_pred_out, int64_t ldp, double* var_out, double* pip_out,
                                   int64_t ldpip) {
  RoctxRange r_("gbm_bayes_fit_multi");
  set_error("");
  GBM_TRY(multi_check_shape("gbm_bayes_fit_multi", nchains, models, X, Y, r2, df0, prob_in, counts, seeds, b_hat_out,
                            n, p, ldy, ldb, y_pred_out, ldp, pip_out, ldpip));
  int dev = 0;
  for (int64_t c = 0; c < nchains; c++) {
    const std::string who = "gbm_bayes_fit_multi: chain " + std::to_string(c);
    GBM_TRY(bayes_check_args(who.c_str(), models[c], X, Y + c * ldy, b_hat_out, n, p, ldx, n_iter, n_burnin, thin, r2[c],
                             df0[c], prob_in[c], counts[c]));
    // the phenotype checks speak of "phenotype 1": put the chain in front
    const int rc = check_y(Y + c * ldy, n, n, 1);
    if (rc != GBM_OK) return fail(rc, who + ": " + last_error());
  }
  GBM_TRY(gibbs_check_run("gbm_bayes_fit_multi", Y, n, n_iter, n_burnin, thin, device, dev));
  return bayes_fit_multi_impl(nchains, models, X, n, p, ldx, Y, ldy, n_iter, n_burnin, thin, r2, df0, prob_in, counts,
                              seeds, dev, b_hat_out, ldb, y_pred_out, ldp, var_out, pip_out, ldpip);
}

extern "C" int gbm_bayes_fit_multi_rows(int64_t nchains, const int* models, const double* X, int64_t n, int64_t p,
                                        int64_t ldx, const double* Y, int64_t ldy, int64_t nsets, const uint8_t* rows,
                                        int64_t ldrows, const int* set_of, int64_t n_iter, int64_t n_burnin,
                                        int64_t thin, const double* r2, const double* df0, const double* prob_in,
                                        const double* counts, const uint64_t* seeds, int device, double* b_hat_out,
                                        int64_t ldb, double* y_pred_out, int64_t ldp, double* var_out, double* pip_out,
                                        int64_t ldpip) {
  const char* entry = "gbm_bayes_fit_multi_rows";
  RoctxRange r_(entry);
  set_error("");
  const std::string who(entry);
  GBM_TRY(multi_check_shape(entry, nchains, models, X, Y, r2, df0, prob_in, counts, seeds, b_hat_out, n, p, ldy, ldb,
                            y_pred_out, ldp, pip_out, ldpip));
  if (nsets < 1 || nsets > nchains) return fail(GBM_E_ARG, who + ": 1 <= nsets <= nchains");
  if (!rows || !set_of) return fail(GBM_E_ARG, who + ": rows and set_of are required");
  if (n < 3 || ldx < n || ldrows < n) return fail(GBM_E_ARG, who + ": bad arguments (n >= 3, ldx >= n, ldrows >= n)");
  RowSetsHost rsh;
  rsh.nsets = nsets;
  rsh.rows = rows;
  rsh.ldrows = ldrows;
  rsh.set_of = set_of;
  rsh.nrows.assign((size_t)nsets, 0);
  for (int64_t t = 0; t < nsets; t++) {
    const uint8_t* r = rows + t * ldrows;
    int64_t nc = 0;
    for (int64_t i = 0; i < n; i++) {
      if (r[i] > 1)
        return fail(GBM_E_ARG, who + ": set " + std::to_string(t) + " has a byte other than 0 or 1 at row " +
                                   std::to_string(i));
      nc += r[i];
    }
    if (nc < 3) return fail(GBM_E_ARG, who + ": set " + std::to_string(t) + " has fewer than 3 rows");
    rsh.nrows[(size_t)t] = nc;
  }
  std::vector<double> ys;
  for (int64_t c = 0; c < nchains; c++) {
    const std::string whoc = who + ": chain " + std::to_string(c);
    if (set_of[c] < 0 || set_of[c] >= nsets)
      return fail(GBM_E_ARG, whoc + ": set_of is " + std::to_string(set_of[c]) + ", outside [0, nsets)");
    const uint8_t* r = rows + set_of[c] * ldrows;
    const int64_t nc = rsh.nrows[(size_t)set_of[c]];
    // gbm_bayes_fit's checks with the chain's own n_c (ldx >= n is checked above)
    GBM_TRY(bayes_check_args(whoc.c_str(), models[c], X, Y + c * ldy, b_hat_out, nc, p, nc, n_iter, n_burnin, thin,
                             r2[c], df0[c], prob_in[c], counts[c]));
    ys.clear();  // the phenotype checks on the chain's rows: Y is not read as a number elsewhere
    for (int64_t i = 0; i < n; i++)
      if (r[i]) ys.push_back(Y[c * ldy + i]);
    const int rc = check_y(ys.data(), nc, nc, 1);  // its "entry k" is the k-th row of the set
    if (rc != GBM_OK) return fail(rc, whoc + ": " + last_error());
  }
  int dev = 0;
  GBM_TRY(gibbs_check_run(entry, nullptr, n, n_iter, n_burnin, thin, device, dev));
  return bayes_fit_multi_impl(nchains, models, X, n, p, ldx, Y, ldy, n_iter, n_burnin, thin, r2, df0, prob_in, counts,
                              seeds, dev, b_hat_out, ldb, y_pred_out, ldp, var_out, pip_out, ldpip, &rsh);
}

extern "C" int gbm_debug_bayes_rows_stats(int64_t* calls, int64_t* chains) {
  if (calls) *calls = g_rows_calls.load(std::memory_order_relaxed);
  if (chains) *chains = g_rows_chains.load(std::memory_order_relaxed);
  return GBM_OK;
}

extern "C" int gbm_debug_bayes_multi_stats(int64_t* calls, int64_t* chains) {
  if (calls) *calls = g_multi_calls.load(std::memory_order_relaxed);
  if (chains) *chains = g_multi_chains.load(std::memory_order_relaxed);
  return GBM_OK;
}
