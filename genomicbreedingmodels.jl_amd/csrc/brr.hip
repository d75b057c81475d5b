// Bayesian ridge regression (BGLR model "BRR") by Gibbs sampling — SURVEY.md §8f row 3 (config
// C4); replaces the Rscript/BGLR round trip of reference src/bayes.jl:28-105,158-224.
//
// The chain is BGLR's single-site sampler (intercept, then every marker j in order with the
// residual update e += (b_old − b_new) x_j, then σ²_b and σ²_e from scaled-inverse-χ² draws;
// BGLR defaults df0 = 5, R2 = 0.5; running posterior means every `thin` iterations after
// burn-in). MI355X mapping: markers go in blocks of 64 (128 per launch with byte storage). For a
// block, x_kᵀe of its markers comes from per-chunk partial dots (computed by the previous launch),
// and the block's sequential single-site steps are one unit-lower-triangular solve (I + L) δ = r̃
// whose inverse M is rebuilt for every block once per iteration (it depends on σ²_e/σ²_b): every
// workgroup applies δ = M r̃ redundantly from identical inputs (deterministic), updates e += X_B δ
// on its individuals and computes the next block's partial dots, so a block costs one launch and
// no device-wide synchronisation; one Gibbs iteration is captured as a hipGraph and replayed.
// With byte storage and n <= 48 x CUs the iteration is instead ONE persistent sweep launch
// (brr_sweep.hip); otherwise the per-block launches of this file run. The setup, the pooled
// context and the graph replay are shared with BayesA/B/C (gibbs_setup.hip, gibbs_common.h).
#include <atomic>

#include "gibbs_common.h"

namespace gbm {
namespace {

// intercept: BGLR adds μ back, samples μ ~ N(Σe/n, σ²_e/n), subtracts it again (one workgroup)
__global__ void __launch_bounds__(1024) brr_mu_kernel(double* __restrict__ e, int64_t n, BrrState* __restrict__ st) {
  __shared__ double red[16];
  const double mu_old = st->mu;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) s += e[i] + mu_old;
  s = brr_block_sum<1024>(s, red);
  const double varE = st->varE;
  const double mu = s / (double)n + sqrt(varE / (double)n) * brr_normal(st->seed, 4 * (uint64_t)st->it, 0xFFFFFFFFull);
  for (int64_t i = threadIdx.x; i < n; i += 1024) e[i] = (e[i] + mu_old) - mu;
  __syncthreads();
  if (threadIdx.x == 0) st->mu = mu;
}

// The single-site steps of a 64-marker block as one triangular solve. Marker k's conditional draw
// is b_new = α_k d_k + β_k with d_k = x_kᵀe at its turn, so δ_k = b_old − b_new = γ_k − α_k d_k
// (γ = b_old − β). Step s changes every later d_k by δ_s W[s][k], hence with d⁰ = x_kᵀe at block
// start and r̃ = γ − α∘d⁰:
//   δ_s + α_s Σ_{t<s} W[s][t] δ_t = r̃_s,  i.e.  (I + L) δ = r̃,  L[s][t] = α_s W[s][t] (t < s).
// α_k = 1 / (x_kᵀx_k + σ²_e/σ²_b) and γ depend only on the iteration's variances, b_old and the
// iteration's normals, so M = (I + L)⁻¹ (unit lower triangular) and γ are computed for every block
// once per iteration (brr_prep_kernel) and a launch applies δ = M r̃ as one GEMV — no chain of 64
// dependent steps. Two halves A, B of a 128-marker launch: B's d⁰ also misses A's changes
// (d_B = d⁰_B + W_BA δ_A), so δ_B = M_B r̃_B + O r̃_A with O = −M_B diag(α_B) W_BA M_A.
//
// brr_prep_kernel: α, γ of every marker; per 64-marker half-block, lane j of one wave solves column
// j of M by forward substitution (its column in registers, W's rows broadcast from LDS).
// nw = 1 (64-marker launches): 4 blocks per workgroup, Mb[b] = M_b. nw = 3 (128-marker launches):
// one 128-marker block per workgroup, Mb[3b] = M_A, Mb[3b + 1] = O, Mb[3b + 2] = M_B (row-major).
__global__ void __launch_bounds__(256) brr_prep_kernel(const double* __restrict__ W, int64_t p, int64_t nblk, int nw,
                                                       const double* __restrict__ x2, const double* __restrict__ b,
                                                       const BrrState* __restrict__ st, double* __restrict__ Mb,
                                                       double* __restrict__ alpha, double* __restrict__ gamma,
                                                       double* __restrict__ MSd) {
  __shared__ __attribute__((aligned(16))) double S[4][BB * BB];
  // nw = 3 outputs: Mb's three 64x64 blocks, or (MSd, the super-block sweep) the 128x128 diagonal
  // block of M_S it belongs to (row pitch SBK; its upper right stays zero from the setup memset)
  const int64_t sb_s = (int64_t)blockIdx.x / SBN, sb_i = (int64_t)blockIdx.x % SBN;
  double* const dgo = MSd ? MSd + sb_s * SBK * SBK + sb_i * 2 * BB * (SBK + 1) : nullptr;
  __shared__ double alB[BB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the 64-marker half-block this wave inverts (nw = 3: waves 0, 1 = halves A, B)
  const bool solver = nw == 1 ? (int64_t)blockIdx.x * 4 + wave < nblk : wave < 2;
  const int64_t hb = nw == 1 ? (int64_t)blockIdx.x * 4 + wave : 2 * (int64_t)blockIdx.x + wave;
  double* Sw = S[wave];
  if (solver) {
    const double* Wsrc = W + (nw == 1 ? hb : 3 * (int64_t)blockIdx.x + (wave == 0 ? 0 : 2)) * BB * BB;
    double2 v[32];
#pragma unroll
    for (int u = 0; u < 32; u++) v[u] = *reinterpret_cast<const double2*>(Wsrc + 2 * (lane + 64 * u));
    const int64_t j = hb * BB + lane;
    const bool on = j < p;
    const double varE = st->varE, varB = st->varB;
    const double xx = on ? x2[j] : 0.0;
    const double bo = on ? b[(st->it & 1) * p + j] : 0.0;
    const double c = 1.0 / (xx / varE + 1.0 / varB);
    const double al = on ? c / varE : 0.0;
    const double xi = on ? brr_normal(st->seed, 4 * (uint64_t)st->it, (uint64_t)j) : 0.0;
    alpha[j] = al;  // padded to whole launches
    gamma[j] = on ? bo - (xx * bo * al + sqrt(c) * xi) : 0.0;
    if (nw == 3 && wave == 1) alB[lane] = al;
#pragma unroll
    for (int u = 0; u < 32; u++) *reinterpret_cast<double2*>(Sw + 2 * (lane + 64 * u)) = v[u];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's W rows are in LDS
    // column `lane` of M: m_t = [t = lane] − α_t Σ_{u<t} W[t][u] m_u
    double m[BB];
#pragma unroll
    for (int t = 0; t < BB; t++) {
      double a0 = 0.0, a1 = 0.0;
      if (t > 0) asm volatile("" : "+v"(m[t - 1])::"memory");  // row t's loads after row t − 1
#pragma unroll
      for (int c = 0; c < t; c += 32) {
        // at most 32 values of W's row in flight: this chunk's loads wait for the previous
        // chunk's FMAs (else the scheduler hoists every load of the solve and spills)
        asm volatile("" : "+v"(a0), "+v"(a1)::"memory");
#pragma unroll
        for (int u = c; u + 1 < t && u < c + 32; u += 2) {
          const double2 w2 = *reinterpret_cast<const double2*>(Sw + t * BB + u);
          a0 = fma(w2.x, m[u], a0);
          a1 = fma(w2.y, m[u + 1], a1);
        }
      }
      if (t & 1) a0 = fma(Sw[t * BB + t - 1], m[t - 1], a0);
      // α_t from lane t (in this form, not readlane_f64: the kernel's code is pinned instruction for instruction)
      union {
        double f;
        int i[2];
      } at;
      at.f = al;
      at.i[0] = __builtin_amdgcn_readlane(at.i[0], t);
      at.i[1] = __builtin_amdgcn_readlane(at.i[1], t);
      m[t] = (lane == t ? 1.0 : 0.0) - at.f * (a0 + a1);
    }
    // M[t][lane] (coalesced rows); nw = 3 keeps M_A, M_B in LDS (this wave's W is no longer read)
    double* Mo = Mb + (nw == 1 ? hb : 3 * (int64_t)blockIdx.x + (wave == 0 ? 0 : 2)) * BB * BB + lane;
    int64_t mo_ld = BB;
    if (dgo) {
      Mo = dgo + (wave == 0 ? 0 : BB * (SBK + 1)) + lane;
      mo_ld = SBK;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < BB; t++) {
      Mo[t * mo_ld] = m[t];
      if (nw == 3) Sw[t * BB + lane] = m[t];
    }
  } else if (nw == 3) {
    // waves 2-3 stage W_BA (row k = marker B_k) into S[2] meanwhile
    const double* Wsrc = W + (3 * (int64_t)blockIdx.x + 1) * BB * BB;
    const int t = tid - 128;
    double2 v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = *reinterpret_cast<const double2*>(Wsrc + 2 * (t + 128 * u));
#pragma unroll
    for (int u = 0; u < 16; u++) *reinterpret_cast<double2*>(S[2] + 2 * (t + 128 * u)) = v[u];
  }
  if (nw != 3) return;
  __syncthreads();
  // K = diag(α_B) W_BA M_A into S[3]: thread (wave w, lane j) makes K[16w .. 16w + 15][j]
  {
    double col[BB];
#pragma unroll
    for (int s = 0; s < BB; s++) col[s] = S[0][s * BB + lane];
#pragma unroll 1
    for (int kk = 0; kk < 16; kk++) {
      const int k = 16 * wave + kk;
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int c = 0; c < BB; c += 32) {
        asm volatile("" : "+v"(a0), "+v"(a1)::"memory");
#pragma unroll
        for (int s = c; s < c + 32; s += 2) {
          const double2 w2 = *reinterpret_cast<const double2*>(S[2] + k * BB + s);
          a0 = fma(w2.x, col[s], a0);
          a1 = fma(w2.y, col[s + 1], a1);
        }
      }
      S[3][k * BB + lane] = alB[k] * (a0 + a1);
    }
  }
  __syncthreads();
  // O = −M_B K
  {
    double col[BB];
#pragma unroll
    for (int s = 0; s < BB; s++) col[s] = S[3][s * BB + lane];
    double* Oo = dgo ? dgo + BB * SBK + lane : Mb + (3 * (int64_t)blockIdx.x + 1) * BB * BB + lane;
    const int64_t oo_ld = dgo ? SBK : BB;
#pragma unroll 1
    for (int kk = 0; kk < 16; kk++) {
      const int k = 16 * wave + kk;
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int c = 0; c < BB; c += 32) {
        asm volatile("" : "+v"(a0), "+v"(a1)::"memory");
#pragma unroll
        for (int s = c; s < c + 32; s += 2) {
          const double2 w2 = *reinterpret_cast<const double2*>(S[1] + k * BB + s);
          a0 = fma(w2.x, col[s], a0);
          a1 = fma(w2.y, col[s + 1], a1);
        }
      }
      Oo[k * oo_ld] = -(a0 + a1);
    }
  }
}

// δ_k = Σ_s M[k][s] r̃_s with lane k's row of M in registers and r̃ broadcast from LDS (four chains)
__device__ __forceinline__ double brr_apply_row(const double (&w)[BB], const double* rt) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int s = 0; s < BB; s += 4) {
    const double2 r01 = *reinterpret_cast<const double2*>(rt + s);
    const double2 r23 = *reinterpret_cast<const double2*>(rt + s + 2);
    a0 = fma(w[s], r01.x, a0);
    a1 = fma(w[s + 1], r01.y, a1);
    a2 = fma(w[s + 2], r23.x, a2);
    a3 = fma(w[s + 3], r23.y, a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// One block of 64 markers: d⁰ = Σ_c partial_in[c] (fixed order), the block's single-site steps as
// δ = M r̃ (wave 0 of every workgroup, identical inputs → identical results; lane k's row of M in
// registers, r̃ broadcast from LDS), e += X_B δ on this workgroup's individuals, then the partials
// of the next block from the updated e. Workgroup 0 stores b and the running posterior mean.
// (fp64 storage only; the unnamed double keeps the argument layout of the kernel's byte form, pruned in round 4.)
__global__ void __launch_bounds__(256) brr_step_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t n,
                                                       int64_t p, double, const double* __restrict__ Mb, int64_t blk,
                                                       int64_t nblk, const double* __restrict__ partial_in,
                                                       double* __restrict__ partial_out, double* __restrict__ b,
                                                       double* __restrict__ bbar, const double* __restrict__ alpha,
                                                       const double* __restrict__ gamma, double* __restrict__ e,
                                                       const BrrState* __restrict__ st) {
  // next block's genotypes for this chunk of individuals: 64 rows x IW, row pitch 2064 B
  // (≡ 16 B mod 256 B: the ds_read_b128 lane groups of the partials loop are conflict-free)
  constexpr int RP = IW + 2;  // doubles
  __shared__ __attribute__((aligned(16))) double Xn[BB * RP];
  __shared__ double delta[BB];
  __shared__ __attribute__((aligned(16))) double rt[BB];
  __shared__ double es[IW];
  __shared__ double part4[4][BB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j0 = blk * BB;
  const int nb = (int)((p - j0) < BB ? (p - j0) : BB);
  const int C = (int)gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  const int64_t i = i0 + tid;
  const bool more = blk + 1 < nblk;
  const int64_t j1 = j0 + BB;
  const int nb1 = more ? (int)((p - j1) < BB ? (p - j1) : BB) : 0;
  // every load that does not depend on this block's δ goes out first:
  // (1) the next block's rows into LDS (global_load_lds: 1 KB per wave instruction)
  for (int q = wave; q < 2 * nb1; q += 4) {
    const int k = q >> 1, h = q & 1;
    const double* src = Xt + (j1 + k) * ldx + i0 + h * 128 + lane * 2;
    __builtin_amdgcn_global_load_lds((const void*)src, (void*)(Xn + k * RP + h * 128), 16, 0, 0);
  }
  // (2) this thread's 64 genotypes of the block, for e += X_B δ (rows past p clamped; δ = 0)
  double xv[BB];
#pragma unroll
  for (int s2 = 0; s2 < BB; s2++) xv[s2] = Xt[(j0 + (s2 < nb ? s2 : 0)) * ldx + i];
  const double e_old = e[i];
  // (3) wave 0's operands: its row of M, α, γ (padded arrays)
  double w[BB];
  double al = 0.0, ga = 0.0, bo = 0.0;
  const bool on = lane < nb;
  const int64_t j = j0 + lane;
  if (tid < 64) {
    const double* wr = Mb + (blk * BB + lane) * BB;
#pragma unroll
    for (int q = 0; q < BB; q += 2) {
      const double2 v = *reinterpret_cast<const double2*>(wr + q);
      w[q] = v.x;
      w[q + 1] = v.y;
    }
    al = alpha[j];
    ga = gamma[j];
    // b ping-pongs between two copies by iteration parity: a workgroup that starts late never
    // reads a value workgroup 0 already updated in this iteration (both copies load at once with
    // st: no st -> b dependent round trip)
    if (blockIdx.x == 0) {
      const double b0 = on ? b[j] : 0.0, b1 = on ? b[p + j] : 0.0;
      bo = (st->it & 1) ? b1 : b0;
    }
  }
  const double bb_old = (blockIdx.x == 0 && tid < 64 && on) ? bbar[j] : 0.0;
  {
    // r = Σ_c partial_in[c]: wave w sums c ≡ w (mod 4), 16 loads in flight per round, then a
    // fixed-order combine — every workgroup gets bit-identical r
    double a = 0.0;
    for (int c0 = wave; c0 < C; c0 += 64) {
      double v[16];
#pragma unroll
      for (int m = 0; m < 16; m++) v[m] = partial_in[min(c0 + 4 * m, C - 1) * BB + lane];  // unconditional loads
#pragma unroll
      for (int m = 0; m < 16; m++) a += c0 + 4 * m < C ? v[m] : 0.0;
    }
    part4[wave][lane] = a;
  }
  __syncthreads();
  if (tid < 64) {
    const double d = ((part4[0][lane] + part4[1][lane]) + part4[2][lane]) + part4[3][lane];
    rt[lane] = fma(d, -al, ga);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's r̃ is in LDS
    const double dlt = brr_apply_row(w, rt);
    const double bfin = bo - dlt;
    delta[lane] = dlt;
    if (blockIdx.x == 0 && on) {
      b[((st->it & 1) ^ 1) * p + j] = bfin;
      if (brr_accumulate(st)) {
        const double k = (double)(st->nsum + 1);
        bbar[j] = bb_old * ((k - 1.0) / k) + bfin / k;
      }
    }
  }
  __syncthreads();
  double ei = 0.0;
  if (i < n) {
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int s2 = 0; s2 < BB; s2 += 2) {
      acc0 = fma(delta[s2], xv[s2], acc0);
      acc1 = fma(delta[s2 + 1], xv[s2 + 1], acc1);
    }
    ei = e_old + (acc0 + acc1);
    e[i] = ei;
  }
  if (more) {
    es[tid] = ei;
    __syncthreads();  // also completes the global_load_lds of Xn
    // partial[c][k] = Σ_u Xn[k][w*64 + u] es[w*64 + u]: lane k = marker, wave w = quarter
    double s0 = 0.0, s1 = 0.0;
    if (lane < nb1) {
      const double* er = es + wave * 64;
      const double* xr = Xn + lane * RP + wave * 64;
#pragma unroll
      for (int u = 0; u < 64; u += 2) {
        const double2 xv2 = *reinterpret_cast<const double2*>(xr + u);
        s0 = fma(xv2.x, er[u], s0);
        s1 = fma(xv2.y, er[u + 1], s1);
      }
    }
    part4[wave][lane] = s0 + s1;
    __syncthreads();
    if (tid < 64)
      partial_out[blockIdx.x * BB + lane] = ((part4[0][lane] + part4[1][lane]) + part4[2][lane]) + part4[3][lane];
  }
}

// ---- byte storage: 128-marker launches ------------------------------------------------------
// With genotypes stored as bytes (x = d·xs exact), one launch runs 128 markers as two halves
// A = [j0, j0 + 64) and B = [j0 + 64, j0 + 128): wave 3 forms r̃ of both halves from the partial
// dots, then waves 0-2 apply δ_A = M_A r̃_A and δ_B = M_B r̃_B + O r̃_A (brr_prep_kernel) at once.
// Half the dependent launches per iteration of the 64-marker kernel, same sample path (markers
// in order).

// Dt[b][i][s] = D[(128 b + s) ldx + i] (0 for markers past p): the e update reads its 128
// genotypes of block b as 128 contiguous bytes per individual (coalesced b128 loads).
__global__ void __launch_bounds__(256) brr_block_transpose_kernel(const uint8_t* __restrict__ D, int64_t ldx,
                                                                  int64_t p, uint8_t* __restrict__ Dt) {
  __shared__ uint8_t T[BK2][65];
  const int64_t b = blockIdx.y, i0 = (int64_t)blockIdx.x * 64;
  const int tid = threadIdx.x;
  for (int e = tid; e < BK2 * 64; e += 256) {
    const int s = e >> 6, i = e & 63;
    const int64_t j = b * BK2 + s;
    T[s][i] = j < p ? D[j * ldx + i0 + i] : (uint8_t)0;
  }
  __syncthreads();
  for (int e = tid; e < BK2 * 64; e += 256) {
    const int i = e >> 7, s = e & 127;
    Dt[(b * ldx + i0 + i) * BK2 + s] = T[s][i];
  }
}

// partials of the 128 markers of block j0 (two rows per thread pair of passes), from es
__device__ __forceinline__ void brr_partials128(const uint8_t* __restrict__ D, int64_t ldx, int64_t i0, int64_t j0,
                                                int nb, double xs, const double* es, double* __restrict__ out) {
  const int tid = threadIdx.x, k = tid >> 2, qt = tid & 3;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int kk = k + 64 * h;
    double s = 0.0, s1 = 0.0;
    if (kk < nb) {
      const uint8_t* row = D + (j0 + kk) * ldx + i0 + qt * 64;
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const uint4*>(row + 16 * u);
      brr_dot64_u8(v, es + qt * 64, s, s1);
      s = s * xs + s1 * xs;
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (qt == 0) out[blockIdx.x * BK2 + 2 * k + h] = s;  // interleaved halves; kk >= nb writes 0
  }
}

__global__ void __launch_bounds__(256) brr_dots0_128_kernel(const uint8_t* __restrict__ D, int64_t ldx, int64_t n,
                                                            int64_t p, double xs, const double* __restrict__ e,
                                                            double* __restrict__ partial) {
  __shared__ double es[IW];
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  es[threadIdx.x] = i0 + threadIdx.x < n ? e[i0 + threadIdx.x] : 0.0;
  __syncthreads();
  brr_partials128(D, ldx, i0, 0, (int)(p < BK2 ? p : BK2), xs, es, partial);
}

__global__ void __launch_bounds__(256) brr_step128_kernel(const uint8_t* __restrict__ D, const uint8_t* __restrict__ Dt,
                                                          int64_t ldx, int64_t n, int64_t p, double xs,
                                                          const double* __restrict__ Mb, int64_t blk, int64_t nblk,
                                                          const double* __restrict__ partial_in,
                                                          double* __restrict__ partial_out, double* __restrict__ b,
                                                          double* __restrict__ bbar, const double* __restrict__ alpha,
                                                          const double* __restrict__ gamma, double* __restrict__ e,
                                                          const BrrState* __restrict__ st) {
  __shared__ __attribute__((aligned(16))) uint8_t Xb[BK2 * IW];  // next block's rows (swizzled 16-B chunks)
  __shared__ __attribute__((aligned(16))) double rt[BK2];        // r̃ = γ − α∘d⁰ of the block's markers
  __shared__ double dA[BB], dU[BB], dV[BB];                      // δ_A, M_B r̃_B, O r̃_A (δ_B = dU + dV)
  __shared__ double es[IW];
  __shared__ double part4[4][BK2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j0 = blk * BK2;
  const int C = (int)gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  const int64_t i = i0 + tid;
  const bool more = blk + 1 < nblk;
  const int64_t j1 = j0 + BK2;
  const int nb1 = more ? (int)((p - j1) < BK2 ? (p - j1) : BK2) : 0;
  const double* Mblk = Mb + blk * 3 * BB * BB;
  // Loads are issued in the order they are needed: vmcnt retires in order, so a load queued behind
  // the next block's rows would wait for them.
  // (1) the critical ones: wave 3 sums the partial dots of both halves over the C chunks (in chunk
  // order: bit-identical in every workgroup) and forms r̃; waves 0-2 load their rows of M_A, M_B, O
  double w[BB];
  double bo = 0.0, bbo = 0.0;
  const int64_t jm = j0 + (wave == 1 ? BB : 0) + lane;  // wave 0: marker A_lane, wave 1: B_lane
  const bool on = jm < p;
  if (wave == 3) {
    // partials are stored interleaved (A_k, B_k adjacent): one 16-B load per chunk
    const double2* pin = reinterpret_cast<const double2*>(partial_in) + lane;
    const double alA = alpha[j0 + lane], alBv = alpha[j0 + BB + lane];
    const double gaA = gamma[j0 + lane], gaB = gamma[j0 + BB + lane];
    double rA = 0.0, rB = 0.0;
    // one batch of loads in flight (C <= 48 up to n = 12 288), issued unconditionally (clamped
    // index): a branch or loop between them makes the compiler wait on earlier loads
    auto batch = [&](int c0) {
      double2 v[48];
#pragma unroll
      for (int m = 0; m < 48; m++) v[m] = pin[(int64_t)min(c0 + m, C - 1) * BB];
#pragma unroll
      for (int m = 0; m < 48; m++) {
        rA += c0 + m < C ? v[m].x : 0.0;
        rB += c0 + m < C ? v[m].y : 0.0;
      }
    };
    if (C <= 48) {
      batch(0);
    } else {
      for (int c0 = 0; c0 < C; c0 += 48) batch(c0);
    }
    rt[lane] = fma(rA, -alA, gaA);
    rt[BB + lane] = fma(rB, -alBv, gaB);
  } else {
    const double* wr = Mblk + (wave == 0 ? 0 : wave == 1 ? 2 * BB * BB : BB * BB) + lane * BB;
#pragma unroll
    for (int q = 0; q < BB; q += 2) {
      const double2 v = *reinterpret_cast<const double2*>(wr + q);
      w[q] = v.x;
      w[q + 1] = v.y;
    }
    // WG 0 stores b and keeps the running means: both parity copies of b and the old means load
    // now, not after the GEMVs
    if (blockIdx.x == 0 && wave < 2) {
      const int64_t jc = on ? jm : 0;  // unconditional loads (no branch between them)
      const double b0 = b[jc], b1 = b[p + jc];
      bbo = bbar[jc];
      bo = (st->it & 1) ? b1 : b0;
    }
  }
  // (2) needed later: this individual's 128 genotypes of the block (8 x 16 B) for e += X_B δ,
  // and the next block's rows into LDS (4 rows per wave instruction, row r's 16-byte chunk c at
  // position c ^ (r & 15); rows past the block re-read row nb1 − 1, never summed). The DMA is
  // inline asm: with the builtin the compiler would wait for it before every LDS read.
  uint4 xv[8];
  {
    const uint4* src = reinterpret_cast<const uint4*>(Dt + (blk * ldx + i) * BK2);
#pragma unroll
    for (int u = 0; u < 8; u++) xv[u] = src[u];
  }
  const double e_old = e[i];
  for (int q = wave; q < (nb1 + 3) / 4; q += 4) {
    const int r = 4 * q + (lane >> 4), c = lane & 15;
    const uint8_t* src = D + (j1 + (r < nb1 ? r : nb1 - 1)) * ldx + i0 + ((c ^ (r & 15)) * 16);
    const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(Xb + q * 4 * IW));
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(m0v), "v"(src) : "memory");
  }
  lds_barrier();
  // (3) the block's steps as three GEMVs: δ_A = M_A r̃_A (wave 0), M_B r̃_B (wave 1), O r̃_A (wave 2)
  if (wave < 3) {
    const double v = brr_apply_row(w, rt + (wave == 1 ? BB : 0));
    (wave == 0 ? dA : wave == 1 ? dU : dV)[lane] = v;
  }
  lds_barrier();
  // (4) workgroup 0 stores b and the running means
  if (blockIdx.x == 0 && wave < 2 && on) {
    const double dlt = wave == 0 ? dA[lane] : dU[lane] + dV[lane];
    const double bn = bo - dlt;
    b[((st->it & 1) ^ 1) * p + jm] = bn;
    if (brr_accumulate(st)) {
      const double k = (double)(st->nsum + 1);
      bbar[jm] = bbo * ((k - 1.0) / k) + bn / k;
    }
  }
  // (5) e += X_B δ over this workgroup's individuals (markers past p have δ = 0), four chains
  double ei = 0.0;
  if (i < n) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const uint32_t wd[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int bb = 0; bb < 4; bb++) {
          const int s = 16 * u + 4 * q + bb;
          const double dl = s < BB ? dA[s] : dU[s - BB] + dV[s - BB];
          acc[bb] = fma(dl, (double)((wd[q] >> (8 * bb)) & 0xFFu), acc[bb]);
        }
    }
    ei = e_old + ((acc[0] + acc[1]) + (acc[2] + acc[3])) * xs;
    e[i] = ei;
  }
  // (6) the next block's partial dots from the updated e
  if (more) {
    es[tid] = ei;
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0): this wave's rows of Xb have landed
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = lane + BB * h;
      double s0 = 0.0, s1 = 0.0;
      if (k < nb1) {
        const uint8_t* xr = Xb + k * IW;
        uint4 v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = *reinterpret_cast<const uint4*>(xr + (((4 * wave + t) ^ (k & 15)) * 16));
        brr_dot64_u8(v, es + wave * 64, s0, s1);
      }
      part4[wave][k] = s0 * xs + s1 * xs;
    }
    lds_barrier();
    if (tid < BK2)
      partial_out[blockIdx.x * BK2 + 2 * (tid & 63) + (tid >> 6)] =
          ((part4[0][tid] + part4[1][tid]) + part4[2][tid]) + part4[3][tid];
  }
}

// σ²_b, σ²_e draws, running means of μ and the variances, next iteration (one workgroup)
__global__ void __launch_bounds__(1024) brr_var_kernel(const double* __restrict__ b, int64_t p,
                                                       const double* __restrict__ e, int64_t n,
                                                       BrrState* __restrict__ st) {
  __shared__ double red[16];
  double sb = 0.0, se = 0.0;
  const double* bn = b + ((st->it & 1) ^ 1) * p;  // this iteration's samples
  // eight loads in flight per thread (one 1024-thread workgroup: latency, not bandwidth, bound)
  {
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t j = threadIdx.x;
    for (; j + 7 * 1024 < p; j += 8 * 1024)
#pragma unroll
      for (int u = 0; u < 8; u++) a[u] = fma(bn[j + u * 1024], bn[j + u * 1024], a[u]);
    for (; j < p; j += 1024) a[0] = fma(bn[j], bn[j], a[0]);
    sb = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    double c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t i = threadIdx.x;
    for (; i + 7 * 1024 < n; i += 8 * 1024)
#pragma unroll
      for (int u = 0; u < 8; u++) c[u] = fma(e[i + u * 1024], e[i + u * 1024], c[u]);
    for (; i < n; i += 1024) c[0] = fma(e[i], e[i], c[0]);
    se = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
  }
  sb = brr_block_sum<1024>(sb, red);
  se = brr_block_sum<1024>(se, red);
  if (threadIdx.x == 0) {
    const uint64_t a = 4 * (uint64_t)st->it;
    st->varB = (sb + st->S0b) / brr_chisq(st->seed, a + 1, st->df0b + (double)p);
    st->varE = (se + st->S0e) / brr_chisq(st->seed, a + 2, st->df0e + (double)n);
    if (brr_accumulate(st)) {
      const double k = (double)(st->nsum + 1);
      st->mubar = st->mubar * ((k - 1.0) / k) + st->mu / k;
      st->varEbar = st->varEbar * ((k - 1.0) / k) + st->varE / k;
      st->varBbar = st->varBbar * ((k - 1.0) / k) + st->varB / k;
      st->nsum += 1;
    }
    st->it += 1;
  }
}

}  // namespace
}  // namespace gbm

using namespace gbm;

// Timing tool (GBM_BRR_TRACE=1): per super-block timestamps of every workgroup of a traced fit's
// sweep (C x nsb x 8 int64, s_memrealtime at 100 MHz), recorded into the leasing context's own
// buffer and copied to the host when that fit completes; gbm_debug_brr_trace reads the copy of the
// last traced fit (no device buffer is shared between concurrent fits).
static std::mutex g_brr_trace_mu;
static std::vector<int64_t> g_brr_trace_host;

extern "C" int64_t gbm_debug_brr_trace(int64_t* host, int64_t cap) {
  std::lock_guard<std::mutex> lock(g_brr_trace_mu);
  if (!host || g_brr_trace_host.empty()) return 0;
  const int64_t n = std::min<int64_t>((int64_t)g_brr_trace_host.size(), cap);
  std::copy(g_brr_trace_host.begin(), g_brr_trace_host.begin() + n, host);
  return n;
}

// Which schedule the last completed fit took (0 per-launch, 4 the super-block sweep; 1-3 were the
// earlier sweeps of rounds 2-3, no longer built) and how many fits fell back to the per-launch path
// after a sweep hand-off timed out (tests).
static std::atomic<int> g_brr_last_path{-1};
static std::atomic<int64_t> g_brr_fallbacks{0};
extern "C" int gbm_debug_brr_stats(int* last_path, int64_t* fallbacks) {
  if (last_path) *last_path = g_brr_last_path.load();
  if (fallbacks) *fallbacks = g_brr_fallbacks.load();
  return GBM_OK;
}
// chunk shape of the last super-block sweep (C workgroups, O owners of R rows, Ko / Kn individuals)
static std::atomic<int64_t> g_brr_shape{0};
extern "C" int gbm_debug_brr_shape(int* C, int* O, int* R, int* Ko, int* Kn) {
  const int64_t v = g_brr_shape.load();
  if (C) *C = (int)(v & 0xFFF);
  if (O) *O = (int)((v >> 12) & 0xFFF);
  if (R) *R = (int)((v >> 24) & 0xFF);
  if (Ko) *Ko = (int)((v >> 32) & 0xFFF);
  if (Kn) *Kn = (int)((v >> 44) & 0xFFF);
  return 0;
}

// One BRR fit on a leased context; sweep_mode: -1 = per GBM_BRR_SWEEP (default on), 0 = off.
static int brr_fit_impl(const double* X, int64_t n, int64_t p, int64_t ldx, const double* y, int64_t n_iter,
                        int64_t n_burnin, int64_t thin, double r2, double df0, uint64_t seed, int dev,
                        int sweep_mode, double* b_hat_out, double* y_pred_out, double* var_out, bool* sweep_timeout) {
  *sweep_timeout = false;
  BrrLease lease;
  GBM_TRY(CtxPool<BrrCtx>::instance().acquire(dev, lease.c));
  BrrCtx& cx = *lease.c;
  GBM_HIP_TRY(hipSetDevice(dev));
  hipStream_t s = cx.stream.s;
  GBM_TRY(ensure(cx.stm, dev, sizeof(BrrState)));
  GibbsData g;
  GBM_TRY(gibbs_upload(cx, X, n, p, ldx, g));
  const int64_t npad = g.npad;
  const double xs = g.xs;
  // byte storage on (up to) every CU: the super-block sweep where brr_sweep_plan admits the shape
  int cus = 0;
  GBM_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  SweepPlan pl;
  if (xs > 0.0 && sweep_mode != 0) GBM_TRY(brr_sweep_plan(n, cus, pl));
  const bool sweep = pl.on;
  // markers per launch: 128 with byte storage (two halves), 64 with fp64 storage; the Gram blocks
  // each launch needs (brr_gram_kernel), and the block-transposed bytes of the byte path. The
  // super-block sweep rounds the 128-blocks up to whole super-blocks (α = γ = 0 past p).
  const int64_t bk = xs > 0.0 ? BK2 : BB;
  const int64_t nsb = (p + SBK - 1) / SBK;
  const int64_t nblk = sweep ? nsb * SBN : (p + bk - 1) / bk;
  const int nw = xs > 0.0 ? 3 : 1;
  // per-iteration block inverses (same shape as W) and step constants α, γ (padded to whole launches)
  GBM_TRY(ensure(cx.Mb, dev, nblk * nw * BB * BB * 8));
  GBM_TRY(ensure(cx.alph, dev, nblk * bk * 8));
  GBM_TRY(ensure(cx.gamm, dev, nblk * bk * 8));
  GBM_TRY(gibbs_gram(cx, n, p, npad, nblk, nw));
  const bool traced = sweep && knob("GBM_BRR_TRACE") != nullptr;
  const int64_t trace_n = traced ? (int64_t)pl.C * nsb * 8 : 0;
  if (sweep) GBM_TRY(brr_sweep_setup(cx, pl, n, p, npad, nsb, trace_n));
  if (xs > 0.0 && !sweep) {  // the per-launch path's individual-major copy of the bytes
    GBM_TRY(ensure(cx.Dt, dev, nblk * npad * BK2));
    brr_block_transpose_kernel<<<dim3((unsigned)(npad / 64), (unsigned)nblk), 256, 0, s>>>((const uint8_t*)cx.D.p, npad,
                                                                                            p, (uint8_t*)cx.Dt.p);
    GBM_LAUNCH_CHECK();
  }
  GBM_HIP_TRY(hipStreamSynchronize(s));
  GibbsPrior pr;
  GBM_TRY(gibbs_prior("gbm_brr_fit", y, n, p, g, pr));
  BrrState st0{};
  st0.mu = pr.ym;
  st0.S0e = pr.vy * (1.0 - r2) * (df0 + 2.0);
  st0.S0b = pr.vy * r2 / pr.msx * (df0 + 2.0);
  st0.df0e = df0;
  st0.df0b = df0;
  st0.varE = st0.S0e / (df0 + 2.0);
  st0.varB = st0.S0b / (df0 + 2.0);
  st0.burnin = n_burnin;
  st0.thin = thin;
  st0.seed = seed;
  static std::atomic<uint64_t> fit_epoch{1};
  st0.epoch = fit_epoch.fetch_add(1, std::memory_order_relaxed);
  GBM_HIP_TRY(hipMemcpyAsync(cx.e.p, pr.e0.data(), npad * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.b.p, 0, 2 * p * 8, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.bbar.p, 0, p * 8, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.stm.p, &st0, sizeof(BrrState), hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  // one Gibbs iteration
  auto* stp = (BrrState*)cx.stm.p;
  const unsigned C = (unsigned)g.C64;
  const unsigned prep_grid = (unsigned)(xs > 0.0 ? nblk : (nblk + 3) / 4);
  int64_t* trace_dev = traced ? (int64_t*)cx.trace.p : nullptr;
  auto enqueue_iteration = [&]() -> int {
    brr_prep_kernel<<<prep_grid, 256, 0, s>>>((const double*)cx.W.p, p, nblk, nw, (const double*)cx.x2.p,
                                              (const double*)cx.b.p, stp, (double*)cx.Mb.p, (double*)cx.alph.p,
                                              (double*)cx.gamm.p, sweep ? (double*)cx.MS.p : nullptr);
    brr_mu_kernel<<<1, 1024, 0, s>>>((double*)cx.e.p, n, stp);
    if (sweep) {
      brr_sweep_enqueue(cx, pl, n, p, npad, nsb, xs, trace_dev);
    } else {
      if (xs > 0.0)
        brr_dots0_128_kernel<<<C, 256, 0, s>>>((const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.e.p,
                                               (double*)cx.r.p);
      else
        gibbs_dots0(cx, n, p, g, false);
      for (int64_t k = 0; k < nblk; k++) {
        double* pin = (double*)cx.r.p + (k & 1) * (int64_t)C * bk;
        double* pout = (double*)cx.r.p + ((k + 1) & 1) * (int64_t)C * bk;
        if (xs > 0.0)
          brr_step128_kernel<<<C, 256, 0, s>>>((const uint8_t*)cx.D.p, (const uint8_t*)cx.Dt.p, npad, n, p, xs,
                                               (const double*)cx.Mb.p, k, nblk, pin, pout, (double*)cx.b.p,
                                               (double*)cx.bbar.p, (const double*)cx.alph.p, (const double*)cx.gamm.p,
                                               (double*)cx.e.p, stp);
        else
          brr_step_kernel<<<C, 256, 0, s>>>((const double*)cx.Xt.p, npad, n, p, 1.0, (const double*)cx.Mb.p, k, nblk, pin,
                                            pout, (double*)cx.b.p, (double*)cx.bbar.p, (const double*)cx.alph.p,
                                            (const double*)cx.gamm.p, (double*)cx.e.p, stp);
      }
    }
    brr_var_kernel<<<1, 1024, 0, s>>>((const double*)cx.b.p, p, (const double*)cx.e.p, n, stp);
    return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, "gbm_brr_fit: launch failed");
  };
  // captured once and replayed (kept with the context while the shape and the buffers are the same)
  cx.brr_graph.ensure({n, p, npad, (int64_t)(xs * 64.0), sweep ? 1 : 0, key_of(cx.Xt), key_of(cx.D), key_of(cx.Dt),
                       key_of(cx.W), key_of(cx.Mb), key_of(cx.r), key_of(cx.e), key_of(cx.b), key_of(cx.bbar),
                       key_of(cx.alph), key_of(cx.gamm), key_of(cx.x2), key_of(cx.stm), pl.K, pl.Cu, pl.Ru, pl.Ko, pl.O,
                       pl.Kn, pl.R, pl.C, key_of(cx.MS), key_of(cx.Wsb), key_of(cx.Ssc), key_of(cx.Pb), key_of(cx.Rt),
                       key_of(cx.Dl), key_of(cx.sbcnt), (int64_t)(uintptr_t)trace_dev, key_of(cx.CS), key_of(cx.CS2)},
                      s, enqueue_iteration);
  {
    std::unique_lock<std::mutex> sweep_guard;
    if (sweep) sweep_guard = std::unique_lock<std::mutex>(brr_sweep_lock(dev));
    GBM_TRY(cx.brr_graph.run(n_iter, s, "gbm_brr_fit", enqueue_iteration));
  }
  if (sweep) {
    int32_t inf = 0;
    GBM_HIP_TRY(hipMemcpyAsync(&inf, brr_sweep_error_cell(cx), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
    if (knob("GBM_BRR_TEST_SWEEP_TIMEOUT")) inf = -1;  // tests: the fall-back's reporting, no device timeout
    if (inf < 0) {
      *sweep_timeout = true;
      return fail(GBM_E_HIP, "gbm_brr_fit: a sweep hand-off between workgroups timed out");
    }
    if (traced) {
      std::vector<int64_t> tr((size_t)trace_n);
      GBM_HIP_TRY(hipMemcpy(tr.data(), cx.trace.p, (size_t)trace_n * 8, hipMemcpyDeviceToHost));
      std::lock_guard<std::mutex> lock(g_brr_trace_mu);
      g_brr_trace_host.swap(tr);
    }
  }
  g_brr_last_path.store(sweep ? 4 : 0);
  if (sweep)
    g_brr_shape.store((int64_t)pl.C | ((int64_t)pl.O << 12) | ((int64_t)pl.R << 24) | ((int64_t)pl.Ko << 32) |
                      ((int64_t)pl.Kn << 44));
  BrrState fin{};
  GBM_TRY(gibbs_outputs(cx, n, p, npad, cx.stm, &fin, sizeof(fin), &fin.mubar, b_hat_out, nullptr, y_pred_out));
  if (var_out) {
    var_out[0] = fin.varEbar;
    var_out[1] = fin.varBbar;
  }
  return GBM_OK;
}

extern "C" int gbm_brr_fit(const double* X, int64_t n, int64_t p, int64_t ldx, const double* y, int64_t n_iter,
                           int64_t n_burnin, int64_t thin, double r2, double df0, uint64_t seed, int device,
                           double* b_hat_out, double* y_pred_out, double* var_out) {
  RoctxRange r_("gbm_brr_fit");
  set_error("");  // rc 0 with a non-empty gbm_last_error() reports a fall-back (below)
  int dev = 0;
  GBM_TRY(gibbs_check_args("gbm_brr_fit", X, y, b_hat_out, n, p, ldx, n_iter, n_burnin, thin, r2, df0));
  GBM_TRY(gibbs_check_run("gbm_brr_fit", y, n, n_iter, n_burnin, thin, device, dev));
  bool timeout = false;
  int rc = brr_fit_impl(X, n, p, ldx, y, n_iter, n_burnin, thin, r2, df0, seed, dev, -1, b_hat_out, y_pred_out,
                        var_out, &timeout);
  // a sweep whose workgroups could not all be resident (another process or library filling the
  // device) times out loudly on the device; the fit is then run again, from the start, on the
  // per-launch path (same chain; the two paths agree to rounding). The call still returns GBM_OK —
  // the results are valid — but says so: gbm_last_error() holds the warning (the Python mirror
  // raises a RuntimeWarning, the Julia binding an @warn) and gbm_debug_brr_stats counts it.
  if (rc != GBM_OK && timeout) {
    g_brr_fallbacks.fetch_add(1);
    rc = brr_fit_impl(X, n, p, ldx, y, n_iter, n_burnin, thin, r2, df0, seed, dev, 0, b_hat_out, y_pred_out, var_out,
                      &timeout);
    if (rc == GBM_OK)
      set_error("warning: gbm_brr_fit: the persistent super-block sweep timed out (were all its workgroups resident? "
                "another process may share the device); the fit was re-run on the per-launch path");
  }
  return rc;
}

