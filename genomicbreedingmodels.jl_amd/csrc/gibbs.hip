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
// With byte storage and n <= 48 x CUs the iteration is instead ONE persistent sweep launch over
// 512-marker super-blocks on up to every CU (brr_sweep_la2_kernel: see "super-block sweep" below);
// otherwise the per-block launches above run. (Rounds 2-3 also kept a 128-block sweep and two
// earlier super-block schedules; they are in git history, e.g. `git show 3599bea:<this file>`.)
//
// Random numbers: a counter-based hash of (seed, stream, counter) (no sampler state), Box-Muller
// normals and Marsaglia-Tsang gammas, restated bit-for-bit in oracle/oracle.py (brr_*), so the
// device chain and the oracle's un-blocked BGLR loop follow the same sample path.
//
// BayesA, BayesB and BayesC (gbm_bayes_fit, the models behind reference src/linear.jl:440-626) reuse
// the per-launch skeleton, but their indicator draw is not affine in x_kᵀe: a block's 64 steps run
// as a serial chain on the block's Gram matrix (bayes_chain_kernel, below brr_quantize_kernel).
#include <atomic>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "gbm_internal.h"
#include "host_util.h"

namespace gbm {
namespace {

constexpr int BB = 64;  // markers per block (one wave)
constexpr int SBK = 512;  // markers per super-block (the super-block sweep, below)
constexpr int SBN = SBK / (2 * BB);  // 128-marker sub-blocks per super-block

__device__ __forceinline__ uint64_t bmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double brr_u01(uint64_t seed, uint64_t a, uint64_t b) {
  const uint64_t h = bmix64(bmix64(seed ^ (a * 0xD1B54A32D192ED03ull)) ^ (b * 0x8CB92BA72F3D8DD7ull));
  return ((double)(h >> 11) + 0.5) * 0x1.0p-53;
}
__device__ __forceinline__ double brr_normal(uint64_t seed, uint64_t a, uint64_t b) {
  const double u1 = brr_u01(seed, a, 2 * b), u2 = brr_u01(seed, a, 2 * b + 1);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
// χ²(df) = 2 Gamma(df/2) by Marsaglia-Tsang (df/2 >= 1); attempt t uses normal (a, 2t) and
// uniform (a, 4t + 2)
__device__ double brr_chisq(uint64_t seed, uint64_t a, double df) {
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

struct BrrState {
  double mu, varE, varB, S0e, S0b, df0e, df0b;
  double mubar, varEbar, varBbar;
  int64_t it, burnin, thin, nsum;
  uint64_t seed;
  uint64_t epoch;  // distinct per fit: part of the super-block sweep's hand-off tags (pooled buffers)
};

__device__ __forceinline__ bool brr_accumulate(const BrrState* st) {
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

// column means and Σx² of every marker (one workgroup per marker row of Xt)
__global__ void __launch_bounds__(256) brr_colstats_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                           int64_t n, double* __restrict__ colmean,
                                                           double* __restrict__ x2) {
  __shared__ double red[4];
  for (int64_t j = blockIdx.x; j < p; j += gridDim.x) {
    const double* row = Xt + j * ldx;
    double s = 0.0, ss = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const double v = row[i];
      s += v;
      ss += v * v;
    }
    s = brr_block_sum<256>(s, red);
    ss = brr_block_sum<256>(ss, red);
    if (threadIdx.x == 0) {
      colmean[j] = s / (double)n;
      x2[j] = ss;
    }
  }
}

// Gram blocks, one 64x64 block per workgroup (row-major; rows/cols past p are zero), individuals
// in chunks of 64 staged through LDS; one-time setup. nw = 1: W[b] = X_BᵀX_B for the 64-marker
// blocks B = [64b, 64b + 64). nw = 3 (128-marker launches of the byte path, halves A and B of
// block b = [128b, 128b + 128)): W[3b] = X_AᵀX_A, W[3b + 1] = X_BᵀX_A (row k = marker B_k),
// W[3b + 2] = X_BᵀX_B.
__global__ void __launch_bounds__(256) brr_gram_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                       int64_t n, int nw, double* __restrict__ W) {
  __shared__ double TR[BB][BB + 1];
  __shared__ double TC[BB][BB + 1];
  const int64_t blk = blockIdx.x / nw;
  const int w = (int)(blockIdx.x % nw);
  const int64_t r0 = nw == 1 ? blk * BB : blk * 2 * BB + (w >= 1 ? BB : 0);
  const int64_t c0 = nw == 1 ? blk * BB : blk * 2 * BB + (w == 2 ? BB : 0);
  const int tid = threadIdx.x, a = tid >> 2, b0 = (tid & 3) * 16;
  double acc[16];
#pragma unroll
  for (int u = 0; u < 16; u++) acc[u] = 0.0;
  for (int64_t k0 = 0; k0 < n; k0 += BB) {
    for (int e = tid; e < BB * BB; e += 256) {
      const int r = e / BB, c = e % BB;
      TR[r][c] = (r0 + r < p && k0 + c < n) ? Xt[(r0 + r) * ldx + k0 + c] : 0.0;
      TC[r][c] = (c0 + r < p && k0 + c < n) ? Xt[(c0 + r) * ldx + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < BB; k++) {
      const double xa = TR[a][k];
#pragma unroll
      for (int u = 0; u < 16; u++) acc[u] += xa * TC[b0 + u][k];
    }
    __syncthreads();
  }
  double* out = W + (int64_t)blockIdx.x * BB * BB + a * BB + b0;
#pragma unroll
  for (int u = 0; u < 16; u++) out[u] = acc[u];
}

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

constexpr int IW = 256;  // individuals per workgroup in the block kernels

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

// partials of block 0 at the start of an iteration (after the intercept update)
template <typename T>
__global__ void __launch_bounds__(256) brr_dots0_kernel(const T* __restrict__ Xt, int64_t ldx, int64_t n,
                                                        int64_t p, double xs, const double* __restrict__ e,
                                                        double* __restrict__ partial) {
  __shared__ double es[IW];
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  es[threadIdx.x] = i0 + threadIdx.x < n ? e[i0 + threadIdx.x] : 0.0;
  __syncthreads();
  brr_partials<T>(Xt, ldx, n, i0, 0, (int)(p < BB ? p : BB), xs, es, partial);
}

// One block of 64 markers: d⁰ = Σ_c partial_in[c] (fixed order), the block's single-site steps as
// δ = M r̃ (wave 0 of every workgroup, identical inputs → identical results; lane k's row of M in
// registers, r̃ broadcast from LDS), e += X_B δ on this workgroup's individuals, then the partials
// of the next block from the updated e. Workgroup 0 stores b and the running posterior mean.
template <typename T>
__global__ void __launch_bounds__(256) brr_step_kernel(const T* __restrict__ Xt, int64_t ldx, int64_t n,
                                                       int64_t p, double xs, const double* __restrict__ Mb, int64_t blk,
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
  uint8_t* Xb = reinterpret_cast<uint8_t*>(Xn);  // byte storage: rows of IW bytes, unpadded
  if constexpr (sizeof(T) == 8) {
    for (int q = wave; q < 2 * nb1; q += 4) {
      const int k = q >> 1, h = q & 1;
      const T* src = Xt + (j1 + k) * ldx + i0 + h * 128 + lane * 2;
      __builtin_amdgcn_global_load_lds((const void*)src, (void*)(Xn + k * RP + h * 128), 16, 0, 0);
    }
  } else {
    // 4 rows per wave instruction; row r's 16-byte chunk c is stored at position c ^ (r & 15)
    // (swizzled source address), so the partials loop's lanes (one row each) read distinct banks.
    // Rows past the block (last block) re-read row nb1 − 1: valid memory, never summed.
    for (int q = wave; q < (nb1 + 3) / 4; q += 4) {
      const int r = 4 * q + (lane >> 4), c = lane & 15;
      const T* src = Xt + (j1 + (r < nb1 ? r : nb1 - 1)) * ldx + i0 + ((c ^ (r & 15)) * 16);
      __builtin_amdgcn_global_load_lds((const void*)src, (void*)(Xb + q * 4 * IW), 16, 0, 0);
    }
  }
  // (2) this thread's 64 genotypes of the block, for e += X_B δ (rows past p clamped; δ = 0)
  double xv[BB];
#pragma unroll
  for (int s2 = 0; s2 < BB; s2++) xv[s2] = gval<T>(Xt[(j0 + (s2 < nb ? s2 : 0)) * ldx + i], xs);
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
      if constexpr (sizeof(T) == 8) {
        const double* xr = Xn + lane * RP + wave * 64;
#pragma unroll
        for (int u = 0; u < 64; u += 2) {
          const double2 xv2 = *reinterpret_cast<const double2*>(xr + u);
          s0 = fma(xv2.x, er[u], s0);
          s1 = fma(xv2.y, er[u + 1], s1);
        }
      } else {
        const uint8_t* xr = Xb + lane * IW;
        uint4 v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = *reinterpret_cast<const uint4*>(xr + (((4 * wave + t) ^ (lane & 15)) * 16));
        brr_dot64_u8(v, er, s0, s1);
        s0 *= xs;
        s1 *= xs;
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
constexpr int BK2 = 2 * BB;  // markers per launch

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

// Workgroup barrier that waits for this wave's LDS operations only (__syncthreads also waits for
// every outstanding global load, e.g. the next block's rows that are needed much later).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
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

// ---- hand-off helpers of the persistent sweep ---------------------------------------------------
// Buffer resource over a device array, for the `sc1` (write-through / L2-coherent) loads and stores
// of the sweep's inter-workgroup hand-offs (per-XCD L2s are not coherent).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brr_rsrc(const void* p, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

// ---- byte storage: super-block sweep over all CUs (round 3) ------------------------------------
// One 256-individual chunk per CU (⌈n/256⌉ = 40 CUs at C4) with a hand-off after every 128-marker
// block is bound by one CU's work per block and one hand-off per block. Instead the markers go in
// super-blocks of SBK = 512: the whole
// super-block's single-site steps are ONE affine map of its start dots,
//   δ_S = M_S (γ_S − α_S ∘ d⁰_S),  M_S = (I + D_S L_S)⁻¹  (unit lower, 512 x 512),
// built once per iteration by block forward substitution over the four 128-marker sub-blocks
// (brr_sb_prep_kernel, from brr_prep_kernel's 128-block inverses and the super-block's Gram
// blocks). The individuals are split into chunks of K (<= 64) over (up to) every CU. Per super-
// block, three hand-offs between all chunk workgroups:
//   1. every chunk publishes its partial dots X_{S,c}ᵀ e_c (512 values);
//   2. workgroup c sums the partials of its R owned rows of d⁰_S over all chunks (fixed order),
//      forms r̃ = γ − α∘d⁰ there and publishes those rows;
//   3. workgroup c computes its rows of δ_S = M_S r̃ from all of r̃, updates b and b̄ of those
//      markers and publishes its δ rows;
// then every chunk applies e += X_S δ_S to its individuals. Each hand-off is a set of self-
// validating granules (below: one write-through store per value, no flag, counter or drain).
// Granule slots alternate by super-block parity (a workgroup writes super-block s + 2's values only
// after every workgroup has passed s + 1's second hand-off, i.e. finished reading s's). Each
// genotype byte is read from HBM once per iteration: the super-block's rows of the chunk land in
// LDS by DMA (wave 3, during the previous super-block's hand-offs) and serve both the dots and the
// e update. Same chain as the literal BGLR loop, rounding aside. Waits are bounded (~1 s:
// *info = −1, every workgroup leaves; the host falls back).
static_assert(SBN * BK2 == SBK, "super-blocks are whole 128-marker blocks");
constexpr int SB_PAIRS = SBN * (SBN - 1) / 2;
constexpr int SB_RMAX = 8;             // owned rows per workgroup (at most)

__device__ __forceinline__ int sb_pair_index(int i, int m) { return i * (i - 1) / 2 + m; }  // i > m

// Wsb[s][pair(i, m)] = X_{4s+i}ᵀ X_{4s+m} over the 128-marker sub-blocks i > m of super-block s
// (128 x 128 row-major; rows/columns past p are zero): one 64x64 quadrant per workgroup, as
// brr_gram_kernel. One-time setup.
__global__ void __launch_bounds__(256) brr_gram_sb_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                          int64_t n, double* __restrict__ Wsb) {
  __shared__ double TR[BB][BB + 1];
  __shared__ double TC[BB][BB + 1];
  const int quad = (int)(blockIdx.x & 3);
  const int64_t sp = blockIdx.x >> 2;
  const int64_t s = sp / SB_PAIRS;
  const int pair = (int)(sp % SB_PAIRS);
  int i = 1;
  while ((i + 1) * i / 2 <= pair) i++;
  const int m = pair - i * (i - 1) / 2;
  const int64_t r0 = s * SBK + i * BK2 + (quad >> 1) * BB, c0 = s * SBK + m * BK2 + (quad & 1) * BB;
  const int tid = threadIdx.x, a = tid >> 2, b0 = (tid & 3) * 16;
  double acc[16];
#pragma unroll
  for (int u = 0; u < 16; u++) acc[u] = 0.0;
  for (int64_t k0 = 0; k0 < n; k0 += BB) {
    for (int e = tid; e < BB * BB; e += 256) {
      const int r = e / BB, c = e % BB;
      TR[r][c] = (r0 + r < p && k0 + c < n) ? Xt[(r0 + r) * ldx + k0 + c] : 0.0;
      TC[r][c] = (c0 + r < p && k0 + c < n) ? Xt[(c0 + r) * ldx + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < BB; k++) {
      const double xa = TR[a][k];
#pragma unroll
      for (int u = 0; u < 16; u++) acc[u] += xa * TC[b0 + u][k];
    }
    __syncthreads();
  }
  double* out = Wsb + sp * BK2 * BK2 + ((quad >> 1) * BB + a) * BK2 + (quad & 1) * BB + b0;
#pragma unroll
  for (int u = 0; u < 16; u++) out[u] = acc[u];
}

typedef double sbd4 __attribute__((ext_vector_type(4)));
typedef double sbd2 __attribute__((ext_vector_type(2)));

// acc (this wave's 64x64 quadrant wm, wn of a 128x128 product) += A · B over K = 128 on the fp64
// MFMA (A, B row-major with pitches lda, ldb). The operands go global -> LDS by DMA
// (global_load_lds, no registers) in eight 16-deep chunks, double-buffered: chunk c + 1 is in
// flight while chunk c's MFMAs run, and two workgroups share a CU, so one's loads, barriers and
// epilogue overlap the other's MFMAs. A lands row-major with its 16-byte pairs XOR-swizzled by row
// (pair p of row r at slot p ^ (r & 7)): a lane's MFMA A operand A[r][k] (r = 16 rows, k = 4 deep)
// is then a near conflict-free LDS read. B lands row-major, one 1 KB row per wave instruction.
// acc[m][q][r] = C[64 wm + 16 m + fr + 4 r][64 wn + 16 q + fc].
constexpr int SBP = BK2 + 4;       // LDS pitch of B rows (doubles)
constexpr int GK = 16;             // k per chunk
constexpr int GA = BK2 * GK;       // A chunk (doubles)
constexpr int GBUF = GA + GK * SBP;  // one buffer: A chunk + B chunk
__device__ __forceinline__ void sb_gemm128(const double* __restrict__ A, int64_t lda, const double* __restrict__ B,
                                           int64_t ldb, double* lds, sbd4 (&acc)[4][4], int lane, int wave, int wm,
                                           int wn, int fr, int fc) {
  auto stage = [&](int c, int bf) {
    const int k0 = c * GK;
    double* base = lds + bf * GBUF;
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
      const int j = wave * 4 + jj;  // A: 16 instructions of 64 16-byte slots
      const int slot = j * 64 + lane, r = slot >> 3, p = (slot & 7) ^ (r & 7);
      __builtin_amdgcn_global_load_lds((const void*)(A + (int64_t)r * lda + k0 + 2 * p), (void*)(base + j * 128), 16, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
      const int k = wave * 4 + jj;  // B: one row per instruction
      __builtin_amdgcn_global_load_lds((const void*)(B + (int64_t)(k0 + k) * ldb + 2 * lane), (void*)(base + GA + k * SBP),
                                       16, 0, 0);
    }
  };
  stage(0, 0);
#pragma unroll 1
  for (int c = 0; c < BK2 / GK; c++) {
    if (c + 1 < BK2 / GK) {
      stage(c + 1, (c + 1) & 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // chunk c's eight DMAs of this wave have landed
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();  // ... and every wave's
    const double* As = lds + (c & 1) * GBUF;
    const double* Bs = As + GA;
#pragma unroll
    for (int ks = 0; ks < GK; ks += 4) {
      double a[4], b[4];
      const int k = ks + fr;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int r = wm * 64 + u * 16 + fc;
        a[u] = As[(r * 8 + ((k >> 1) ^ (r & 7))) * 2 + (k & 1)];
        b[u] = Bs[k * SBP + wn * 64 + u * 16 + fc];
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mm = 0; mm < 4; mm++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[mm][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mm], b[q], acc[mm][q], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();  // buffer c & 1 is free for chunk c + 2
  }
}

// M_S of every super-block (row-major SBK x SBK; blocks above the diagonal stay zero from the
// setup memset): the inverse of the unit lower triangular I + D L over its four 128-marker sub-blocks
// (D = diag(α), L = the strictly lower part of the super-block's Gram), from the diagonal blocks
//   M_ii = [[M_A, 0], [O, M_B]]   (brr_prep_kernel writes them into M_S) and
//   M_ij = −M_ii D_i Σ_{m=j}^{i−1} W_im M_mj  (i > j),
// by recursive doubling in three launches (each workgroup one 128x128 output block; the blocks a
// level reads were written by an earlier launch or, level 0, by the same workgroup):
//   level 0: X_{a+1,a} = D_{a+1} W_{a+1,a} M_aa, then M_{a+1,a} = −M_{a+1,a+1} X_{a+1,a} (a = 0, 2);
//   level 2: X_ij = D_i Σ_{m=j}^{1} W_im M_mj (i = 2, 3; j = 0, 1);
//   level 3: M_ij = −Σ_{m=2}^{i} M_im X_mj.
// X lives in the scratch Xsc: 6 blocks per super-block, slot(i, j) = {10: 0, 32: 1, 20: 2, 21: 3,
// 30: 4, 31: 5}. Two workgroups per CU (67 KB of LDS each).
__device__ __forceinline__ int sb_xslot(int i, int j) {
  return i == 1 ? 0 : i == 2 ? (j == 0 ? 2 : 3) : (j == 2 ? 1 : j == 0 ? 4 : 5);
}
__global__ void __launch_bounds__(256, 2) brr_sb_prep_kernel(int level, const double* __restrict__ Wsb,
                                                             const double* __restrict__ alpha, double* __restrict__ MS,
                                                             double* __restrict__ Xsc) {
  __shared__ __attribute__((aligned(16))) double lds[2 * GBUF];
  const int ntask = level == 0 ? 2 : 4;
  const int64_t s = blockIdx.x / ntask;
  const int task = (int)(blockIdx.x % ntask);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane >> 4, fc = lane & 15;
  double* Ms = MS + s * (int64_t)SBK * SBK;
  double* X = Xsc + s * 6 * (int64_t)BK2 * BK2;
  auto Wb = [&](int i, int m) { return Wsb + (s * SB_PAIRS + sb_pair_index(i, m)) * (int64_t)BK2 * BK2; };
  auto Mblk = [&](int i, int j) { return Ms + (int64_t)(i * BK2) * SBK + j * BK2; };
  auto Xblk = [&](int i, int j) { return X + sb_xslot(i, j) * (int64_t)BK2 * BK2; };
  // epilogues: rows scaled by α of sub-block i (into X), or negated (into M_S)
  auto store_scaled = [&](const sbd4 (&acc)[4][4], double* out, int64_t ld, int i) {
    const double* al = alpha + (s * SBN + i) * BK2;
#pragma unroll
    for (int mm = 0; mm < 4; mm++)
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = wm * 64 + mm * 16 + fr + 4 * r;
          out[(int64_t)row * ld + wn * 64 + q * 16 + fc] = acc[mm][q][r] * al[row];
        }
  };
  auto store_neg = [&](const sbd4 (&acc)[4][4], double* out, int64_t ld) {
#pragma unroll
    for (int mm = 0; mm < 4; mm++)
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          out[(int64_t)(wm * 64 + mm * 16 + fr + 4 * r) * ld + wn * 64 + q * 16 + fc] = -acc[mm][q][r];
  };
  sbd4 acc[4][4];
  auto zero = [&]() {
#pragma unroll
    for (int mm = 0; mm < 4; mm++)
#pragma unroll
      for (int q = 0; q < 4; q++) acc[mm][q] = (sbd4){0.0, 0.0, 0.0, 0.0};
  };
  zero();
  if (level == 0) {
    const int a = 2 * task;
    sb_gemm128(Wb(a + 1, a), BK2, Mblk(a, a), SBK, lds, acc, lane, wave, wm, wn, fr, fc);
    store_scaled(acc, Xblk(a + 1, a), BK2, a + 1);
    __threadfence_block();
    __syncthreads();  // X_{a+1,a} (this workgroup's stores) before it is read back as B
    zero();
    sb_gemm128(Mblk(a + 1, a + 1), SBK, Xblk(a + 1, a), BK2, lds, acc, lane, wave, wm, wn, fr, fc);
    store_neg(acc, Mblk(a + 1, a), SBK);
  } else if (level == 2) {
    const int i = 2 + task / 2, j = task % 2;
    for (int m = j; m <= 1; m++) sb_gemm128(Wb(i, m), BK2, Mblk(m, j), SBK, lds, acc, lane, wave, wm, wn, fr, fc);
    store_scaled(acc, Xblk(i, j), BK2, i);
  } else {
    const int i = 2 + task / 2, j = task % 2;
    for (int m = 2; m <= i; m++) sb_gemm128(Mblk(i, m), SBK, Xblk(m, j), BK2, lds, acc, lane, wave, wm, wn, fr, fc);
    store_neg(acc, Mblk(i, j), SBK);
  }
}

// Hand-off granules of the super-block sweep: 16 bytes {v, bits(v) XOR key(tag)} written by one
// write-through (sc1) store; a reader polls the granule with sc1 loads until the second half
// matches the first for the tag it expects (tag = iteration · nsb + super-block: never reused), so
// no flag, counter or drain is needed, and a torn or stale read can only fail the check and be
// read again.
typedef unsigned int sbu4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint64_t sb_key(uint64_t tag) { return bmix64(tag * 0x9E3779B97F4A7C15ull + 0x5DEECE66Dull); }
__device__ __forceinline__ void sb_put(__amdgpu_buffer_rsrc_t r, uint32_t off, double v, uint64_t key) {
  const uint64_t a = __builtin_bit_cast(uint64_t, v), b = a ^ key;
  const sbu4 w = {(unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)};
  __builtin_amdgcn_raw_buffer_store_b128(w, r, (int)off, 0, 16);  // sc1
}
// A poll is a compiler-visible load with cache policy sc1 (so the compiler counts it and waits just
// before the first use of its value; an inline-asm load made it wait for everything in flight). A
// poll loop starts each round with sb_fence(), so that the load is not hoisted out of the loop (as
// LLVM did with the builtin's "read-only" load before the fence). A poll must not sit under a
// divergent branch: the compiler may then copy its register at the merge before the data lands.
__device__ __forceinline__ sbu4 sb_getv(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16);
}
__device__ __forceinline__ void sb_fence() { asm volatile("" ::: "memory"); }
// Sum over the wave, returned to every lane (wave-uniform): DPP within each row of 16 lanes (quad
// swaps, half-row and row mirrors), then the four row sums read into scalars. Latency of a few
// VALU ops per step instead of the LDS round trip of each __shfl_xor.
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, kCtrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), kCtrl, 0xF, 0xF, false);
  return __builtin_bit_cast(double, (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32));
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)u, l);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32));
}
__device__ __forceinline__ double wave_sum_f64(double x) {
  x += dpp_f64<0xB1>(x);   // quad_perm [1,0,3,2]
  x += dpp_f64<0x4E>(x);   // quad_perm [2,3,0,1]
  x += dpp_f64<0x141>(x);  // row_half_mirror
  x += dpp_f64<0x140>(x);  // row_mirror
  return (readlane_f64(x, 0) + readlane_f64(x, 16)) + (readlane_f64(x, 32) + readlane_f64(x, 48));
}
__device__ __forceinline__ bool sb_ok(const sbu4& w, uint64_t key, double& v) {
  const uint64_t a = (uint64_t)w.x | ((uint64_t)w.y << 32), b = (uint64_t)w.z | ((uint64_t)w.w << 32);
  v = __builtin_bit_cast(double, a);
  return (a ^ key) == b;
}
// poll bookkeeping of one wave: true while some lane still waits; gives up (*info = −1) after
// ~1 s or when another workgroup gave up
__device__ __forceinline__ bool sb_spin(bool lane_done, int64_t& spin, int32_t* info, bool& failed) {
  if (__builtin_amdgcn_ballot_w64(!lane_done) == 0) return false;
  if ((++spin & 255) == 255) {
    if (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0 || spin > ((int64_t)1 << 22)) {
      __hip_atomic_store(info, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      failed = true;
      return false;
    }
  }
  __builtin_amdgcn_s_sleep(1);
  return true;
}

// ---- byte storage: look-ahead super-block sweep (round 3) -----------------------------------------
// A plain super-block sweep would run three hand-offs per super-block in a row: partial dots ->
// owners, r̃ -> everyone, δ -> everyone, with the e update and the next dots between them. Here the
// dots leave the chain: with e⁽ˢ⁾ the residual after super-block s,
//   d⁰_s = X_sᵀ e⁽ˢ⁻¹⁾ = X_sᵀ e⁽ˢ⁻²⁾ + X_sᵀ X_{s−1} δ_{s−1} = Q_s + C_s δ_{s−1},
// so Q_s (partial dots over chunks of individuals, summed by the row owners) is computed from the
// residual one super-block earlier, and only the 512 x 512 cross-Gram C_s = X_sᵀ X_{s−1} (one-time
// setup, brr_xgram_kernel) applied to δ_{s−1} sits on the chain. Step s of the launch:
//   (A) every workgroup gathers δ_{s−1}; the owners also sum their rows of Q_s over the chunks;
//   (B) owners: r̃_s = γ − α ∘ (Q_s + C_s δ_{s−1}) on their rows, published;
//   (C) every workgroup: e += X_{s−1} δ_{s−1} on its chunk, then the partial dots X_{s+1}ᵀ e of
//       Q_{s+1}, published (this runs while r̃_s travels);
//   (D) owners: gather r̃_s, δ_s = M_s r̃_s on their rows, b and b̄ updated, δ_s published.
// Two hand-offs per super-block on the chain (δ, r̃) and the e update and dots beside the second.
// A chunk's rows of super-blocks s − 1 .. s + 2 are in LDS (four buffers; s + 2 lands by DMA during
// step s). Granule slots rotate over four super-blocks (a slot is rewritten only after every
// reader of its previous tag has passed a later hand-off). Same chain as the literal loop, rounding
// aside; waits bounded (sb_spin: ~1 s, then *info = −1 and every workgroup leaves).
constexpr int LA_KMAX = 48;  // individuals per chunk (at most)

// C_s = X_sᵀ X_{s−dist} for s = dist .. nsb − 1 (row-major 512 x 512 at CS + s·512²; rows of markers past
// p repeat marker p − 1: they meet α = γ = δ = 0): one 128x128 block per workgroup, fp64 MFMA over
// the individuals in 16-deep chunks staged by DMA (both operands marker-major, XOR-swizzled as A in
// sb_gemm128), double-buffered, two workgroups per CU. One-time setup.
__global__ void __launch_bounds__(256, 2) brr_xgram_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                           int64_t npad, int dist, double* __restrict__ CS) {
  __shared__ __attribute__((aligned(16))) double lds[2 * 2 * GA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane >> 4, fc = lane & 15;
  const int64_t s = dist + blockIdx.x / 16;
  const int ti = (int)((blockIdx.x >> 2) & 3), tj = (int)(blockIdx.x & 3);
  const int64_t ra = s * SBK + ti * BK2, rb = (s - dist) * SBK + tj * BK2;
  auto stage = [&](int64_t k0, int bf) {
    double* base = lds + bf * 2 * GA;
#pragma unroll
    for (int o = 0; o < 2; o++) {
      const int64_t r0 = o ? rb : ra;
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        const int j = wave * 4 + jj;
        const int slot = j * 64 + lane, r = slot >> 3, pp = (slot & 7) ^ (r & 7);
        int64_t row = r0 + r;
        row = row < p ? row : p - 1;
        __builtin_amdgcn_global_load_lds((const void*)(Xt + row * ldx + k0 + 2 * pp), (void*)(base + o * GA + j * 128), 16,
                                         0, 0);
      }
    }
  };
  sbd4 acc[4][4];
#pragma unroll
  for (int mm = 0; mm < 4; mm++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[mm][q] = (sbd4){0.0, 0.0, 0.0, 0.0};
  const int64_t nch = npad / GK;
  stage(0, 0);
#pragma unroll 1
  for (int64_t c = 0; c < nch; c++) {
    if (c + 1 < nch) {
      stage((c + 1) * GK, (int)((c + 1) & 1));
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const double* As = lds + (c & 1) * 2 * GA;
    const double* Bs = As + GA;
#pragma unroll
    for (int ks = 0; ks < GK; ks += 4) {
      double a[4], bq[4];
      const int k = ks + fr;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int r = wm * 64 + u * 16 + fc, cc = wn * 64 + u * 16 + fc;
        a[u] = As[(r * 8 + ((k >> 1) ^ (r & 7))) * 2 + (k & 1)];
        bq[u] = Bs[(cc * 8 + ((k >> 1) ^ (cc & 7))) * 2 + (k & 1)];
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mm = 0; mm < 4; mm++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[mm][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mm], bq[q], acc[mm][q], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
  }
  double* out = CS + s * (int64_t)SBK * SBK + (int64_t)(ti * BK2) * SBK + tj * BK2;
#pragma unroll
  for (int mm = 0; mm < 4; mm++)
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        out[(int64_t)(wm * 64 + mm * 16 + fr + 4 * r) * SBK + wn * 64 + q * 16 + fc] = acc[mm][q][r];
}

// Two super-blocks of slack for the partial dots (the default look-ahead form): with the second
// cross-Gram C2_s = X_sᵀX_{s−2},
//   d⁰_s = X_sᵀ e⁽ˢ⁻³⁾ + C2_s δ_{s−2} + C_s δ_{s−1},
// so step s's chunk dots are those of super-block s + 2 (from the residual after s − 1) and the
// owners sum them a whole step later (end of step s + 1): no chunk's e update and dots sit between
// a δ and the next r̃ any more. A chunk keeps the rows of five super-blocks in LDS (s − 1 for the e
// update, s + 2 for the dots, s + 3 arriving; 120 KB at K = 48), so every genotype byte is brought
// in once per iteration (24 KB of DMA per step at K = 48, beside the e update's reduction: the
// chunks' DMA bursts run at HBM speed). δ_{s−2} stays in LDS from its own gather.
// The first O workgroups own R rows of every super-block each and take Ko individuals; the others
// take Kn (both multiples of 16, <= LA_KMAX): the owners' e update and dots sit on the chain of
// hand-offs, so they get the smaller chunks.
template <bool kTrace>
__global__ void __launch_bounds__(256) brr_sweep_la2_kernel(const uint8_t* __restrict__ D, int64_t ldx, int64_t n,
                                                           int64_t p, double xs, const double* __restrict__ MS,
                                                           const double* __restrict__ CS,
                                                           const double* __restrict__ CS2, int64_t nsb, int Ko, int O,
                                                           int Kn, int R,
                                                           double* __restrict__ Pb, double* __restrict__ Rt,
                                                           double* __restrict__ Dl, int32_t* __restrict__ info,
                                                           double* __restrict__ b, double* __restrict__ bbar,
                                                           const double* __restrict__ alpha,
                                                           const double* __restrict__ gamma, double* __restrict__ e,
                                                           const BrrState* __restrict__ st, int64_t* __restrict__ trace) {
  __shared__ __attribute__((aligned(16))) uint8_t Drow[5][SBK * LA_KMAX];  // super-block j at Drow[j % 5]
  __shared__ __attribute__((aligned(16))) double es[LA_KMAX];
  __shared__ __attribute__((aligned(16))) double rt[SBK];
  __shared__ __attribute__((aligned(16))) double dlb[2][SBK];  // δ_j at dlb[j & 1]
  __shared__ double red[4][SB_RMAX];
  __shared__ __attribute__((aligned(16))) double eacc[1536];  // e update partial sums [row group][individual]
  __shared__ double eq[4][LA_KMAX];
  __shared__ int s_fail;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = (int)gridDim.x, c = (int)blockIdx.x;
  const int K = c < O ? Ko : Kn;
  const int64_t i0 = c < O ? (int64_t)c * Ko : (int64_t)O * Ko + (int64_t)(c - O) * Kn;
  const int r0 = c * R;
  const int nown = r0 >= SBK ? 0 : (SBK - r0 < R ? SBK - r0 : R);
  const bool tr_on = kTrace && threadIdx.x == 0;
  int64_t* trw = kTrace ? trace + (int64_t)c * nsb * 8 : nullptr;  // every workgroup: 8 per super-block
  auto mark = [&](int64_t s, int k) {
    if (tr_on) trw[s * 8 + k] = (int64_t)__builtin_amdgcn_s_memrealtime();
  };
  const int it_odd = (int)(st->it & 1);
  const bool accum = brr_accumulate(st);
  const double kk = (double)(st->nsum + 1);
  const uint64_t tag0 = (st->epoch << 40) + (uint64_t)st->it * (uint64_t)nsb;
  const __amdgpu_buffer_rsrc_t rP = brr_rsrc(Pb, (int64_t)4 * C * SBK * 16);
  const __amdgpu_buffer_rsrc_t rR = brr_rsrc(Rt, (int64_t)4 * SBK * 16);
  const __amdgpu_buffer_rsrc_t rD = brr_rsrc(Dl, (int64_t)4 * SBK * 16);
  if (tid == 0) s_fail = 0;
  const int kpc = K / 16, kinv = (65536 + kpc - 1) / kpc;  // q / kpc = (q · kinv) >> 16 for q < 2^14
  auto xrow = [&](int64_t j) { return Drow[(int)j % 5]; };
  auto dma_rows = [&](int64_t sb, uint8_t* dst) {  // wave 3: the chunk's rows of super-block sb -> dst
    const int pieces = SBK * kpc;
    for (int q0 = 0; q0 < pieces; q0 += 64) {
      const int q = q0 + lane;
      const int row = (q * kinv) >> 16, part = q - row * kpc;
      int64_t jr = sb * SBK + row;
      jr = jr < p ? jr : p - 1;
      const uint8_t* src = D + jr * ldx + i0 + part * 16;
      const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(dst + q0 * 16));
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(m0v), "v"(src) : "memory");
    }
  };
  // partial dots of super-block sb over this chunk from es (thread t: rows 2t, 2t + 1) -> P granules
  auto dots_publish = [&](int64_t sb, const uint8_t* Dr) {
    double a0 = 0.0, a1 = 0.0, c0 = 0.0, c1 = 0.0;
    const uint8_t* ra = Dr + (2 * tid) * K;
    const uint8_t* rb = ra + K;
    for (int u = 0; u < K; u += 16) {
      const uint4 va = *reinterpret_cast<const uint4*>(ra + u);
      const uint4 vb = *reinterpret_cast<const uint4*>(rb + u);
      const uint32_t wa[4] = {va.x, va.y, va.z, va.w};
      const uint32_t wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int bb = 0; bb < 4; bb += 2) {
          const double2 e2 = *reinterpret_cast<const double2*>(es + u + 4 * q + bb);
          a0 = fma((double)((wa[q] >> (8 * bb)) & 0xFFu), e2.x, a0);
          a1 = fma((double)((wa[q] >> (8 * bb + 8)) & 0xFFu), e2.y, a1);
          c0 = fma((double)((wb[q] >> (8 * bb)) & 0xFFu), e2.x, c0);
          c1 = fma((double)((wb[q] >> (8 * bb + 8)) & 0xFFu), e2.y, c1);
        }
    }
    const uint64_t key = sb_key(tag0 + (uint64_t)sb);
    const uint32_t off = (uint32_t)((((int64_t)(sb & 3) * C + c) * SBK + 2 * tid) * 16);
    sb_put(rP, off, a0 * xs + a1 * xs, key);
    sb_put(rP, off + 16, c0 * xs + c1 * xs, key);
  };
  // all 512 granules of super-block sb from buffer r into LDS out (waves 0-1, four per lane); the
  // pause between polls grows (up to ~0.2 µs) the longer the wait: 209 workgroups polling one 8 KB
  // block is what the hop pays. (Every lane re-reads all four granules: an asm load under a
  // divergent branch lets the compiler copy its register before the data lands.)
  auto gather512 = [&](__amdgpu_buffer_rsrc_t r, int64_t sb, double* out) {
    if (wave < 2) {
      const uint64_t key = sb_key(tag0 + (uint64_t)sb);
      bool failed = false;
      int64_t spin = 0;
      double x[4] = {0.0, 0.0, 0.0, 0.0};
      for (;;) {
        sb_fence();
        sbu4 w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = sb_getv(r, (uint32_t)(((int64_t)(sb & 3) * SBK + tid * 4 + q) * 16));
        bool all = true;
#pragma unroll
        for (int q = 0; q < 4; q++) all = sb_ok(w[q], key, x[q]) && all;
        if (!sb_spin(all, spin, info, failed)) break;
        for (int64_t z = spin >> 3; z > 0 && z < 8; z--) __builtin_amdgcn_s_sleep(1);
        if (spin >= 64) {
#pragma unroll
          for (int z = 0; z < 7; z++) __builtin_amdgcn_s_sleep(1);
        }
      }
      if (failed) s_fail = 1;
#pragma unroll
      for (int q = 0; q < 4; q++) out[tid * 4 + q] = x[q];
    }
  };
  // e update: thread t < 192 -> 8 individuals (column t % kq of 8 bytes) of row group g = t / kq:
  // rows g, g + ng, g + 2 ng, ... (interleaved, so a wave's lanes read consecutive rows: no LDS bank
  // conflicts); partial sums eacc[g][individual] summed over the groups by 4 K threads
  const int kq = K / 8, ng = 192 / kq, rpg = (SBK + ng - 1) / ng;
  const int ecq = tid % kq, eg = tid / kq;
  // e += X_sb δ (δ in dl) over the chunk, rows from Dr; ends with a barrier
  auto e_update = [&](const uint8_t* Dr, const double* dl, int64_t ms, auto&& between) {
    if (eg < ng) {
      double acc[8];
#pragma unroll
      for (int bb = 0; bb < 8; bb++) acc[bb] = 0.0;
      for (int k0 = 0; k0 < rpg; k0 += 8) {
        uint2 w[8];
        double d[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int r = eg + (k0 + u) * ng;
          const bool v = k0 + u < rpg && r < SBK;
          w[u] = v ? *reinterpret_cast<const uint2*>(Dr + r * K + ecq * 8) : uint2{0u, 0u};
          d[u] = v ? dl[r] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
          for (int bb = 0; bb < 4; bb++) {
            acc[bb] = fma((double)((w[u].x >> (8 * bb)) & 0xFFu), d[u], acc[bb]);
            acc[4 + bb] = fma((double)((w[u].y >> (8 * bb)) & 0xFFu), d[u], acc[4 + bb]);
          }
      }
      double2* ea = reinterpret_cast<double2*>(eacc + eg * K + ecq * 8);
#pragma unroll
      for (int q = 0; q < 4; q++) ea[q] = double2{acc[2 * q], acc[2 * q + 1]};
    }
    lds_barrier();
    if (ms >= 0) mark(ms, 6);
    between();  // runs beside the reduction (tid >= 4 K: wave 3 when K <= 48)
    if (tid < 4 * K) {
      const int ind = tid % K, q = tid / K;
      double u = 0.0;
      for (int g = q; g < ng; g += 4) u += eacc[g * K + ind];
      eq[q][ind] = u;
    }
    lds_barrier();
    if (ms >= 0) mark(ms, 7);
    if (tid < K && i0 + tid < n) es[tid] += (((eq[0][tid] + eq[1][tid]) + eq[2][tid]) + eq[3][tid]) * xs;
    lds_barrier();
  };

  if (tid < LA_KMAX) es[tid] = (tid < K && i0 + tid < n) ? e[i0 + tid] : 0.0;
  if (wave == 3) {
    for (int64_t j = 0; j < 3 && j < nsb; j++) dma_rows(j, xrow(j));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  dots_publish(0, xrow(0));  // Q_0 = X_0ᵀ e
  if (nsb > 1) dots_publish(1, xrow(1));  // Q_1 = X_1ᵀ e
  // owners: their rows of Q_sb summed over all chunks (waves 2-3, beside the δ gather of waves 0-1:
  // lane -> chunks lane + 64 (w − 2) and + 128 (C <= 256), summed in that order, xor-tree;
  // red[w − 2][r], the two waves summed in order by the reader)
  auto gather_q = [&](int64_t sb) {
    if (nown > 0 && wave >= 2) {
      const int wv = wave - 2;
      const uint64_t key = sb_key(tag0 + (uint64_t)sb);
      double v[SB_RMAX];
#pragma unroll
      for (int r = 0; r < SB_RMAX; r++) v[r] = 0.0;
      // both chunks' granules in one round trip: they were published a step ago, so the first poll
      // normally finds them all
      const int cc0 = lane + 64 * wv, cc1 = cc0 + 128;
      const bool has1 = cc1 < C;
      const uint32_t base0 = (uint32_t)((((int64_t)(sb & 3) * C + (cc0 < C ? cc0 : 0)) * SBK + r0) * 16);
      const uint32_t base1 = (uint32_t)((((int64_t)(sb & 3) * C + (has1 ? cc1 : 0)) * SBK + r0) * 16);
      bool failed = false;
      int64_t spin = 0;
      double x0[SB_RMAX], x1[SB_RMAX];
#pragma unroll
      for (int r = 0; r < SB_RMAX; r++) x0[r] = x1[r] = 0.0;
      for (;;) {
        sb_fence();
        sbu4 w0[SB_RMAX], w1[SB_RMAX];
#pragma unroll
        for (int r = 0; r < SB_RMAX; r++)
          if (r < R) {
            w0[r] = sb_getv(rP, base0 + r * 16);
            w1[r] = sb_getv(rP, base1 + r * 16);
          }
        bool all = true;
#pragma unroll
        for (int r = 0; r < SB_RMAX; r++)
          if (r < R && r < nown) {
            all = (cc0 >= C || sb_ok(w0[r], key, x0[r])) && all;
            all = (!has1 || sb_ok(w1[r], key, x1[r])) && all;
          }
        if (!sb_spin(all, spin, info, failed)) break;
      }
      if (failed) s_fail = 1;
#pragma unroll
      for (int r = 0; r < SB_RMAX; r++) v[r] = (cc0 < C && r < nown ? x0[r] : 0.0) + (has1 && r < nown ? x1[r] : 0.0);
#pragma unroll
      for (int r = 0; r < SB_RMAX; r++) {
        const double x = wave_sum_f64(v[r]);
        if (lane == 0) red[wv][r] = x;
      }
    }
  };
  // owned-row indices of this wave's GEMV rows (wave-uniform)
  const int wrow0 = __builtin_amdgcn_readfirstlane(wave), wrow1 = wrow0 + 4;
  for (int64_t s = 0; s < nsb; s++) {
    const int64_t j0 = s * SBK;
    const uint64_t key = sb_key(tag0 + (uint64_t)s);
    // operands of the owned rows (plain loads: written before this launch): C_s's rows now (for
    // (B)); M_s's rows once the δ gather is done (for (D)), so that gather queues behind 16 KB of
    // loads in the CU's memory pipeline instead of 32 KB
    double mrow[2][8], crow[2][8], crow2[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int w = h ? wrow1 : wrow0;
      const int jr = w < nown ? r0 + w : 0;
      const double* cr = CS + (s * SBK + jr) * (int64_t)SBK;
      const double* cr2 = CS2 + (s * SBK + jr) * (int64_t)SBK;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        crow[h][t] = (w < nown && s > 0) ? cr[lane + 64 * t] : 0.0;
        crow2[h][t] = (w < nown && s > 1) ? cr2[lane + 64 * t] : 0.0;
      }
    }
    // the step constants and the sample of this wave's rows (each wave publishes its own rows)
    double alv[2] = {0.0, 0.0}, gav[2] = {0.0, 0.0}, bo[2] = {0.0, 0.0}, bbo[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int w = h ? wrow1 : wrow0;
      if (w < nown) {
        const int64_t jm = j0 + r0 + w;
        alv[h] = alpha[jm];
        gav[h] = gamma[jm];
        const int64_t jc = jm < p ? jm : 0;
        bbo[h] = bbar[jc];
        bo[h] = b[it_odd * p + jc];
      }
    }
    // (A) δ_{s−1} -> dlb (every workgroup, waves 0-1) and the owners' rows of Q_s (waves 2-3; its
    // partial dots were published in (C) of step s − 2); wave 3: the DMA of step s − 1 (rows of
    // super-block s + 2) has landed before this step's barrier
    const double* dl1 = dlb[(s - 1) & 1];  // δ_{s−1}
    const double* dl2 = dlb[s & 1];        // δ_{s−2}
    if (s > 0) {
      // a workgroup that owns no rows has slack (its dots are needed two steps on): it first waits
      // for one granule of δ_{s−1}, one lane polling one line slowly, so that the owners' sweeps of
      // the 8 KB do not queue behind its own
      if (nown == 0 && wave == 0) {
        const uint64_t key1 = sb_key(tag0 + (uint64_t)(s - 1));
        const uint32_t off = (uint32_t)((((int64_t)((s - 1) & 3) * SBK) + SBK - 1) * 16);
        bool failed = false;
        int64_t spin = 0;
        for (;;) {
          sb_fence();
          const sbu4 w = sb_getv(rD, off);
          double x;
          if (!sb_spin(sb_ok(w, key1, x), spin, info, failed)) break;
#pragma unroll
          for (int z = 0; z < 7; z++) __builtin_amdgcn_s_sleep(2);
        }
        if (failed) s_fail = 1;
      }
      if (nown == 0) lds_barrier();
      gather512(rD, s - 1, dlb[(s - 1) & 1]);
    }
    gather_q(s);
    if (wave == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // C_s's rows are in registers by now; consumed here, so that the wait the compiler puts before
    // their first use (it cannot count the gathers' loads, and waits for all) comes before M_s's
    // loads are issued, not in (B) behind them
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int t = 0; t < 8; t++) asm volatile("" : "+v"(crow[h][t]), "+v"(crow2[h][t]));
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int w = h ? wrow1 : wrow0;
      const int jr = w < nown ? r0 + w : 0;
      const double* mr = MS + (s * SBK + jr) * (int64_t)SBK;
#pragma unroll
      for (int t = 0; t < 8; t++) mrow[h][t] = (w < nown) ? mr[lane + 64 * t] : 0.0;
    }
    lds_barrier();
    mark(s, 0);
    if (s_fail) return;
    // (B) owners: C_s δ_{s−1} + C2_s δ_{s−2} on their rows (wave w: rows w, w + 4), and each wave
    // publishes its rows of r̃_s (no barrier)
    if (nown > 0 && wrow0 < nown) {
      double dv1[8], dv2[8];
#pragma unroll
      for (int t = 0; t < 8; t++) {
        dv1[t] = s > 0 ? dl1[lane + 64 * t] : 0.0;
        dv2[t] = s > 1 ? dl2[lane + 64 * t] : 0.0;
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int w = h ? wrow1 : wrow0;
        if (w < nown) {
          double a = 0.0;
#pragma unroll
          for (int t = 0; t < 8; t++) a = fma(crow2[h][t], dv2[t], a);
#pragma unroll
          for (int t = 0; t < 8; t++) a = fma(crow[h][t], dv1[t], a);
          const double d0 = (red[0][w] + red[1][w]) + wave_sum_f64(a);
          if (lane == 0) sb_put(rR, (uint32_t)(((int64_t)(s & 3) * SBK + r0 + w) * 16), fma(d0, -alv[h], gav[h]), key);
        }
      }
    }
    mark(s, 1);
    // (C) e += X_{s−1} δ_{s−1}, then the partial dots of Q_{s+2} (from the residual after s − 1).
    // Wave 3 brings in the rows of super-block s + 3 (for step s + 1's dots) into the slot of s − 2,
    // read by step s − 1's e update, while waves 0-2 run the e update's row groups: the chunks' DMA
    // bursts run at HBM speed (~1.2 µs at K = 48), so the wave that issues them takes no row group.
    // (Issued in (A) instead, the burst slows the δ hop by more than that.)
    if (wave == 3 && s + 3 < nsb) dma_rows(s + 3, xrow(s + 3));
    if (s > 0) e_update(xrow(s - 1), dl1, s, [] {});
    mark(s, 5);
    if (s + 2 < nsb) dots_publish(s + 2, xrow(s + 2));
    mark(s, 2);
    // (D) owners: all of r̃_s, δ_s = M_s r̃_s on their rows, b and b̄, δ_s published
    if (nown > 0) {
      gather512(rR, s, rt);
      lds_barrier();
      if (s_fail) return;
      // each wave: δ_s, b and b̄ of its rows, δ_s published (no barrier)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int w = h ? wrow1 : wrow0;
        if (w < nown) {
          double a = 0.0;
#pragma unroll
          for (int t = 0; t < 8; t++) a = fma(mrow[h][t], rt[lane + 64 * t], a);
          const double dlt = wave_sum_f64(a);
          if (lane == 0) {
            const int64_t jm = j0 + r0 + w;
            if (jm < p) {
              const double bn = bo[h] - dlt;
              b[(it_odd ^ 1) * p + jm] = bn;
              if (accum) bbar[jm] = bbo[h] * ((kk - 1.0) / kk) + bn / kk;
            }
            sb_put(rD, (uint32_t)(((int64_t)(s & 3) * SBK + r0 + w) * 16), dlt, key);
          }
        }
      }
      mark(s, 4);
    }
    mark(s, 3);
  }
  // the last super-block's δ, and its e update
  gather512(rD, nsb - 1, dlb[(nsb - 1) & 1]);
  if (wave == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();
  if (s_fail) return;
  e_update(xrow(nsb - 1), dlb[(nsb - 1) & 1], -1, [] {});
  if (tid < K && i0 + tid < n) e[i0 + tid] = es[tid];
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

// D = X·s as bytes when that is exact for every stored value (padding included, which is 0);
// *bad counts the values that are not integers in [0, 255] after scaling
__global__ void __launch_bounds__(256) brr_quantize_kernel(const double* __restrict__ Xt, int64_t count, double s,
                                                           uint8_t* __restrict__ D, int* __restrict__ bad) {
  int nbad = 0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) {
    const double v = Xt[t] * s;
    const double r = rint(v);
    const bool ok = r == v && r >= 0.0 && r <= 255.0;
    nbad += ok ? 0 : 1;
    D[t] = ok ? (uint8_t)r : (uint8_t)0;
  }
  if (nbad) atomicAdd(bad, nbad);
}

// ---- BayesA, BayesB, BayesC (include/gbm.h gbm_bayes_fit states the sampler) -----------------
// Marker j has an effect b_j, an inclusion indicator d_j (BayesA: always 1) and (A, B) its own
// variance varB_j. The indicator's probability is a non-linear function of x_jᵀe at the marker's
// turn, so a block's 64 single-site steps are no triangular solve (no δ = M r̃): they run as a
// serial chain on wave 0 of every chunk workgroup, lane k holding r_k = x_kᵀe + x2_k d_k b_k and
// column k of the block's Gram matrix. bayes_prep_kernel forms, for every marker and in parallel,
// everything of its step that does not depend on the chain (the normal, logit(u), 1/C, the square
// roots), so that a chain step is FMAs, one compare, selects and one lane broadcast.
constexpr int GBM_MODEL_A = 1, GBM_MODEL_B = 2, GBM_MODEL_C = 3;

struct BayesState {
  double mu, varE, varBc, S, pi;  // varBc: BayesC's common σ²_b
  double S0e, df0, rate0, shape0, cIn, cOut;
  double mubar, varEbar, varBbar, pibar;
  int64_t it, burnin, thin, nsum;
  uint64_t seed;
  int model;
};

__device__ __forceinline__ bool bayes_accumulate(const BayesState* st) {
  const int64_t i = st->it + 1;
  return (i % st->thin == 0) && (i > st->burnin);
}

__device__ __forceinline__ double bayes_readlane(double v, int l) {
  union {
    double f;
    int i[2];
  } u;
  u.f = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], l);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], l);
  return u.f;
}

// the intercept step of brr_mu_kernel on the stream A = 8 it
__global__ void __launch_bounds__(1024) bayes_mu_kernel(double* __restrict__ e, int64_t n,
                                                        BayesState* __restrict__ st) {
  __shared__ double red[16];
  const double mu_old = st->mu;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) s += e[i] + mu_old;
  s = brr_block_sum<1024>(s, red);
  const double varE = st->varE;
  const double mu = s / (double)n + sqrt(varE / (double)n) * brr_normal(st->seed, 8 * (uint64_t)st->it, 0xFFFFFFFFull);
  for (int64_t i = threadIdx.x; i < n; i += 1024) e[i] = (e[i] + mu_old) - mu;
  __syncthreads();
  if (threadIdx.x == 0) st->mu = mu;
}

// Per marker j (one thread each, padded to whole blocks with zeros), the step constants pk[8 j ..]:
//   0: x2 eff   1: eff = d b (old)   2: a = 1/(varE C)   3: c = sqrt(1/C) ξ   4: sqrt(varB) ξ
//   5: b/(2 varE)   6: −b x2   7: log(π/(1−π)) − logit(u)
// so that with r = x_jᵀe + x2 eff:  logOdds − logit(u) = pk5 (2 r + pk6) + pk7,  b_in = a r + c.
// BayesA: pk5 = pk6 = 0, pk7 = 1 (always included).
__global__ void __launch_bounds__(256) bayes_prep_kernel(int64_t p, int64_t ppad, const double* __restrict__ x2,
                                                         const double* __restrict__ b, const double* __restrict__ d,
                                                         const double* __restrict__ varB,
                                                         const BayesState* __restrict__ st, double* __restrict__ pk) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ppad) return;
  double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (j < p) {
    const int64_t par = st->it & 1;
    const uint64_t A = 8 * (uint64_t)st->it;
    const double varE = st->varE, iv = 1.0 / varE;
    const double vb = st->model == GBM_MODEL_C ? st->varBc : varB[j];
    const double bo = b[par * p + j], eff = d[par * p + j] * bo, xx = x2[j];
    const double xi = brr_normal(st->seed, A, (uint64_t)j);
    const double ic = 1.0 / (xx / varE + 1.0 / vb);
    q[0] = xx * eff;
    q[1] = eff;
    q[2] = iv * ic;
    q[3] = sqrt(ic) * xi;
    q[4] = sqrt(vb) * xi;
    if (st->model == GBM_MODEL_A) {
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
template <typename T>
__global__ void __launch_bounds__(256) bayes_chain_kernel(const T* __restrict__ Xt, int64_t ldx, int64_t n,
                                                          int64_t p, double xs, const double* __restrict__ W,
                                                          int64_t blk, int64_t nblk,
                                                          const double* __restrict__ partial_in,
                                                          double* __restrict__ partial_out,
                                                          const double* __restrict__ pk, double* __restrict__ b,
                                                          double* __restrict__ d, double* __restrict__ bbar,
                                                          double* __restrict__ dbar, double* __restrict__ e,
                                                          const BayesState* __restrict__ st) {
  constexpr int RP = IW + 2;  // doubles (row pitch 2064 B, as brr_step_kernel)
  __shared__ __attribute__((aligned(16))) double Xn[BB * RP];
  __shared__ double delta[BB];
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
  const double e_old = e[i];
  // (3) wave 0's operands: column `lane` of W (= its row: W is symmetric) and the step constants
  double w[BB];
  double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool on = lane < nb;
  const int64_t j = j0 + lane;
  if (tid < 64) {
    const double* wr = W + (blk * BB + lane) * BB;
#pragma unroll
    for (int s = 0; s < BB; s += 2) {
      const double2 v = *reinterpret_cast<const double2*>(wr + s);
      w[s] = v.x;
      w[s + 1] = v.y;
    }
    const double2* pq = reinterpret_cast<const double2*>(pk + 8 * j);  // padded to whole blocks
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double2 v = pq[u];
      q[2 * u] = v.x;
      q[2 * u + 1] = v.y;
    }
  }
  const bool keeper = blockIdx.x == 0 && tid < 64 && on;
  const double bb_old = keeper ? bbar[j] : 0.0, db_old = keeper ? dbar[j] : 0.0;
  {
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
    const double d0 = ((part4[0][lane] + part4[1][lane]) + part4[2][lane]) + part4[3][lane];
#pragma unroll
    for (int s = 0; s < BB; s++) w[s] = lane > s ? w[s] : 0.0;
    const double eff = q[1], qa = q[2], qc = q[3], bout = q[4], qbh = q[5], qm = q[6], qthr = q[7];
    double r = d0 + q[0];
#pragma unroll
    for (int s = 0; s < BB; s++) {
      const double lo = fma(qbh, fma(2.0, r, qm), qthr);
      const double bin = fma(r, qa, qc);
      const double cand = lo > 0.0 ? eff - bin : eff;
      r = fma(bayes_readlane(cand, s), w[s], r);
    }
    const double lo = fma(qbh, fma(2.0, r, qm), qthr);
    const double bin = fma(r, qa, qc);
    const bool inc = lo > 0.0;
    delta[lane] = inc ? eff - bin : eff;
    if (keeper) {
      const double bfin = inc ? bin : bout, dfin = inc ? 1.0 : 0.0;
      const int64_t o = ((st->it & 1) ^ 1) * p + j;
      b[o] = bfin;
      d[o] = dfin;
      if (bayes_accumulate(st)) {
        const double k = (double)(st->nsum + 1);
        bbar[j] = bb_old * ((k - 1.0) / k) + (inc ? bfin : 0.0) / k;
        dbar[j] = db_old * ((k - 1.0) / k) + dfin / k;
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
    double s0 = 0.0, s1 = 0.0;
    if (lane < nb1) {
      const double* er = es + wave * 64;
      if constexpr (sizeof(T) == 8) {
        const double* xr = Xn + lane * RP + wave * 64;
#pragma unroll
        for (int u = 0; u < 64; u += 2) {
          const double2 xv2 = *reinterpret_cast<const double2*>(xr + u);
          s0 = fma(xv2.x, er[u], s0);
          s1 = fma(xv2.y, er[u + 1], s1);
        }
      } else {
        const uint8_t* xr = Xb + lane * IW;
        uint4 v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = *reinterpret_cast<const uint4*>(xr + (((4 * wave + t) ^ (lane & 15)) * 16));
        brr_dot64_u8(v, er, s0, s1);
        s0 *= xs;
        s1 *= xs;
      }
    }
    part4[wave][lane] = s0 + s1;
    __syncthreads();
    if (tid < 64)
      partial_out[blockIdx.x * BB + lane] = ((part4[0][lane] + part4[1][lane]) + part4[2][lane]) + part4[3][lane];
  }
}

// Per-marker variances (BayesA, BayesB: varB_j = (S + b_j²)/χ²(df0 + 1) on the stream PM(it, j))
// and, per workgroup, the partial sums vpart[5 blk ..] = Σ 1/varB_j, Σ d_j, Σ b_j², Σ varB_j over
// its 256 markers and Σ e_i² over its 256 individuals (no atomics: bayes_final_kernel adds the
// workgroups' partials in index order).
__global__ void __launch_bounds__(256) bayes_var_kernel(const double* __restrict__ b, const double* __restrict__ d,
                                                        double* __restrict__ varB, int64_t p,
                                                        const double* __restrict__ e, int64_t n,
                                                        const BayesState* __restrict__ st,
                                                        double* __restrict__ vpart) {
  __shared__ double red[4];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t par = (st->it & 1) ^ 1;  // this iteration's samples
  double v[5] = {0, 0, 0, 0, 0};
  if (j < p) {
    const double bj = b[par * p + j];
    v[1] = d[par * p + j];
    v[2] = bj * bj;
    if (st->model != GBM_MODEL_C) {
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
// means of μ, varE, mean_j varB_j and π; next iteration.
__global__ void __launch_bounds__(256) bayes_final_kernel(const double* __restrict__ vpart, int64_t nvb, int64_t p,
                                                          int64_t n, BayesState* __restrict__ st) {
  __shared__ double red[4];
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
  if (st->model == GBM_MODEL_C) {
    const double vb = (sum[2] + st->S) / brr_chisq(seed, A + 1, df0 + (double)p);
    st->varBc = vb;
    st->S = brr_chisq(seed, A + 4, 2.0 * (0.5 * df0 + shape0)) / (2.0 * (1.0 / (2.0 * vb) + rate0));
    vbmean = vb;
  } else {
    st->S = brr_chisq(seed, A + 4, 2.0 * (0.5 * (double)p * df0 + shape0)) / (2.0 * (0.5 * sum[0] + rate0));
    vbmean = sum[3] / (double)p;
  }
  if (st->model != GBM_MODEL_A) {
    const double m = sum[1];
    const double g1 = 0.5 * brr_chisq(seed, A + 5, 2.0 * (m + st->cIn));
    const double g2 = 0.5 * brr_chisq(seed, A + 6, 2.0 * (((double)p - m) + st->cOut));
    st->pi = g1 / (g1 + g2);
  }
  st->varE = (sum[4] + st->S0e) / brr_chisq(seed, A + 2, df0 + (double)n);
  if (bayes_accumulate(st)) {
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
}  // namespace gbm

using namespace gbm;


namespace gbm {
namespace {

// Pooled per-device BRR contexts (as capi.cpp pools the GBLUP fit contexts): a fit leases one, its
// buffers only grow, so repeated fits of one shape allocate no device memory after the first
// (cvmultithread! runs bayesian("BRR") once per fold). The captured iteration graph is kept with the
// context and reused while the call's shape and buffers are unchanged.
struct BrrCtx {
  int dev = 0;
  Stream stream;
  DevBuf Xt, colmean, x2, e, b, bbar, r, stm, D, badm, W, Mb, alph, gamm, Dt, pb, part, pout;
  DevBuf Wsb, MS, Ssc, Pb, Rt, Dl, sbcnt;  // the super-block sweep
  DevBuf CS, CS2;                          // its cross-Grams C_s = X_sᵀ X_{s−1}, C2_s = X_sᵀ X_{s−2}
  DevBuf trace;                            // GBM_BRR_TRACE timestamps of this context's last sweep
  DevBuf dind, dbar, varBj, pk, vpart, bst;  // gbm_bayes_fit: indicators, PIP, varB_j, step constants, partial sums, state
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  std::vector<int64_t> key;  // what the captured graph was built for
  void drop_graph() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
    key.clear();
  }
  // gbm_bayes_fit's captured iteration (its own slot: BRR and BayesA/B/C fits that alternate on
  // one context keep both graphs)
  hipGraphExec_t bayes_exec = nullptr;
  hipGraph_t bayes_graph = nullptr;
  std::vector<int64_t> bayes_key;
  void drop_bayes_graph() {
    if (bayes_exec) (void)hipGraphExecDestroy(bayes_exec);
    if (bayes_graph) (void)hipGraphDestroy(bayes_graph);
    bayes_exec = nullptr;
    bayes_graph = nullptr;
    bayes_key.clear();
  }
  ~BrrCtx() {
    (void)hipSetDevice(dev);
    drop_graph();
    drop_bayes_graph();
  }
};

class BrrPool {
 public:
  int acquire(int dev, std::unique_ptr<BrrCtx>& out) {
    {
      std::lock_guard<std::mutex> lock(mu_);
      auto& v = idle_[dev];
      if (!v.empty()) {
        out = std::move(v.back());
        v.pop_back();
        return GBM_OK;
      }
    }
    auto c = std::make_unique<BrrCtx>();
    c->dev = dev;
    c->stream.dev = dev;
    GBM_HIP_TRY(hipSetDevice(dev));
    GBM_HIP_TRY(hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking));
    out = std::move(c);
    return GBM_OK;
  }
  void release(std::unique_ptr<BrrCtx> c) {
    (void)hipSetDevice(c->dev);
    if (hipStreamSynchronize(c->stream.s) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    std::lock_guard<std::mutex> lock(mu_);
    idle_[c->dev].push_back(std::move(c));
  }
  void clear() {
    std::map<int, std::vector<std::unique_ptr<BrrCtx>>> drop;
    std::lock_guard<std::mutex> lock(mu_);
    drop.swap(idle_);
  }
  // drops the idle contexts of one device (buffers and graphs freed outside the lock); returns how many
  int64_t trim(int dev) {
    std::vector<std::unique_ptr<BrrCtx>> drop;
    {
      std::lock_guard<std::mutex> lock(mu_);
      auto it = idle_.find(dev);
      if (it != idle_.end()) drop.swap(it->second);
    }
    return (int64_t)drop.size();
  }
  // the persistent sweep needs all its workgroups resident at once: sweeps of concurrent fits on one
  // device take turns (held for a whole fit), so two of them can never be partly resident and spin
  // on each other
  std::mutex& sweep_lock(int dev) {
    std::lock_guard<std::mutex> lock(mu_);
    auto& m = sweep_mu_[dev];
    if (!m) m = std::make_unique<std::mutex>();
    return *m;
  }

 private:
  std::mutex mu_;
  std::map<int, std::vector<std::unique_ptr<BrrCtx>>> idle_;
  std::map<int, std::unique_ptr<std::mutex>> sweep_mu_;
};

BrrPool& brr_pool() {
  static BrrPool* p = [] {
    auto* bp = new BrrPool;  // never destroyed (device memory outlives the runtime otherwise)
    // an allocation (of any entry point) that runs out of device memory also frees the idle BRR
    // contexts of its device before its retry (host_util.h dalloc)
    register_trim_hook([](int dev) { return brr_pool().trim(dev); });
    return bp;
  }();
  return *p;
}

struct BrrLease {
  std::unique_ptr<BrrCtx> c;
  ~BrrLease() {
    if (c) brr_pool().release(std::move(c));
  }
};

}  // namespace
}  // namespace gbm

namespace gbm {
void brr_release_cache() { brr_pool().clear(); }
}  // namespace gbm

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
  using namespace gbm;
  *sweep_timeout = false;
  BrrLease lease;
  GBM_TRY(brr_pool().acquire(dev, lease.c));
  BrrCtx& cx = *lease.c;
  GBM_HIP_TRY(hipSetDevice(dev));
  hipStream_t s = cx.stream.s;
  // Xt rows and e padded to whole IW-individual chunks (the block kernels read full chunks)
  const int64_t npad = round_up(n, IW);
  const int64_t C64 = (n + IW - 1) / IW;
  GBM_TRY(ensure(cx.Xt, dev, p * npad * 8));
  GBM_TRY(ensure(cx.colmean, dev, p * 8));
  GBM_TRY(ensure(cx.x2, dev, p * 8));
  GBM_TRY(ensure(cx.e, dev, npad * 8));
  GBM_TRY(ensure(cx.b, dev, 2 * p * 8));  // two copies (iteration parity)
  GBM_TRY(ensure(cx.bbar, dev, p * 8));
  GBM_TRY(ensure(cx.r, dev, 2 * C64 * BK2 * 8));  // ping-pong partial dots
  GBM_TRY(ensure(cx.stm, dev, sizeof(BrrState)));
  GBM_HIP_TRY(hipMemsetAsync(cx.Xt.p, 0, (size_t)(p * npad * 8), s));
  GBM_HIP_TRY(hipMemcpy2DAsync(cx.Xt.p, npad * 8, X, ldx * 8, n * 8, p, hipMemcpyHostToDevice, s));
  brr_colstats_kernel<<<(unsigned)std::min<int64_t>(p, 4096), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n,
                                                                           (double*)cx.colmean.p, (double*)cx.x2.p);
  GBM_LAUNCH_CHECK();
  std::vector<double> cm(p), xx(p);
  GBM_HIP_TRY(hipMemcpyAsync(cm.data(), cx.colmean.p, p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(xx.data(), cx.x2.p, p * 8, hipMemcpyDeviceToHost, s));
  // byte storage for the sampler's sweeps when X = D/s exactly (s = 2: diploid allele
  // frequencies; then 4, 1): the chain is identical, the per-iteration stream 8× smaller.
  // GBM_BRR_I8=0 keeps fp64 storage (read per call).
  double xs = 0.0;  // 0: fp64 storage
  {
    const char* ev = ::gbm::knob("GBM_BRR_I8");
    if (!(ev && ev[0] == '0')) {
      GBM_TRY(ensure(cx.D, dev, p * npad + 4096));  // + slack: the super-block sweep's last chunk reads past n
      GBM_TRY(ensure(cx.badm, dev, sizeof(int)));
      const double scales[3] = {2.0, 4.0, 1.0};
      for (double sc : scales) {
        int nbad = -1;
        GBM_HIP_TRY(hipMemsetAsync(cx.badm.p, 0, sizeof(int), s));
        brr_quantize_kernel<<<2048, 256, 0, s>>>((const double*)cx.Xt.p, p * npad, sc, (uint8_t*)cx.D.p, (int*)cx.badm.p);
        GBM_LAUNCH_CHECK();
        GBM_HIP_TRY(hipMemcpyAsync(&nbad, cx.badm.p, sizeof(int), hipMemcpyDeviceToHost, s));
        GBM_HIP_TRY(hipStreamSynchronize(s));
        if (nbad == 0) {
          xs = 1.0 / sc;
          break;
        }
      }
    }
  }
  // byte storage on (up to) every CU: the super-block sweep (brr_sweep_la2_kernel) when its chunk
  // workgroups (K <= LA_KMAX individuals each: n <= 48 x CUs) can all be resident, one per CU, and own
  // <= SB_RMAX rows of a super-block each; GBM_BRR_SWEEP=0 (read per call) keeps the per-launch path
  int cus = 0;
  GBM_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  bool sweep = false;
  int sbK = 0, sbC = 0, sbR = 0;
  int la2Ko = 0, la2Kn = 0, la2R = 0, la2O = 0, la2C = 0;
  if (xs > 0.0 && sweep_mode != 0) {
    const char* ev = ::gbm::knob("GBM_BRR_SWEEP");
    int per_cu = 0;
    GBM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, brr_sweep_la2_kernel<false>, 256, 0));
    sbK = (int)round_up(std::max<int64_t>(16, (n + cus - 1) / cus), 16);
    if (const char* ek = ::gbm::knob("GBM_BRR_SB_K"))  // (timing experiments) a larger chunk
      sbK = std::max<int>(sbK, (int)round_up(std::max<int64_t>(16, atoll(ek)), 16));
    sbC = (int)((n + sbK - 1) / sbK);
    sbR = (int)round_up((SBK + sbC - 1) / sbC, 2);
    sweep = !(ev && ev[0] == '0') && per_cu >= 1 && sbK <= LA_KMAX && sbC <= std::min(cus, 256) && sbR <= SB_RMAX;
    // the chunk split: O = 512 / R owners of Ko individuals, the rest Kn (both <= LA_KMAX), all on
    // <= min(CUs, 256) workgroups; the owners get the smallest Ko that fits. Off unless GBM_BRR_OWN_R=
    // 2|4|6|8 (read per call) sets R: at C4 the extra workgroups' polls cost the hops more than the
    // owners' lighter chunks save (2.58 ms at R = 4, 3.32 at R = 8, vs 2.41 uniform). Uniform
    // chunks (Ko = Kn = K, O = 512 / R) otherwise.
    la2Ko = sbK;
    la2Kn = sbK;
    la2R = sbR;
    la2O = (SBK + sbR - 1) / sbR;
    la2C = sbC;
    if (sweep) {
      int R2 = 0;
      if (const char* er = ::gbm::knob("GBM_BRR_OWN_R")) R2 = std::max(2, std::min<int>(SB_RMAX, atoi(er) & ~1));
      const int O2 = R2 > 0 ? (SBK + R2 - 1) / R2 : 0;
      const int ncu = std::min(cus, 256);
      for (int Ko = 16; R2 > 0 && Ko <= LA_KMAX && O2 < ncu; Ko += 16) {
        const int64_t rest = n - (int64_t)O2 * Ko;
        if (rest < 16) break;
        const int Kn = (int)round_up(std::max<int64_t>(16, (rest + (ncu - O2) - 1) / (ncu - O2)), 16);
        if (Kn > LA_KMAX) continue;
        if (Kn <= Ko) break;  // no lighter owners than the uniform split
        la2Ko = Ko;
        la2Kn = Kn;
        la2R = R2;
        la2O = O2;
        la2C = O2 + (int)((rest + Kn - 1) / Kn);
        break;
      }
    }
  }
  // markers per launch: 128 with byte storage (two halves), 64 with fp64 storage; the Gram blocks
  // each launch needs (brr_gram_kernel), and the block-transposed bytes of the byte path. The
  // super-block sweep rounds the 128-blocks up to whole super-blocks (α = γ = 0 past p).
  const int64_t bk = xs > 0.0 ? BK2 : BB;
  const int64_t nsb = (p + SBK - 1) / SBK;
  const int64_t nblk = sweep ? nsb * SBN : (p + bk - 1) / bk;
  const int nw = xs > 0.0 ? 3 : 1;
  GBM_TRY(ensure(cx.W, dev, nblk * nw * BB * BB * 8));
  // per-iteration block inverses (same shape as W) and step constants α, γ (padded to whole launches)
  GBM_TRY(ensure(cx.Mb, dev, nblk * nw * BB * BB * 8));
  GBM_TRY(ensure(cx.alph, dev, nblk * bk * 8));
  GBM_TRY(ensure(cx.gamm, dev, nblk * bk * 8));
  brr_gram_kernel<<<(unsigned)(nblk * nw), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n, nw, (double*)cx.W.p);
  GBM_LAUNCH_CHECK();
  const bool traced = sweep && ::gbm::knob("GBM_BRR_TRACE") != nullptr;
  const int64_t trace_n = traced ? (int64_t)la2C * nsb * 8 : 0;
  if (sweep) {
    GBM_TRY(ensure(cx.Wsb, dev, nsb * SB_PAIRS * BK2 * BK2 * 8));
    GBM_TRY(ensure(cx.MS, dev, nsb * SBK * SBK * 8));
    GBM_TRY(ensure(cx.Ssc, dev, nsb * 6 * BK2 * BK2 * 8));
    GBM_TRY(ensure(cx.Pb, dev, (int64_t)4 * la2C * SBK * 16));  // 16-B hand-off granules (4 slots)
    GBM_TRY(ensure(cx.Rt, dev, 4 * SBK * 16));
    GBM_TRY(ensure(cx.Dl, dev, 4 * SBK * 16));
    GBM_TRY(ensure(cx.CS, dev, nsb * SBK * SBK * 8));
    if (nsb > 1) {
      brr_xgram_kernel<<<(unsigned)((nsb - 1) * 16), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, npad, 1,
                                                                  (double*)cx.CS.p);
      GBM_LAUNCH_CHECK();
    }
    GBM_TRY(ensure(cx.CS2, dev, nsb * SBK * SBK * 8));
    if (nsb > 2) {
      brr_xgram_kernel<<<(unsigned)((nsb - 2) * 16), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, npad, 2,
                                                                  (double*)cx.CS2.p);
      GBM_LAUNCH_CHECK();
    }
    GBM_TRY(ensure(cx.sbcnt, dev, 32 * sizeof(int32_t)));
    GBM_HIP_TRY(hipMemsetAsync(cx.MS.p, 0, (size_t)(nsb * SBK * SBK * 8), s));  // blocks above the diagonal
    GBM_HIP_TRY(hipMemsetAsync(cx.sbcnt.p, 0, 32 * sizeof(int32_t), s));
    GBM_HIP_TRY(hipMemsetAsync(cx.alph.p, 0, (size_t)(nblk * bk * 8), s));
    GBM_HIP_TRY(hipMemsetAsync(cx.gamm.p, 0, (size_t)(nblk * bk * 8), s));
    brr_gram_sb_kernel<<<(unsigned)(nsb * SB_PAIRS * 4), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n, (double*)cx.Wsb.p);
    GBM_LAUNCH_CHECK();
    if (traced) GBM_TRY(ensure(cx.trace, dev, trace_n * 8));
  }
  if (xs > 0.0 && !sweep) {  // the per-launch path's individual-major copy of the bytes
    GBM_TRY(ensure(cx.Dt, dev, nblk * npad * BK2));
    brr_block_transpose_kernel<<<dim3((unsigned)(npad / 64), (unsigned)nblk), 256, 0, s>>>((const uint8_t*)cx.D.p, npad,
                                                                                            p, (uint8_t*)cx.Dt.p);
    GBM_LAUNCH_CHECK();
  }
  GBM_HIP_TRY(hipStreamSynchronize(s));
  // BGLR defaults (setLT.BRR and the residual prior): var(y) with ddof 1
  double ym = 0.0;
  for (int64_t i = 0; i < n; i++) ym += y[i];
  ym /= (double)n;
  double vy = 0.0;
  for (int64_t i = 0; i < n; i++) vy += (y[i] - ym) * (y[i] - ym);
  vy /= (double)(n - 1);
  double msx = 0.0, smsq = 0.0;
  for (int64_t j = 0; j < p; j++) {
    msx += xx[j];
    smsq += cm[j] * cm[j];
  }
  msx = msx / (double)n - smsq;
  if (!(msx > 0.0)) return fail(GBM_E_DATA, "gbm_brr_fit: the markers have no variance");
  BrrState st0{};
  st0.mu = ym;
  st0.S0e = vy * (1.0 - r2) * (df0 + 2.0);
  st0.S0b = vy * r2 / msx * (df0 + 2.0);
  st0.df0e = df0;
  st0.df0b = df0;
  st0.varE = st0.S0e / (df0 + 2.0);
  st0.varB = st0.S0b / (df0 + 2.0);
  st0.burnin = n_burnin;
  st0.thin = thin;
  st0.seed = seed;
  static std::atomic<uint64_t> fit_epoch{1};
  st0.epoch = fit_epoch.fetch_add(1, std::memory_order_relaxed);
  std::vector<double> e0(npad, 0.0);
  for (int64_t i = 0; i < n; i++) e0[i] = y[i] - ym;
  GBM_HIP_TRY(hipMemcpyAsync(cx.e.p, e0.data(), npad * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.b.p, 0, 2 * p * 8, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.bbar.p, 0, p * 8, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.stm.p, &st0, sizeof(BrrState), hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  // one Gibbs iteration, captured once and replayed (kept with the context while the shape and the
  // buffers are the same)
  auto* stp = (BrrState*)cx.stm.p;
  const unsigned C = (unsigned)C64;
  const unsigned prep_grid = (unsigned)(xs > 0.0 ? nblk : (nblk + 3) / 4);
  int64_t* trace_dev = traced ? (int64_t*)cx.trace.p : nullptr;
  auto enqueue_iteration = [&]() -> int {
    brr_prep_kernel<<<prep_grid, 256, 0, s>>>((const double*)cx.W.p, p, nblk, nw, (const double*)cx.x2.p,
                                              (const double*)cx.b.p, stp, (double*)cx.Mb.p, (double*)cx.alph.p,
                                              (double*)cx.gamm.p, sweep ? (double*)cx.MS.p : nullptr);
    brr_mu_kernel<<<1, 1024, 0, s>>>((double*)cx.e.p, n, stp);
    if (sweep) {
      for (int level : {0, 2, 3})
        brr_sb_prep_kernel<<<(unsigned)(nsb * (level == 0 ? 2 : 4)), 256, 0, s>>>(
            level, (const double*)cx.Wsb.p, (const double*)cx.alph.p, (double*)cx.MS.p, (double*)cx.Ssc.p);
      int32_t* cn = (int32_t*)cx.sbcnt.p + 24;  // the error cell (zeroed at setup)
      if (traced)
        brr_sweep_la2_kernel<true><<<(unsigned)la2C, 256, 0, s>>>(
            (const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.MS.p, (const double*)cx.CS.p,
            (const double*)cx.CS2.p, nsb, la2Ko, la2O, la2Kn, la2R, (double*)cx.Pb.p, (double*)cx.Rt.p, (double*)cx.Dl.p, cn,
            (double*)cx.b.p, (double*)cx.bbar.p, (const double*)cx.alph.p, (const double*)cx.gamm.p,
            (double*)cx.e.p, stp, trace_dev);
      else
        brr_sweep_la2_kernel<false><<<(unsigned)la2C, 256, 0, s>>>(
            (const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.MS.p, (const double*)cx.CS.p,
            (const double*)cx.CS2.p, nsb, la2Ko, la2O, la2Kn, la2R, (double*)cx.Pb.p, (double*)cx.Rt.p, (double*)cx.Dl.p, cn,
            (double*)cx.b.p, (double*)cx.bbar.p, (const double*)cx.alph.p, (const double*)cx.gamm.p,
            (double*)cx.e.p, stp, nullptr);
      brr_var_kernel<<<1, 1024, 0, s>>>((const double*)cx.b.p, p, (const double*)cx.e.p, n, stp);
      return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, "gbm_brr_fit: launch failed");
    }
    if (xs > 0.0)
      brr_dots0_128_kernel<<<C, 256, 0, s>>>((const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.e.p,
                                             (double*)cx.r.p);
    else
      brr_dots0_kernel<double><<<C, 256, 0, s>>>((const double*)cx.Xt.p, npad, n, p, 1.0, (const double*)cx.e.p,
                                                 (double*)cx.r.p);
    for (int64_t k = 0; k < nblk; k++) {
      double* pin = (double*)cx.r.p + (k & 1) * (int64_t)C * bk;
      double* pout = (double*)cx.r.p + ((k + 1) & 1) * (int64_t)C * bk;
      if (xs > 0.0)
        brr_step128_kernel<<<C, 256, 0, s>>>((const uint8_t*)cx.D.p, (const uint8_t*)cx.Dt.p, npad, n, p, xs,
                                             (const double*)cx.Mb.p, k, nblk, pin, pout, (double*)cx.b.p,
                                             (double*)cx.bbar.p, (const double*)cx.alph.p, (const double*)cx.gamm.p,
                                             (double*)cx.e.p, stp);
      else
        brr_step_kernel<double><<<C, 256, 0, s>>>((const double*)cx.Xt.p, npad, n, p, 1.0, (const double*)cx.Mb.p, k,
                                                  nblk, pin, pout, (double*)cx.b.p, (double*)cx.bbar.p,
                                                  (const double*)cx.alph.p, (const double*)cx.gamm.p, (double*)cx.e.p,
                                                  stp);
    }
    brr_var_kernel<<<1, 1024, 0, s>>>((const double*)cx.b.p, p, (const double*)cx.e.p, n, stp);
    return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, "gbm_brr_fit: launch failed");
  };
  const std::vector<int64_t> key = {n, p, npad, (int64_t)(xs * 64.0), sweep ? 1 : 0,
                                    (int64_t)(uintptr_t)cx.Xt.p, (int64_t)(uintptr_t)cx.D.p, (int64_t)(uintptr_t)cx.Dt.p,
                                    (int64_t)(uintptr_t)cx.W.p, (int64_t)(uintptr_t)cx.Mb.p, (int64_t)(uintptr_t)cx.r.p,
                                    (int64_t)(uintptr_t)cx.e.p, (int64_t)(uintptr_t)cx.b.p,
                                    (int64_t)(uintptr_t)cx.bbar.p, (int64_t)(uintptr_t)cx.alph.p,
                                    (int64_t)(uintptr_t)cx.gamm.p, (int64_t)(uintptr_t)cx.x2.p,
                                    (int64_t)(uintptr_t)cx.stm.p, sbK, sbC, sbR, la2Ko, la2O, la2Kn, la2R, la2C,
                                    (int64_t)(uintptr_t)cx.MS.p, (int64_t)(uintptr_t)cx.Wsb.p, (int64_t)(uintptr_t)cx.Ssc.p,
                                    (int64_t)(uintptr_t)cx.Pb.p, (int64_t)(uintptr_t)cx.Rt.p, (int64_t)(uintptr_t)cx.Dl.p,
                                    (int64_t)(uintptr_t)cx.sbcnt.p, (int64_t)(uintptr_t)trace_dev,
                                    (int64_t)(uintptr_t)cx.CS.p, (int64_t)(uintptr_t)cx.CS2.p};
  int rc = GBM_OK;
  if (cx.key != key) {
    cx.drop_graph();
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      rc = enqueue_iteration();
      if (hipStreamEndCapture(s, &cx.graph) != hipSuccess || rc != GBM_OK ||
          hipGraphInstantiate(&cx.exec, cx.graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        cx.drop_graph();
        rc = GBM_OK;  // fall back to direct launches (same kernels, same order)
      } else {
        cx.key = key;
      }
    }
  }
  {
    std::unique_lock<std::mutex> sweep_guard;
    if (sweep) sweep_guard = std::unique_lock<std::mutex>(brr_pool().sweep_lock(dev));
    for (int64_t it = 0; it < n_iter && rc == GBM_OK; it++) {
      if (cx.exec) {
        if (hipGraphLaunch(cx.exec, s) != hipSuccess) rc = fail(GBM_E_HIP, "gbm_brr_fit: graph launch failed");
      } else {
        rc = enqueue_iteration();
      }
    }
    if (rc == GBM_OK) GBM_HIP_TRY(hipStreamSynchronize(s));
  }
  if (rc != GBM_OK) return rc;
  if (sweep) {
    int32_t inf = 0;
    GBM_HIP_TRY(hipMemcpyAsync(&inf, (int32_t*)cx.sbcnt.p + 24, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
    if (::gbm::knob("GBM_BRR_TEST_SWEEP_TIMEOUT")) inf = -1;  // tests: the fall-back's reporting, no device timeout
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
    g_brr_shape.store((int64_t)la2C | ((int64_t)la2O << 12) | ((int64_t)la2R << 24) | ((int64_t)la2Ko << 32) |
                      ((int64_t)la2Kn << 44));
  BrrState fin{};
  GBM_HIP_TRY(hipMemcpyAsync(&fin, cx.stm.p, sizeof(BrrState), hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(b_hat_out + 1, cx.bbar.p, p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  b_hat_out[0] = fin.mubar;
  if (var_out) {
    var_out[0] = fin.varEbar;
    var_out[1] = fin.varBbar;
  }
  if (y_pred_out) {
    const int64_t nchunks = predict_chunks(n, p);
    GBM_TRY(ensure(cx.pb, dev, (p + 1) * 8));
    GBM_TRY(ensure(cx.part, dev, nchunks * npad * 8));
    GBM_TRY(ensure(cx.pout, dev, npad * 8));
    GBM_HIP_TRY(hipMemcpyAsync(cx.pb.p, b_hat_out, (p + 1) * 8, hipMemcpyHostToDevice, s));
    GBM_TRY(launch_predict((const double*)cx.Xt.p, npad, p, n, (const double*)cx.pb.p, p + 1, 1, (double*)cx.part.p,
                           nchunks, (double*)cx.pout.p, npad, s));
    GBM_HIP_TRY(hipMemcpyAsync(y_pred_out, cx.pout.p, n * 8, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
  }
  return GBM_OK;
}

extern "C" int gbm_brr_fit(const double* X, int64_t n, int64_t p, int64_t ldx, const double* y, int64_t n_iter,
                           int64_t n_burnin, int64_t thin, double r2, double df0, uint64_t seed, int device,
                           double* b_hat_out, double* y_pred_out, double* var_out) {
  using namespace gbm;
  RoctxRange r_("gbm_brr_fit");
  set_error("");  // rc 0 with a non-empty gbm_last_error() reports a fall-back (below)
  if (!X || !y || !b_hat_out || n < 3 || p < 1 || ldx < n || n_iter < 1 || n_burnin < 0 || thin < 1 ||
      !(r2 > 0.0 && r2 < 1.0) || !(df0 > 0.0))
    return fail(GBM_E_ARG, "gbm_brr_fit: bad arguments (n >= 3, p >= 1, ldx >= n, n_iter >= 1, n_burnin >= 0, "
                           "thin >= 1, 0 < r2 < 1, df0 > 0)");
  if (n_iter <= n_burnin || (n_iter / thin) <= (n_burnin / thin))
    return fail(GBM_E_ARG, "gbm_brr_fit: no post-burn-in sample (need a multiple of thin in (n_burnin, n_iter])");
  GBM_TRY(check_y(y, n, n, 1));
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  bool timeout = false;
  int rc = brr_fit_impl(X, n, p, ldx, y, n_iter, n_burnin, thin, r2, df0, seed, devs[0], -1, b_hat_out, y_pred_out,
                        var_out, &timeout);
  // a sweep whose workgroups could not all be resident (another process or library filling the
  // device) times out loudly on the device; the fit is then run again, from the start, on the
  // per-launch path (same chain; the two paths agree to rounding). The call still returns GBM_OK —
  // the results are valid — but says so: gbm_last_error() holds the warning (the Python mirror
  // raises a RuntimeWarning, the Julia binding an @warn) and gbm_debug_brr_stats counts it.
  if (rc != GBM_OK && timeout) {
    g_brr_fallbacks.fetch_add(1);
    rc = brr_fit_impl(X, n, p, ldx, y, n_iter, n_burnin, thin, r2, df0, seed, devs[0], 0, b_hat_out, y_pred_out,
                      var_out, &timeout);
    if (rc == GBM_OK)
      set_error("warning: gbm_brr_fit: the persistent super-block sweep timed out (were all its workgroups resident? "
                "another process may share the device); the fit was re-run on the per-launch path");
  }
  return rc;
}

// One BayesA / BayesB / BayesC fit on a leased context (include/gbm.h gbm_bayes_fit): the setup of
// brr_fit_impl (genotypes, column statistics, byte quantisation, Gram blocks), then per iteration
// the linear chain prep, μ, block 0's partial dots, one chain launch per 64-marker block, the
// variances — captured once as a graph and replayed. Never the super-block sweep or its lock; the
// BRR path statistics are not written.
static int bayes_fit_impl(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                          int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                          double counts, uint64_t seed, int dev, double* b_hat_out, double* y_pred_out,
                          double* var_out, double* pip_out) {
  using namespace gbm;
  BrrLease lease;
  GBM_TRY(brr_pool().acquire(dev, lease.c));
  BrrCtx& cx = *lease.c;
  GBM_HIP_TRY(hipSetDevice(dev));
  hipStream_t s = cx.stream.s;
  const int64_t npad = round_up(n, IW);
  const int64_t C64 = (n + IW - 1) / IW;
  const int64_t nblk = (p + BB - 1) / BB, ppad = nblk * BB;
  const int64_t nvb = (std::max(n, p) + 255) / 256;
  GBM_TRY(ensure(cx.Xt, dev, p * npad * 8));
  GBM_TRY(ensure(cx.colmean, dev, p * 8));
  GBM_TRY(ensure(cx.x2, dev, p * 8));
  GBM_TRY(ensure(cx.e, dev, npad * 8));
  GBM_TRY(ensure(cx.b, dev, 2 * p * 8));  // two copies (iteration parity), as are the indicators
  GBM_TRY(ensure(cx.dind, dev, 2 * p * 8));
  GBM_TRY(ensure(cx.bbar, dev, p * 8));
  GBM_TRY(ensure(cx.dbar, dev, p * 8));
  GBM_TRY(ensure(cx.varBj, dev, p * 8));
  GBM_TRY(ensure(cx.pk, dev, ppad * 8 * 8));
  GBM_TRY(ensure(cx.vpart, dev, nvb * 5 * 8));
  GBM_TRY(ensure(cx.r, dev, 2 * C64 * BK2 * 8));  // ping-pong partial dots (BRR's size: one buffer, one pointer)
  GBM_TRY(ensure(cx.bst, dev, sizeof(BayesState)));
  GBM_TRY(ensure(cx.W, dev, nblk * BB * BB * 8));
  GBM_HIP_TRY(hipMemsetAsync(cx.Xt.p, 0, (size_t)(p * npad * 8), s));
  GBM_HIP_TRY(hipMemcpy2DAsync(cx.Xt.p, npad * 8, X, ldx * 8, n * 8, p, hipMemcpyHostToDevice, s));
  brr_colstats_kernel<<<(unsigned)std::min<int64_t>(p, 4096), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n,
                                                                           (double*)cx.colmean.p, (double*)cx.x2.p);
  GBM_LAUNCH_CHECK();
  std::vector<double> cm(p), xx(p);
  GBM_HIP_TRY(hipMemcpyAsync(cm.data(), cx.colmean.p, p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(xx.data(), cx.x2.p, p * 8, hipMemcpyDeviceToHost, s));
  // byte storage when X = D/s exactly, as brr_fit_impl (GBM_BRR_I8=0 keeps fp64 storage)
  double xs = 0.0;
  {
    const char* ev = ::gbm::knob("GBM_BRR_I8");
    if (!(ev && ev[0] == '0')) {
      GBM_TRY(ensure(cx.D, dev, p * npad + 4096));
      GBM_TRY(ensure(cx.badm, dev, sizeof(int)));
      const double scales[3] = {2.0, 4.0, 1.0};
      for (double sc : scales) {
        int nbad = -1;
        GBM_HIP_TRY(hipMemsetAsync(cx.badm.p, 0, sizeof(int), s));
        brr_quantize_kernel<<<2048, 256, 0, s>>>((const double*)cx.Xt.p, p * npad, sc, (uint8_t*)cx.D.p, (int*)cx.badm.p);
        GBM_LAUNCH_CHECK();
        GBM_HIP_TRY(hipMemcpyAsync(&nbad, cx.badm.p, sizeof(int), hipMemcpyDeviceToHost, s));
        GBM_HIP_TRY(hipStreamSynchronize(s));
        if (nbad == 0) {
          xs = 1.0 / sc;
          break;
        }
      }
    }
  }
  brr_gram_kernel<<<(unsigned)nblk, 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n, 1, (double*)cx.W.p);
  GBM_LAUNCH_CHECK();
  GBM_HIP_TRY(hipStreamSynchronize(s));
  double ym = 0.0;
  for (int64_t i = 0; i < n; i++) ym += y[i];
  ym /= (double)n;
  double vy = 0.0;
  for (int64_t i = 0; i < n; i++) vy += (y[i] - ym) * (y[i] - ym);
  vy /= (double)(n - 1);
  double msx = 0.0, smsq = 0.0;
  for (int64_t j = 0; j < p; j++) {
    msx += xx[j];
    smsq += cm[j] * cm[j];
  }
  msx = msx / (double)n - smsq;
  if (!(msx > 0.0)) return fail(GBM_E_DATA, "gbm_bayes_fit: the markers have no variance");
  const double shape0 = 1.1;
  double S0 = vy * r2 / msx * (df0 + 2.0);
  if (model != GBM_MODEL_A) S0 /= prob_in;
  BayesState st0{};
  st0.mu = ym;
  st0.S0e = vy * (1.0 - r2) * (df0 + 2.0);
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
  std::vector<double> e0(npad, 0.0);
  for (int64_t i = 0; i < n; i++) e0[i] = y[i] - ym;
  std::vector<double> init(2 * p, 1.0);  // d = 1; then varB_j = S0/(df0 + 2)
  GBM_HIP_TRY(hipMemcpyAsync(cx.e.p, e0.data(), npad * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.dind.p, init.data(), 2 * p * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  std::fill(init.begin(), init.begin() + p, st0.varBc);
  GBM_HIP_TRY(hipMemcpyAsync(cx.varBj.p, init.data(), p * 8, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.b.p, 0, 2 * p * 8, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.bbar.p, 0, p * 8, s));
  GBM_HIP_TRY(hipMemsetAsync(cx.dbar.p, 0, p * 8, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.bst.p, &st0, sizeof(BayesState), hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  auto* stp = (BayesState*)cx.bst.p;
  const unsigned C = (unsigned)C64;
  auto enqueue_iteration = [&]() -> int {
    bayes_prep_kernel<<<(unsigned)(ppad / 256 + 1), 256, 0, s>>>(p, ppad, (const double*)cx.x2.p, (const double*)cx.b.p,
                                                                 (const double*)cx.dind.p, (const double*)cx.varBj.p, stp,
                                                                 (double*)cx.pk.p);
    bayes_mu_kernel<<<1, 1024, 0, s>>>((double*)cx.e.p, n, stp);
    if (xs > 0.0)
      brr_dots0_kernel<uint8_t><<<C, 256, 0, s>>>((const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.e.p,
                                                  (double*)cx.r.p);
    else
      brr_dots0_kernel<double><<<C, 256, 0, s>>>((const double*)cx.Xt.p, npad, n, p, 1.0, (const double*)cx.e.p,
                                                 (double*)cx.r.p);
    for (int64_t k = 0; k < nblk; k++) {
      double* pin = (double*)cx.r.p + (k & 1) * (int64_t)C * BB;
      double* pout = (double*)cx.r.p + ((k + 1) & 1) * (int64_t)C * BB;
      if (xs > 0.0)
        bayes_chain_kernel<uint8_t><<<C, 256, 0, s>>>((const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.W.p, k,
                                                      nblk, pin, pout, (const double*)cx.pk.p, (double*)cx.b.p,
                                                      (double*)cx.dind.p, (double*)cx.bbar.p, (double*)cx.dbar.p,
                                                      (double*)cx.e.p, stp);
      else
        bayes_chain_kernel<double><<<C, 256, 0, s>>>((const double*)cx.Xt.p, npad, n, p, 1.0, (const double*)cx.W.p, k,
                                                     nblk, pin, pout, (const double*)cx.pk.p, (double*)cx.b.p,
                                                     (double*)cx.dind.p, (double*)cx.bbar.p, (double*)cx.dbar.p,
                                                     (double*)cx.e.p, stp);
    }
    bayes_var_kernel<<<(unsigned)nvb, 256, 0, s>>>((const double*)cx.b.p, (const double*)cx.dind.p, (double*)cx.varBj.p, p,
                                                   (const double*)cx.e.p, n, stp, (double*)cx.vpart.p);
    bayes_final_kernel<<<1, 256, 0, s>>>((const double*)cx.vpart.p, nvb, p, n, stp);
    return hipGetLastError() == hipSuccess ? GBM_OK : fail(GBM_E_HIP, "gbm_bayes_fit: launch failed");
  };
  const std::vector<int64_t> key = {model, n, p, npad, (int64_t)(xs * 64.0),
                                    (int64_t)(uintptr_t)cx.Xt.p, (int64_t)(uintptr_t)cx.D.p, (int64_t)(uintptr_t)cx.W.p,
                                    (int64_t)(uintptr_t)cx.r.p, (int64_t)(uintptr_t)cx.e.p, (int64_t)(uintptr_t)cx.b.p,
                                    (int64_t)(uintptr_t)cx.dind.p, (int64_t)(uintptr_t)cx.bbar.p,
                                    (int64_t)(uintptr_t)cx.dbar.p, (int64_t)(uintptr_t)cx.varBj.p,
                                    (int64_t)(uintptr_t)cx.pk.p, (int64_t)(uintptr_t)cx.vpart.p,
                                    (int64_t)(uintptr_t)cx.x2.p, (int64_t)(uintptr_t)cx.bst.p};
  int rc = GBM_OK;
  if (cx.bayes_key != key) {
    cx.drop_bayes_graph();
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      rc = enqueue_iteration();
      if (hipStreamEndCapture(s, &cx.bayes_graph) != hipSuccess || rc != GBM_OK ||
          hipGraphInstantiate(&cx.bayes_exec, cx.bayes_graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        cx.drop_bayes_graph();
        rc = GBM_OK;  // fall back to direct launches (same kernels, same order)
      } else {
        cx.bayes_key = key;
      }
    }
  }
  for (int64_t it = 0; it < n_iter && rc == GBM_OK; it++) {
    if (cx.bayes_exec) {
      if (hipGraphLaunch(cx.bayes_exec, s) != hipSuccess) rc = fail(GBM_E_HIP, "gbm_bayes_fit: graph launch failed");
    } else {
      rc = enqueue_iteration();
    }
  }
  if (rc != GBM_OK) return rc;
  GBM_HIP_TRY(hipStreamSynchronize(s));
  BayesState fin{};
  GBM_HIP_TRY(hipMemcpyAsync(&fin, cx.bst.p, sizeof(BayesState), hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(b_hat_out + 1, cx.bbar.p, p * 8, hipMemcpyDeviceToHost, s));
  if (pip_out) GBM_HIP_TRY(hipMemcpyAsync(pip_out, cx.dbar.p, p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  b_hat_out[0] = fin.mubar;
  if (var_out) {
    var_out[0] = fin.varEbar;
    var_out[1] = fin.varBbar;
    var_out[2] = fin.pibar;
  }
  if (y_pred_out) {
    const int64_t nchunks = predict_chunks(n, p);
    GBM_TRY(ensure(cx.pb, dev, (p + 1) * 8));
    GBM_TRY(ensure(cx.part, dev, nchunks * npad * 8));
    GBM_TRY(ensure(cx.pout, dev, npad * 8));
    GBM_HIP_TRY(hipMemcpyAsync(cx.pb.p, b_hat_out, (p + 1) * 8, hipMemcpyHostToDevice, s));
    GBM_TRY(launch_predict((const double*)cx.Xt.p, npad, p, n, (const double*)cx.pb.p, p + 1, 1, (double*)cx.part.p,
                           nchunks, (double*)cx.pout.p, npad, s));
    GBM_HIP_TRY(hipMemcpyAsync(y_pred_out, cx.pout.p, n * 8, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
  }
  return GBM_OK;
}

extern "C" int gbm_bayes_fit(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                             int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                             double counts, uint64_t seed, int device, double* b_hat_out, double* y_pred_out,
                             double* var_out, double* pip_out) {
  using namespace gbm;
  RoctxRange r_("gbm_bayes_fit");
  set_error("");
  if (model != GBM_BAYES_A && model != GBM_BAYES_B && model != GBM_BAYES_C)
    return fail(GBM_E_ARG, "gbm_bayes_fit: model must be GBM_BAYES_A, GBM_BAYES_B or GBM_BAYES_C");
  if (!X || !y || !b_hat_out || n < 3 || p < 1 || ldx < n || n_iter < 1 || n_burnin < 0 || thin < 1 ||
      !(r2 > 0.0 && r2 < 1.0) || !(df0 > 0.0))
    return fail(GBM_E_ARG, "gbm_bayes_fit: bad arguments (n >= 3, p >= 1, ldx >= n, n_iter >= 1, n_burnin >= 0, "
                           "thin >= 1, 0 < r2 < 1, df0 > 0)");
  // the gamma sampler (Marsaglia-Tsang) needs shapes >= 1: (df0 + 1)/2 of the per-marker variances
  // and counts·prob_in, counts·(1 − prob_in) of π's Beta draw
  if (!(df0 >= 1.0) || !(prob_in > 0.0 && prob_in < 1.0) || !(counts * prob_in >= 1.0) ||
      !(counts * (1.0 - prob_in) >= 1.0))
    return fail(GBM_E_ARG, "gbm_bayes_fit: bad prior (df0 >= 1, 0 < prob_in < 1, counts*prob_in >= 1, "
                           "counts*(1 - prob_in) >= 1)");
  // the per-marker random streams are (iteration, marker) packed into 23 + 40 bits
  if (n_iter > ((int64_t)1 << 23) || p >= ((int64_t)1 << 40))
    return fail(GBM_E_ARG, "gbm_bayes_fit: n_iter <= 2^23 and p < 2^40");
  if (n_iter <= n_burnin || (n_iter / thin) <= (n_burnin / thin))
    return fail(GBM_E_ARG, "gbm_bayes_fit: no post-burn-in sample (need a multiple of thin in (n_burnin, n_iter])");
  GBM_TRY(check_y(y, n, n, 1));
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  return bayes_fit_impl(model, X, n, p, ldx, y, n_iter, n_burnin, thin, r2, df0, prob_in, counts, seed, devs[0],
                        b_hat_out, y_pred_out, var_out, pip_out);
}
