// Kernels of the epistasis feature scan (driver: gbm_session_pair_scan, session_pairscan.cpp): the
// slope of the simple regression y ~ [1, f(x_i, x_j)] for every ordered pair of loci (reference transform2,
// src/transformation.jl:319-468) or f(x_j) for every locus (transform1, :130-238), and the K largest |slope|.
//
//   pair_prep_kernel   gathers the training rows and the chosen loci of the resident Xt into the compact
//                      locus-major work matrix W (+ ε, abs on request), with each locus' ddof-1 variance and its
//                      skip flag, and writes yc = y − ȳ
//   pair_scan_kernel   one workgroup per 64 x 64 tile of pairs, a 4 x 4 register tile of pairs per thread; three
//                      running sums per pair over the n_train individuals, then the slope
//   sel_*              radix select of the K-th largest |slope| bit pattern over a panel of slopes, then an
//                      ordered compaction (ties to the lower flat index)
//
// One thread owns a pair for the whole individual range and adds its terms in the order k = 0, 1, …: a pair's
// slope depends on its two columns and on yc only, never on the pair's place in the grid. The counters are
// integers (atomic adds commute), so two calls give the same bits.
#include <cfloat>
#include <cstring>

#include "gbm_internal.h"

namespace gbm {

namespace {

constexpr int kPT = 64;   // tile side (loci)
constexpr int kPK = 32;   // individuals per staged chunk
constexpr int kPL = 66;   // LDS pitch of a chunk row (64 loci + 2: 16-byte aligned rows, staggered banks)
constexpr int kSelChunk = 4096;  // slopes per workgroup of the ordered compaction
constexpr int kSelHistBlocks = 1024;

template <int OP>
__device__ __forceinline__ double pair_f(double a, double b) {
#pragma clang fp contract(off)
  if (OP == GBM_PAIR_OP_MULT) return a * b;
  if (OP == GBM_PAIR_OP_ADDNORM) return (a + b) / 2.0;
  if (OP == GBM_PAIR_OP_RAISE) return pow(a, b);
  if (OP == GBM_PAIR_OP_SQUARE) return b * b;
  if (OP == GBM_PAIR_OP_INVONEPLUS) return 1.0 / (1.0 + b);
  return log10(b + DBL_EPSILON) / log10(DBL_EPSILON);  // GBM_PAIR_OP_LOG10EPS
}

__device__ __forceinline__ double block_sum(double v, double* red) {  // fixed order: lane tree, then the 4 waves
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// One workgroup per chosen locus j: W[j, k] = Xt[loci[j], idx[k]] + eps (abs on request) for k < n, zeros on the
// padding [n, ldw); var[j] = the ddof-1 variance of the row (two passes); skip[j] = var < var_threshold.
// Workgroup 0 also writes yc = y − ybar (zeros on the padding).
__global__ void __launch_bounds__(256) pair_prep_kernel(const double* __restrict__ Xt, int64_t ldx,
                                                        const int64_t* __restrict__ idx, int64_t n,
                                                        const int64_t* __restrict__ loci, double eps, int use_abs,
                                                        double var_threshold, const double* __restrict__ y, double ybar,
                                                        double* __restrict__ W, int64_t ldw, double* __restrict__ var,
                                                        int32_t* __restrict__ skip, double* __restrict__ yc) {
  __shared__ double red[256];
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x;
  const double* x = Xt + (loci ? loci[j] : j) * ldx;
  double* w = W + j * ldw;
  double s = 0.0;
  for (int64_t k = tid; k < ldw; k += 256) {
    double v = 0.0;
    if (k < n) {
      v = x[idx[k]] + eps;
      if (use_abs) v = fabs(v);
      s += v;
    }
    w[k] = v;
  }
  const double mean = block_sum(s, red) / (double)n;
  double ss = 0.0;
  for (int64_t k = tid; k < n; k += 256) {  // each thread re-reads what it wrote
    const double d = w[k] - mean;
    ss += d * d;
  }
  const double v = block_sum(ss, red) / (double)(n - 1);
  if (tid == 0) {
    var[j] = v;
    skip[j] = v < var_threshold ? 1 : 0;
  }
  if (j == 0)
    for (int64_t k = tid; k < ldw; k += 256) yc[k] = k < n ? y[k] - ybar : 0.0;
}

// Slopes of the pairs (i, j), i in [i0, i0 + rows), j in [0, l): beta[(i − i0)·l + j]. Grid (ceil(l/64), rows/64
// rounded up). Thread (tx, ty) = (tid & 15, tid >> 4) owns i = tile_i + 4ty + a, j = tile_j + 4tx + b.
// Unary operations: li = 1 (one row of "pairs", f ignores its first argument and no i-row is loaded).
// cnt[0] tested pairs, cnt[1] degenerate pairs, cnt[2] pairs with a non-finite sum or slope.
// Loci past l are staged as 1.0 and their pairs are discarded (never stored, never counted); individuals past n
// are never read: the k loop of the last chunk stops at n.
template <int OP>
__global__ void __launch_bounds__(256) pair_scan_kernel(const double* __restrict__ W, int64_t ldw, int64_t n, int64_t l,
                                                        int64_t li, int64_t i0, const double* __restrict__ yc,
                                                        const int32_t* __restrict__ skip, int commutative,
                                                        double* __restrict__ beta,
                                                        unsigned long long* __restrict__ cnt) {
#pragma clang fp contract(off)
  constexpr bool unary = OP >= GBM_PAIR_OP_SQUARE;
  __shared__ __attribute__((aligned(16))) double As[kPK][kPL];
  __shared__ __attribute__((aligned(16))) double Bs[kPK][kPL];
  __shared__ double ys[kPK];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t ti = i0 + (int64_t)blockIdx.y * kPT, tj = (int64_t)blockIdx.x * kPT;
  double* out = beta + ((int64_t)blockIdx.y * kPT) * l;
  if (commutative && tj + kPT - 1 < ti) {  // the whole tile has j < i
    for (int a = 0; a < 4; a++)
      for (int b = 0; b < 4; b++) {
        const int64_t i = ti + 4 * ty + a, j = tj + 4 * tx + b;
        if (i < li && j < l) out[(int64_t)(4 * ty + a) * l + j] = 0.0;
      }
    return;
  }
  double s1[4][4], s2[4][4], s3[4][4], c[4][4];
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++) s1[a][b] = s2[a][b] = s3[a][b] = c[a][b] = 0.0;
  double sy = 0.0;  // Σ yc as rounded, in the pairs' own order
  const int lk = tid & 31, lr = tid >> 5;
  for (int64_t k0 = 0; k0 < n; k0 += kPK) {
    const int kc = (int)(n - k0 < kPK ? n - k0 : kPK);
    __syncthreads();
    for (int q = 0; q < 8; q++) {
      const int r = lr + 8 * q;
      double va = 1.0, vb = 1.0;
      if (lk < kc) {
        if (!unary && ti + r < l) va = W[(ti + r) * ldw + k0 + lk];
        if (tj + r < l) vb = W[(tj + r) * ldw + k0 + lk];
      }
      As[lk][r] = va;
      Bs[lk][r] = vb;
    }
    if (tid < kPK) ys[tid] = tid < kc ? yc[k0 + tid] : 0.0;
    __syncthreads();
    if (k0 == 0) {  // the shift: the pair's mean f over the first chunk (k < 32), summed in the order k = 0, 1, …
      for (int kk = 0; kk < kc; kk++)
        for (int a = 0; a < 4; a++)
          for (int b = 0; b < 4; b++) c[a][b] += pair_f<OP>(As[kk][4 * ty + a], Bs[kk][4 * tx + b]);
      for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) c[a][b] /= (double)kc;
    }
    for (int kk = 0; kk < kc; kk++) {
      double av[4], bv[4];
      for (int a = 0; a < 4; a++) av[a] = As[kk][4 * ty + a];
      for (int b = 0; b < 4; b++) bv[b] = Bs[kk][4 * tx + b];
      const double yk = ys[kk];
      sy += yk;
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const double d = pair_f<OP>(av[a], bv[b]) - c[a][b];
          s1[a][b] += d;
          s2[a][b] = __builtin_fma(d, d, s2[a][b]);
          s3[a][b] = __builtin_fma(d, yk, s3[a][b]);
        }
    }
  }
  const double nn = (double)n;
  const double thr = (2.0 * DBL_EPSILON) * (2.0 * DBL_EPSILON);
  unsigned tested = 0, degen = 0, bad = 0;
  for (int a = 0; a < 4; a++) {
    const int64_t i = ti + 4 * ty + a;
    if (i >= li) continue;
    const bool skip_i = !unary && skip[i];
    for (int b = 0; b < 4; b++) {
      const int64_t j = tj + 4 * tx + b;
      if (j >= l) continue;
      double bt = 0.0;
      if (!(skip_i || skip[j] || (commutative && j < i))) {
        tested++;
        const double S1 = s1[a][b], S2 = s2[a][b], cc = c[a][b];
        const double sff = S2 - S1 * S1 / nn;
        const double sf2 = S2 + 2.0 * cc * S1 + nn * cc * cc;
        const double m = sf2 > nn ? sf2 : nn;
        if (!isfinite(S1) || !isfinite(S2) || !isfinite(s3[a][b]) || !isfinite(sf2)) {
          bad++;
        } else if (nn * sff <= thr * m * m) {
          degen++;
        } else {
          // S_fy = Σ(f − f̄)·yc: the residual Σyc of the rounded yc enters with no factor at all
          bt = (s3[a][b] - S1 / nn * sy) / sff;
          if (!isfinite(bt)) {
            bad++;
            bt = 0.0;
          }
        }
      }
      out[(int64_t)(4 * ty + a) * l + j] = bt;
    }
  }
  // integer counters: wave sums, then one atomic add per wave and counter
  for (int off = 32; off > 0; off >>= 1) {
    tested += __shfl_down(tested, off);
    degen += __shfl_down(degen, off);
    bad += __shfl_down(bad, off);
  }
  if ((tid & 63) == 0) {
    if (tested) atomicAdd(&cnt[0], (unsigned long long)tested);
    if (degen) atomicAdd(&cnt[1], (unsigned long long)degen);
    if (bad) atomicAdd(&cnt[2], (unsigned long long)bad);
  }
}

// ---- selection --------------------------------------------------------------------------------------------------
// |beta| >= 0, so its bit pattern orders as an unsigned integer. Candidates are the slopes with key > epskey
// (|beta| > ε). SelState: the radix select's running prefix, then the compaction's thresholds.
struct SelState {
  unsigned long long prefix, mask;  // the bits of the K-th key fixed so far
  long long krem;                   // rank still to find among the keys that match the prefix
  long long greater;                // candidates above the matched prefix
  int all;                          // fewer than K candidates: every candidate is selected
  int pad;
};

__device__ __forceinline__ unsigned long long abs_key(double v) {
  return (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
}

__global__ void sel_init_kernel(SelState* st, unsigned long long* hist, long long k) {
  if (threadIdx.x == 0) {
    st->prefix = st->mask = 0;
    st->krem = k;
    st->greater = 0;
    st->all = 0;
    st->pad = 0;
  }
  hist[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256) sel_hist_kernel(const double* __restrict__ beta, int64_t m,
                                                       unsigned long long epskey, int shift,
                                                       const SelState* __restrict__ st,
                                                       unsigned long long* __restrict__ hist) {
  __shared__ unsigned h[256];
  if (st->all) return;
  const unsigned long long prefix = st->prefix, mask = st->mask;
  h[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
    const unsigned long long key = abs_key(beta[e]);
    if (key > epskey && (key & mask) == prefix) atomicAdd(&h[(key >> shift) & 255], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// One workgroup: walks the 256 bins from the top to the one that holds rank krem, fixes that byte and clears hist.
__global__ void sel_pick_kernel(SelState* st, unsigned long long* hist, int shift) {
  __shared__ unsigned long long h[256];
  h[threadIdx.x] = hist[threadIdx.x];
  hist[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x != 0 || st->all) return;
  long long acc = 0, krem = st->krem;
  int bin = 255;
  for (; bin >= 0; bin--) {
    if (acc + (long long)h[bin] >= krem) break;
    acc += (long long)h[bin];
  }
  if (bin < 0) {  // only in the first pass: fewer candidates than K
    st->all = 1;
    st->greater = acc;
    return;
  }
  st->greater += acc;
  st->krem = krem - acc;
  st->prefix |= (unsigned long long)bin << shift;
  st->mask |= 255ull << shift;
}

// Per workgroup b (slopes [b·4096, (b + 1)·4096) of the panel): the counts of keys above and equal to the K-th key.
__global__ void __launch_bounds__(256) sel_count_kernel(const double* __restrict__ beta, int64_t m,
                                                        unsigned long long epskey, const SelState* __restrict__ st,
                                                        long long* __restrict__ cnt) {
  __shared__ int g[256], q[256];
  const unsigned long long T = st->all ? epskey : st->prefix;
  const bool all = st->all;
  const int64_t e0 = (int64_t)blockIdx.x * kSelChunk;
  int ng = 0, nq = 0;
  for (int t = threadIdx.x; t < kSelChunk; t += 256) {
    const int64_t e = e0 + t;
    if (e >= m) break;
    const unsigned long long key = abs_key(beta[e]);
    if (key > epskey) {
      ng += key > T;
      nq += !all && key == T;
    }
  }
  g[threadIdx.x] = ng;
  q[threadIdx.x] = nq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      g[threadIdx.x] += g[threadIdx.x + s];
      q[threadIdx.x] += q[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    cnt[2 * (int64_t)blockIdx.x] = g[0];
    cnt[2 * (int64_t)blockIdx.x + 1] = q[0];
  }
}

// One workgroup: cnt[2b], cnt[2b + 1] become the exclusive prefix sums over the nb workgroups; tot[0], tot[1] the totals.
__global__ void __launch_bounds__(256) sel_scan_kernel(long long* __restrict__ cnt, int64_t nb, long long* __restrict__ tot) {
  __shared__ long long pg[256], pq[256];
  const int tid = threadIdx.x;
  const int64_t per = (nb + 255) / 256, b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
  long long sg = 0, sq = 0;
  for (int64_t b = b0; b < b1; b++) {
    sg += cnt[2 * b];
    sq += cnt[2 * b + 1];
  }
  pg[tid] = sg;
  pq[tid] = sq;
  __syncthreads();
  if (tid == 0) {
    long long ag = 0, aq = 0;
    for (int t = 0; t < 256; t++) {
      const long long vg = pg[t], vq = pq[t];
      pg[t] = ag;
      pq[t] = aq;
      ag += vg;
      aq += vq;
    }
    tot[0] = ag;
    tot[1] = aq;
  }
  __syncthreads();
  long long ag = pg[tid], aq = pq[tid];
  for (int64_t b = b0; b < b1; b++) {
    const long long vg = cnt[2 * b], vq = cnt[2 * b + 1];
    cnt[2 * b] = ag;
    cnt[2 * b + 1] = aq;
    ag += vg;
    aq += vq;
  }
}

// Ordered compaction: the keys above the K-th key go to slots [0, G) in flat-index order, the keys equal to it to
// [G, K) in flat-index order (the first K − G of them). cand_idx holds base + the panel-local flat index.
__global__ void __launch_bounds__(256) sel_write_kernel(const double* __restrict__ beta, int64_t m, int64_t base,
                                                        unsigned long long epskey, int64_t k,
                                                        const SelState* __restrict__ st,
                                                        const long long* __restrict__ cnt,
                                                        const long long* __restrict__ tot,
                                                        int64_t* __restrict__ cand_idx, double* __restrict__ cand_beta) {
  __shared__ int wg[4], wq[4];
  const unsigned long long T = st->all ? epskey : st->prefix;
  const bool all = st->all;
  const long long G = tot[0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long og = cnt[2 * (int64_t)blockIdx.x], oq = cnt[2 * (int64_t)blockIdx.x + 1];
  const int64_t e0 = (int64_t)blockIdx.x * kSelChunk;
  for (int t0 = 0; t0 < kSelChunk; t0 += 256) {
    if (e0 + t0 >= m) break;  // uniform
    const int64_t e = e0 + t0 + tid;
    double v = 0.0;
    bool fg = false, fq = false;
    if (e < m) {
      v = beta[e];
      const unsigned long long key = abs_key(v);
      if (key > epskey) {
        fg = key > T;
        fq = !all && key == T;
      }
    }
    const unsigned long long bg = __ballot(fg), bq = __ballot(fq);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int rg = __popcll(bg & below), rq = __popcll(bq & below);
    __syncthreads();
    if (lane == 0) {
      wg[wave] = __popcll(bg);
      wq[wave] = __popcll(bq);
    }
    __syncthreads();
    int pg = 0, pq = 0, tg = 0, tq = 0;
    for (int w = 0; w < 4; w++) {
      if (w < wave) {
        pg += wg[w];
        pq += wq[w];
      }
      tg += wg[w];
      tq += wq[w];
    }
    if (fg) {
      const long long slot = og + pg + rg;
      if (slot < k) {
        cand_idx[slot] = base + e;
        cand_beta[slot] = v;
      }
    }
    if (fq) {
      const long long slot = G + oq + pq + rq;
      if (slot < k) {
        cand_idx[slot] = base + e;
        cand_beta[slot] = v;
      }
    }
    og += tg;
    oq += tq;
  }
}

template <int OP>
int launch_scan_op(const double* W, int64_t ldw, int64_t n, int64_t l, int64_t li, int64_t i0, int64_t rows,
                   const double* yc, const int32_t* skip, int commutative, double* beta, unsigned long long* cnt,
                   hipStream_t s) {
  const dim3 grid((unsigned)((l + kPT - 1) / kPT), (unsigned)((rows + kPT - 1) / kPT));
  hipLaunchKernelGGL(pair_scan_kernel<OP>, grid, dim3(256), 0, s, W, ldw, n, l, li, i0, yc, skip, commutative, beta, cnt);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

}  // namespace

int64_t pair_scan_ldw(int64_t n) { return round_up(n, 32); }
int64_t pair_sel_blocks(int64_t m) { return (m + kSelChunk - 1) / kSelChunk; }
int64_t pair_sel_state_bytes() { return (int64_t)sizeof(SelState) + 256 * 8 + 2 * 8; }

int launch_pair_prep(const double* Xt, int64_t ldx, const int64_t* idx, int64_t n, const int64_t* loci, int64_t l,
                     double eps, int use_abs, double var_threshold, const double* y, double ybar, double* W,
                     int64_t ldw, double* var, int32_t* skip, double* yc, hipStream_t s) {
  hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)l), dim3(256), 0, s, Xt, ldx, idx, n, loci, eps, use_abs,
                     var_threshold, y, ybar, W, ldw, var, skip, yc);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

int launch_pair_scan(int op, const double* W, int64_t ldw, int64_t n, int64_t l, int64_t li, int64_t i0, int64_t rows,
                     const double* yc, const int32_t* skip, int commutative, double* beta, unsigned long long* cnt,
                     hipStream_t s) {
  switch (op) {
    case GBM_PAIR_OP_MULT: return launch_scan_op<GBM_PAIR_OP_MULT>(W, ldw, n, l, li, i0, rows, yc, skip, commutative, beta, cnt, s);
    case GBM_PAIR_OP_ADDNORM: return launch_scan_op<GBM_PAIR_OP_ADDNORM>(W, ldw, n, l, li, i0, rows, yc, skip, commutative, beta, cnt, s);
    case GBM_PAIR_OP_RAISE: return launch_scan_op<GBM_PAIR_OP_RAISE>(W, ldw, n, l, li, i0, rows, yc, skip, commutative, beta, cnt, s);
    case GBM_PAIR_OP_SQUARE: return launch_scan_op<GBM_PAIR_OP_SQUARE>(W, ldw, n, l, li, i0, rows, yc, skip, commutative, beta, cnt, s);
    case GBM_PAIR_OP_INVONEPLUS: return launch_scan_op<GBM_PAIR_OP_INVONEPLUS>(W, ldw, n, l, li, i0, rows, yc, skip, commutative, beta, cnt, s);
    case GBM_PAIR_OP_LOG10EPS: return launch_scan_op<GBM_PAIR_OP_LOG10EPS>(W, ldw, n, l, li, i0, rows, yc, skip, commutative, beta, cnt, s);
  }
  return fail(GBM_E_ARG, "pair scan: unknown operation");
}

// The (at most k) largest |beta| > eps of the m slopes of a panel, ties to the lower index: cand_idx / cand_beta
// slots [0, min(k, candidates)), unordered between the two groups' values (the host orders them). state:
// pair_sel_state_bytes(); cnt: 2·pair_sel_blocks(m) int64. *tot (device, 2 int64 at the end of state): the counts
// above and equal to the k-th key, for the host to derive the number of slots written.
int launch_pair_select(const double* beta, int64_t m, int64_t base, double eps, int64_t k, void* state, int64_t* cnt,
                       int64_t* cand_idx, double* cand_beta, hipStream_t s) {
  SelState* st = (SelState*)state;
  unsigned long long* hist = (unsigned long long*)((char*)state + sizeof(SelState));
  long long* tot = (long long*)(hist + 256);
  unsigned long long epskey;
  static_assert(sizeof(epskey) == sizeof(eps), "key width");
  memcpy(&epskey, &eps, 8);
  hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(256), 0, s, st, hist, (long long)k);
  GBM_LAUNCH_CHECK();
  const int64_t want = (m + 255) / 256;
  const unsigned hb = (unsigned)(want < kSelHistBlocks ? want : kSelHistBlocks);
  for (int shift = 56; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(sel_hist_kernel, dim3(hb), dim3(256), 0, s, beta, m, epskey, shift, st, hist);
    GBM_LAUNCH_CHECK();
    hipLaunchKernelGGL(sel_pick_kernel, dim3(1), dim3(256), 0, s, st, hist, shift);
    GBM_LAUNCH_CHECK();
  }
  const int64_t nb = pair_sel_blocks(m);
  hipLaunchKernelGGL(sel_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, beta, m, epskey, st, (long long*)cnt);
  GBM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(256), 0, s, (long long*)cnt, nb, tot);
  GBM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sel_write_kernel, dim3((unsigned)nb), dim3(256), 0, s, beta, m, base, epskey, k, st,
                     (const long long*)cnt, (const long long*)tot, cand_idx, cand_beta);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

}  // namespace gbm
