// Lasso / elastic-net paths by cyclic coordinate descent on an active set — DESIGN.md §4.10; the
// device side of gbm_session_enet_path (session_linear.cpp), which replaces the GLMNet.glmnetcv(alpha = 1)
// call of reference lasso (src/linear.jl:333-343).
//
// The active markers' centred rows are packed in admission order into Za (A x lda fp64 locus rows,
// lda a multiple of 256, zero past n). One coordinate-descent pass over them is one launch per
// 64-marker block (enet_chain_kernel): bayes_chain_kernel<double>'s skeleton (bayes_abc.hip, DESIGN.md
// §4.6.1) with the soft threshold as the step. A soft threshold is piecewise affine in r, not affine,
// so as there the block's 64 steps are no triangular solve: they run as a serial chain on wave 0 of
// every chunk workgroup, lane k holding r_k = x_kᵀe + x2_k b_k and column k of the block's Gram
// matrix, one lane broadcast per step. Everything is deterministic (fixed summation orders, no
// floating-point atomics): two runs give the same bits.
#include <algorithm>
#include <cmath>

#include "gbm_internal.h"

namespace gbm {
namespace {

constexpr int BB = 64;   // markers per block (one wave)
constexpr int IW = 256;  // individuals per chunk workgroup

__device__ __forceinline__ double enet_readlane(double v, int l) {
  union {
    double f;
    int i[2];
  } u;
  u.f = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], l);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], l);
  return u.f;
}

// sum over a 256-thread workgroup in a fixed order (red: 4 doubles of LDS)
__device__ __forceinline__ double enet_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// x2_j = Σ_i z_ji² of every locus row (one workgroup per row, grid-strided)
__global__ void __launch_bounds__(256) enet_x2_kernel(const double* __restrict__ Z, int64_t ldz, int64_t p, int64_t n,
                                                      double* __restrict__ x2) {
  __shared__ double red[4];
  for (int64_t j = blockIdx.x; j < p; j += gridDim.x) {
    const double* row = Z + j * ldz;
    double ss = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) ss = fma(row[i], row[i], ss);
    ss = enet_block_sum(ss, red);
    if (threadIdx.x == 0) x2[j] = ss;
  }
}

// Append the rows rows[0..cnt) of Z to Za at slots a0.. (zero past n) with their x2
__global__ void __launch_bounds__(256) enet_gather_kernel(const double* __restrict__ Z, int64_t ldz, int64_t n,
                                                          const int32_t* __restrict__ rows, int64_t a0,
                                                          const double* __restrict__ x2, double* __restrict__ Za,
                                                          int64_t lda, double* __restrict__ x2a) {
  const int64_t j = rows[blockIdx.x];
  const double* src = Z + j * ldz;
  double* dst = Za + (a0 + blockIdx.x) * lda;
  for (int64_t i = threadIdx.x; i < lda; i += 256) dst[i] = i < n ? src[i] : 0.0;
  if (threadIdx.x == 0) x2a[a0 + blockIdx.x] = x2[j];
}

// Gram blocks W[b] = X_BᵀX_B of the 64-marker blocks b = blk0 + blockIdx.x of the A packed rows
// (row-major 64 x 64, rows and columns past A zero); individuals in chunks of 64 through LDS. The
// individuals are split into gridDim.y slices of `slice` (a multiple of 64): slice y's sums go to
// part[(blockIdx.x gridDim.y + y)] and enet_gram_sum_kernel adds the slices in order (one slice:
// part = W + blk0 blocks, no second kernel).
__global__ void __launch_bounds__(256) enet_gram_kernel(const double* __restrict__ Za, int64_t lda, int64_t A,
                                                        int64_t n, int64_t blk0, int64_t slice,
                                                        double* __restrict__ part) {
  __shared__ double T[BB][BB + 1];
  const int64_t r0 = (blk0 + blockIdx.x) * BB;
  const int tid = threadIdx.x, a = tid >> 2, b0 = (tid & 3) * 16;
  const int64_t lo = (int64_t)blockIdx.y * slice, hi = lo + slice < n ? lo + slice : n;
  double acc[16];
#pragma unroll
  for (int u = 0; u < 16; u++) acc[u] = 0.0;
  for (int64_t k0 = lo; k0 < hi; k0 += BB) {
    for (int e = tid; e < BB * BB; e += 256) {
      const int r = e / BB, c = e % BB;
      T[r][c] = (r0 + r < A && k0 + c < hi) ? Za[(r0 + r) * lda + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < BB; k++) {
      const double xa = T[a][k];
#pragma unroll
      for (int u = 0; u < 16; u++) acc[u] = fma(xa, T[b0 + u][k], acc[u]);
    }
    __syncthreads();
  }
  double* out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * BB * BB + a * BB + b0;
#pragma unroll
  for (int u = 0; u < 16; u++) out[u] = acc[u];
}

// W[blk0 + blockIdx.x] = Σ_y part[blockIdx.x S + y], y ascending
__global__ void __launch_bounds__(256) enet_gram_sum_kernel(const double* __restrict__ part, int S, int64_t blk0,
                                                            double* __restrict__ W) {
  const double* src = part + (int64_t)blockIdx.x * S * BB * BB;
  double* dst = W + (blk0 + blockIdx.x) * BB * BB;
  for (int e = threadIdx.x; e < BB * BB; e += 256) {
    double v = 0.0;
    for (int y = 0; y < S; y++) v += src[(int64_t)y * BB * BB + e];
    dst[e] = v;
  }
}

// 1/den_a = 1/(x2_a + l2) of the active slots for this λ; 0 for a pinned column (x2 = 0) and past A
__global__ void __launch_bounds__(256) enet_prep_kernel(int64_t A, int64_t Apad, const double* __restrict__ x2a,
                                                        double l2, double* __restrict__ invden) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a >= Apad) return;
  double v = 0.0;
  if (a < A) {
    const double xx = x2a[a];
    if (xx > 0.0) v = 1.0 / (xx + l2);
  }
  invden[a] = v;
}

// partial[c][k] = Σ_{i in chunk c} x_{k,i} e_i of block 0's markers at the start of a pass
__global__ void __launch_bounds__(256) enet_dots0_kernel(const double* __restrict__ Za, int64_t lda, int64_t n,
                                                         int64_t A, const double* __restrict__ e,
                                                         double* __restrict__ partial) {
  __shared__ double es[IW];
  const int tid = threadIdx.x, k = tid >> 2, qt = tid & 3;
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  es[tid] = i0 + tid < n ? e[i0 + tid] : 0.0;
  __syncthreads();
  const int nb = (int)(A < BB ? A : BB);
  double s0 = 0.0, s1 = 0.0;
  if (k < nb) {
    const double* row = Za + (int64_t)k * lda + i0 + qt * 64;  // rows are zero past n up to lda (a multiple of IW)
#pragma unroll 8
    for (int u = 0; u < 64; u += 2) {
      const double2 v = *reinterpret_cast<const double2*>(row + u);
      s0 = fma(v.x, es[qt * 64 + u], s0);
      s1 = fma(v.y, es[qt * 64 + u + 1], s1);
    }
  }
  double s = s0 + s1;
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  if (qt == 0) partial[blockIdx.x * BB + k] = s;  // k >= nb writes 0
}

// One block of 64 active markers. d⁰ = Σ_c partial_in[c] (fixed order), r_k = d⁰_k + x2_k b_k; step
// s: every lane forms its soft-thresholded b_new and δ = b_old − b_new from its current r, lane s's
// δ is broadcast and the lanes k > s do r_k += δ_s W[s][k] (lane k holds W[·][k] with the entries
// s >= k zeroed, so a lane's r stops changing at its own step and its δ is formed again from it
// after the chain: same operands, same bits as the value it broadcast). Wave 0 of every workgroup
// runs the chain from identical inputs; then e += X_B δ on this workgroup's individuals and the next
// block's partial dots. Workgroup 0 stores b (into the other parity's copy: the other workgroups
// may still be reading this pass's) and the block's max_k x2_k δ_k²/n.
__global__ void __launch_bounds__(256) enet_chain_kernel(const double* __restrict__ Za, int64_t lda, int64_t n,
                                                         int64_t A, const double* __restrict__ W, int64_t blk,
                                                         int64_t nblk, const double* __restrict__ partial_in,
                                                         double* __restrict__ partial_out,
                                                         const double* __restrict__ x2a,
                                                         const double* __restrict__ invden,
                                                         const double* __restrict__ b_in, double* __restrict__ b_out,
                                                         double thr, double inv_n, double* __restrict__ blkmax,
                                                         double* __restrict__ e) {
  constexpr int RP = IW + 2;  // doubles (row pitch 2064 B, as bayes_chain_kernel)
  __shared__ __attribute__((aligned(16))) double Xn[BB * RP];
  __shared__ double delta[BB];
  __shared__ double es[IW];
  __shared__ double part4[4][BB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j0 = blk * BB;
  const int nb = (int)((A - j0) < BB ? (A - j0) : BB);
  const int C = (int)gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  const int64_t i = i0 + tid;  // < lda (a multiple of IW, C = lda / IW chunks at most)
  const bool more = blk + 1 < nblk;
  const int64_t j1 = j0 + BB;
  const int nb1 = more ? (int)((A - j1) < BB ? (A - j1) : BB) : 0;
  // (1) the next block's rows into LDS
  for (int q = wave; q < 2 * nb1; q += 4) {
    const int k = q >> 1, h = q & 1;
    const double* src = Za + (j1 + k) * lda + i0 + h * 128 + lane * 2;
    __builtin_amdgcn_global_load_lds((const void*)src, (void*)(Xn + k * RP + h * 128), 16, 0, 0);
  }
  // (2) this thread's 64 genotypes of the block (rows past A clamped; their δ = 0)
  double xv[BB];
#pragma unroll
  for (int s2 = 0; s2 < BB; s2++) xv[s2] = Za[(j0 + (s2 < nb ? s2 : 0)) * lda + i];
  const double e_old = e[i];
  // (3) wave 0's operands: column `lane` of W (= its row: W is symmetric) and the step constants
  // (the per-slot arrays are padded to whole blocks)
  double w[BB];
  double bold = 0.0, xx = 0.0, idn = 0.0;
  if (tid < 64) {
    const double* wr = W + (j0 + lane) * BB;
#pragma unroll
    for (int s = 0; s < BB; s += 2) {
      const double2 v = *reinterpret_cast<const double2*>(wr + s);
      w[s] = v.x;
      w[s + 1] = v.y;
    }
    bold = b_in[j0 + lane];
    xx = x2a[j0 + lane];
    idn = invden[j0 + lane];
  }
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
    double r = fma(xx, bold, d0);
#pragma unroll
    for (int s = 0; s < BB; s++) {
      const double t = fabs(r) - thr;
      const double bn = t > 0.0 ? copysign(t, r) * idn : 0.0;
      r = fma(enet_readlane(bold - bn, s), w[s], r);
    }
    const double t = fabs(r) - thr;
    const double bn = t > 0.0 ? copysign(t, r) * idn : 0.0;
    const double dl = bold - bn;
    delta[lane] = dl;
    if (blockIdx.x == 0) {
      b_out[j0 + lane] = bn;  // lanes past A: invden = 0, so 0
      double m = xx * dl * dl * inv_n;
      for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
      if (lane == 0) blkmax[blk] = m;
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

// out[0] = max over the pass's block maxima, out[1] = ‖e‖² (one workgroup, fixed order)
__global__ void __launch_bounds__(256) enet_reduce_kernel(const double* __restrict__ blkmax, int64_t nblk,
                                                          const double* __restrict__ e, int64_t n,
                                                          double* __restrict__ out) {
  __shared__ double red[4];
  __shared__ double mx[4];
  double m = 0.0, ss = 0.0;
  for (int64_t k = threadIdx.x; k < nblk; k += 256) m = fmax(m, blkmax[k]);
  for (int64_t i = threadIdx.x; i < n; i += 256) ss = fma(e[i], e[i], ss);
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = m;
  ss = enet_block_sum(ss, red);  // its barriers also publish mx
  if (threadIdx.x == 0) {
    out[0] = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
    out[1] = ss;
  }
}

}  // namespace

int64_t enet_lda(int64_t n) { return round_up(n < 1 ? 1 : n, IW); }

int launch_enet_x2(const double* Z, int64_t ldz, int64_t p, int64_t n, double* x2, hipStream_t s) {
  enet_x2_kernel<<<(unsigned)(p < 8192 ? p : 8192), 256, 0, s>>>(Z, ldz, p, n, x2);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

int launch_enet_gather(const double* Z, int64_t ldz, int64_t n, const int32_t* rows, int64_t a0, int64_t cnt,
                       const double* x2, double* Za, int64_t lda, double* x2a, hipStream_t s) {
  if (cnt < 1) return GBM_OK;
  enet_gather_kernel<<<(unsigned)cnt, 256, 0, s>>>(Z, ldz, n, rows, a0, x2, Za, lda, x2a);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

// slices of individuals per Gram block and blocks per launch (the partial sums' workspace)
int64_t enet_gram_slices(int64_t n) { return std::min<int64_t>(32, std::max<int64_t>(1, (n + 511) / 512)); }
int64_t enet_gram_workspace(int64_t n) { return enet_gram_slices(n) > 1 ? 16 * enet_gram_slices(n) * BB * BB * 8 : 16; }

int launch_enet_gram(const double* Za, int64_t lda, int64_t A, int64_t n, int64_t blk0, double* W, double* ws,
                     hipStream_t s) {
  const int64_t nblk = (A + BB - 1) / BB, S = enet_gram_slices(n);
  if (S == 1) {
    if (blk0 < nblk) enet_gram_kernel<<<dim3((unsigned)(nblk - blk0), 1), 256, 0, s>>>(Za, lda, A, n, blk0, n, W + blk0 * BB * BB);
  } else {
    const int64_t slice = round_up((n + S - 1) / S, BB);
    for (int64_t b = blk0; b < nblk; b += 16) {
      const unsigned cnt = (unsigned)std::min<int64_t>(16, nblk - b);
      enet_gram_kernel<<<dim3(cnt, (unsigned)S), 256, 0, s>>>(Za, lda, A, n, b, slice, ws);
      enet_gram_sum_kernel<<<cnt, 256, 0, s>>>(ws, (int)S, b, W);
    }
  }
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

int launch_enet_prep(int64_t A, const double* x2a, double l2, double* invden, hipStream_t s) {
  const int64_t Apad = round_up(A, BB);
  if (Apad < 1) return GBM_OK;
  enet_prep_kernel<<<(unsigned)((Apad + 255) / 256), 256, 0, s>>>(A, Apad, x2a, l2, invden);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

// One coordinate-descent pass over the A packed rows (A >= 1): b_in → b_out (per-slot, padded to whole
// blocks), e updated in place, red[0] = max_a x2_a δ_a²/n, red[1] = ‖e‖².
int launch_enet_pass(const double* Za, int64_t lda, int64_t n, int64_t A, const double* W, const double* x2a,
                     const double* invden, const double* b_in, double* b_out, double thr, double* partial,
                     double* blkmax, double* e, double* red, hipStream_t s) {
  const int64_t nblk = (A + BB - 1) / BB;
  const unsigned C = (unsigned)((n + IW - 1) / IW);
  if (A < 1 || (int64_t)C * IW > lda) return fail(GBM_E_ARG, "elastic-net pass: bad arguments");
  enet_dots0_kernel<<<C, 256, 0, s>>>(Za, lda, n, A, e, partial);
  for (int64_t k = 0; k < nblk; k++) {
    const double* pin = partial + (k & 1) * (int64_t)C * BB;
    double* pout = partial + ((k + 1) & 1) * (int64_t)C * BB;
    enet_chain_kernel<<<C, 256, 0, s>>>(Za, lda, n, A, W, k, nblk, pin, pout, x2a, invden, b_in, b_out, thr,
                                        1.0 / (double)n, blkmax, e);
  }
  enet_reduce_kernel<<<1, 256, 0, s>>>(blkmax, nblk, e, n, red);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

// red[1] = ‖e‖² alone (a λ with an empty active list)
int launch_enet_norm(const double* e, int64_t n, double* red, hipStream_t s) {
  enet_reduce_kernel<<<1, 256, 0, s>>>(nullptr, 0, e, n, red);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

}  // namespace gbm
