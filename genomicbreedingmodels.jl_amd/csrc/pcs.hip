// Kernels of the block eigensolver on a session's cached GRM (driver: gbm_session_pcs, session_pcs.cpp; DESIGN.md
// §4.11): the symmetric fill of K from the GRM's defined elements, the skinny product Yt = Qt·K on fp64 MFMA, and
// the small per-iteration kernels (Gram products, 32x32 row transforms, Ritz residuals, the reference operator's
// rank-one corrections, column statistics, traces, the start block).
//
// A block of B vectors is a B x ld row-major array like the locus rows (individuals contiguous, ld >= npad even,
// 16-byte aligned, padding columns [n, ld) zero). Every reduction runs in a fixed order (no atomics): two calls
// give the same bits, and a row's result never depends on the other rows of the launch.
#include "chol_device.h"
#include "counter_hash.h"

namespace gbm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int kSymT = 64;    // tile of the symmetric fill
constexpr int kQP = 18;      // LDS pitch of a wave's 16-individual slice of Qt: A-fragment reads conflict-free
constexpr int kGramChunk = 64;  // individuals per workgroup of the Gram products
constexpr int kGP = kGramChunk + 1;

// ---- symmetric fill -----------------------------------------------------------------------------------------
// One workgroup per 64x64 tile pair (bi <= bj): reads G's tile (bi, bj) — for bi == bj only the elements with
// row <= column — and writes scale·G to K's tiles (bi, bj) and, transposed through LDS, (bj, bi). Every element
// it reads has tile-row <= tile-column and 16-block-row <= 16-block-column, which gbm_dev_grm and the exact GRM
// define; rows and columns >= n are never read and come out as zeros.
__global__ void __launch_bounds__(256) symmetrize_kernel(const double* __restrict__ G, int64_t ldg, int64_t n,
                                                         double scale, double* __restrict__ K, int64_t ldk) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  __shared__ double t[kSymT][kSymT + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)bi * kSymT, c0 = (int64_t)bj * kSymT;
  for (int r = ty; r < kSymT; r += 4) {
    const int64_t gi = r0 + r, gj = c0 + tx;
    double v = 0.0;
    if (gi < n && gj < n && (bi < bj || r <= tx)) v = scale * G[gi * ldg + gj];
    t[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < kSymT; r += 4) {
    if (bi < bj) {
      K[(r0 + r) * ldk + c0 + tx] = t[r][tx];
      K[(c0 + r) * ldk + r0 + tx] = t[tx][r];
    } else {
      K[(r0 + r) * ldk + c0 + tx] = r <= tx ? t[r][tx] : t[tx][r];
    }
  }
}

// ---- block product Yt = Qt·K --------------------------------------------------------------------------------
// Grid (npad/64 column strips, S splits of the individual range); 4 waves. The workgroup's individuals are the
// 64-row chunks [c0, c1) of K; in a chunk wave w takes rows 16w..16w+15, for all 64 columns of the strip: per
// 4-row step two 16-byte loads per lane (a wave instruction reads four 256-byte row pieces) feed 4·RB MFMAs.
// Accumulator (vb, h, e) holds vectors 16vb.. and the columns j0 + 32h + 2fc + e (fc = lane & 15). The next
// chunk's K rows are loaded before the current chunk's MFMAs. The four waves' sums are added in wave order
// through LDS, and the S partials in split order by rows_reduce_kernel.
template <int RB>
__global__ void __launch_bounds__(256) rows_times_sym_kernel(const double* __restrict__ K, int64_t ldk, int64_t nchunk,
                                                             const double* __restrict__ Qt, int64_t ldq,
                                                             double* __restrict__ out, int64_t ldo, int64_t split_stride) {
  // a wave's Qt slice (RB·16 x 16, pitch kQP) while it multiplies; the four waves' 16 x 64 sums in the epilogue
  __shared__ __attribute__((aligned(16))) double lds[(4 * RB * 16 * kQP > 4 * 16 * 64) ? 4 * RB * 16 * kQP : 4 * 16 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane >> 4, fc = lane & 15;
  const int S = gridDim.y, sp = blockIdx.y;
  const int64_t c0 = nchunk * sp / S, c1 = nchunk * (sp + 1) / S;
  const int64_t j0 = (int64_t)blockIdx.x * 64;
  double* Qs = lds + wave * (RB * 16 * kQP);
  d4 acc[RB][2][2];
#pragma unroll
  for (int vb = 0; vb < RB; vb++)
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int e = 0; e < 2; e++) acc[vb][h][e] = (d4){0.0, 0.0, 0.0, 0.0};
  d2 kb[4][2];
  auto load_k = [&](int64_t c, d2 (&dst)[4][2]) {
    const double* base = K + (c * 64 + wave * 16 + fr) * ldk + j0 + 2 * fc;
#pragma unroll
    for (int ks = 0; ks < 4; ks++)
#pragma unroll
      for (int h = 0; h < 2; h++) dst[ks][h] = *reinterpret_cast<const d2*>(base + (int64_t)ks * 4 * ldk + 32 * h);
  };
  if (c0 < c1) load_k(c0, kb);
  for (int64_t c = c0; c < c1; c++) {
    // this wave's Qt slice: rows 0..16RB-1, individuals 64c + 16w .. +15 (8 rows of 128 B per wave instruction)
    const int64_t i0 = c * 64 + wave * 16;
#pragma unroll
    for (int ps = 0; ps < 2 * RB; ps++) {
      const int row = ps * 8 + (lane >> 3), col = (lane & 7) * 2;
      *reinterpret_cast<d2*>(&Qs[row * kQP + col]) = *reinterpret_cast<const d2*>(Qt + row * ldq + i0 + col);
    }
    d2 kn[4][2];
    if (c + 1 < c1) load_k(c + 1, kn);
    // the slice is in LDS before other lanes read it (LDS operations of one wave complete in order)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
#pragma unroll
      for (int vb = 0; vb < RB; vb++) {
        const double a = Qs[(vb * 16 + fc) * kQP + ks * 4 + fr];
#pragma unroll
        for (int h = 0; h < 2; h++) {
          acc[vb][h][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, kb[ks][h][0], acc[vb][h][0], 0, 0, 0);
          acc[vb][h][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, kb[ks][h][1], acc[vb][h][1], 0, 0, 0);
        }
      }
    }
    // the reads of this slice are done before the next chunk's stores overwrite it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (c + 1 < c1) {
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
#pragma unroll
        for (int h = 0; h < 2; h++) kb[ks][h] = kn[ks][h];
    }
  }
  double* dst = out + (int64_t)sp * split_stride;
#pragma unroll
  for (int vb = 0; vb < RB; vb++) {
    __syncthreads();  // the slices (first round) or the previous round's sums are no longer read
    double* red = lds + wave * (16 * 64);
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int h = 0; h < 2; h++)
        *reinterpret_cast<d2*>(&red[(fr + 4 * r) * 64 + 32 * h + 2 * fc]) = (d2){acc[vb][h][0][r], acc[vb][h][1][r]};
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int e = 2 * tid + 512 * k;  // element pair of the 16 x 64 block
      d2 s = *reinterpret_cast<const d2*>(&lds[e]);
      s += *reinterpret_cast<const d2*>(&lds[1024 + e]);
      s += *reinterpret_cast<const d2*>(&lds[2048 + e]);
      s += *reinterpret_cast<const d2*>(&lds[3072 + e]);
      *reinterpret_cast<d2*>(dst + (int64_t)(vb * 16 + (e >> 6)) * ldo + j0 + (e & 63)) = s;
    }
  }
}

// Yt[v, j] = Σ_s part[s][v][j], s ascending (part: S x rows x npad)
__global__ void __launch_bounds__(256) rows_reduce_kernel(const double* __restrict__ part, int S, int64_t rows,
                                                          int64_t npad, double* __restrict__ Yt, int64_t ldy) {
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  if (e >= rows * npad) return;
  d2 s = *reinterpret_cast<const d2*>(part + e);
  for (int k = 1; k < S; k++) s += *reinterpret_cast<const d2*>(part + (int64_t)k * rows * npad + e);
  *reinterpret_cast<d2*>(Yt + (e / npad) * ldy + e % npad) = s;
}

// ---- fixed-order workgroup sum (256 threads); every thread gets the result ------------------------------------
__device__ __forceinline__ double block_sum(double x, double* sh, int tid) {
  __syncthreads();
  sh[tid] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  return sh[0];
}

// ---- column statistics of K: m_j = Σ_i K_ij / n, s_j = sqrt(Σ_i (K_ij − m_j)² / (n − 1)) -----------------------
// 64 columns per workgroup, the rows split over 4 thread groups whose sums are added in group order.
__global__ void __launch_bounds__(256) pcs_colstats_kernel(const double* __restrict__ K, int64_t ldk, int64_t n,
                                                           double* __restrict__ m, double* __restrict__ s) {
  __shared__ double sh[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + tx;  // < npad
  double a = 0.0;
  for (int64_t i = ty; i < n; i += 4) a += K[i * ldk + j];
  sh[ty][tx] = a;
  __syncthreads();
  const double mean = (((sh[0][tx] + sh[1][tx]) + sh[2][tx]) + sh[3][tx]) / (double)n;
  __syncthreads();
  double q = 0.0;
  for (int64_t i = ty; i < n; i += 4) {
    const double d = K[i * ldk + j] - mean;
    q = fma(d, d, q);
  }
  sh[ty][tx] = q;
  __syncthreads();
  if (ty == 0) {
    const double ss = ((sh[0][tx] + sh[1][tx]) + sh[2][tx]) + sh[3][tx];
    const bool in = j < n;
    m[j] = in ? mean : 0.0;
    s[j] = in ? sqrt(ss / (double)(n - 1)) : 0.0;
  }
}

// Row i's share of tr M of the reference operator: Σ_j (K̃_ij − r_i)², K̃_ij = (K_ij − m_j)/s_j, r_i its row mean
__global__ void __launch_bounds__(256) pcs_rowtrace_kernel(const double* __restrict__ K, int64_t ldk, int64_t n,
                                                           const double* __restrict__ m, const double* __restrict__ s,
                                                           double* __restrict__ out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const double* row = K + (int64_t)blockIdx.x * ldk;
  double a = 0.0;
  for (int64_t j = tid; j < n; j += 256) a += (row[j] - m[j]) / s[j];
  const double r = block_sum(a, sh, tid) / (double)n;
  double q = 0.0;
  for (int64_t j = tid; j < n; j += 256) {
    const double d = (row[j] - m[j]) / s[j] - r;
    q = fma(d, d, q);
  }
  q = block_sum(q, sh, tid);
  if (tid == 0) out[blockIdx.x] = q;
}

// out[0] = Σ_i x[i·stride], i < n (one workgroup)
__global__ void __launch_bounds__(256) pcs_sum_kernel(const double* __restrict__ x, int64_t stride, int64_t n,
                                                      double* __restrict__ out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t i = tid; i < n; i += 256) a += x[i * stride];
  a = block_sum(a, sh, tid);
  if (tid == 0) out[0] = a;
}

// ---- the reference operator's rank-one corrections (one workgroup per vector) ----------------------------------
// Wt = D⁻¹H D⁻¹(P − c mᵀ): c = Σ_i Qt[v, i]; u_j = (P[v, j] − c m_j)/s_j; Wt[v, j] = (u_j − ū)/s_j
__global__ void __launch_bounds__(256) pcs_ref_mid_kernel(const double* __restrict__ Qt, int64_t ldq,
                                                          const double* __restrict__ P, int64_t ldp, int64_t n,
                                                          int64_t npad, const double* __restrict__ m,
                                                          const double* __restrict__ s, double* __restrict__ Wt,
                                                          int64_t ldw) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const double* q = Qt + (int64_t)blockIdx.x * ldq;
  const double* p = P + (int64_t)blockIdx.x * ldp;
  double* w = Wt + (int64_t)blockIdx.x * ldw;
  double a = 0.0;
  for (int64_t i = tid; i < n; i += 256) a += q[i];
  const double c = block_sum(a, sh, tid);
  a = 0.0;
  for (int64_t j = tid; j < n; j += 256) {
    const double u = (p[j] - c * m[j]) / s[j];
    w[j] = u;
    a += u;
  }
  const double ubar = block_sum(a, sh, tid) / (double)n;
  for (int64_t j = tid; j < npad; j += 256) w[j] = j < n ? (w[j] - ubar) / s[j] : 0.0;
}

// Yt = P − 1(mᵀW): Yt[v, j] −= Σ_i m_i Wt[v, i], in place on the product P = Wt·K (padding stays 0)
__global__ void __launch_bounds__(256) pcs_ref_post_kernel(const double* __restrict__ Wt, int64_t ldw, int64_t n,
                                                           const double* __restrict__ m, double* __restrict__ Yt,
                                                           int64_t ldy) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const double* w = Wt + (int64_t)blockIdx.x * ldw;
  double* y = Yt + (int64_t)blockIdx.x * ldy;
  double a = 0.0;
  for (int64_t i = tid; i < n; i += 256) a = fma(m[i], w[i], a);
  const double d = block_sum(a, sh, tid);
  for (int64_t j = tid; j < n; j += 256) y[j] -= d;
}

// ---- Gram products of two 32-vector blocks -------------------------------------------------------------------
// part[chunk][pair][a][b] = Σ_{i in chunk} A_pair[a, i] B_pair[b, i]; pair 0: (A, B), pair 1 (gridDim.y == 2): (B, B)
__global__ void __launch_bounds__(256) pcs_gram_kernel(const double* __restrict__ A, int64_t lda,
                                                       const double* __restrict__ B, int64_t ldb,
                                                       double* __restrict__ part) {
  __shared__ double As[32 * kGP], Bs[32 * kGP];
  const int tid = threadIdx.x;
  const double* L = blockIdx.y == 0 ? A : B;
  const int64_t ldl = blockIdx.y == 0 ? lda : ldb;
  const int64_t i0 = (int64_t)blockIdx.x * kGramChunk;  // chunks tile [0, npad)
  for (int e = tid; e < 32 * kGramChunk; e += 256) {
    const int r = e / kGramChunk, c = e % kGramChunk;
    As[r * kGP + c] = L[r * ldl + i0 + c];
    Bs[r * kGP + c] = B[r * ldb + i0 + c];
  }
  __syncthreads();
  const int a = tid >> 3, b0 = (tid & 7) * 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < kGramChunk; i++) {
    const double x = As[a * kGP + i];
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = fma(x, Bs[(b0 + k) * kGP + i], acc[k]);
  }
  double* o = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 1024 + a * 32 + b0;
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = acc[k];
}
// out[e] = Σ_chunk part[chunk][e] over the `total` = npairs·1024 entries: 16 thread groups each add a contiguous
// sixteenth of the chunks in ascending order, and the 16 sums are added in group order
__global__ void __launch_bounds__(256) pcs_gram_reduce_kernel(const double* __restrict__ part, int64_t nchunks,
                                                              int total, double* __restrict__ out) {
  __shared__ double sh[16][16];
  const int tx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + tx;  // < total (a multiple of 16)
  double a = 0.0;
  for (int64_t c = nchunks * g / 16; c < nchunks * (g + 1) / 16; c++) a += part[c * total + e];
  sh[g][tx] = a;
  __syncthreads();
  if (g == 0) {
    double t = sh[0][tx];
#pragma unroll
    for (int k = 1; k < 16; k++) t += sh[k][tx];
    out[e] = t;
  }
}

// ---- Out[v, j] = Σ_u Mx[v][u] In[u, j], v < nout (Mx 32 x 32 row-major in device memory), u ascending ----------
// 64 columns per workgroup; the output rows are dealt to 4 thread groups, 8 consecutive rows each
__global__ void __launch_bounds__(256) pcs_transform_kernel(const double* __restrict__ Mx, const double* __restrict__ In,
                                                            int64_t ldi, int64_t npad, int nout, double* __restrict__ Out,
                                                            int64_t ldo) {
  __shared__ double M[1024];
  const int tid = threadIdx.x;
  for (int e = tid; e < 1024; e += 256) M[e] = Mx[e];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * 64 + (tid & 63);  // < npad (a multiple of 64)
  const int v0 = (tid >> 6) * 8, v1 = v0 + 8 < nout ? v0 + 8 : nout;
  if (v0 >= v1) return;
  double x[32];
#pragma unroll
  for (int u = 0; u < 32; u++) x[u] = In[u * ldi + j];
  for (int v = v0; v < v1; v++) {
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 32; u++) a = fma(M[v * 32 + u], x[u], a);
    Out[v * ldo + j] = a;
  }
}

// ---- Ritz residuals: part[chunk][i] = Σ_{j in chunk} (Σ_u St[i][u] (Y[u, j] − θ_i Q[u, j]))², i < k --------------
// St (32 x 32 row-major): row i = Ritz vector s_i; theta at St + 1024
__global__ void __launch_bounds__(256) pcs_resid_kernel(const double* __restrict__ St, const double* __restrict__ Q,
                                                        int64_t ldq, const double* __restrict__ Y, int64_t ldy,
                                                        int64_t npad, int k, double* __restrict__ part) {
  __shared__ double M[1024 + 32];
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  for (int e = tid; e < 1024 + 32; e += 256) M[e] = St[e];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * 256 + tid;
  const bool in = j < npad;
  double y[32], q[32];
#pragma unroll
  for (int u = 0; u < 32; u++) {
    y[u] = in ? Y[u * ldy + j] : 0.0;
    q[u] = in ? Q[u * ldq + j] : 0.0;
  }
  for (int i = 0; i < k; i++) {
    const double th = M[1024 + i];
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 32; u++) a = fma(M[i * 32 + u], fma(-th, q[u], y[u]), a);
    const double r = block_sum(a * a, sh, tid);
    if (tid == 0) part[(int64_t)blockIdx.x * 16 + i] = r;
  }
}

// ---- deterministic start block (mix64: counter_hash.h, the synthetic generator's hash) ---------------------------
// Q[v, i] uniform in (−1, 1) from hash(seed, v, i), i < n; 0 on the padding
__global__ void __launch_bounds__(256) pcs_start_kernel(double* __restrict__ Q, int64_t ldq, int64_t n, int64_t npad,
                                                        uint64_t seed) {
  const int v = blockIdx.y;
  const uint64_t base = mix64(seed * 0xD1B54A32D192ED03ull + (uint64_t)v);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  double x = 0.0;
  if (i < n) {
    const uint64_t h = mix64(base ^ ((uint64_t)i * 0x8CB92BA72F3D8DD7ull));
    x = (double)(h >> 11) * (1.0 / 4503599627370496.0) - 1.0;  // 53 bits onto [−1, 1)
  }
  Q[v * ldq + i] = x;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// Splits of the individual range of the block product: enough workgroups for every compute unit at a few
// thousand individuals, never more than the 64-row chunks (npad >= 128: at least 2). A function of n alone (not
// of rows): a row's bits do not depend on the call it was in.
int64_t rows_times_sym_splits(int64_t n) {
  const int64_t nchunk = npad_of(n) / 64;
  int64_t S = (768 + nchunk - 1) / nchunk;
  if (S > nchunk) S = nchunk;
  if (S > 16) S = 16;
  return S < 1 ? 1 : S;
}

int launch_pcs_colstats(const double* K, int64_t ldk, int64_t n, double* m, double* s, hipStream_t st) {
  pcs_colstats_kernel<<<(unsigned)(npad_of(n) / 64), 256, 0, st>>>(K, ldk, n, m, s);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int launch_pcs_rowtrace(const double* K, int64_t ldk, int64_t n, const double* m, const double* s, double* rows_out,
                        hipStream_t st) {
  pcs_rowtrace_kernel<<<(unsigned)n, 256, 0, st>>>(K, ldk, n, m, s, rows_out);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int launch_pcs_sum(const double* x, int64_t stride, int64_t n, double* out, hipStream_t st) {
  pcs_sum_kernel<<<1, 256, 0, st>>>(x, stride, n, out);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int launch_pcs_ref_mid(const double* Qt, int64_t ldq, const double* P, int64_t ldp, int64_t n, const double* m,
                       const double* s, double* Wt, int64_t ldw, hipStream_t st) {
  pcs_ref_mid_kernel<<<kPcsBlock, 256, 0, st>>>(Qt, ldq, P, ldp, n, npad_of(n), m, s, Wt, ldw);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int launch_pcs_ref_post(const double* Wt, int64_t ldw, int64_t n, const double* m, double* Yt, int64_t ldy,
                        hipStream_t st) {
  pcs_ref_post_kernel<<<kPcsBlock, 256, 0, st>>>(Wt, ldw, n, m, Yt, ldy);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int64_t pcs_gram_workspace(int64_t n) { return npad_of(n) / kGramChunk * 2 * 1024 * 8; }
int launch_pcs_gram(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t n, int npairs, double* part,
                    double* out, hipStream_t st) {
  const int64_t nchunks = npad_of(n) / kGramChunk;
  pcs_gram_kernel<<<dim3((unsigned)nchunks, (unsigned)npairs), 256, 0, st>>>(A, lda, B, ldb, part);
  GBM_LAUNCH_CHECK();
  pcs_gram_reduce_kernel<<<(unsigned)(npairs * 64), 256, 0, st>>>(part, nchunks, npairs * 1024, out);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int launch_pcs_transform(const double* Mx, const double* In, int64_t ldi, int64_t n, int nout, double* Out, int64_t ldo,
                         hipStream_t st) {
  const int64_t npad = npad_of(n);
  pcs_transform_kernel<<<(unsigned)(npad / 64), 256, 0, st>>>(Mx, In, ldi, npad, nout, Out, ldo);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int64_t pcs_resid_chunks(int64_t n) { return (npad_of(n) + 255) / 256; }
int launch_pcs_resid(const double* St, const double* Q, int64_t ldq, const double* Y, int64_t ldy, int64_t n, int k,
                     double* part, hipStream_t st) {
  pcs_resid_kernel<<<(unsigned)pcs_resid_chunks(n), 256, 0, st>>>(St, Q, ldq, Y, ldy, npad_of(n), k, part);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
int launch_pcs_start(double* Q, int64_t ldq, int64_t n, uint64_t seed, hipStream_t st) {
  const int64_t npad = npad_of(n);
  pcs_start_kernel<<<dim3((unsigned)((npad + 255) / 256), kPcsBlock), 256, 0, st>>>(Q, ldq, n, npad, seed);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

}  // namespace gbm

using namespace gbm;

extern "C" int gbm_dev_grm_symmetrize(const double* G, int64_t ldg, int64_t n, double scale, double* K, int64_t ldk,
                                      void* stream) {
  if (!G || !K || G == K || n < 1 || !std::isfinite(scale) || ldg < npad_of(n) || ldk < npad_of(n) || (ldk & 1) ||
      !aligned16(K))
    return fail(GBM_E_ARG, "gbm_dev_grm_symmetrize: bad arguments (G and K distinct, n >= 1, finite scale, ldg >= "
                           "npad(n), even ldk >= npad(n), K 16-byte aligned)");
  const unsigned nt = (unsigned)(npad_of(n) / kSymT);
  if (nt > 65535) return fail(GBM_E_ARG, "gbm_dev_grm_symmetrize: n is too large for one launch");
  symmetrize_kernel<<<dim3(nt, nt), 256, 0, (hipStream_t)stream>>>(G, ldg, n, scale, K, ldk);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

extern "C" int64_t gbm_dev_rows_times_sym_workspace(int64_t n, int64_t rows) {
  if (n < 1 || rows < 1) return 0;
  return rows_times_sym_splits(n) * round_up(rows, 16) * npad_of(n) * 8;
}

extern "C" int gbm_dev_rows_times_sym(const double* K, int64_t ldk, int64_t n, const double* Qt, int64_t ldq,
                                      int64_t rows, double* Yt, int64_t ldy, void* workspace, int64_t ws_bytes,
                                      void* stream) {
  if (n < 1) return fail(GBM_E_ARG, "gbm_dev_rows_times_sym: n must be >= 1");
  const int64_t npad = npad_of(n);
  if (rows < 16 || rows > 64 || (rows & 15))
    return fail(GBM_E_ARG, "gbm_dev_rows_times_sym: rows must be 16, 32, 48 or 64");
  if (!K || !Qt || !Yt || Qt == Yt || !aligned16(K) || !aligned16(Qt) || !aligned16(Yt) || ldk < npad || (ldk & 1) ||
      ldq < npad || (ldq & 1) || ldy < npad || (ldy & 1))
    return fail(GBM_E_ARG, "gbm_dev_rows_times_sym: bad arguments (K, Qt, Yt 16-byte aligned, Qt and Yt distinct, "
                           "even ldk, ldq, ldy >= npad(n))");
  if (!workspace || !aligned16(workspace) || ws_bytes < gbm_dev_rows_times_sym_workspace(n, rows))
    return fail(GBM_E_ARG, "gbm_dev_rows_times_sym: the workspace is NULL, misaligned or smaller than "
                           "gbm_dev_rows_times_sym_workspace(n, rows)");
  const int64_t S = rows_times_sym_splits(n), nchunk = npad / 64;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nchunk, (unsigned)S);
  double* part = (double*)workspace;  // S x rows x npad
  const int64_t stride = rows * npad;
  switch (rows / 16) {
    case 1: rows_times_sym_kernel<1><<<grid, 256, 0, st>>>(K, ldk, nchunk, Qt, ldq, part, npad, stride); break;
    case 2: rows_times_sym_kernel<2><<<grid, 256, 0, st>>>(K, ldk, nchunk, Qt, ldq, part, npad, stride); break;
    case 3: rows_times_sym_kernel<3><<<grid, 256, 0, st>>>(K, ldk, nchunk, Qt, ldq, part, npad, stride); break;
    default: rows_times_sym_kernel<4><<<grid, 256, 0, st>>>(K, ldk, nchunk, Qt, ldq, part, npad, stride); break;
  }
  GBM_LAUNCH_CHECK();
  rows_reduce_kernel<<<(unsigned)((rows * npad / 2 + 255) / 256), 256, 0, st>>>(part, (int)S, rows, npad, Yt, ldy);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}
