// Bayesian ridge regression: the persistent super-block sweep over all CUs. With byte storage and
// n <= 48 x CUs a Gibbs iteration of gbm_brr_fit (brr.hip) is ONE persistent launch over 512-marker
// super-blocks on up to every CU (brr_sweep_la2_kernel) instead of one launch per marker block. This
// file holds the sweep's device code and, at its end, the narrow host interface of gibbs_common.h
// (brr_sweep_plan, brr_sweep_setup, brr_sweep_enqueue, brr_sweep_lock): the host driver never sees
// the hand-off code. (Rounds 2-3 also kept a 128-block sweep and two earlier super-block schedules;
// they are in git history, e.g. `git show 3599bea:genomicbreedingmodels.jl_amd/csrc/gibbs.hip`.)
#include <map>
#include <memory>

#include "gibbs_common.h"

namespace gbm {
namespace {

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
  const int quad = (int)(blockIdx.x & 3);
  const int64_t sp = blockIdx.x >> 2;
  const int64_t s = sp / SB_PAIRS;
  const int pair = (int)(sp % SB_PAIRS);
  int i = 1;
  while ((i + 1) * i / 2 <= pair) i++;
  const int m = pair - i * (i - 1) / 2;
  const int64_t r0 = s * SBK + i * BK2 + (quad >> 1) * BB, c0 = s * SBK + m * BK2 + (quad & 1) * BB;
  brr_gram_tile(Xt, ldx, p, n, r0, c0, Wsb + sp * BK2 * BK2 + (quad >> 1) * BB * BK2 + (quad & 1) * BB, BK2);
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
__device__ __forceinline__ uint64_t sb_key(uint64_t tag) { return mix64(tag * 0x9E3779B97F4A7C15ull + 0x5DEECE66Dull); }
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

}  // namespace

// ---- host interface (gibbs_common.h) --------------------------------------------------------------
// The sweep runs when its chunk workgroups (K <= LA_KMAX individuals each: n <= 48 x CUs) can all be
// resident, one per CU, and own <= SB_RMAX rows of a super-block each; GBM_BRR_SWEEP=0 keeps the
// per-launch path.
int brr_sweep_plan(int64_t n, int cus, SweepPlan& pl) {
  const char* ev = knob("GBM_BRR_SWEEP");
  int per_cu = 0;
  GBM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, brr_sweep_la2_kernel<false>, 256, 0));
  pl.K = (int)round_up(std::max<int64_t>(16, (n + cus - 1) / cus), 16);
  if (const char* ek = knob("GBM_BRR_SB_K"))  // (timing experiments) a larger chunk
    pl.K = std::max<int>(pl.K, (int)round_up(std::max<int64_t>(16, atoll(ek)), 16));
  pl.Cu = (int)((n + pl.K - 1) / pl.K);
  pl.Ru = (int)round_up((SBK + pl.Cu - 1) / pl.Cu, 2);
  pl.on = !(ev && ev[0] == '0') && per_cu >= 1 && pl.K <= LA_KMAX && pl.Cu <= std::min(cus, 256) && pl.Ru <= SB_RMAX;
  // the chunk split: O = 512 / R owners of Ko individuals, the rest Kn (both <= LA_KMAX), all on
  // <= min(CUs, 256) workgroups; the owners get the smallest Ko that fits. Off unless GBM_BRR_OWN_R=
  // 2|4|6|8 (read per call) sets R: at C4 the extra workgroups' polls cost the hops more than the
  // owners' lighter chunks save (2.58 ms at R = 4, 3.32 at R = 8, vs 2.41 uniform). Uniform
  // chunks (Ko = Kn = K, O = 512 / R) otherwise.
  pl.Ko = pl.Kn = pl.K;
  pl.R = pl.Ru;
  pl.O = (SBK + pl.Ru - 1) / pl.Ru;
  pl.C = pl.Cu;
  if (!pl.on) return GBM_OK;
  int R2 = 0;
  if (const char* er = knob("GBM_BRR_OWN_R")) R2 = std::max(2, std::min<int>(SB_RMAX, atoi(er) & ~1));
  const int O2 = R2 > 0 ? (SBK + R2 - 1) / R2 : 0;
  const int ncu = std::min(cus, 256);
  for (int Ko = 16; R2 > 0 && Ko <= LA_KMAX && O2 < ncu; Ko += 16) {
    const int64_t rest = n - (int64_t)O2 * Ko;
    if (rest < 16) break;
    const int Kn = (int)round_up(std::max<int64_t>(16, (rest + (ncu - O2) - 1) / (ncu - O2)), 16);
    if (Kn > LA_KMAX) continue;
    if (Kn <= Ko) break;  // no lighter owners than the uniform split
    pl.Ko = Ko;
    pl.Kn = Kn;
    pl.R = R2;
    pl.O = O2;
    pl.C = O2 + (int)((rest + Kn - 1) / Kn);
    break;
  }
  return GBM_OK;
}

int brr_sweep_setup(BrrCtx& cx, const SweepPlan& pl, int64_t n, int64_t p, int64_t npad, int64_t nsb, int64_t trace_n) {
  const int dev = cx.dev;
  hipStream_t s = cx.stream.s;
  GBM_TRY(ensure(cx.Wsb, dev, nsb * SB_PAIRS * BK2 * BK2 * 8));
  GBM_TRY(ensure(cx.MS, dev, nsb * SBK * SBK * 8));
  GBM_TRY(ensure(cx.Ssc, dev, nsb * 6 * BK2 * BK2 * 8));
  GBM_TRY(ensure(cx.Pb, dev, (int64_t)4 * pl.C * SBK * 16));  // 16-B hand-off granules (4 slots)
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
  // α = γ = 0 past p: the 128-blocks are rounded up to whole super-blocks
  GBM_HIP_TRY(hipMemsetAsync(cx.alph.p, 0, (size_t)(nsb * SBK * 8), s));
  GBM_HIP_TRY(hipMemsetAsync(cx.gamm.p, 0, (size_t)(nsb * SBK * 8), s));
  brr_gram_sb_kernel<<<(unsigned)(nsb * SB_PAIRS * 4), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n, (double*)cx.Wsb.p);
  GBM_LAUNCH_CHECK();
  if (trace_n > 0) GBM_TRY(ensure(cx.trace, dev, trace_n * 8));
  return GBM_OK;
}

void brr_sweep_enqueue(BrrCtx& cx, const SweepPlan& pl, int64_t n, int64_t p, int64_t npad, int64_t nsb, double xs,
                       int64_t* trace_dev) {
  hipStream_t s = cx.stream.s;
  for (int level : {0, 2, 3})
    brr_sb_prep_kernel<<<(unsigned)(nsb * (level == 0 ? 2 : 4)), 256, 0, s>>>(
        level, (const double*)cx.Wsb.p, (const double*)cx.alph.p, (double*)cx.MS.p, (double*)cx.Ssc.p);
  auto* sweep = trace_dev ? brr_sweep_la2_kernel<true> : brr_sweep_la2_kernel<false>;
  sweep<<<(unsigned)pl.C, 256, 0, s>>>((const uint8_t*)cx.D.p, npad, n, p, xs, (const double*)cx.MS.p,
                                       (const double*)cx.CS.p, (const double*)cx.CS2.p, nsb, pl.Ko, pl.O, pl.Kn, pl.R,
                                       (double*)cx.Pb.p, (double*)cx.Rt.p, (double*)cx.Dl.p, brr_sweep_error_cell(cx),
                                       (double*)cx.b.p, (double*)cx.bbar.p, (const double*)cx.alph.p,
                                       (const double*)cx.gamm.p, (double*)cx.e.p, (const BrrState*)cx.stm.p, trace_dev);
}

// The persistent sweep needs all its workgroups resident at once: sweeps of concurrent fits on one
// device take turns (held for a whole fit), so two of them can never be partly resident and spin on
// each other.
std::mutex& brr_sweep_lock(int dev) {
  static std::mutex mu;
  static auto* locks = new std::map<int, std::unique_ptr<std::mutex>>;  // never destroyed
  std::lock_guard<std::mutex> lock(mu);
  auto& m = (*locks)[dev];
  if (!m) m = std::make_unique<std::mutex>();
  return *m;
}

}  // namespace gbm

