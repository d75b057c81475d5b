// Internal helpers shared by the libgbm translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>

#include "../../include/gbm.h"

namespace gbm {

// Tile geometry (see DESIGN.md "Data layout in HBM").
constexpr int64_t kNPadTile = 128;  // individuals padded to a multiple of the GRM tile
constexpr int64_t kRhsRows = 64;    // bordered right-hand-side rows appended to V
constexpr int kCholNB = 64;         // Cholesky panel width

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int64_t npad_of(int64_t n) { return round_up(n < 1 ? 1 : n, kNPadTile); }
inline int64_t gdim_of(int64_t n) { return npad_of(n) + kRhsRows; }

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
const std::string& last_error();  // the calling thread's message (gbm_last_error)

// GBM_* tuning/test knobs (knobs.cpp): the environment is read once, at the first lookup; afterwards
// values change only through gbm_debug_set. knob() returns the value (a pointer valid for the life of
// the process) or nullptr when unset; knob_i64 parses it (def when unset or empty).
const char* knob(const char* name);
int64_t knob_i64(const char* name, int64_t def);

#define GBM_HIP_TRY(expr)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return ::gbm::fail(GBM_E_HIP, std::string("HIP error '") + hipGetErrorString(e_) +       \
                                        "' at " __FILE__ ":" + std::to_string(__LINE__) + " (" #expr ")"); \
  } while (0)

#define GBM_LAUNCH_CHECK() GBM_HIP_TRY(hipGetLastError())

#define GBM_TRY(expr)              \
  do {                             \
    int rc_ = (expr);              \
    if (rc_ != GBM_OK) return rc_; \
  } while (0)

// Stage launchers (device pointers, stream-ordered); defined in the .hip files.
// accum = 1: G += the GRM of these loci (only where grm_can_accumulate(n, p)). err_out (device
// int32, optional): the in-order carry's error cell is copied there (< 0: a wait timed out, G
// invalid) instead of being read back with a stream sync.
int launch_grm(const double* Zt, int64_t ldz, int64_t p, int64_t n, double* G, int64_t ldg,
               void* ws, int64_t ws_bytes, hipStream_t s, int accum = 0, int32_t* err_out = nullptr);
bool grm_can_accumulate(int64_t n, int64_t p);
// the GBLUP standardisation of fp64 locus rows (stats.hip; gbm_dev_standardize without its argument checks).
// beside_tiles: the launch runs concurrently with the persistent GRM tile workgroups and takes a kernel that is
// resident beside them (same bits), which exists where standardize_fits_beside_tiles(n)
int launch_standardize_rows(const double* Xt, int64_t ldx, int64_t p, int64_t n, double* Zt, int64_t ldz, double* mean,
                            double* sd, int32_t* keep, int64_t* q_dev, hipStream_t s, bool beside_tiles = false);
bool standardize_fits_beside_tiles(int64_t n);
int64_t grm_workspace_bytes(int64_t n, int64_t p);
int launch_grm_export(const double* G, int64_t ldg, int64_t n, double inv_q, double* out, int64_t ldo, hipStream_t s);
int launch_predict(const double* Xt, int64_t ldx, int64_t p, int64_t n, const double* b, int64_t ldb, int64_t nrhs,
                   double* partial, int64_t nchunks, double* out, int64_t ldo, hipStream_t s);
int64_t predict_chunks(int64_t n, int64_t p);
int launch_add_inplace(double* a, const double* b, int64_t n, hipStream_t s);
// centre the columns only (Z = X − m; every column kept, sd = 1): the ploidy-aware GRM
// standardisation straight from int8 dosage rows (x = d / ploidy), out of place into Zt
int launch_standardize_i8(const int8_t* D, int64_t ldd, int64_t p, int64_t n, int ploidy, double* Zt, int64_t ldz,
                          double* mean, double* sd, int32_t* keep, int64_t* q_dev, hipStream_t s);
// marker effects in pieces (effects.hip): B rows of fp64 standardised rows or of int8 dosage rows
// (z rebuilt bit-identically), and msum = Σ_j mean_j B[t, j] over p loci
int launch_marker_rows(const double* Zt, int64_t ldz, int64_t p, int64_t n, const double* A, int64_t lda, int64_t nrhs,
                       double inv_q, const int64_t* q_dev, const double* sd, const int32_t* keep, double* B,
                       int64_t ldb, hipStream_t s);
int launch_marker_rows_i8(const int8_t* D, int64_t ldd, int64_t p, int64_t n, int ploidy, const double* A, int64_t lda,
                          int64_t nrhs, double inv_q, const int64_t* q_dev, const double* mean, const double* sd,
                          const int32_t* keep, double* B, int64_t ldb, hipStream_t s);
// the exact-integer GRM of diploid dosage rows (grm_exact.hip)
int launch_grm_exact(const int8_t* D, int64_t ldd, int64_t p, int64_t n, int ploidy, double* G, int64_t ldg,
                     double* mean, double* sd, int32_t* keep, int64_t* q_dev, int accum, void* ws, int64_t ws_bytes,
                     int32_t* slices_out, hipStream_t s);
// after launch_grm_exact (syncs the stream): GBM_E_HIP when a weight overflowed its digits (XgInfo bit 2)
int grm_exact_status(const void* ws, int64_t n, int64_t p, hipStream_t s);
// training-set dosages 2·Xt[j, idx[i]] (resident genotypes that are dosages/2) for the exact GRM
int launch_gather_dosage(const double* Xt, int64_t ldx, int64_t p, const int32_t* idx, int64_t nT, int8_t* D,
                         hipStream_t s);
// dosage detection (grm_mode exact / auto): D = 2·X as bytes (D may be NULL: check only), *bad = 1 when any
// 2x is not 0, 1 or 2; the same check on dosage bytes
int launch_dosage_from_f64(const double* X, int64_t ldx, int64_t n, int64_t p, int8_t* D, int64_t ldd, int32_t* bad,
                           hipStream_t s);
int launch_dosage_check_i8(const int8_t* D, int64_t ldd, int64_t n, int64_t p, int32_t* bad, hipStream_t s);
// host packing (hostpack.cpp): fp64 columns (column j at X + j·ld) → dosage bytes 2x (n per column); false when
// some 2x is not exactly 0, 1 or 2. host_pack_threads: the packing workers of one call (GBM_PACK_THREADS)
bool pack_dosage_columns(const double* X, int64_t ld, int64_t n, int64_t p, int8_t* dst);
int host_pack_threads();
// Packs the loci chunks sched[k] = (first locus, count) of fp64 columns (column j at X + j·ld) into dosage bytes,
// chunk k into ring slot k mod slots (slot_bytes each, n bytes per locus), by `threads` workers that split each
// chunk in order. wait(k): chunk k's packed bytes, or nullptr once any chunk was not dosage-valued (the workers then
// stop); release_upto(k): the slots of chunks < k may be overwritten. The destructor stops and joins the workers.
class ChunkPacker {
 public:
  ChunkPacker(const double* X, int64_t ld, int64_t n, const std::vector<std::pair<int64_t, int64_t>>& sched,
              int8_t* ring, int64_t slot_bytes, int slots, int threads);
  ~ChunkPacker();
  ChunkPacker(const ChunkPacker&) = delete;
  ChunkPacker& operator=(const ChunkPacker&) = delete;
  const int8_t* wait(int64_t k);
  void release_upto(int64_t k);

 private:
  struct Impl;
  Impl* d_;
};
// GBM_GRM_* of a call: grm_mode, or for GBM_GRM_DEFAULT the GBM_GRM environment variable, else fp64
int resolve_grm_mode(int grm_mode);
int launch_weighted_sum(const double* mean, const double* B, int64_t ldb, int64_t p, int64_t nrhs, double* msum,
                        hipStream_t s);
// GWAS statistics of locus rows (effects.hip): A⁻¹ (row-major, pitch 8) and A⁻¹u of the kcov covariate rows
// (1 ≤ kcov ≤ 8, the intercept first), zscale on z; see gwas_stats_kernel
struct GwasCoef {
  double Ainv[64];
  double Au[8];
  double zscale;
  int32_t kcov;
};
int launch_gwas_stats(const double* W, int64_t ldw, int64_t rows, int64_t n, const double* Cw, int64_t ldcw,
                      const double* yw, const GwasCoef& co, const int32_t* keep, double* z, double* b, double* s_out,
                      unsigned long long* tested, hipStream_t s);
int launch_center_columns(const double* Xt, int64_t ldx, int64_t p, int64_t n, double* Zt, int64_t ldz, double* mean,
                          double* sd, int32_t* keep, int64_t* q_dev, hipStream_t s);

// Elastic-net coordinate descent on the packed active rows Za (enet.hip; driver: gbm_session_enet_path).
// lda = enet_lda(n) (a multiple of the 256-individual chunk); the per-slot arrays (x2a, invden, b) and W are
// padded to whole 64-marker blocks. launch_enet_pass: one pass, b_in → b_out, e in place, red[0] = the pass's
// max x2 δ²/n and red[1] = ‖e‖²; `partial` holds 2 x ceil(n/256) x 64 doubles, blkmax one per block.
int64_t enet_lda(int64_t n);
int launch_enet_x2(const double* Z, int64_t ldz, int64_t p, int64_t n, double* x2, hipStream_t s);
int launch_enet_gather(const double* Z, int64_t ldz, int64_t n, const int32_t* rows, int64_t a0, int64_t cnt,
                       const double* x2, double* Za, int64_t lda, double* x2a, hipStream_t s);
int64_t enet_gram_workspace(int64_t n);  // bytes of launch_enet_gram's ws (the Gram blocks' partial sums)
int launch_enet_gram(const double* Za, int64_t lda, int64_t A, int64_t n, int64_t blk0, double* W, double* ws,
                     hipStream_t s);
int launch_enet_prep(int64_t A, const double* x2a, double l2, double* invden, hipStream_t s);
int launch_enet_pass(const double* Za, int64_t lda, int64_t n, int64_t A, const double* W, const double* x2a,
                     const double* invden, const double* b_in, double* b_out, double thr, double* partial,
                     double* blkmax, double* e, double* red, hipStream_t s);
int launch_enet_norm(const double* e, int64_t n, double* red, hipStream_t s);

// Block eigensolver on the symmetric K (pcs.hip; driver: gbm_session_pcs). Vector blocks are kPcsBlock x ld
// row-major with zero padding columns; every reduction runs in a fixed order. The symmetric fill and the block
// product are the ABI entries gbm_dev_grm_symmetrize / gbm_dev_rows_times_sym.
constexpr int kPcsBlock = 32;
int64_t rows_times_sym_splits(int64_t n);
// m_j = Σ_i K_ij / n and the ddof-1 column standard deviation s_j (two passes); 0 on the padding
int launch_pcs_colstats(const double* K, int64_t ldk, int64_t n, double* m, double* s, hipStream_t st);
// rows_out[i] = Σ_j (K̃_ij − mean_j K̃_ij)², K̃ = (K − 1mᵀ)D⁻¹: row i's share of the reference operator's trace
int launch_pcs_rowtrace(const double* K, int64_t ldk, int64_t n, const double* m, const double* s, double* rows_out,
                        hipStream_t st);
int launch_pcs_sum(const double* x, int64_t stride, int64_t n, double* out, hipStream_t st);  // out[0] = Σ x[i·stride]
// the reference operator around its two block products: Wt = D⁻¹H D⁻¹(P − c mᵀ) with c = Qt·1, then Yt −= 1(mᵀW)
int launch_pcs_ref_mid(const double* Qt, int64_t ldq, const double* P, int64_t ldp, int64_t n, const double* m,
                       const double* s, double* Wt, int64_t ldw, hipStream_t st);
int launch_pcs_ref_post(const double* Wt, int64_t ldw, int64_t n, const double* m, double* Yt, int64_t ldy,
                        hipStream_t st);
// out[0] = A Bᵀ and, with npairs = 2, out[1] = B Bᵀ (32 x 32 row-major each); part: pcs_gram_workspace(n) bytes
int64_t pcs_gram_workspace(int64_t n);
int launch_pcs_gram(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t n, int npairs, double* part,
                    double* out, hipStream_t st);
// Out[v, :] = Σ_u Mx[v][u] In[u, :], v < nout (Mx 32 x 32 row-major, device)
int launch_pcs_transform(const double* Mx, const double* In, int64_t ldi, int64_t n, int nout, double* Out, int64_t ldo,
                         hipStream_t st);
// part[c·16 + i] = chunk c's share of ‖s_iᵀY − θ_i s_iᵀQ‖², i < k <= 16 (St: rows s_i, then θ at St + 1024)
int64_t pcs_resid_chunks(int64_t n);
int launch_pcs_resid(const double* St, const double* Q, int64_t ldq, const double* Y, int64_t ldy, int64_t n, int k,
                     double* part, hipStream_t st);
int launch_pcs_start(double* Q, int64_t ldq, int64_t n, uint64_t seed, hipStream_t st);

// Epistasis feature scan (pairscan.hip; driver: gbm_session_pair_scan). W is l x ldw locus-major with
// ldw = pair_scan_ldw(n). launch_pair_scan: the slopes of the i-rows [i0, i0 + rows) into beta (rows x l; unary
// operations: li = rows = 1, else li = l) and the counters cnt[0..2] (tested, degenerate, non-finite).
// launch_pair_select: the k largest |beta| > eps of a panel's m slopes into cand_idx (base + index) / cand_beta;
// state: pair_sel_state_bytes() (its last 16 bytes: the counts above and equal to the k-th value),
// blk: 2·pair_sel_blocks(m) int64.
int64_t pair_scan_ldw(int64_t n);
int64_t pair_sel_blocks(int64_t m);
int64_t pair_sel_state_bytes();
int launch_pair_prep(const double* Xt, int64_t ldx, const int64_t* idx, int64_t n, const int64_t* loci, int64_t l,
                     double eps, int use_abs, double var_threshold, const double* y, double ybar, double* W,
                     int64_t ldw, double* var, int32_t* skip, double* yc, hipStream_t s);
int launch_pair_scan(int op, const double* W, int64_t ldw, int64_t n, int64_t l, int64_t li, int64_t i0, int64_t rows,
                     const double* yc, const int32_t* skip, int commutative, double* beta, unsigned long long* cnt,
                     hipStream_t s);
int launch_pair_select(const double* beta, int64_t m, int64_t base, double eps, int64_t k, void* state, int64_t* blk,
                       int64_t* cand_idx, double* cand_beta, hipStream_t s);

// REML choice of λ (session_reml.cpp; reference loglikreml src/gwas.jl:450-483 with X = 1)
struct RemlEval {
  double g, s2u, s2e;  // objective, σ²_u, σ²_e at one λ (σ²_u profiled inside the box [eps, 1]²)
};
struct RemlResult {
  double lambda, s2e, s2u, objective;
};
double reml_objective(int64_t n, double logdet, double c11, double Q, double s2u);
RemlEval reml_profile(int64_t n, double lambda, const double t[4]);
int reml_search(const std::function<int(double, RemlEval&)>& eval, RemlResult& out);
std::vector<double> standardise_y(const double* y, int64_t n);
// frees the idle pooled BRR contexts (gibbs_setup.hip; part of gbm_release_device_cache)
void brr_release_cache();

}  // namespace gbm
