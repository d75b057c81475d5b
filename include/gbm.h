/*
 * gbm.h — C ABI of the MI355X-native GRM + GBLUP core (libgbm.so).
 *
 * This is the drop-in boundary for GenomicBreedingModels.jl's model-function path
 * (SURVEY.md §8b). A Julia `gblup(; genomes, phenomes, idx_entries, idx_loci_alleles,
 * idx_trait, verbose, λ)::Fit` built exactly like `ridge` (reference src/linear.jl:162-239)
 * calls `gbm_gblup_fit` where `ridge` calls `GLMNet.glmnetcv` (src/linear.jl:193-203);
 * the Julia/ctypes bindings are shown in INTEGRATION.md.
 *
 * Conventions
 *  - All matrices crossing the host entry points are Julia column-major Float64:
 *    X[i, j] lives at X[i + j*ldx] (i = entry/individual, j = locus-allele/SNP).
 *    A SNP column is therefore contiguous, and the device view of X is the row-major
 *    p x n matrix Xt ("locus rows"), whose rows are loaded coalesced along individuals.
 *  - The model is V = G + λI with G = Z Zᵀ / q, Z the column-standardised (ddof = 1)
 *    genotypes over the q non-monomorphic loci (reference src/gwas.jl:112-115,127-130;
 *    V = σ²_u·GRM + σ²_e·I with Z = I at src/gwas.jl:462-471, λ = σ²_e/σ²_u).
 *  - Fixed effect: GLS intercept μ̂ = 1ᵀV⁻¹y / 1ᵀV⁻¹1 (src/gwas.jl:596-597 with X = 1).
 *  - GEBVs / y_pred = μ̂ + G·a with a = V⁻¹(y − 1μ̂).
 *  - b_hat = [b0; b] with b_j = (Zᵀa)_j / (q·s_j) for kept loci (0 for monomorphic ones)
 *    and b0 = μ̂ − Σ_j m_j b_j, so the reference's linear `predict`
 *    (`b_hat[1] .+ X*b_hat[2:end]`, src/prediction.jl:228) reproduces y_pred exactly.
 *  - Return codes: 0 on success, negative GBM_E_* on failure; gbm_last_error() returns a
 *    thread-local message for the last failing call on the calling thread.
 *  - Re-entrant: every call leases its own pooled context (stream + device buffers) per
 *    SNP shard and returns it afterwards; concurrent calls (as `cvmultithread!` makes,
 *    src/cross_validation.jl:159) never share one. Pooled buffers only grow, so repeated calls
 *    of one shape allocate no device memory (gbm_device_allocations); gbm_release_device_cache
 *    frees the idle ones.
 *  - Devices: an explicit `devices` list gives one SNP-column shard per entry (an ordinal may
 *    repeat). With devices == NULL / ndev == 0, each calling thread is given one device,
 *    round-robin over GBM_DEVICES ("0,1,2,..."; re-read per call) or over all visible devices:
 *    the k-th thread to call gets entry k mod len — folds farmed over the GPUs under an
 *    unchanged `cvmultithread!`.
 */
#ifndef GBM_H
#define GBM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBM_VERSION 212 /* 0.2.1.2: knobs read once (gbm_debug_set), gbm_dev_grm_exact_status */

#define GBM_OK 0
#define GBM_E_ARG (-1)    /* bad argument (ArgumentError on the Julia side, src/prediction.jl:67-127 style) */
#define GBM_E_NOTPD (-2)  /* G + λI not positive definite (non-finite input or λ <= 0) */
#define GBM_E_HIP (-3)    /* HIP runtime error */
#define GBM_E_RCCL (-4)   /* RCCL error */
#define GBM_E_OOM (-5)    /* device allocation failed */
#define GBM_E_NODEV (-6)  /* no usable MI355X device */
#define GBM_E_DATA (-7)   /* data problem: < 2 entries, zero phenotype variance, no polymorphic locus */

/* GRM arithmetic of a fit (the grm_mode argument of the _ex entries and gbm_session_set_grm_mode):
 *   GBM_GRM_FP64   the fp64-MFMA SYRK of the standardised genotypes (the north star's GRM; any X).
 *   GBM_GRM_EXACT  the exact-integer GRM of diploid dosages (int8-MFMA digit GEMMs + int128 centring, one fp64
 *                  rounding): X must hold dosages/2, i.e. 2x exactly 0, 1 or 2 in every cell
 *                  (the allele frequencies extractxyetc hands a diploid gblup, src/prediction.jl:129), int8
 *                  input needs ploidy 2; otherwise GBM_E_ARG. More accurate than fp64 and ~3x faster.
 *   GBM_GRM_AUTO   EXACT when the genotypes are diploid dosages (checked on the device: for fp64 X while it is
 *                  converted to bytes, one chunk of loci first), else FP64.
 *   GBM_GRM_DEFAULT the environment variable GBM_GRM ("fp64" | "exact" | "auto"; read once, gbm_debug_set), else FP64.
 *   GBM_GRM_DROPIN  GBM_GRM when it is set, else AUTO: the default of the drop-in gblup (Julia and Python), so a
 *                   GBM_GRM=fp64 set by a user or CI pins the fp64 SYRK there as everywhere else.
 * The entries without _ex pass GBM_GRM_DEFAULT. */
#define GBM_GRM_DEFAULT (-1)
#define GBM_GRM_FP64 0
#define GBM_GRM_EXACT 1
#define GBM_GRM_AUTO 2
#define GBM_GRM_DROPIN 3

/* Library version (GBM_VERSION) — used by bindings to check the ABI. */
int gbm_version(void);

/* Message for the last failing call on this thread ("" if none). Never NULL. */
const char* gbm_last_error(void);

/* Number of visible HIP devices (0 when none). Returns GBM_OK or GBM_E_HIP. */
int gbm_device_count(int* count);

/* Device allocations (hipMalloc calls) libgbm has made since it was loaded. */
int64_t gbm_device_allocations(void);

/* Free the idle pooled fit contexts of the GBLUP and BRR entries (device buffers, streams and the
 * BRR iteration graphs kept between calls). */
int gbm_release_device_cache(void);

/* --------------------------------------------------------------------------------------
 * Host-buffer entry points (what a Julia `ccall` binds; buffers owned by the caller,
 * no pointer is retained after return).
 * ------------------------------------------------------------------------------------ */

/*
 * GBLUP fit of nrhs traits that share the same entries and loci.
 *   X          n x p column-major allele frequencies (ldx >= n); replaces the matrix that
 *              `extractxyetc(...; add_intercept=false)` returns (src/prediction.jl:129)
 *   Y          n x nrhs column-major phenotypes (ldy >= n), already filtered for missing
 *              values (src/prediction.jl:114-124)
 *   lambda     λ = σ²_e/σ²_u > 0
 *   devices    device ordinals (NULL/ndev = 0: this thread's device, see "Devices" above).
 *              With ndev > 1 SNP columns are sharded into contiguous blocks, one per entry;
 *              the partial GRMs of shards on one device are added there, and summed across
 *              devices with an RCCL all-reduce (communicators cached per device set).
 * Outputs (caller allocated):
 *   b_hat_out  (p+1) x nrhs column-major: [b0; b_1..b_p] per trait (src/linear.jl:218-221 layout)
 *   y_pred_out n x nrhs column-major GEBVs (= fitted values)
 *   mu_out     nrhs GLS intercepts μ̂ (may be NULL)
 *   q_out      number of polymorphic loci used (may be NULL)
 * Replaces: GLMNet.glmnetcv(X, y; alpha=0, ...) + coefficient selection, src/linear.jl:193-221.
 */
int gbm_gblup_fit(const double* X, int64_t n, int64_t p, int64_t ldx,
                  const double* Y, int64_t ldy, int64_t nrhs, double lambda,
                  const int* devices, int ndev,
                  double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out);

/* gbm_gblup_fit with the GRM arithmetic chosen per call (grm_mode: GBM_GRM_*); grm_used_out (may be NULL)
 * receives GBM_GRM_FP64 or GBM_GRM_EXACT, the GRM the fit used. The same for the entries below. */
int gbm_gblup_fit_ex(const double* X, int64_t n, int64_t p, int64_t ldx,
                     const double* Y, int64_t ldy, int64_t nrhs, double lambda,
                     const int* devices, int ndev, int grm_mode,
                     double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out, int* grm_used_out);

/*
 * gbm_gblup_fit with λ chosen per trait by REML — the drop-in `gblup(...; λ = :reml)` (Julia) /
 * `lambda_="reml"` (Python mirror). For each trait column, on the summed GRM of the call (built
 * once): minimise reference loglikreml (src/gwas.jl:450-483 with X = 1, V = σ²_u GRM + σ²_e I) for
 * y standardised as gwasprep does (src/gwas.jl:127-128), over the box σ²_e, σ²_u ∈ [eps, 1]
 * (src/gwas.jl:585; gwasreml's LBFGS at :577-590), σ²_u profiled in closed form per λ = σ²_e/σ²_u and
 * a scan + golden-section search over log λ (the same search as gbm_session_reml); then the GBLUP fit
 * of that trait at its λ (the original, unstandardised y). Outputs as gbm_gblup_fit, plus per trait
 * (nrhs each, any may be NULL): lambda_out, sigma2_e_out, sigma2_u_out. n >= 3.
 */
int gbm_gblup_fit_reml(const double* X, int64_t n, int64_t p, int64_t ldx,
                       const double* Y, int64_t ldy, int64_t nrhs,
                       const int* devices, int ndev,
                       double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out,
                       double* lambda_out, double* sigma2_e_out, double* sigma2_u_out);
int gbm_gblup_fit_reml_ex(const double* X, int64_t n, int64_t p, int64_t ldx,
                          const double* Y, int64_t ldy, int64_t nrhs,
                          const int* devices, int ndev, int grm_mode,
                          double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out,
                          double* lambda_out, double* sigma2_e_out, double* sigma2_u_out, int* grm_used_out);

/*
 * Same as gbm_gblup_fit for int8 dosages: X[i, j] = D[i + j*ldd] / ploidy (exact in fp64).
 * 1 byte per genotype cell over PCIe instead of 8.
 */
int gbm_gblup_fit_dosage_i8(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy,
                            const double* Y, int64_t ldy, int64_t nrhs, double lambda,
                            const int* devices, int ndev,
                            double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out);
int gbm_gblup_fit_dosage_i8_ex(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy,
                               const double* Y, int64_t ldy, int64_t nrhs, double lambda,
                               const int* devices, int ndev, int grm_mode,
                               double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out,
                               int* grm_used_out);

/*
 * Same as gbm_gblup_fit on the synthetic genotypes of gbm_dev_synth_genotypes (seed, loci
 * 0..p-1), generated on each device for its SNP-column shard: benchmark-scale
 * fits (config C3: 240 GB of fp64 X) with no host copy of X and no PCIe transfer.
 */
int gbm_gblup_fit_synthetic(uint64_t seed, int64_t n, int64_t p,
                            const double* Y, int64_t ldy, int64_t nrhs, double lambda,
                            const int* devices, int ndev,
                            double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out);
int gbm_gblup_fit_synthetic_ex(uint64_t seed, int64_t n, int64_t p,
                               const double* Y, int64_t ldy, int64_t nrhs, double lambda,
                               const int* devices, int ndev, int grm_mode,
                               double* b_hat_out, double* y_pred_out, double* mu_out, int64_t* q_out,
                               int* grm_used_out);

/*
 * Genomic relationship matrix only: G = Z Zᵀ / q (n x n, column-major == row-major since
 * symmetric, ldg >= n). Replaces GenomicBreedingCore.grmsimple(genomes).genomic_relationship_matrix
 * at src/gwas.jl:124-125 under the north-star formula (the Core implementation is un-vendored).
 */
int gbm_grm(const double* X, int64_t n, int64_t p, int64_t ldx, const int* devices, int ndev,
            double* G_out, int64_t ldg, int64_t* q_out);

/*
 * Ploidy-aware genomic relationship matrix, replacing
 * GenomicBreedingCore.grmploidyaware(genomes, ploidy=ploidy).genomic_relationship_matrix at
 * src/gwas.jl:117-121 (its caller infers ploidy = round(1 / min nonzero X), :119). The Core
 * implementation is un-vendored (parity unpinned); restated as VanRaden (2008) generalised to
 * ploidy k: with f_j = mean_i X[i, j] (allele frequency) and dosages kX,
 *   G = (kX − k1fᵀ)(kX − k1fᵀ)ᵀ / (k Σ_j f_j (1 − f_j)) = k (X − 1fᵀ)(X − 1fᵀ)ᵀ / Σ_j f_j (1 − f_j).
 * Every column is used (monomorphic ones centre to zero). denom_out (may be NULL) = Σ_j f_j (1 − f_j).
 * Same sharding over devices as gbm_grm.
 */
int gbm_grm_ploidy_aware(const double* X, int64_t n, int64_t p, int64_t ldx, int ploidy,
                         const int* devices, int ndev, double* G_out, int64_t ldg, double* denom_out);

/*
 * Column statistics of X: mean, std (ddof = 1, Julia `std`), keep = (std > eps(Float64) and
 * finite), q = Σ keep. Mirrors src/gwas.jl:112-113. Any of mean/sd/keep may be NULL.
 */
int gbm_colstats(const double* X, int64_t n, int64_t p, int64_t ldx, int device,
                 double* mean_out, double* sd_out, uint8_t* keep_out, int64_t* q_out);

/*
 * Linear predictor of `predict` (src/prediction.jl:228): out[i, t] = b_hat[0, t] + Σ_j X[i, j] b_hat[1 + j, t].
 * X n x p column-major (ldx >= n); b_hat (p+1) x nrhs column-major; out n x nrhs column-major.
 */
int gbm_predict(const double* X, int64_t n, int64_t p, int64_t ldx,
                const double* b_hat, int64_t ldb, int64_t nrhs, int device,
                double* out, int64_t ldo);

/* --------------------------------------------------------------------------------------
 * Device-level, stream-ordered entry points (all pointers are device pointers, `stream`
 * is a hipStream_t or NULL for the null stream). Nothing here synchronises the stream.
 * These are the stages the host entry points are built from; the multi-process
 * (one rank per GPU, RCCL all-reduce between grm and solve) path calls them directly.
 *
 * Device layout ("plan geometry", all row-major):
 *   Xt  p x ldx,  ldx >= gbm_dev_npad(n): locus j's n genotypes in Xt[j*ldx + 0..n-1]
 *   G   gbm_dev_gdim(n) x gbm_dev_gdim(n) with ld == gbm_dev_gdim(n): the GRM occupies
 *       rows/cols [0, npad); rows [npad, gdim) are the bordered right-hand sides used by
 *       the fused forward substitution of the Cholesky.
 * ------------------------------------------------------------------------------------ */

/* Padded individual count (multiple of the 128-row tile). */
int64_t gbm_dev_npad(int64_t n);
/* Dimension of the bordered V matrix: npad + 64 (room for 1 + nrhs <= 64 right-hand sides). */
int64_t gbm_dev_gdim(int64_t n);
/* Bytes of device workspace gbm_dev_grm needs for (n, p). */
int64_t gbm_dev_grm_workspace(int64_t n, int64_t p);
/* Bytes of device workspace gbm_dev_gblup_solve needs for (n, nrhs). */
int64_t gbm_dev_solve_workspace(int64_t n, int64_t nrhs);

/* Fill Xt with synthetic genotypes: locus (j0 + j) of a counter-based hash of (seed, i, j0 + j);
 * MAF f ~ U(0.05, 0.5) per locus, dosage ~ Binomial(2, f), X = dosage / 2.
 * Bit-identical to oracle/gbm_oracle.c:gbm_ref_synth_genotype. Zero-fills columns [n, ldx). */
int gbm_dev_synth_genotypes(double* Xt, int64_t ldx, int64_t p, int64_t n, uint64_t seed,
                            int64_t j0, void* stream);

/* The same synthetic genotypes as int8 dosages d = 2X (0, 1, 2), column-major n x p (ldd >= n):
 * locus j0 + j's n dosages at D + j*ldd. 1 byte per cell — the device-resident input of the
 * loci-streamed fit (config C3 on one GPU: 30 GB instead of 240 GB of fp64 X). */
int gbm_dev_synth_dosage_i8(int8_t* D, int64_t ldd, int64_t p, int64_t n, uint64_t seed, int64_t j0,
                            void* stream);

/* Expand int8 dosages (column-major D, n x p, ldd) into Xt (row-major p x ldx) as D/ploidy. */
int gbm_dev_expand_dosage_i8(const int8_t* D, int64_t ldd, int64_t n, int64_t p, int ploidy,
                             double* Xt, int64_t ldx, void* stream);

/* Zt row j <- (x_j − m_j)/s_j for kept loci, 0 for dropped ones and for the padding columns
 * [n, ldz). Zt may be Xt itself (in place, ldz == ldx). Writes mean/sd (p each), keep (p, int32)
 * and atomically adds the kept count into *q_dev (caller zeroes it). Replaces the column std,
 * monomorphic filter and standardisation of reference src/gwas.jl:112-115,127-130. */
int gbm_dev_standardize(const double* Xt, int64_t ldx, int64_t p, int64_t n, double* Zt, int64_t ldz,
                        double* mean, double* sd, int32_t* keep, int64_t* q_dev, void* stream);
/* As gbm_dev_standardize straight from int8 dosage rows (column-major D, n x p, ldd >= n; x = d/ploidy):
 * bit-identical to gbm_dev_expand_dosage_i8 followed by gbm_dev_standardize, out of place into Zt. */
int gbm_dev_standardize_i8(const int8_t* D, int64_t ldd, int64_t p, int64_t n, int ploidy, double* Zt, int64_t ldz,
                           double* mean, double* sd, int32_t* keep, int64_t* q_dev, void* stream);
/* As gbm_dev_standardize over the entry subset idx[0..n) of Xt's columns (gathered in the same
 * pass; out of place): the training-set extraction of reference src/prediction.jl:129 fused
 * with the standardisation. center_only != 0 centres without scaling and keeps every column
 * (sd reported as 1): the X that GLMNet sees with standardize=false (src/linear.jl:193-203). */
int gbm_dev_standardize_gather(const double* Xt, int64_t ldx, int64_t p, const int32_t* idx, int64_t n,
                               double* Zt, int64_t ldz, double* mean, double* sd, int32_t* keep,
                               int64_t* q_dev, int center_only, void* stream);

/* G[0:npad, 0:npad] (upper-triangular 128x128 tiles: rows <= columns) = Σ_j z_j z_jᵀ over
 * the p locus rows of Zt (unscaled: the RCCL all-reduce of multi-GPU shards sums this).
 * Zt and G 16-byte aligned, ldz and ldg even and >= gbm_dev_npad(n).
 * fp64 MFMA SYRK; = gbm_dev_grm_syrk followed by gbm_dev_grm_reduce. Replaces the GRM product
 * of GenomicBreedingCore.grmsimple (called at reference src/gwas.jl:124). */
int gbm_dev_grm(const double* Zt, int64_t ldz, int64_t p, int64_t n, double* G, int64_t ldg,
                void* workspace, int64_t ws_bytes, void* stream);
/* G += Σ_j z_j z_jᵀ over these p locus rows (same tiles and workspace as gbm_dev_grm): the loci-streamed
 * fit adds each chunk of loci into one G. Needs a multi-range plan (gbm_dev_grm_slices(n, p) > 1). */
int gbm_dev_grm_accumulate(const double* Zt, int64_t ldz, int64_t p, int64_t n, double* G, int64_t ldg,
                           void* workspace, int64_t ws_bytes, void* stream);
/* The two launches of gbm_dev_grm, separately (so a caller can time the SYRK kernel alone).
 * The SYRK splits the loci into ranges (gbm_dev_grm_slices of them) and writes one partial tile
 * per range into the workspace, which the reduce sums into G in a fixed order (bit-reproducible
 * run to run); with a single range the SYRK writes G directly and the reduce is a no-op. */
int gbm_dev_grm_syrk(const double* Zt, int64_t ldz, int64_t p, int64_t n, double* G, int64_t ldg,
                     void* workspace, int64_t ws_bytes, void* stream);
int gbm_dev_grm_reduce(int64_t n, int64_t p, double* G, int64_t ldg, const void* workspace, void* stream);
/* gbm_dev_standardize followed by gbm_dev_grm_syrk in one call, with the same bits in Zt, mean, sd, keep,
 * *q_dev (caller zeroes it) and, after gbm_dev_grm_reduce, G. Where the plan has several loci ranges and the
 * standardisation kernel fits beside the GRM tile workgroups (n <= 5120), only the first range's rows are
 * standardised ahead of the tiles; the rest are standardised on a helper stream beside the first range's
 * tiles. On return the caller's stream is ordered after all of it. GBM_GRM_STD_OVERLAP=0: always serial. */
int gbm_dev_standardize_grm_syrk(const double* Xt, int64_t ldx, int64_t p, int64_t n, double* Zt, int64_t ldz,
                                 double* mean, double* sd, int32_t* keep, int64_t* q_dev, double* G, int64_t ldg,
                                 void* workspace, int64_t ws_bytes, void* stream);
/* The upper 128x128 tiles of G as one contiguous array (packed size in doubles; pack; unpack):
 * half the bytes of G's npad x gdim rows, the form the multi-GPU partial-GRM all-reduce moves. */
int64_t gbm_dev_grm_packed_size(int64_t n);
int gbm_dev_grm_pack(const double* G, int64_t ldg, int64_t n, double* packed, void* stream);
int gbm_dev_grm_unpack(const double* packed, int64_t n, double* G, int64_t ldg, void* stream);
/* Number of loci ranges (split-K slices) the GRM plan uses for (n, p) on the current device. */
int gbm_dev_grm_slices(int64_t n, int64_t p);

/*
 * Solve the GBLUP system on G (as left by gbm_dev_grm, summed over shards):
 *   V = G/q + λI ; LLᵀ = V (blocked fp64 Cholesky, in place) ; μ̂ = 1ᵀV⁻¹y/1ᵀV⁻¹1,
 *   a = V⁻¹(y − 1μ̂), gebv = μ̂ + (y − 1μ̂) − λa  (reference src/gwas.jl:462-472,591-597).
 *   inv_q / q_dev  1/q given on the host, or (q_dev != NULL) read on the device from *q_dev
 *   Y      nrhs x ldy row-major (trait t's n phenotypes contiguous), 1 <= nrhs <= 63
 *   A_out  nrhs x lda row-major: a vectors (lda >= npad; zero in the padding)
 *   gebv   nrhs x lda row-major; mu nrhs; info (device int32): 0 or the 1-based failing pivot.
 *   workspace  >= gbm_dev_solve_workspace(n, nrhs) bytes.
 */
int gbm_dev_gblup_solve(double* G, int64_t ldg, int64_t n, double inv_q, const int64_t* q_dev, double lambda,
                        const double* Y, int64_t ldy, int64_t nrhs,
                        double* A_out, double* gebv, int64_t lda, double* mu, int32_t* info,
                        void* workspace, int64_t ws_bytes, void* stream);

/*
 * The same solve in phases, for a factorisation distributed over ranks (one process or device per
 * rank, each holding the full summed G): gbm_dev_gblup_solve == prepare; for kb = 0 .. npad/64 − 1
 * step gbm_dev_chol_group_size(n, kb): group(kb, rank = 0, nranks = 1); finish.
 * Distributed (nranks > 1, groups of >= 2 panels starting on a 128-row boundary), per group:
 *   [after an earlier distributed group] area_pack(kb, g) → all-gather of gbm_dev_chol_area_doubles
 *                                   per rank → area_unpack; factor_diag(kb): the group's diagonal
 *                                   area (64g x 64g), whose columns other ranks updated;
 *   group_panels(kb, rank, nranks)  the group's panels and row updates on the rank's own 128-column
 *                                   tiles (J ≡ rank mod nranks), the group's diagonal area and the
 *                                   right-hand sides;
 *   strip_pack(kb, g) → all-gather of gbm_dev_chol_strip_doubles per rank → strip_unpack_rows: every
 *                                   rank then holds the group's final rows at every column (and their
 *                                   lower copy, which the back substitution reads);
 *   group_update(kb, rank, nranks)  the trailing update on the rank's own tiles and the right-hand
 *                                   sides — 1/nranks of the O(n³) work per rank (or group_update_tiles
 *                                   over row ranges: the look-ahead, see below).
 * Before switching back to nranks = 1 for the tail, the ranks exchange every remaining row once
 * (strip_pack → all-gather → strip_unpack) and factor its first diagonal block (factor_diag).
 * gbm_dev_chol_group itself takes rank 0 of 1 only (the arguments stay for ABI stability).
 * Bit-identical to gbm_dev_gblup_solve. Replaces the redundant per-rank pinv/Cholesky of V at
 * reference src/gwas.jl:472,595 at multi-GPU scale.
 */
int gbm_dev_chol_prepare(double* G, int64_t ldg, int64_t n, double inv_q, const int64_t* q_dev, double lambda,
                         const double* Y, int64_t ldy, int64_t nrhs, int32_t* info, void* workspace,
                         int64_t ws_bytes, void* stream);
/* gbm_dev_chol_prepare for rank `rank` of a distributed factorisation (nranks > 1): V only on the columns
 * the rank reads before an exchange overwrites them (its own 128-column tiles, the first panel group's
 * area, the right-hand sides); nranks = 1 is gbm_dev_chol_prepare. */
int gbm_dev_chol_prepare_cols(double* G, int64_t ldg, int64_t n, double inv_q, const int64_t* q_dev, double lambda,
                              const double* Y, int64_t ldy, int64_t nrhs, int rank, int nranks, int32_t* info,
                              void* workspace, int64_t ws_bytes, void* stream);
/* Panels in the group that starts at 64-row block kb (0 past the end). At the dataflow tail (at most
 * GBM_CHOL_TAIL_FLOW rows left, default 8192 when npad > 12 288; never kb = 0) every remaining panel:
 * gbm_dev_chol_group then factors the rest in one launch, and group_panels / group_update refuse it. */
int64_t gbm_dev_chol_group_size(int64_t n, int64_t kb);
int gbm_dev_chol_group(double* G, int64_t ldg, int64_t n, int64_t kb, int rank, int nranks, int32_t* info,
                       void* workspace, int64_t ws_bytes, void* stream);
int gbm_dev_chol_group_panels(double* G, int64_t ldg, int64_t n, int64_t kb, int rank, int nranks, int32_t* info,
                              void* workspace, int64_t ws_bytes, void* stream);
int gbm_dev_chol_group_update(double* G, int64_t ldg, int64_t n, int64_t kb, int rank, int nranks, int32_t* info,
                              void* workspace, int64_t ws_bytes, void* stream);
/* group_update restricted to the rank's tiles with columns in [col_lo, col_hi) (col_lo on a 128-column
 * tile; the right-hand sides when col_hi >= gdim(n)); nranks >= 2. Two calls covering [64 (kb + g),
 * gdim) equal one group_update: the first (the next group's area) lets the area exchange run beside
 * the second. */
int gbm_dev_chol_group_update_cols(double* G, int64_t ldg, int64_t n, int64_t kb, int rank, int nranks,
                                   int64_t col_lo, int64_t col_hi, int32_t* info, void* workspace, int64_t ws_bytes,
                                   void* stream);
/* group_update_cols further restricted to the rows [row_lo, row_hi) (row_lo on a 128-row tile): the
 * look-ahead updates the next group's rows first, so that group's panels (group_panels) and row exchange
 * run beside the rest of the update (rows from the end of the next group on). */
int gbm_dev_chol_group_update_tiles(double* G, int64_t ldg, int64_t n, int64_t kb, int rank, int nranks,
                                    int64_t row_lo, int64_t row_hi, int64_t col_lo, int64_t col_hi, int32_t* info,
                                    void* workspace, int64_t ws_bytes, void* stream);
int gbm_dev_chol_factor_diag(double* G, int64_t ldg, int64_t n, int64_t kb, int32_t* info, void* workspace,
                             int64_t ws_bytes, void* stream);
/* Doubles per rank of the strip of rows [64 kb, 64 (kb + rows64)) over the tiles from column 64 kb. */
int64_t gbm_dev_chol_strip_doubles(int64_t n, int64_t kb, int64_t rows64, int nranks);
int gbm_dev_chol_strip_pack(const double* G, int64_t ldg, int64_t n, int64_t kb, int64_t rows64, int rank,
                            int nranks, double* buf, void* stream);
/* gathered: nranks consecutive packs (rank order), e.g. the output of an all-gather. */
int gbm_dev_chol_strip_unpack(double* G, int64_t ldg, int64_t n, int64_t kb, int64_t rows64, int nranks,
                              const double* gathered, void* stream);
/* The same over the square [64 kb, 64 (kb + rows64)) only (rows64 even): a group's diagonal area. */
int64_t gbm_dev_chol_area_doubles(int64_t n, int64_t kb, int64_t rows64, int nranks);
int gbm_dev_chol_area_pack(const double* G, int64_t ldg, int64_t n, int64_t kb, int64_t rows64, int rank,
                           int nranks, double* buf, void* stream);
int gbm_dev_chol_area_unpack(double* G, int64_t ldg, int64_t n, int64_t kb, int64_t rows64, int nranks,
                             const double* gathered, void* stream);
/* The transposed lower copy (read only by gbm_dev_chol_finish) of the rows [64 kb, 64 (kb + rows64)) for the
 * chunks other ranks solved. A driver may defer it to a stream of its own (the rows are final; nothing before
 * finish reads or writes those entries). */
int gbm_dev_chol_lower_copy(double* G, int64_t ldg, int64_t n, int64_t kb, int64_t rows64, int rank, int nranks,
                            void* stream);
/* strip_unpack of final factor rows (after group_panels) plus their lower copy for the columns this
 * rank did not compute (= strip_unpack + lower_copy). */
int gbm_dev_chol_strip_unpack_rows(double* G, int64_t ldg, int64_t n, int64_t kb, int64_t rows64, int rank,
                                   int nranks, const double* gathered, void* stream);
int gbm_dev_chol_finish(double* G, int64_t ldg, int64_t n, const double* Y, int64_t ldy, int64_t nrhs,
                        double lambda, double* A_out, double* gebv, int64_t lda, double* mu, int32_t* info,
                        void* workspace, int64_t ws_bytes, void* stream);

/* REML ingredients of a finished gbm_dev_gblup_solve (same G, workspace, n, nrhs), into device
 * memory: terms[0] = logdet(G/q + λI), terms[1] = 1ᵀV⁻¹1, terms[2+2t] = 1ᵀV⁻¹y_t,
 * terms[3+2t] = y_tᵀV⁻¹y_t — everything reference loglikreml (src/gwas.jl:450-483) needs with
 * X = 1, read off the bordered factorisation. */
int gbm_dev_gblup_terms(const double* G, int64_t ldg, int64_t n, int64_t nrhs, const void* workspace,
                        double* terms, void* stream);

/* Whitening of locus rows against the factor a finished gbm_dev_gblup_solve left behind (same G, n and
 * workspace; V = G/q + λI = UᵀU): every row r of R (rows x ldr row-major, individuals contiguous like Zt,
 * ldr >= gbm_dev_npad(n) even, 16-byte aligned) becomes r·U⁻¹ = U⁻ᵀr, in place. It reads the off-diagonal
 * 64x64 blocks of U in G's upper part and the inverses of the diagonal blocks in the workspace, on fp64 MFMA;
 * one workgroup per strip of 64 rows, strips independent. A row's result depends on that row alone (not on
 * rows, the strip or the launch it fell into); the padding columns [n, npad) stay 0 when they are 0. */
int gbm_dev_whiten_rows(const double* G, int64_t ldg, int64_t n, const void* solve_workspace, double* R,
                        int64_t ldr, int64_t rows, void* stream);

/* Symmetric fill of a GRM: K (npad x ldk row-major, out of place, ldk >= gbm_dev_npad(n) even, 16-byte aligned) gets
 * scale·G in both triangles, read only from the elements gbm_dev_grm / gbm_dev_grm_exact_i8 define: the 128x128
 * tiles with tile-row <= tile-column and, inside a diagonal tile, the 16x16 blocks with block-row <= block-column
 * (the row <= column half of the diagonal blocks). Everything else of G is never read; rows and columns [n, npad)
 * of K are zeros whatever G's padding holds; K[i, j] and K[j, i] are the same bits. ldg >= gbm_dev_npad(n). */
int gbm_dev_grm_symmetrize(const double* G, int64_t ldg, int64_t n, double scale, double* K, int64_t ldk,
                           void* stream);

/* Skinny product Yt = Qt·K with the symmetric K of gbm_dev_grm_symmetrize (zero padding). Qt, Yt: rows x ld
 * row-major vector blocks stored like locus rows (individuals contiguous, ld >= gbm_dev_npad(n) even, 16-byte
 * aligned, padding columns zero); rows = 16, 32, 48 or 64. fp64 MFMA, HBM-bound on K: the individual range is split
 * over workgroups (a count that depends on n alone) and the partial sums are added in a fixed order, so two calls
 * give the same bits and a row's result does not depend on the other rows of the call. workspace:
 * gbm_dev_rows_times_sym_workspace(n, rows) bytes, 16-byte aligned. */
int64_t gbm_dev_rows_times_sym_workspace(int64_t n, int64_t rows);
int gbm_dev_rows_times_sym(const double* K, int64_t ldk, int64_t n, const double* Qt, int64_t ldq, int64_t rows,
                           double* Yt, int64_t ldy, void* workspace, int64_t ws_bytes, void* stream);

/*
 * Marker effects on the standardised locus rows: B[t, j] = (Zt_j · a_t)/(q·sd_j) for kept
 * loci, 0 otherwise (B nrhs x ldb row-major), and msum[t] = Σ_j mean_j B[t, j] over this
 * shard (so that b0 = μ̂ − Σ_shards msum). q from inv_q or, if q_dev != NULL, from *q_dev.
 */
int gbm_dev_marker_effects(const double* Zt, int64_t ldz, int64_t p, int64_t n,
                           const double* A, int64_t lda, int64_t nrhs, double inv_q, const int64_t* q_dev,
                           const double* mean, const double* sd, const int32_t* keep,
                           double* B, int64_t ldb, double* msum, void* stream);

/* Bytes of device workspace gbm_dev_grm_exact_i8 needs for (n, p): the individual-major operand copies
 * (2 x npad x p bytes), the per-locus digits and the 128-bit centring terms. */
int64_t gbm_dev_grm_exact_workspace(int64_t n, int64_t p);
/* The GRM of diploid dosages (column-major D, n x p, ldd >= n, d in {0, 1, 2}, x = d/2) computed EXACTLY up to
 * the fp64 rounding of each locus weight 1/var_j: G = Σ_j w_j (d_j − t_j/n)(d_j − t_j/n)ᵀ, the GRM of the
 * standardised genotypes (reference src/gwas.jl:112-126 before the 1/q), as int8 MFMA GEMMs over the base-128
 * digits of the fixed-point weights with 128-bit centring. Also writes what
 * gbm_dev_standardize_i8 writes except Z: mean, sd, keep (per locus) and adds the kept count to *q_dev.
 * accum != 0: G += this GRM. *slices_out (optional): the digit count S (8-10) the weights needed.
 * Upper tiles of G are written (ldg >= gbm_dev_npad(n)); one host synchronisation per call (sizes S).
 * GBM_E_ARG on a dosage outside {0, 1, 2} or ploidy != 2. */
int gbm_dev_grm_exact_i8(const int8_t* D, int64_t ldd, int64_t p, int64_t n, int ploidy, double* G, int64_t ldg,
                         double* mean, double* sd, int32_t* keep, int64_t* q_dev, int accum, void* workspace,
                         int64_t ws_bytes, int32_t* slices_out, void* stream);
/* The status a gbm_dev_grm_exact_i8 launch left in its workspace (same n, p, workspace; synchronises the
 * stream): GBM_E_HIP when a locus weight did not fit its S base-128 digits (G invalid; xg_choose's bound rules it
 * out, this makes a violation loud), GBM_E_ARG for a dosage outside {0, 1, 2}, else GBM_OK. The C-ABI fits and
 * sessions call it after every exact GRM. */
int gbm_dev_grm_exact_status(const void* workspace, int64_t n, int64_t p, void* stream);

/* gbm_dev_marker_effects on int8 dosage rows (column-major D, n x p, ldd >= n, x = d/ploidy) instead of the
 * standardised fp64 rows: z = (x − mean_j)/sd_j is rebuilt in registers exactly as gbm_dev_standardize_i8
 * wrote it, so B and msum are bit-identical, at 1 byte read per cell (the loci-streamed fit's back-solve,
 * which keeps no fp64 Z). lda >= gbm_dev_npad(n), even. */
int gbm_dev_marker_effects_i8(const int8_t* D, int64_t ldd, int64_t p, int64_t n, int ploidy,
                              const double* A, int64_t lda, int64_t nrhs, double inv_q, const int64_t* q_dev,
                              const double* mean, const double* sd, const int32_t* keep,
                              double* B, int64_t ldb, double* msum, void* stream);

/*
 * ---- Device-resident genotype sessions: cross-validation fold farming and REML λ -----------
 * A session holds X (n x p, uploaded once) on one device and fits GBLUP on entry subsets; the
 * standardised training genotypes and their GRM are cached per training set, so further traits,
 * λ values and REML evaluations on the same set skip the SYRK. Replaces the per-fold model calls
 * of reference cvmultithread! (src/cross_validation.jl:151-207); use one session per device and
 * one host thread per session. Entry indices are 0-based rows of X, strictly increasing.
 */
typedef struct gbm_session gbm_session;
int gbm_session_create(const double* X, int64_t n, int64_t p, int64_t ldx, int device, gbm_session** out);
int gbm_session_create_dosage_i8(const int8_t* D, int64_t n, int64_t p, int64_t ldd, int ploidy, int device,
                                 gbm_session** out);
/* A session over the synthetic genotypes of gbm_dev_synth_genotypes (seed, loci 0..p-1), generated
 * on the device: benchmark-scale sessions (configs C4/C5) without a host copy of X. */
int gbm_session_create_synthetic(uint64_t seed, int64_t n, int64_t p, int device, gbm_session** out);
void gbm_session_destroy(gbm_session* s);
/* GRM arithmetic of the session's training GRMs (GBM_GRM_*; default GBM_GRM_DEFAULT = the GBM_GRM variable):
 * exact / auto build them with the exact-integer kernels when the genotypes are diploid dosages/2 (checked once
 * on the device). The training-set cache is keyed by the GRM used as well. */
int gbm_session_set_grm_mode(gbm_session* s, int grm_mode);
/* The GRM the cached training set was built with: GBM_GRM_FP64, GBM_GRM_EXACT, or -1 before the first fit. */
int gbm_session_grm_used(gbm_session* s, int* grm_used);
/* gbm_gblup_fit on the rows idx[0..n_train) of the session's X; Y holds the training phenotypes
 * (n_train x nrhs, column-major). */
int gbm_session_gblup_fit(gbm_session* s, const int64_t* idx, int64_t n_train, const double* Y, int64_t ldy,
                          int64_t nrhs, double lambda, double* b_hat_out, double* y_pred_out, double* mu_out,
                          int64_t* q_out);
/* out[t*ldo + i] = b_hat[t*ldb] + X[idx[i], :] · b_hat[t*ldb + 1 : t*ldb + 1 + p] on the device
 * (reference predict, src/prediction.jl:228). */
int gbm_session_predict(gbm_session* s, const int64_t* idx, int64_t n_val, const double* b_hat, int64_t ldb,
                        int64_t nrhs, double* out, int64_t ldo);
/* Reference loglikreml (src/gwas.jl:450-483) with X = 1 (intercept) and GRM = ZZᵀ/q of the
 * training rows: out[k] = 0.5 logdet V + yᵀPy + logdet(XᵀV⁻¹X), V = σ²_u[k] GRM + σ²_e[k] I, for
 * y as given. One Cholesky per (σ²_e, σ²_u) pair. */
int gbm_session_reml_objective(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                               const double* sigma2_e, const double* sigma2_u, int64_t m, double* out);
/* REML choice of λ = σ²_e/σ²_u: minimises that objective for y standardised as gwasprep does
 * (src/gwas.jl:127-128) over the reference's box σ²_e, σ²_u ∈ [eps, 1] (src/gwas.jl:585), with
 * σ²_u profiled in closed form per λ and a scan + golden-section search over log λ. */
int gbm_session_reml(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y, double* lambda_out,
                     double* sigma2_e_out, double* sigma2_u_out, double* objective_out);
/* Ridge path of reference ridge (GLMNet alpha = 0, standardize = false, intercept;
 * src/linear.jl:193-203) on the rows idx[0..n_train): for each lambdas[k] (glmnet scale, objective
 * (1/2n)‖y − a0 − Xb‖² + (λ/2)‖b‖²) the exact minimiser, b_path_out[k*(p+1)] = a0 and
 * b_path_out[k*(p+1) + 1 + j] = b_j; optionally pred_out[k*n_eval + i] = a0 + X[idx_eval[i], :] b. */
int gbm_session_ridge_path(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                           const double* lambdas, int64_t nl, double* b_path_out, const int64_t* idx_eval,
                           int64_t n_eval, double* pred_out);
/* glmnet's largest λ for alpha = 0 (alpha floored at 1e-3): max_j |x_cjᵀ(y − ȳ)| / n / 1e-3. */
int gbm_session_ridge_lambda_max(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                                 double* lambda_max);
/*
 * Lasso / elastic-net path of reference lasso (GLMNet alpha = 1, standardize = false, intercept;
 * src/linear.jl:333-343) on the rows idx[0..n_train), by cyclic coordinate descent on an active set.
 * (Additive: GBM_VERSION stays 212.)
 *
 * Model, for alpha in (0, 1] and a user λ (glmnet's elastic net; σ_y = the population sd of the training y,
 * by which glmnet's elnet divides λ): minimise
 *   (1/2n)‖y − a0 − Xb‖² + λ alpha ‖b‖₁ + (λ (1 − alpha)/(2 σ_y)) ‖b‖².
 * With x_j the centred column, x2_j = x_jᵀx_j, e the residual, thr = n λ alpha and
 * den_j = x2_j + n λ (1 − alpha)/σ_y, one coordinate step is
 *   g = x_jᵀe + x2_j b_j;  b_new = sign(g) max(|g| − thr, 0)/den_j;  e += (b_j − b_new) x_j.
 * A column with x2_j = 0 keeps b_j = 0 and is never admitted (glmnet's ju = 0). a0 = ȳ − Σ_j mean_j b_j.
 * alpha = 0 is refused (GBM_E_ARG): gbm_session_ridge_path solves that case exactly.
 *
 * Schedule per λ (warm start: b, e and the active list are carried from the previous λ on the device):
 *   1. coordinate-descent passes over the active list (in order of admission; within one screen ascending j)
 *      until a pass's max_j (x2_j/n) δ_j² < tol σ_y², or max_passes passes were run at this λ;
 *   2. screen g = Zᵀe over all p loci: every inactive j with |g_j| > thr and x2_j > 0 is admitted;
 *   3. if any was admitted go to 1, else this λ is done.
 * An empty active list skips step 1. The active list never shrinks and is capped at min(p, 2 gbm_dev_npad(n_train))
 * markers: a fit that needs more returns GBM_E_ARG.
 * Early stop (glmnet's elnet): with mnl = min(5, nl), after λ number k >= mnl (from 1) the path stops when
 * dev_k > dev_max or (fdev > 0 and dev_k − dev_{k−1} < fdev dev_k), dev_0 = 0; that λ is the last one kept.
 * glmnet's values are dev_max = 0.999, fdev = 1e-5; fdev = 0 with dev_max = +inf disables the rule.
 *
 * lambdas: nl values, finite, > 0, non-increasing. tol > 0, max_passes >= 1. Outputs as gbm_session_ridge_path
 * (b_path_out nl x (p+1), row k = [a0; b]; pred_out[k*n_eval + i]); rows past *nl_done_out are not written.
 * dev_ratio_out[k] = 1 − ‖e‖²/‖y − ȳ‖², passes_out[k], nnz_out[k] (nl each) and nl_done_out may be NULL.
 * Reaching max_passes at some λ still returns GBM_OK, and gbm_last_error() then holds a message starting
 * "warning:" (it is "" after any other successful call of this function). Uses the training-set cache of
 * gbm_session_ridge_path (a ridge path on the same rows is a cache hit and vice versa). Deterministic: two
 * calls give the same bits. glmnet's first λ for this alpha is gbm_session_ridge_lambda_max · 1e-3/max(alpha, 1e-3).
 */
int gbm_session_enet_path(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y, double alpha,
                          const double* lambdas, int64_t nl, double tol, int64_t max_passes, double dev_max, double fdev,
                          double* b_path_out /* nl x (p+1), as gbm_session_ridge_path */,
                          const int64_t* idx_eval, int64_t n_eval, double* pred_out /* as ridge_path */,
                          int64_t* nl_done_out, double* dev_ratio_out, int64_t* passes_out, int64_t* nnz_out);
/* GRM builds and cache hits so far. */
int gbm_session_stats(gbm_session* s, int64_t* grm_builds, int64_t* grm_hits);
/* GWAS scan over all p loci on the rows idx[0..n_train) (reference gwasreml / gwasols, src/gwas.jl). For the
 * standardised locus column x_j (the session's cached Z) and X = [1, C, x_j]:
 *   model 0 (mixed model): V = σ²_u·ZZᵀ/q + σ²_e·I, z_j = b[end]/sqrt(inv(XᵀV⁻¹X)[end]) (src/gwas.jl:591-599),
 *     computed as a Schur complement on rows whitened against the cached GRM's Cholesky factor
 *     (gbm_dev_whiten_rows, one bordered solve per call); b_j = b[end];
 *   model 1 (OLS): V = I, z_j = b[end]/sqrt(inv(XᵀX)[end]) (src/gwas.jl:241-245; like the reference, no
 *     residual variance enters).
 * y (n_train) is standardised inside as gwasprep does (src/gwas.jl:128). C: extra covariates, column-major
 * n_train x kc (ldc >= n_train), 0 <= kc <= 7; the intercept is always in the model. sigma2_e, sigma2_u (model 0):
 * both > 0 = used as given; either NaN = estimated ONCE by the null-model REML of gbm_session_reml (intercept
 * only). z_out, b_out (p each; b_out may be NULL); sigma2_out (2, may be NULL): the (σ²_e, σ²_u) used (NaN for
 * model 1); tested_out (may be NULL): the loci tested. Loci that are not polymorphic in the training rows, or that
 * lie in the span of the covariates (Schur complement <= 1e-12 x_jᵀV⁻¹x_j), get z = b = 0 and are not counted.
 * Deliberate differences from the reference: (1) the variance components are estimated once under the null
 * model (the usual P3D/EMMAX approximation), where the reference re-runs LBFGS for every marker; (2) the
 * relationship matrix is K = ZZᵀ/q as in gbm_session_reml_objective, where the reference column-standardises K
 * (which makes it non-symmetric); (3) the mixed model uses this simple GRM only (no ploidy-aware variant).
 * The cached Z and GRM are not written: a later fit on the same idx is a cache hit with unchanged bits.
 * GBM_GWAS_CHUNK (loci) overrides the chunk of rows whitened at a time (default: one 64-row strip per compute
 * unit, balanced over the chunks; the chunk buffer stays under 768 MB). */
int gbm_session_gwas(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y, const double* C,
                     int64_t ldc, int64_t kc, int model, double sigma2_e, double sigma2_u, double* z_out,
                     double* b_out, double* sigma2_out, int64_t* tested_out);

/* Leading eigenpairs of the relationship matrix of the rows idx[0..n_train) on the device (the population-structure
 * covariates of a GWAS; reference gwasols' PC1, src/gwas.jl:130,234), from the cached GRM: no n² download.
 *   kind GBM_PCS_GRM:       M = K = ZZᵀ/q, the matrix gbm_session_gwas uses;
 *   kind GBM_PCS_REFERENCE: M = K̃HK̃ᵀ with K̃ = (K − 1mᵀ)D⁻¹ (K's columns standardised: m the column means, D the
 *     ddof-1 column standard deviations) and H = I − 11ᵀ/n: the matrix whose first eigenvector the reference's
 *     fit(PCA, K̃; maxoutdim = 1) returns. M is never formed: MQ = KW − 1(mᵀW), W = D⁻¹H D⁻¹(KQ − m(1ᵀQ)), two
 *     products with K. GBM_E_DATA when a column of K has a standard deviation <= eps·(the largest).
 * Iteration: an orthonormal block Q of 32 vectors (start: a fixed counter-hash block); Y = MQ
 * (gbm_dev_rows_times_sym); T = QᵀY = SΘSᵀ on the host (cyclic Jacobi, gbm_debug_sym_eig); Ritz residuals
 * r_i = ‖Y s_i − θ_i Q s_i‖₂/θ_1 for i < k on the device; stop when max_i r_i < tol or after max_iter iterations;
 * otherwise Q = Y orthonormalised (CholQR, twice). 1 <= k <= 16, n_train >= 64.
 * The block is always 32 wide, whatever k: GBM_E_DATA ("the block lost rank") when a Cholesky pivot of a CholQR pass
 * falls to 1e-13 of its diagonal entry, i.e. when M has fewer than 32 eigenvalues that the block can tell from zero
 * (fewer than about 31 polymorphic loci, since rank K <= q and rank K̃HK̃ᵀ <= q + 1; or a spectrum that decays
 * past about 3e-7·λ₁ within the 32 leading values), also for k = 1; nothing is written to the outputs then. Also
 * GBM_E_DATA: a NaN/Inf in the projected matrix, or no positive Ritz value. A caller with such inputs takes the
 * eigenvectors on the host (as gbm.gwas.gwasols does).
 * vecs_out (n_train x k column-major): v_i = Q s_i with unit 2-norm, signed so that its component of largest
 * magnitude is positive (the lowest index wins ties); vals_out (k): θ_i, descending; trace_out (may be NULL): tr M
 * (kind 0: Σ K_ii, so θ_i/trace is the explained share); resid_out (k, may be NULL): the r_i of the last iteration;
 * iters_out (may be NULL): iterations run. Reaching max_iter returns GBM_OK with resid_out above tol, and
 * gbm_last_error() then starts with "warning:" (it is "" after a converged call). Deterministic: two calls give the
 * same bits. The training set is cached as by gbm_session_gblup_fit (a later fit or scan on the same idx is a cache
 * hit with unchanged bits); the cached Z and GRM are not written, the symmetric K lives in the solve's scratch copy. */
#define GBM_PCS_GRM 0
#define GBM_PCS_REFERENCE 1
int gbm_session_pcs(gbm_session* s, const int64_t* idx, int64_t n_train, int kind, int64_t k, double tol,
                    int64_t max_iter, double* vecs_out /* n_train x k column-major */, double* vals_out /* k */,
                    double* trace_out /* may be NULL */, double* resid_out /* k, may be NULL */,
                    int64_t* iters_out /* may be NULL */);

/* Epistasis feature scan on the training rows idx (0-based, strictly increasing, n_train >= 3) and the loci `loci`
 * (0-based, in range, distinct; NULL: all p, then l = p): reference transform2 (src/transformation.jl:319-468) for
 * the binary operations and transform1 (:130-238) for the unary ones, without their l² (l) least-squares calls.
 * Model: with x_j = X[idx, loci[j]] + eps (|·| of that when use_abs), yc = y − ȳ and f = op(x_i, x_j) (binary) or
 * op(x_j) (unary), the slope of [1, f] \ y is β = S_fy/S_ff, S_fy = Σ_k (f_k − f̄) yc_k, S_ff = Σ_k (f_k − f̄)².
 * Binary: β of the l² ordered pairs, flat index i·l + j, i = j included; with `commutative` only j >= i is computed
 * and the rest are 0 (:374-379). Unary: l slopes, flat index j; `commutative` must be 0.
 * A locus whose ddof-1 variance of x_j is below var_threshold is skipped: every pair that holds it has β = 0
 * (:382-387; :181-186).
 * Accumulation: per pair Σ(f − c), Σ(f − c)² and Σ(f − c)·yc over k < n_train in the order k = 0, 1, …, with the
 * shift c = the pair's own mean of f over its first min(n_train, 32) rows: c lies within the spread of f, so
 * S_ff = Σ(f − c)² − (Σ(f − c))²/n does not cancel (f at k = 0 alone can be an outlier: x = 0 under
 * log10epsdivlog10eps gives f = 0.98 among values near 0.02, which cost a factor 40 in S_ff's rounding);
 * S_fy = Σ(f − c)·yc − (Σ(f − c)/n)·Σyc with Σyc the sum of the rounded yc in the same order, which is Σ(f − f̄)·yc:
 * the rounding of ȳ does not enter the slope; Σf² = Σ(f − c)² + 2cΣ(f − c) + nc².
 * Degenerate rule (a deliberate difference): the reference solves [1, f] \ y by pivoted QR (Julia's ldiv! for
 * QRPivoted) with rcond = min(size)·eps = 2·eps; for [1, f] the squared ratio of R's diagonal is
 * n·S_ff/max(n, Σf²)². A pair with n·S_ff <= (2·eps)²·max(n, Σf²)² is declared degenerate here: β = 0, counted in
 * *degenerate_out, never selected. The reference returns the minimum-norm slope there (a constant feature such
 * as addnorm(x, 1 − x) gets β ≈ 0.4·ȳ and can be selected). The rcond value and the behaviour at the boundary are
 * unpinned against Julia (no Julia build was available to run them).
 * Non-finite f (raise of a negative base, log10 of a negative number, 1/(1 + x) at x = −1, …): seen through the
 * pair's sums; any tested pair with a non-finite sum or slope (an overflow of Σ(f − c)² among them) makes the call
 * return GBM_E_DATA (reference: ArgumentError asking for a larger ϵ / use_abs, :391-405); nothing is written.
 * Selection: the k (1 <= k <= 65 536, k <= the number of slopes) largest |β| among the slopes with |β| > eps, in
 * descending |β|, ties to the lower flat index: the reference's stable sortperm(abs.(β), rev = true)[1:k] followed
 * by its > ϵ filter (:420-428). top_index_out / top_beta_out (k each) receive *n_top_out <= k entries.
 * Panels: the slopes are computed in panels of i-rows, panel_rows of them (a multiple of 64; 0: as many as keep a
 * panel's slopes under 256 MB, at least 64); each panel yields its own k candidates on the device and the host
 * merges the panels' candidates by the same rule, so the result does not depend on panel_rows. beta_out (l·l
 * row-major [i·l + j], or l; may be NULL) receives every slope and is allowed only when one panel holds them all
 * (GBM_E_ARG otherwise). tested_out / degenerate_out (may be NULL): pairs whose sums were formed (not skipped, not
 * below the diagonal under `commutative`), and the degenerate ones among them.
 * Determinism: one thread owns a pair and adds its terms in one fixed order that does not depend on the pair's
 * place in the grid, so two pairs with bitwise equal columns get bitwise equal β, as do (i, j) and (j, i) under
 * mult and addnorm, and two calls return the same bits.
 * GBM_E_ARG: a bad op, k, idx, loci, panel_rows, n_train < 3, eps negative or not finite, NaN/Inf in y.
 * The scan does not touch the session's training-set cache (a later fit on the same idx is a hit or a miss exactly
 * as without the scan, with unchanged bits).
 * Other differences from the reference: f is evaluated by the device's pow / log10 (last-ulp differences); pairs
 * that hold a skipped locus or lie below the diagonal are evaluated and discarded, never reported. */
#define GBM_PAIR_OP_MULT 0
#define GBM_PAIR_OP_ADDNORM 1
#define GBM_PAIR_OP_RAISE 2
#define GBM_PAIR_OP_SQUARE 3
#define GBM_PAIR_OP_INVONEPLUS 4
#define GBM_PAIR_OP_LOG10EPS 5
int gbm_session_pair_scan(gbm_session* s, const int64_t* idx, int64_t n_train, const double* y,
                          const int64_t* loci /* NULL = all p */, int64_t l, int op, double eps, int use_abs,
                          double var_threshold, int commutative, int64_t panel_rows /* 0 = by budget */,
                          int64_t k, int64_t* top_index_out, double* top_beta_out, int64_t* n_top_out,
                          double* beta_out /* l*l (binary) or l (unary), may be NULL */,
                          int64_t* tested_out, int64_t* degenerate_out);

/*
 * ---- Bayesian ridge regression (BGLR model "BRR") by Gibbs sampling -------------------------
 * Replaces the Rscript/BGLR call of reference bglr()/bayesian() (src/bayes.jl:28-105,158-224)
 * for bglr_model = "BRR": BGLR's single-site sampler (intercept, markers in order with residual
 * updates, σ²_b and σ²_e scaled-inverse-χ² draws; priors df0, R2 as BGLR's defaults 5 and 0.5),
 * n_iter iterations, running posterior means every `thin` iterations after n_burnin.
 * b_hat_out (p+1) = [posterior mean of μ; posterior means of b]; y_pred_out (n, optional) =
 * b0 + X b; var_out (2, optional) = posterior means of [σ²_e, σ²_b]. X column-major n x p.
 * Counter-based random numbers from `seed` (no R RNG stream: results are reproducible but the
 * chain is not BGLR's sample path).
 * Schedule: one persistent super-block sweep launch per iteration when its workgroups fit one per CU
 * (byte-exact genotypes, n <= 48 x CUs), else one launch per marker block. If the sweep's
 * inter-workgroup hand-offs time out (its workgroups could not all be resident, e.g. another process
 * fills the device) the fit is re-run from the start on the per-launch path: the call still returns
 * GBM_OK (the results are valid) and gbm_last_error() then holds a message starting "warning:" (it
 * is "" after any other successful call of this function).
 */
int gbm_brr_fit(const double* X, int64_t n, int64_t p, int64_t ldx, const double* y, int64_t n_iter,
                int64_t n_burnin, int64_t thin, double r2, double df0, uint64_t seed, int device,
                double* b_hat_out, double* y_pred_out, double* var_out);

/*
 * ---- BayesA, BayesB and BayesC by Gibbs sampling ---------------------------------------------
 * Replaces the Rscript/BGLR call of reference bglr()/bayesian() (src/bayes.jl:28-105) behind the
 * model functions bayesa, bayesb and bayesc (src/linear.jl:440-626) for the Gaussian response.
 * The sampler is BGLR 1.x's as restated here (BGLR is not vendored: sample-path parity with BGLR
 * itself is unpinned); excluded effects are drawn from their prior and the indicator is drawn
 * conditional on the current b_j.
 *
 * Priors: df0 (BGLR: 5), r2 (0.5), prob_in (0.5), counts (10); shape0 = 1.1.
 * Initial state: vy = var(y) (ddof 1), x2_j = Σ_i x_ij², MSx = Σ_j x2_j/n − Σ_j mean_j²;
 *   S0e = vy (1 − r2)(df0 + 2), varE = S0e/(df0 + 2);
 *   S0 = vy r2/MSx (df0 + 2) (BayesA), that divided by prob_in (BayesB, BayesC);
 *   S = S0, rate0 = (shape0 − 1)/S0, varB_j = S0/(df0 + 2) (BayesC: one common varB);
 *   π = prob_in, cIn = counts prob_in, cOut = counts (1 − prob_in);
 *   μ = mean(y), e = y − μ, b = 0, d = 1.
 * Random numbers: counter-based u01 / normal / χ²(seed, stream, counter) as gbm_brr_fit's, with
 *   Gamma(shape k, rate r) = χ²(2k)/(2r). Iteration `it` uses the streams A = 8 it: marker normals
 *   (A, j), the μ normal (A, 0xFFFFFFFF); A+1: χ² of BayesC's varB; A+2: χ² of varE; A+3: the
 *   indicator uniforms u_j = u01(A+3, j); A+4: the Gamma of S; A+5, A+6: the two Gammas of π's Beta
 *   draw; and 2^63 | it 2^40 | j: the χ² of marker j's variance.
 * One iteration:
 *   1. μ ~ N(Σ(e + μ_old)/n, varE/n); e = (e + μ_old) − μ.
 *   2. For j = 0 … p−1 in order: eff = d_j b_j, r = x_jᵀe + x2_j eff, ξ the marker's normal.
 *      BayesA: d_new = 1. BayesB, BayesC: logOdds = log(π/(1−π)) + (2 b_j r − b_j² x2_j)/(2 varE),
 *      d_new = [logOdds > log(u_j/(1−u_j))]. If d_new = 0: b_new = sqrt(varB_j) ξ; otherwise
 *      C = x2_j/varE + 1/varB_j, b_new = (r/varE)/C + sqrt(1/C) ξ. Then e += (eff − d_new b_new) x_j,
 *      b_j = b_new, d_j = d_new.
 *   3. BayesA, BayesB: varB_j = (S + b_j²)/χ²(df0 + 1) for every j, then
 *      S = Gamma(p df0/2 + shape0, Σ_j 1/varB_j / 2 + rate0). BayesC: varB = (Σ_j b_j² + S)/χ²(df0 + p)
 *      over all b_j, then S = Gamma(df0/2 + shape0, 1/(2 varB) + rate0). BayesB, BayesC: m = Σ d_j,
 *      g1 = Gamma(m + cIn, 1), g2 = Gamma(p − m + cOut, 1), π = g1/(g1 + g2).
 *      All: varE = (Σe² + S0e)/χ²(df0 + n).
 *   4. When (it + 1) % thin == 0 and it + 1 > n_burnin: running means of d_j b_j, d_j, μ, varE,
 *      mean_j varB_j and π.
 * b_hat_out (p+1) = [mean of μ; means of d_j b_j]; y_pred_out (n, optional) = b0 + X b;
 * var_out (3, optional) = means of [varE, mean_j varB_j, π]; pip_out (p, optional) = means of d_j
 * (the posterior inclusion probabilities; all 1 for BayesA). X column-major n x p.
 * GBM_E_ARG for another model, gbm_brr_fit's argument checks, df0 < 1, prob_in outside (0, 1),
 * counts prob_in < 1 or counts (1 − prob_in) < 1 (the gamma sampler needs shapes >= 1),
 * n_iter > 2^23 or p >= 2^40 (the per-marker stream). One launch per 64-marker block (byte or fp64
 * genotype storage as gbm_brr_fit: GBM_BRR_I8); never the super-block sweep.
 */
#define GBM_BAYES_A 1
#define GBM_BAYES_B 2
#define GBM_BAYES_C 3
int gbm_bayes_fit(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                  int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                  double counts, uint64_t seed, int device, double* b_hat_out /* p+1 */,
                  double* y_pred_out /* n, may be NULL */, double* var_out /* 3; may be NULL */,
                  double* pip_out /* p, may be NULL */);

/*
 * ---- Several BayesA / BayesB / BayesC chains over one genotype matrix -------------------------
 * nchains (1 to GBM_BAYES_MAX_CHAINS) independent gbm_bayes_fit chains on the same X in one pass: the
 * models of a cross-validation fold, the traits of a panel, the seeds of a convergence check. Chain c
 * has the model models[c], the phenotypes Y[c ldy .. c ldy + n), the priors r2[c], df0[c], prob_in[c],
 * counts[c] and the seed seeds[c]; the schedule (n_iter, n_burnin, thin) is common. X is uploaded,
 * quantised and its Gram blocks are built once; every launch of an iteration serves all chains (the
 * chain launch runs four chains per workgroup, one per wave). (Additive: GBM_VERSION stays 212.)
 *
 * Every output of chain c has the bits that gbm_bayes_fit returns for the same model, X, y, priors,
 * schedule and seed: b_hat_out[c ldb ..] (p+1), y_pred_out[c ldp ..] (n; may be NULL),
 * var_out[3c ..] (3; may be NULL), pip_out[c ldpip ..] (p; may be NULL).
 * GBM_E_ARG, before any device work: nchains outside [1, 32]; a NULL among models, X, Y, r2, df0,
 * prob_in, counts, seeds, b_hat_out; ldy < n, ldb < p + 1, ldp < n, ldpip < p (of the outputs given);
 * gbm_bayes_fit's checks for every chain, with "chain c" (0-based) in the error text.
 * Not offered: the ordinal response, BRR, more than 32 chains per call, chains on different markers,
 * chain traces. Chains on different individuals: gbm_bayes_fit_multi_rows.
 */
#define GBM_BAYES_MAX_CHAINS 32
int gbm_bayes_fit_multi(int64_t nchains, const int* models, const double* X, int64_t n, int64_t p, int64_t ldx,
                        const double* Y, int64_t ldy, int64_t n_iter, int64_t n_burnin, int64_t thin,
                        const double* r2, const double* df0, const double* prob_in, const double* counts,
                        const uint64_t* seeds /* each of length nchains */, int device,
                        double* b_hat_out, int64_t ldb /* (p+1) x nchains */,
                        double* y_pred_out, int64_t ldp /* n x nchains, may be NULL */,
                        double* var_out /* 3 x nchains, may be NULL */,
                        double* pip_out, int64_t ldpip /* p x nchains, may be NULL */);

/*
 * ---- Several chains over one genotype matrix, each on its own rows (the folds of a cross-validation) ----
 * gbm_bayes_fit_multi with a training set per chain: rows holds nsets sets as n bytes each (pitch ldrows; 1 = a
 * training row, 0 = held out) and chain c trains on the set set_of[c]. Chain c is the sampler of gbm_bayes_fit on
 * the rows S_c = {i : rows[set_of[c] ldrows + i] = 1} taken in increasing order, with the phenotypes Y[S_c, c]:
 * every quantity of gbm_bayes_fit's text that sums over individuals runs over S_c with n_c = |S_c| in place of n
 * (vy, x2_j, MSx, μ's mean and variance, x_jᵀe, Σe², the degrees of freedom df0 + n_c). The random streams are
 * unchanged: they are indexed by marker and iteration, never by individual. Y at rows outside S_c is never read
 * as a number and may be NaN. X is uploaded and quantised once and every launch of an iteration serves all
 * chains; column statistics and Gram blocks are built once per set, so the models of a fold that name one set
 * share them. (Additive: GBM_VERSION stays 212.)
 *
 * y_pred_out[c ldp + i] = b0 + X[i,:] b for all n rows: at the rows outside S_c it is the fold's prediction.
 * b_hat_out, var_out and pip_out as gbm_bayes_fit_multi. With one set of all rows every output has the bits of
 * gbm_bayes_fit_multi; with a set that holds the first n_c rows, b_hat_out, var_out and pip_out have the bits of
 * gbm_bayes_fit on those rows (held-out rows add exact zeros to sums of a fixed order).
 * GBM_E_ARG, before any device work, with "chain c" or "set s" (0-based) in the text: gbm_bayes_fit_multi's own
 * refusals (gbm_bayes_fit's checks on each chain's rows); nsets outside [1, nchains]; a NULL rows or set_of;
 * ldrows < n; a set_of entry outside [0, nsets); a set with fewer than 3 rows or with a byte other than 0 or 1; a
 * non-finite Y inside a chain's set. GBM_E_DATA naming the set: its markers have no variance on its rows
 * (MSx <= 0).
 * Not offered: the ordinal response, BRR, more than 32 chains per call, chains on different markers, chain
 * traces.
 */
int gbm_bayes_fit_multi_rows(int64_t nchains, const int* models, const double* X, int64_t n, int64_t p, int64_t ldx,
                             const double* Y, int64_t ldy,
                             int64_t nsets, const uint8_t* rows /* nsets x n, pitch ldrows >= n; 1 = training row */,
                             int64_t ldrows, const int* set_of /* nchains, each in [0, nsets) */,
                             int64_t n_iter, int64_t n_burnin, int64_t thin, const double* r2, const double* df0,
                             const double* prob_in, const double* counts, const uint64_t* seeds, int device,
                             double* b_hat_out, int64_t ldb, double* y_pred_out, int64_t ldp,
                             double* var_out, double* pip_out, int64_t ldpip);

/*
 * ---- BayesA, BayesB and BayesC with an ordinal response (threshold model) -------------------
 * The reference's bayesian(...; response_type = "ordinal") (src/bayes.jl:28-36, 161-172): BGLR's
 * probit threshold model as restated here (BGLR is not vendored: parity with BGLR itself is
 * unpinned). It is gbm_bayes_fit's chain on a latent liability y* with the residual variance fixed
 * at 1. (Additive: GBM_VERSION stays 212.)
 *
 * Classes and start thresholds: the K classes are the distinct values of y in sorted order
 *   (2 <= K <= 32), z_i in {0 … K−1} the class of individual i; t_0 = −∞, t_K = +∞ and, with cum_k the
 *   number of individuals in the classes below k, t_k = Φ⁻¹(cum_k/n) for k = 1 … K−1. y*_i lies in
 *   [t_{z_i}, t_{z_i+1}]. varE ≡ 1 is never drawn.
 * Truncated normal TN(m; a, b; u), by inverse CDF from one uniform u: α = a − m, β = b − m; if α >= 0
 *   reflect, (α, β) ← (−β, −α); pa = Φ(α), pb = Φ(β); x = Φ⁻¹(pa + u (pb − pa)) clamped to [α, β], or,
 *   when pb − pa is not > 0 or that x is not finite (pa + u (pb − pa) rounded to 0 or to 1, where Φ⁻¹ is
 *   −∞ or +∞, in an interval whose end on that side is infinite), the finite end of [α, β] nearer 0 (at
 *   most one end is infinite); the result is m − x after a reflection, else m + x: always finite.
 *   Φ(x) = erfc(−x/√2)/2 (0 at −∞, 1 at +∞); Φ⁻¹ is Wichura's AS241 PPND16 in fp64, the library's own
 *   routine (csrc/gibbs_common.h), with Φ⁻¹(p <= 0) = −∞ and Φ⁻¹(p >= 1) = +∞.
 * Start: y*_i = TN(0; t_{z_i}, t_{z_i+1}; u01(seed, 2^64 − 1, i)); vy = var(y*) (ddof 1), μ = mean(y*),
 *   e = y* − μ; every other start value and prior quantity as gbm_bayes_fit's from this vy (S0e is
 *   unused), varE = 1.
 * One iteration `it` (A = 8 it): steps 1 and 2 of gbm_bayes_fit unchanged, with varE = 1; then
 *   (a) for every i: ŷ_i = y*_i − e_i, y*_i = TN(ŷ_i; t_{z_i}, t_{z_i+1}; u01(seed, A+7, i)),
 *       e_i = y*_i − ŷ_i;
 *   (b) for m = 2 … K−1 in order: lo = max(max{y*_i : z_i = m−1}, t_{m−1}) (t_{m−1} as just updated),
 *       hi = min(min{y*_i : z_i = m}, t_{m+1}), t_m = lo + (hi − lo) u01(seed, A+7, 0xFFFFFFFF00000000 + m);
 *       t_1 never moves (it identifies μ);
 *   (c) when the iteration is sampled (step 4's gate): running means of t_1 … t_{K−1} and of
 *       P(class k | i) = Φ(t_{k+1} − ŷ_i) − Φ(t_k − ŷ_i), with the ŷ_i of (a) and the thresholds of (b);
 *   then step 3 without the draw of varE (the stream A+2 stays unused) and step 4.
 * b_hat_out, y_pred_out (the liability b0 + X b), pip_out as gbm_bayes_fit; var_out (3, optional) =
 * [1, mean of mean_j varB_j, mean of π]. *nclass_out = K; classes_out (max_classes) receives the K
 * class values; thresholds_out (max_classes − 1; may be NULL) the posterior means of t_1 … t_{K−1};
 * probs_out (may be NULL; n x K column-major, column pitch ldprobs >= n) the posterior means of
 * P(class k | i). GBM_E_ARG, before any device work: gbm_bayes_fit's own checks, K < 2, K > 32,
 * K > max_classes, NaN/Inf in y, n >= 2^32. Genotype storage as gbm_bayes_fit.
 */
int gbm_bayes_fit_ordinal(int model, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                          int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0, double prob_in,
                          double counts, uint64_t seed, int device, double* b_hat_out /* p+1 */,
                          double* y_pred_out /* n, may be NULL */, double* var_out /* 3; may be NULL */,
                          double* pip_out /* p, may be NULL */, int64_t max_classes, int64_t* nclass_out,
                          double* classes_out /* max_classes */,
                          double* thresholds_out /* max_classes - 1; may be NULL */,
                          double* probs_out /* n x K, may be NULL */, int64_t ldprobs);

/* --------------------------------------------------------------------------------------
 * Diagnostics (tests and timing tools; no reference counterpart).
 * ------------------------------------------------------------------------------------ */
/* Which schedule the last completed gbm_brr_fit ran (*last_path: 0 one launch per block, 4 the
 * super-block sweep with two super-blocks of slack for the partial dots; 1-3 were earlier sweeps, no
 * longer built) and how many fits so far fell back to the per-launch schedule after a sweep
 * hand-off timed out (*fallbacks). */
int gbm_debug_brr_stats(int* last_path, int64_t* fallbacks);
/* How many gbm_bayes_fit_multi calls have completed since load and how many chains they ran. */
int gbm_debug_bayes_multi_stats(int64_t* calls, int64_t* chains);
/* The same for gbm_bayes_fit_multi_rows (its calls are not counted above). */
int gbm_debug_bayes_rows_stats(int64_t* calls, int64_t* chains);
/* Chunk shape of the last super-block sweep: C workgroups, the first O own R rows of every
 * super-block and take Ko individuals each, the others Kn. */
int gbm_debug_brr_shape(int* C, int* O, int* R, int* Ko, int* Kn);
/* Allocations that ran out of device memory and were retried after freeing the idle pooled contexts
 * (GBLUP and BRR) of their device, and how many contexts those retries freed. */
int gbm_debug_oom_retries(int64_t* retries, int64_t* contexts_freed);
/* With GBM_BRR_TRACE=1 set for a fit: copies up to cap int64 timestamps (100 MHz) of the last
 * super-block sweep into host; returns the count, 0 when no trace was taken, -1 on a HIP error. */
int64_t gbm_debug_brr_trace(int64_t* host, int64_t cap);
/* With GBM_CHOL_FLOW_TRACE=1 set for a solve: copies up to cap records of 24 int64 (tile, workgroup,
 * 100 MHz timestamps) of the last dataflow factorisation into host; returns the record count. */
int64_t gbm_debug_chol_flow_trace(int64_t* host, int64_t cap);
/* The dataflow factorisation's worker dequeue order for nbc 64-tiles per side (host only, no device work; the
 * variant GBM_CHOL_FLOW_ORDER selects): returns 0 when every task follows the tasks it waits for (so the launch
 * completes with ONE worker), else the first failing position + 1 (−1 for a bad nbc); copies the entries
 * (i << 16) | j, with bit 15 set for a task that covers the tiles (i, j) and (i, j + 1), to order_out when cap
 * allows (gbm_debug_chol_flow_order_size entries; nbc (nbc + 1)/2 − 1 tiles in all). */
int64_t gbm_debug_chol_flow_order(int nbc, int32_t* order_out, int64_t cap);
int64_t gbm_debug_chol_flow_order_size(int nbc);
/* The same check of a caller's order (m entries). */
int64_t gbm_debug_chol_flow_order_check(int nbc, const int32_t* order, int64_t m);
/* Successful RCCL collectives libgbm has issued (partial-GRM all-reduces; Cholesky strip all-gathers). With
 * GBM_FORCE_RCCL=1 set for a call, a fit with one device leader still runs them on a 1-rank communicator
 * (the all-gathers from n >= GBM_DIST_SOLVE_MIN_N), bit-identical to the call without: the RCCL path on a
 * one-GPU box. */
int gbm_debug_rccl_calls(int64_t* allreduce, int64_t* allgather);
/* The exact GRM's digit count S and scale exponent F for kept-locus weights in [wmin, wmax] (host only, no
 * device work; returns 1 when every weight is exact on the 2^-F grid, 0 when the smallest are rounded). */
int gbm_debug_xg_choose(double wmin, double wmax, int* slices_out, int* shift_out);
/* Sets (value != NULL) or clears (NULL) a GBM_* tuning/test knob. libgbm reads the environment's GBM_*
 * variables ONCE, at its first knob lookup, and never calls getenv on a fit path afterwards (no race with a
 * setenv in another thread under Threads.@threads); later changes go through this entry only. Thread-safe.
 * GBM_E_ARG unless name starts with "GBM_". */
int gbm_debug_set(const char* name, const char* value);

/* Eigen-decomposition of the symmetric m x m matrix A (1 <= m <= 64; (A + Aᵀ)/2 is used) by the cyclic Jacobi
 * method gbm_session_pcs runs on its 32 x 32 projected matrix (host only, no device work): w (m) descending,
 * V (m x m): V[i·m + r] = component r of the unit eigenvector of w[i]. */
int gbm_debug_sym_eig(const double* A, int m, double* w, double* V);
/* The ordinal sampler's own Φ, Φ⁻¹ and TN (gbm_bayes_fit_ordinal; csrc/gibbs_common.h) on m items: what 0:
 * Φ(in[i]); 1: Φ⁻¹(in[i]); 2: TN(m; a, b; u) with in[4i … 4i+3] = (m, a, b, u). host_out (m) is the host
 * compilation's result; dev_out (m; may be NULL: then host only, no device work) the device's, one kernel with
 * one thread per item. GBM_E_ARG for NULL in or host_out, m < 1, m > 2^20 or another what. No fit calls it. */
int gbm_debug_ordinal_math(int what, const double* in, int64_t m, int device, double* host_out, double* dev_out);
#ifdef __cplusplus
}
#endif

#endif /* GBM_H */
