// What gbm_brr_fit (brr.hip) and gbm_bayes_fit (bayes_abc.hip) share: the setup kernels (column
// statistics, Gram blocks, byte quantisation, block 0's partial dots), the pooled per-device context
// with its captured iteration graphs, and the host steps around a chain: argument checks, genotype
// upload, prior moments, graph replay, outputs. Declared in gibbs_common.h.
#include "gibbs_common.h"

namespace gbm {
namespace {

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

// The same per set of individuals (gbm_bayes_fit_multi_rows): blockIdx.y is the set s, rows[s·ldx + i] != 0 marks
// its nrows[s] individuals; the others enter as 0.0 in the same order, so a set that is a prefix of the
// individuals has the bits of brr_colstats_kernel on that prefix. colmean and x2 at s·p.
__global__ void __launch_bounds__(256) brr_colstats_sets_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                                int64_t n, const uint8_t* __restrict__ rows,
                                                                const int64_t* __restrict__ nrows,
                                                                double* __restrict__ colmean, double* __restrict__ x2) {
  __shared__ double red[4];
  const int64_t set = blockIdx.y;
  rows += set * ldx;
  for (int64_t j = blockIdx.x; j < p; j += gridDim.x) {
    const double* row = Xt + j * ldx;
    double s = 0.0, ss = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const double v = rows[i] ? row[i] : 0.0;
      s += v;
      ss += v * v;
    }
    s = brr_block_sum<256>(s, red);
    ss = brr_block_sum<256>(ss, red);
    if (threadIdx.x == 0) {
      colmean[set * p + j] = s / (double)nrows[set];
      x2[set * p + j] = ss;
    }
  }
}

// Gram blocks, one 64x64 block per workgroup (brr_gram_tile; row-major; rows/cols past p are
// zero); one-time setup. nw = 1: W[b] = X_BᵀX_B for the 64-marker
// blocks B = [64b, 64b + 64). nw = 3 (128-marker launches of the byte path, halves A and B of
// block b = [128b, 128b + 128)): W[3b] = X_AᵀX_A, W[3b + 1] = X_BᵀX_A (row k = marker B_k),
// W[3b + 2] = X_BᵀX_B.
__global__ void __launch_bounds__(256) brr_gram_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                       int64_t n, int nw, double* __restrict__ W) {
  const int64_t blk = blockIdx.x / nw;
  const int w = (int)(blockIdx.x % nw);
  const int64_t r0 = nw == 1 ? blk * BB : blk * 2 * BB + (w >= 1 ? BB : 0);
  const int64_t c0 = nw == 1 ? blk * BB : blk * 2 * BB + (w == 2 ? BB : 0);
  brr_gram_tile(Xt, ldx, p, n, r0, c0, W + (int64_t)blockIdx.x * BB * BB, BB);
}

// W[s][b] = X_BᵀX_B over the individuals of set s (blockIdx.y; rows as brr_colstats_sets_kernel), at s·wstride
__global__ void __launch_bounds__(256) brr_gram_sets_kernel(const double* __restrict__ Xt, int64_t ldx, int64_t p,
                                                            int64_t n, const uint8_t* __restrict__ rows,
                                                            int64_t wstride, double* __restrict__ W) {
  const int64_t r0 = (int64_t)blockIdx.x * BB;
  brr_gram_tile<true>(Xt, ldx, p, n, r0, r0, W + (int64_t)blockIdx.y * wstride + (int64_t)blockIdx.x * BB * BB, BB,
                      rows + (int64_t)blockIdx.y * ldx);
}

// partials of block 0 at the start of an iteration (after the intercept update); blockIdx.y is the
// chain of a multi-chain fit (e at c·lde, its partials at c·ldr)
template <typename T>
__global__ void __launch_bounds__(256) brr_dots0_kernel(const T* __restrict__ Xt, int64_t ldx, int64_t n,
                                                        int64_t p, double xs, const double* __restrict__ e,
                                                        int64_t lde, double* __restrict__ partial, int64_t ldr) {
  __shared__ double es[IW];
  e += (int64_t)blockIdx.y * lde;
  partial += (int64_t)blockIdx.y * ldr;
  const int64_t i0 = (int64_t)blockIdx.x * IW;
  es[threadIdx.x] = i0 + threadIdx.x < n ? e[i0 + threadIdx.x] : 0.0;
  __syncthreads();
  brr_partials<T>(Xt, ldx, n, i0, 0, (int)(p < BB ? p : BB), xs, es, partial);
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

}  // namespace

void brr_release_cache() { CtxPool<BrrCtx>::instance().clear(); }

void IterGraph::drop() {
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
  exec = nullptr;
  graph = nullptr;
  key.clear();
}

void IterGraph::ensure(const std::vector<int64_t>& k, hipStream_t s, const std::function<int()>& enqueue) {
  if (key == k) return;
  drop();
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return;
  const int rc = enqueue();
  if (hipStreamEndCapture(s, &graph) != hipSuccess || rc != GBM_OK ||
      hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    drop();  // run() falls back to direct launches (same kernels, same order)
  } else {
    key = k;
  }
}

int IterGraph::run(int64_t n_iter, hipStream_t s, const char* entry, const std::function<int()>& enqueue) {
  for (int64_t it = 0; it < n_iter; it++) {
    if (!exec) {
      GBM_TRY(enqueue());
    } else if (hipGraphLaunch(exec, s) != hipSuccess) {
      return fail(GBM_E_HIP, std::string(entry) + ": graph launch failed");
    }
  }
  GBM_HIP_TRY(hipStreamSynchronize(s));
  return GBM_OK;
}

int gibbs_check_args(const char* entry, const double* X, const double* y, const double* b_hat_out, int64_t n, int64_t p,
                     int64_t ldx, int64_t n_iter, int64_t n_burnin, int64_t thin, double r2, double df0) {
  if (!X || !y || !b_hat_out || n < 3 || p < 1 || ldx < n || n_iter < 1 || n_burnin < 0 || thin < 1 ||
      !(r2 > 0.0 && r2 < 1.0) || !(df0 > 0.0))
    return fail(GBM_E_ARG, std::string(entry) + ": bad arguments (n >= 3, p >= 1, ldx >= n, n_iter >= 1, n_burnin >= 0, "
                                                "thin >= 1, 0 < r2 < 1, df0 > 0)");
  return GBM_OK;
}

int gibbs_check_run(const char* entry, const double* y, int64_t n, int64_t n_iter, int64_t n_burnin, int64_t thin,
                    int device, int& dev_out) {
  if (n_iter <= n_burnin || (n_iter / thin) <= (n_burnin / thin))
    return fail(GBM_E_ARG,
                std::string(entry) + ": no post-burn-in sample (need a multiple of thin in (n_burnin, n_iter])");
  if (y) GBM_TRY(check_y(y, n, n, 1));
  std::vector<int> devs;
  GBM_TRY(check_devices(&device, 1, devs));
  dev_out = devs[0];
  return GBM_OK;
}

int gibbs_upload(BrrCtx& cx, const double* X, int64_t n, int64_t p, int64_t ldx, GibbsData& g) {
  const int dev = cx.dev;
  hipStream_t s = cx.stream.s;
  // Xt rows and e padded to whole IW-individual chunks (the block kernels read full chunks)
  const int64_t npad = g.npad = round_up(n, IW);
  g.C64 = (n + IW - 1) / IW;
  GBM_TRY(ensure(cx.Xt, dev, p * npad * 8));
  GBM_TRY(ensure(cx.colmean, dev, p * 8));
  GBM_TRY(ensure(cx.x2, dev, p * 8));
  GBM_TRY(ensure(cx.e, dev, npad * 8));
  GBM_TRY(ensure(cx.b, dev, 2 * p * 8));  // two copies (iteration parity)
  GBM_TRY(ensure(cx.bbar, dev, p * 8));
  GBM_TRY(ensure(cx.r, dev, 2 * g.C64 * BK2 * 8));  // ping-pong partial dots (BRR's size for both samplers)
  GBM_HIP_TRY(hipMemsetAsync(cx.Xt.p, 0, (size_t)(p * npad * 8), s));
  GBM_HIP_TRY(hipMemcpy2DAsync(cx.Xt.p, npad * 8, X, ldx * 8, n * 8, p, hipMemcpyHostToDevice, s));
  brr_colstats_kernel<<<(unsigned)std::min<int64_t>(p, 4096), 256, 0, s>>>((const double*)cx.Xt.p, npad, p, n,
                                                                           (double*)cx.colmean.p, (double*)cx.x2.p);
  GBM_LAUNCH_CHECK();
  g.cm.resize(p);
  g.xx.resize(p);
  GBM_HIP_TRY(hipMemcpyAsync(g.cm.data(), cx.colmean.p, p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(g.xx.data(), cx.x2.p, p * 8, hipMemcpyDeviceToHost, s));
  // byte storage for the samplers' sweeps when X = D/s exactly (s = 2: diploid allele
  // frequencies; then 4, 1): the chain is identical, the per-iteration stream 8× smaller.
  // GBM_BRR_I8=0 keeps fp64 storage (read per call).
  g.xs = 0.0;
  const char* ev = knob("GBM_BRR_I8");
  if (ev && ev[0] == '0') return GBM_OK;
  GBM_TRY(ensure(cx.D, dev, p * npad + 4096));  // + slack: the super-block sweep's last chunk reads past n
  GBM_TRY(ensure(cx.badm, dev, sizeof(int)));
  for (double sc : {2.0, 4.0, 1.0}) {
    int nbad = -1;
    GBM_HIP_TRY(hipMemsetAsync(cx.badm.p, 0, sizeof(int), s));
    brr_quantize_kernel<<<2048, 256, 0, s>>>((const double*)cx.Xt.p, p * npad, sc, (uint8_t*)cx.D.p, (int*)cx.badm.p);
    GBM_LAUNCH_CHECK();
    GBM_HIP_TRY(hipMemcpyAsync(&nbad, cx.badm.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
    if (nbad == 0) {
      g.xs = 1.0 / sc;
      break;
    }
  }
  return GBM_OK;
}

int gibbs_gram(BrrCtx& cx, int64_t n, int64_t p, int64_t npad, int64_t nblk, int nw) {
  GBM_TRY(ensure(cx.W, cx.dev, nblk * nw * BB * BB * 8));
  brr_gram_kernel<<<(unsigned)(nblk * nw), 256, 0, cx.stream.s>>>((const double*)cx.Xt.p, npad, p, n, nw,
                                                                  (double*)cx.W.p);
  GBM_LAUNCH_CHECK();
  return GBM_OK;
}

void gibbs_dots0(BrrCtx& cx, int64_t n, int64_t p, const GibbsData& g, bool bytes, int64_t nchains) {
  const dim3 grid((unsigned)g.C64, (unsigned)nchains);
  const int64_t ldr = 2 * g.C64 * BB;  // a chain's ping-pong pair
  if (bytes)
    brr_dots0_kernel<uint8_t><<<grid, 256, 0, cx.stream.s>>>((const uint8_t*)cx.D.p, g.npad, n, p, g.xs,
                                                             (const double*)cx.e.p, g.npad, (double*)cx.r.p, ldr);
  else
    brr_dots0_kernel<double><<<grid, 256, 0, cx.stream.s>>>((const double*)cx.Xt.p, g.npad, n, p, 1.0,
                                                            (const double*)cx.e.p, g.npad, (double*)cx.r.p, ldr);
}

int gibbs_sets(BrrCtx& cx, int64_t n, int64_t p, int64_t npad, int64_t nblk, int64_t nchains, RowSetsHost& rs) {
  const int dev = cx.dev;
  hipStream_t s = cx.stream.s;
  const int64_t S = rs.nsets, wstride = nblk * BB * BB;
  GBM_TRY(ensure(cx.colmean, dev, S * p * 8));
  GBM_TRY(ensure(cx.x2, dev, S * p * 8));
  GBM_TRY(ensure(cx.W, dev, S * wstride * 8));
  GBM_TRY(ensure(cx.srows, dev, S * npad));
  GBM_TRY(ensure(cx.smask, dev, npad * 4));
  GBM_TRY(ensure(cx.sof, dev, nchains * 4));
  GBM_TRY(ensure(cx.snrows, dev, (nchains + S) * 8));
  std::vector<uint32_t> mask((size_t)npad, 0u);
  std::vector<int64_t> nr((size_t)(nchains + S));
  for (int64_t c = 0; c < nchains; c++) {
    const uint8_t* r = rs.rows + rs.set_of[c] * rs.ldrows;
    for (int64_t i = 0; i < n; i++) mask[(size_t)i] |= r[i] ? 1u << c : 0u;
    nr[(size_t)c] = rs.nrows[(size_t)rs.set_of[c]];
  }
  for (int64_t t = 0; t < S; t++) nr[(size_t)(nchains + t)] = rs.nrows[(size_t)t];
  GBM_HIP_TRY(hipMemsetAsync(cx.srows.p, 0, (size_t)(S * npad), s));
  GBM_HIP_TRY(hipMemcpy2DAsync(cx.srows.p, npad, rs.rows, rs.ldrows, n, S, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.smask.p, mask.data(), npad * 4, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.sof.p, rs.set_of, nchains * 4, hipMemcpyHostToDevice, s));
  GBM_HIP_TRY(hipMemcpyAsync(cx.snrows.p, nr.data(), (nchains + S) * 8, hipMemcpyHostToDevice, s));
  brr_colstats_sets_kernel<<<dim3((unsigned)std::min<int64_t>(p, 4096), (unsigned)S), 256, 0, s>>>(
      (const double*)cx.Xt.p, npad, p, n, (const uint8_t*)cx.srows.p, (const int64_t*)cx.snrows.p + nchains,
      (double*)cx.colmean.p, (double*)cx.x2.p);
  GBM_LAUNCH_CHECK();
  brr_gram_sets_kernel<<<dim3((unsigned)nblk, (unsigned)S), 256, 0, s>>>(
      (const double*)cx.Xt.p, npad, p, n, (const uint8_t*)cx.srows.p, wstride, (double*)cx.W.p);
  GBM_LAUNCH_CHECK();
  rs.cm.resize((size_t)(S * p));
  rs.xx.resize((size_t)(S * p));
  GBM_HIP_TRY(hipMemcpyAsync(rs.cm.data(), cx.colmean.p, S * p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(rs.xx.data(), cx.x2.p, S * p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));  // mask and nr leave scope
  return GBM_OK;
}

int gibbs_prior(const char* entry, const double* y, int64_t n, int64_t p, const GibbsData& g, GibbsPrior& pr) {
  return gibbs_prior_rows(entry, y, n, p, g.npad, nullptr, n, g.cm.data(), g.xx.data(), pr);
}

int gibbs_prior_rows(const char* entry, const double* y, int64_t n, int64_t p, int64_t npad, const uint8_t* rows,
                     int64_t nc, const double* cm, const double* xx, GibbsPrior& pr) {
  // BGLR defaults (setLT.BRR and the residual prior): var(y) with ddof 1
  double ym = 0.0;
  for (int64_t i = 0; i < n; i++)
    if (!rows || rows[i]) ym += y[i];
  ym /= (double)nc;
  double vy = 0.0;
  for (int64_t i = 0; i < n; i++)
    if (!rows || rows[i]) vy += (y[i] - ym) * (y[i] - ym);
  vy /= (double)(nc - 1);
  double msx = 0.0, smsq = 0.0;
  for (int64_t j = 0; j < p; j++) {
    msx += xx[j];
    smsq += cm[j] * cm[j];
  }
  msx = msx / (double)nc - smsq;
  if (!(msx > 0.0)) return fail(GBM_E_DATA, std::string(entry) + ": the markers have no variance");
  pr.ym = ym;
  pr.vy = vy;
  pr.msx = msx;
  pr.e0.assign(npad, 0.0);
  for (int64_t i = 0; i < n; i++)
    if (!rows || rows[i]) pr.e0[i] = y[i] - ym;
  return GBM_OK;
}

int gibbs_outputs(BrrCtx& cx, int64_t n, int64_t p, int64_t npad, const DevBuf& state, void* fin, size_t fin_bytes,
                  const double* mubar, double* b_hat_out, double* pip_out, double* y_pred_out, int64_t chain) {
  const int dev = cx.dev;
  hipStream_t s = cx.stream.s;
  GBM_HIP_TRY(hipMemcpyAsync(fin, (const char*)state.p + chain * (int64_t)fin_bytes, fin_bytes, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(b_hat_out + 1, (const double*)cx.bbar.p + chain * p, p * 8, hipMemcpyDeviceToHost, s));
  if (pip_out)
    GBM_HIP_TRY(hipMemcpyAsync(pip_out, (const double*)cx.dbar.p + chain * p, p * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  b_hat_out[0] = *mubar;
  if (!y_pred_out) return GBM_OK;
  const int64_t nchunks = predict_chunks(n, p);
  GBM_TRY(ensure(cx.pb, dev, (p + 1) * 8));
  GBM_TRY(ensure(cx.part, dev, nchunks * npad * 8));
  GBM_TRY(ensure(cx.pout, dev, npad * 8));
  GBM_HIP_TRY(hipMemcpyAsync(cx.pb.p, b_hat_out, (p + 1) * 8, hipMemcpyHostToDevice, s));
  GBM_TRY(launch_predict((const double*)cx.Xt.p, npad, p, n, (const double*)cx.pb.p, p + 1, 1, (double*)cx.part.p,
                         nchunks, (double*)cx.pout.p, npad, s));
  GBM_HIP_TRY(hipMemcpyAsync(y_pred_out, cx.pout.p, n * 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  return GBM_OK;
}

}  // namespace gbm
