// One shard's genotypes -> its partial GRM on the shard's leased context (fit_ctx.h): resident in one piece,
// host chunks pipelined with the GRM (fp64 / int8, or fp64 packed to dosage bytes on the host), loci-streamed,
// or the exact-integer GRM of resident dosage bytes; and the marker effects of a streamed or exact shard. The
// chunked drivers share one schedule rule, one buffer set-up and one per-chunk GRM step, so that fits over the
// same chunk size are bit-identical whichever driver ran them.
#include "fit_ctx.h"

namespace gbm {

using Sched = std::vector<std::pair<int64_t, int64_t>>;  // (first locus, count) per chunk

// ---- pieces the drivers share --------------------------------------------------------------------

int ensure_copy_stream(FitCtx& c) {
  if (!c.copy.s) {
    c.copy.dev = c.dev;
    // high priority: besides the streamed uploads it carries the distributed solve's latency-bound
    // look-ahead (area exchange, the next group's panels and row exchange) beside the trailing update
    int lo = 0, hi = 0;
    GBM_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    GBM_HIP_TRY(hipStreamCreateWithPriority(&c.copy.s, hipStreamNonBlocking, hi));
  }
  return GBM_OK;
}

static int ensure_events(FitCtx& c, int64_t k) {
  while ((int64_t)c.ev.size() < k) {
    hipEvent_t e;
    GBM_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c.ev.push_back(e);
  }
  return GBM_OK;
}

// per-locus statistics of the shard's pl loci and the kept count
static int ensure_locus_stats(FitCtx& c, int64_t pl) {
  GBM_TRY(ensure(c.mean, c.dev, pl * 8));
  GBM_TRY(ensure(c.sd, c.dev, pl * 8));
  GBM_TRY(ensure(c.keep, c.dev, pl * 4));
  return ensure(c.q, c.dev, 8);
}

// Loci per chunk of the pipelined upload of host genotypes (0: one piece). Re-read per call:
// GBM_HOST_CHUNK = loci per chunk, 0 to disable; by default p/8 (>= 4096 loci) once p >= 16384
// (C2 host path, pageable X: 58.5 ms in one piece, 43.3 ms in 4 chunks, 40.9 ms in 8).
int64_t host_chunk(int64_t p) {
  const char* e = ::gbm::knob("GBM_HOST_CHUNK");
  int64_t c = e ? (int64_t)atoll(e) : -1;
  if (c == 0) return 0;
  if (c < 0) {
    if (p < 16384) return 0;
    c = std::max<int64_t>(4096, (p + 7) / 8);
  }
  return c >= p ? 0 : c;
}

// Chunk schedule of the pipelined upload: chunks of `chunk` loci, the last full-size piece cut
// into halving pieces (1/2, 1/4, 1/8, 1/8 of it, none below 512 loci) when `halve_tail`, so that
// the device work left after the last byte has landed is a small chunk's GRM rather than a full
// one's. That pays where the upload is copy-bound: fp64 X with n below ≈ 9 000 (PCIe ≈ 57 GB/s
// moves 8np bytes while the GRM does n²p flops at ≈ 65 TF/s; C2: 40.7 -> 39.9 ms). Where the device
// is the bound — int8 dosages (an eighth of the bytes; 25.5 -> 26.4 ms at C2) or large n (C3's
// per-GPU shape: 4.06 -> 4.10 s) — extra chunks only add launches, so by default those keep equal
// chunks. With GBM_HOST_CHUNK set, every entry halves the tail: the same partition, chunk GRMs
// summed in the same order, bit-identical fp64 and int8 results.
static Sched chunk_schedule(int64_t pl, int64_t chunk, bool halve_tail) {
  Sched cs;
  int64_t j = 0;
  while (pl - j > chunk) {
    cs.emplace_back(j, chunk);
    j += chunk;
  }
  int64_t r = pl - j;
  for (int d = 0; halve_tail && d < 3 && r / 2 >= 512; d++) {
    const int64_t h = r / 2;
    cs.emplace_back(j, r - h);
    j += r - h;
    r = h;
  }
  if (r > 0) cs.emplace_back(j, r);
  return cs;
}

// The chunks of a shard's GRM (pipelined, host-packed pipelined and streamed alike): halving tail
// for copy-bound fp64 at n <= 8192 or when GBM_HOST_CHUNK is set. One rule, so a streamed fit and a
// pipelined one over the same chunk size sum the same chunk GRMs in the same order.
static Sched shard_schedule(const Problem& pr, int64_t pl, int64_t chunk) {
  return chunk_schedule(pl, chunk, (pr.src == Source::F64 && pr.n <= 8192) || ::gbm::knob("GBM_HOST_CHUNK") != nullptr);
}

// Buffers of a chunked GRM: G, the workspace of the largest chunk (the loci split, and so the
// workspace, is planned per chunk size; *wsb), and a second G only when some chunk k >= 1 cannot
// be added into G in place (a single loci range).
static int ensure_chunked_grm(FitCtx& c, int64_t n, const Sched& sched, int64_t* wsb) {
  const int64_t gdim = gdim_of(n);
  GBM_TRY(ensure(c.G, c.dev, gdim * gdim * 8));
  *wsb = 0;
  for (const auto& jc : sched) *wsb = std::max(*wsb, gbm_dev_grm_workspace(n, jc.second));
  GBM_TRY(ensure(c.wsg, c.dev, *wsb));
  for (size_t k = 1; k < sched.size(); k++)
    if (!grm_can_accumulate(n, sched[k].second)) return ensure(c.Gc, c.dev, gdim * gdim * 8);
  return GBM_OK;
}

// G (+)= the GRM of chunk k's pc standardised rows Z, on the compute stream. Chunk 0 stores into G. A later chunk
// adds inside its reduce: with slabs G_old + ((P0 + P1) + ...), the sums of G plus a separate chunk G; in the
// in-order carry (large n) range 0 adds G_old first, ((G_old + P0) + P1) + ..., which agrees with that only to
// rounding (deterministic either way: the mode is fixed by n and the chunk size). A chunk that cannot accumulate
// goes through Gc and an add. err (device int32, or nullptr: a stream sync reads it back): the carry's error cell.
static int add_chunk_grm(FitCtx& c, const double* Z, int64_t pc, int64_t n, int64_t k, int64_t wsb, int32_t* err) {
  const int64_t npad = npad_of(n), gdim = gdim_of(n);
  hipStream_t s = c.stream.s;
  if (k == 0) return launch_grm(Z, npad, pc, n, (double*)c.G.p, gdim, c.wsg.p, wsb, s, 0, err);
  if (grm_can_accumulate(n, pc)) return launch_grm(Z, npad, pc, n, (double*)c.G.p, gdim, c.wsg.p, wsb, s, 1, err);
  GBM_TRY(launch_grm(Z, npad, pc, n, (double*)c.Gc.p, gdim, c.wsg.p, wsb, s, 0, err));
  return launch_add_inplace((double*)c.G.p, (const double*)c.Gc.p, gdim * gdim, s);
}

// Zb <- the standardised rows of the shard's loci [j, j + pc) (mean/sd/keep at those loci, kept count into q), on
// the compute stream: in place from fp64 rows uploaded into Zb, else straight from the dosage bytes in D8 (no
// fp64 copy of X; the kernel writes Z's padding zeros)
static int standardize_chunk(const Problem& pr, FitCtx& c, int64_t j, int64_t pc, double* Zb, int64_t* q) {
  const int64_t n = pr.n, npad = npad_of(n);
  hipStream_t s = c.stream.s;
  if (pr.src == Source::F64) {
    if (npad > n) GBM_HIP_TRY(hipMemset2DAsync(Zb + n, npad * 8, 0, (npad - n) * 8, pc, s));
    return gbm_dev_standardize(Zb, npad, pc, n, Zb, npad, (double*)c.mean.p + j, (double*)c.sd.p + j,
                               (int32_t*)c.keep.p + j, q, s);
  }
  const int ploidy = pr.src == Source::SYNTH ? 2 : pr.ploidy;
  return launch_standardize_i8((const int8_t*)c.D8.p + j * n, n, pc, n, ploidy, Zb, npad, (double*)c.mean.p + j,
                               (double*)c.sd.p + j, (int32_t*)c.keep.p + j, q, s);
}

static int pack_fail(hipError_t e) {
  return fail(GBM_E_HIP, std::string("host-pack upload: HIP error '") + hipGetErrorString(e) + "'");
}

// fp64 host X of a shard -> dosage bytes D8 = 2x, packed on the HOST: `threads` workers check and pack the
// chunks of `sched` into a ring of `slots` pinned staging slots (ChunkPacker, hostpack.cpp; a slot holds the
// largest chunk), and this thread uploads each chunk as soon as it is packed (the copy stream), records
// ev[k mod nev] behind the copy and runs queued(k) (may be empty); a slot is reused only after its previous
// chunk's copy has landed. Only n·p bytes cross PCIe. Returns kNotDosage as soon as any worker meets a 2x
// that is not exactly 0, 1 or 2.
static int packed_upload(const Problem& pr, Shard& sh, const Sched& sched, int slots, int64_t nev, int threads,
                         const std::function<int(int64_t)>& queued) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n;
  int64_t pmax = 0;
  for (const auto& jc : sched) pmax = std::max(pmax, jc.second);
  GBM_TRY(ensure_copy_stream(c));
  GBM_TRY(ensure_pinned(c.pack, slots * pmax * n));
  GBM_TRY(ensure_events(c, nev));
  int rc = GBM_OK;
  {
    ChunkPacker packer(pr.X + sh.j0 * pr.ld, pr.ld, n, sched, static_cast<int8_t*>(c.pack.p), pmax * n, slots, threads);
    for (int64_t k = 0; k < (int64_t)sched.size() && rc == GBM_OK; k++) {
      const int8_t* src = packer.wait(k);
      if (!src) {
        rc = kNotDosage;
        break;
      }
      const int64_t j = sched[k].first, pc = sched[k].second;
      hipError_t e = hipMemcpyAsync((int8_t*)c.D8.p + j * n, src, pc * n, hipMemcpyHostToDevice, c.copy.s);
      if (e == hipSuccess) e = hipEventRecord(c.ev[k % nev], c.copy.s);
      if (e != hipSuccess) rc = pack_fail(e);
      if (rc == GBM_OK && queued) rc = queued(k);
      // the previous chunk has landed: its slot (and every earlier one) goes back to the packer
      if (rc == GBM_OK && k >= 1 && (e = hipEventSynchronize(c.ev[(k - 1) % nev])) != hipSuccess) rc = pack_fail(e);
      if (rc == GBM_OK) packer.release_upto(k);  // (after a failure no slot is handed back: a copy may still read it)
    }
  }  // (the packer's workers have stopped)
  GBM_HIP_TRY(hipStreamSynchronize(c.copy.s));  // no copy still reads a staging slot
  return rc;
}

// ---- resident shard: one piece, or host chunks pipelined with the GRM -----------------------------
// Upload the shard's columns and standardise them in place (center_only: centre them only, the
// ploidy-aware GRM); reads back the shard's kept count (valid once the stream has synchronised:
// here with sync, else by the caller after it has queued more work behind it).
int prepare_shard(const Problem& pr, Shard& sh, bool center_only, bool sync) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  GBM_TRY(ensure(c.Xt, c.dev, pl * npad * 8));
  GBM_TRY(ensure_locus_stats(c, pl));
  if (pr.src == Source::F64) {
    GBM_HIP_TRY(hipMemcpy2DAsync(c.Xt.p, npad * 8, pr.X + sh.j0 * pr.ld, pr.ld * 8, n * 8, pl, hipMemcpyHostToDevice, s));
    if (npad > n) GBM_HIP_TRY(hipMemset2DAsync((double*)c.Xt.p + n, npad * 8, 0, (npad - n) * 8, pl, s));
  } else if (pr.src == Source::SYNTH) {
    GBM_TRY(gbm_dev_synth_genotypes((double*)c.Xt.p, npad, pl, n, pr.seed, sh.j0, s));
  } else {
    GBM_TRY(ensure(c.D8, c.dev, pl * n));
    GBM_HIP_TRY(hipMemcpy2DAsync(c.D8.p, n, pr.D + sh.j0 * pr.ld, pr.ld, n, pl, hipMemcpyHostToDevice, s));
    GBM_TRY(gbm_dev_expand_dosage_i8((const int8_t*)c.D8.p, n, n, pl, pr.ploidy, (double*)c.Xt.p, npad, s));
  }
  GBM_HIP_TRY(hipMemsetAsync(c.q.p, 0, 8, s));
  if (center_only)
    GBM_TRY(launch_center_columns((const double*)c.Xt.p, npad, pl, n, (double*)c.Xt.p, npad, (double*)c.mean.p,
                                  (double*)c.sd.p, (int32_t*)c.keep.p, (int64_t*)c.q.p, s));
  else
    GBM_TRY(gbm_dev_standardize((const double*)c.Xt.p, npad, pl, n, (double*)c.Xt.p, npad, (double*)c.mean.p,
                                (double*)c.sd.p, (int32_t*)c.keep.p, (int64_t*)c.q.p, s));
  GBM_HIP_TRY(hipMemcpyAsync(&sh.q_host, c.q.p, 8, hipMemcpyDeviceToHost, s));
  if (sync) GBM_HIP_TRY(hipStreamSynchronize(s));
  return GBM_OK;
}

int grm_shard(const Problem& pr, Shard& sh) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), gdim = gdim_of(n);
  GBM_HIP_TRY(hipSetDevice(c.dev));
  GBM_TRY(ensure(c.G, c.dev, gdim * gdim * 8));
  const int64_t wsb = gbm_dev_grm_workspace(n, sh.p);
  GBM_TRY(ensure(c.wsg, c.dev, wsb));
  return gbm_dev_grm((const double*)c.Xt.p, npad, sh.p, n, (double*)c.G.p, gdim, c.wsg.p, wsb, c.stream.s);
}

// Upload + standardise + partial GRM of one shard, queued back to back on its stream, then one sync.
int prepare_grm_shard(const Problem& pr, Shard& sh) {
  GBM_TRY(prepare_shard(pr, sh, false, false));
  GBM_TRY(grm_shard(pr, sh));
  GBM_HIP_TRY(hipStreamSynchronize(sh.x().stream.s));
  return GBM_OK;
}

// Upload, standardise and GRM of one shard with the PCIe transfer of the genotypes overlapped
// with the device work: chunk k's copy (on the context's copy stream; from pageable memory the
// call itself returns when the copy is done) runs while the compute stream standardises chunk
// k − 1 and adds its loci to G (chunk GRMs summed in chunk order: deterministic). At C2 the
// 2 GB of fp64 X take ~35 ms over PCIe and the GRM ~19 ms: pipelined, the call costs about the
// copy plus the last (small) chunk's GRM instead of their sum.
int upload_grm_pipelined(const Problem& pr, Shard& sh, int64_t chunk) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  GBM_TRY(ensure_copy_stream(c));
  const Sched sched = shard_schedule(pr, pl, chunk);
  const int64_t nch = (int64_t)sched.size();
  GBM_TRY(ensure_events(c, nch));
  GBM_TRY(ensure(c.Xt, c.dev, pl * npad * 8));
  GBM_TRY(ensure_locus_stats(c, pl));
  if (pr.src == Source::I8) GBM_TRY(ensure(c.D8, c.dev, pl * n));
  int64_t wsb = 0;
  GBM_TRY(ensure_chunked_grm(c, n, sched, &wsb));
  GBM_HIP_TRY(hipMemsetAsync(c.q.p, 0, 8, s));
  double* Xt = (double*)c.Xt.p;
  for (int64_t k = 0; k < nch; k++) {
    const int64_t j = sched[k].first, pc = sched[k].second;
    if (pr.src == Source::F64)
      GBM_HIP_TRY(hipMemcpy2DAsync(Xt + j * npad, npad * 8, pr.X + (sh.j0 + j) * pr.ld, pr.ld * 8, n * 8, pc,
                                   hipMemcpyHostToDevice, c.copy.s));
    else
      GBM_HIP_TRY(hipMemcpy2DAsync((int8_t*)c.D8.p + j * n, n, pr.D + (sh.j0 + j) * pr.ld, pr.ld, n, pc,
                                   hipMemcpyHostToDevice, c.copy.s));
    GBM_HIP_TRY(hipEventRecord(c.ev[k], c.copy.s));
    GBM_HIP_TRY(hipStreamWaitEvent(s, c.ev[k], 0));
    GBM_TRY(standardize_chunk(pr, c, j, pc, Xt + j * npad, (int64_t*)c.q.p));
    GBM_TRY(add_chunk_grm(c, Xt + j * npad, pc, n, k, wsb, nullptr));
  }
  GBM_HIP_TRY(hipMemcpyAsync(&sh.q_host, c.q.p, 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  return GBM_OK;
}

// The pipelined fp64 upload + GRM (upload_grm_pipelined) of fp64 host X whose values are dosages/2, through the
// host packer (grm_mode fp64, GBM_HOST_PACK): each pipeline chunk (the fp64 schedule, so the chunk GRMs are summed
// exactly as there) is packed to bytes by the host workers into a pinned slot, uploaded at 1 B per cell and
// standardised straight from the bytes (launch_standardize_i8: the same Z bits as the fp64 standardisation of
// d/2), then its GRM added into G as in the fp64 path. Returns kNotDosage (G untouched by later chunks) when a
// chunk is not dosage-valued: the caller then runs the plain fp64 upload for the shard.
int upload_grm_pipelined_packed(const Problem& pr, Shard& sh, int64_t chunk, int threads) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  const Sched sched = shard_schedule(pr, pl, chunk);
  GBM_TRY(ensure(c.Xt, c.dev, pl * npad * 8));
  GBM_TRY(ensure(c.D8, c.dev, pl * n));
  GBM_TRY(ensure_locus_stats(c, pl));
  int64_t wsb = 0;
  GBM_TRY(ensure_chunked_grm(c, n, sched, &wsb));
  GBM_HIP_TRY(hipMemsetAsync(c.q.p, 0, 8, s));
  double* Xt = (double*)c.Xt.p;
  // behind each chunk's copy (one event per chunk): standardise it from the bytes, add its GRM
  const int rc = packed_upload(pr, sh, sched, 3, (int64_t)sched.size(), threads, [&](int64_t k) -> int {
    const int64_t j = sched[k].first, pc = sched[k].second;
    const hipError_t e = hipStreamWaitEvent(s, c.ev[k], 0);
    if (e != hipSuccess) return pack_fail(e);
    GBM_TRY(launch_standardize_i8((const int8_t*)c.D8.p + j * n, n, pc, n, 2, Xt + j * npad, npad, (double*)c.mean.p + j,
                                  (double*)c.sd.p + j, (int32_t*)c.keep.p + j, (int64_t*)c.q.p, s));
    return add_chunk_grm(c, Xt + j * npad, pc, n, k, wsb, nullptr);
  });
  if (rc == kNotDosage) GBM_HIP_TRY(hipStreamSynchronize(s));  // the chunks already queued are done before the fp64 path reuses G
  GBM_TRY(rc);
  GBM_HIP_TRY(hipMemcpyAsync(&sh.q_host, c.q.p, 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  return GBM_OK;
}

// ---- loci-streamed mode --------------------------------------------------------------------------
// A shard whose fp64 locus rows do not fit its device next to G (config C3 on one GPU: 600 000 loci
// x 50 048 individuals x 8 B = 240 GB beside a 20 GB G) is streamed. Its genotypes stay resident as
// int8 dosages (synthetic and int8 sources: 1 B per cell, 30 GB at C3) or stay on the host (fp64
// source), and the loci pass through one reusable fp64 chunk buffer: each chunk is standardised and
// its GRM added into G in place (chunk GRMs summed in chunk order, as the pipelined host upload
// does; same chunk partition => bit-identical G). After the solve the marker effects re-read the
// dosages with z rebuilt in registers (bit-identical to the resident kernels), or re-upload the
// fp64 chunks. Peak HBM: G + dosages + one or two chunk buffers.

// Decide, per device, whether its shards' fp64 rows fit (resident, the default) or are streamed,
// and the chunk size: GBM_STREAM_CHUNK (re-read per call) forces it (loci per chunk; 0 never
// streams); otherwise a device streams when the resident buffers of its shards exceed its free
// memory (plus what their pooled contexts already hold, minus a margin) even after its idle pooled
// contexts are freed; the chunk is then the largest equal split of the shard whose buffers fit.
int plan_streaming(const Problem& pr, Shards& shards, bool reml) {
  const int64_t forced = knob_i64("GBM_STREAM_CHUNK", -1);
  const int64_t n = pr.n, npad = npad_of(n), gdim = gdim_of(n);
  const bool bytes = pr.src != Source::F64;
  if (forced >= 0) {
    for (auto& sh : shards) sh->stream = (forced > 0 && forced < sh->p) ? forced : 0;
    return GBM_OK;
  }
  std::map<int, std::vector<Shard*>> bydev;
  for (auto& sh : shards) bydev[sh->x().dev].push_back(sh.get());
  for (auto& dv : bydev) {
    const int dev = dv.first;
    std::vector<Shard*>& v = dv.second;
    GBM_HIP_TRY(hipSetDevice(dev));
    int64_t held = 0, fixed = 0, resident = 0, dosage = 0, pmax = 0;
    for (Shard* sh : v) {
      FitCtx& c = sh->x();
      // D8 counts only where this call's path refills it (int8 or synthetic dosages); an fp64 source never reuses it
      held += c.Xt.cap + (pr.src != Source::F64 ? c.D8.cap : 0) + c.G.cap + c.Gc.cap + c.wsg.cap;
      fixed += gdim * gdim * 8 * (reml ? 2 : 1) + gbm_dev_solve_workspace(n, 63) + sh->p * 40;
      resident += sh->p * npad * 8 + (pr.src == Source::I8 ? sh->p * n : 0) + gbm_dev_grm_workspace(n, sh->p);
      dosage += bytes ? sh->p * n : 0;
      pmax = std::max(pmax, sh->p);
    }
    size_t fr = 0, tot = 0;
    GBM_HIP_TRY(hipMemGetInfo(&fr, &tot));
    const int64_t margin = ((int64_t)1 << 30) + (int64_t)tot / 50;
    if (resident + fixed + margin <= (int64_t)fr + held) continue;
    pool().trim(dev);  // idle pooled contexts of this device hold memory the fit could use
    GBM_HIP_TRY(hipMemGetInfo(&fr, &tot));
    if (resident + fixed + margin <= (int64_t)fr + held) continue;
    const int nbuf = bytes ? 1 : 2;
    int64_t budget = (int64_t)fr + held - fixed - dosage - margin;
    int64_t cmax = budget / ((int64_t)v.size() * nbuf * npad * 8);
    if (cmax >= 16) budget -= (int64_t)v.size() * gbm_dev_grm_workspace(n, std::min(cmax, pmax));  // slabs at small n
    cmax = budget / ((int64_t)v.size() * nbuf * npad * 8);
    if (cmax < 512)
      return fail(GBM_E_OOM, "device " + std::to_string(dev) + ": too little memory for a loci-streamed fit at n = " +
                                 std::to_string(n) + " (need G " + std::to_string(gdim * gdim * 8) + " B plus chunk buffers)");
    for (Shard* sh : v) {
      const int64_t nch = (sh->p + cmax - 1) / cmax;
      const int64_t chunk = round_up((sh->p + nch - 1) / nch, 16);
      sh->stream = chunk < sh->p ? chunk : 0;
    }
  }
  return GBM_OK;
}

// Upload (fp64: into its chunk buffer; int8: into the resident dosages) of chunk k on the copy
// stream, recording ev[k]. An fp64 chunk reuses buffer k % 2 after the work that read chunk k − 2
// (ev[nch + k % 2], recorded on the compute stream) is done.
static int stream_upload(const Problem& pr, Shard& sh, const Sched& sched, int64_t k) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), nch = (int64_t)sched.size();
  const int64_t j = sched[k].first, pc = sched[k].second;
  if (pr.src == Source::F64) {
    if (k >= 2) GBM_HIP_TRY(hipStreamWaitEvent(c.copy.s, c.ev[nch + k % 2], 0));
    double* Zb = (double*)c.Xt.p + (k % 2) * sh.stream * npad;
    GBM_HIP_TRY(hipMemcpy2DAsync(Zb, npad * 8, pr.X + (sh.j0 + j) * pr.ld, pr.ld * 8, n * 8, pc, hipMemcpyHostToDevice,
                                 c.copy.s));
  } else if (pr.src == Source::I8) {
    GBM_HIP_TRY(hipMemcpy2DAsync((int8_t*)c.D8.p + j * n, n, pr.D + (sh.j0 + j) * pr.ld, pr.ld, n, pc,
                                 hipMemcpyHostToDevice, c.copy.s));
  }
  GBM_HIP_TRY(hipEventRecord(c.ev[k], c.copy.s));
  return GBM_OK;
}

// Chunk k's standardised rows in its chunk buffer (mean/sd/keep at the chunk's loci, kept count into
// q); returns the buffer.
static int stream_standardize(const Problem& pr, Shard& sh, const Sched& sched, int64_t k, int64_t* q, double** Zb_out) {
  FitCtx& c = sh.x();
  *Zb_out = (double*)c.Xt.p + (pr.src == Source::F64 ? (k % 2) * sh.stream * npad_of(pr.n) : 0);
  if (pr.src != Source::SYNTH) GBM_HIP_TRY(hipStreamWaitEvent(c.stream.s, c.ev[k], 0));
  return standardize_chunk(pr, c, sched[k].first, sched[k].second, *Zb_out, q);
}

// Standardise + GRM of a streamed shard: every chunk's GRM added into G (a chunk planned as a single
// loci range goes through Gc), the copy of chunk k + 1 overlapping chunk k's GRM.
int stream_grm_shard(const Problem& pr, Shard& sh) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  const Sched sched = shard_schedule(pr, pl, sh.stream);
  const int64_t nch = (int64_t)sched.size();
  const bool bytes = pr.src != Source::F64;
  if (pr.src != Source::SYNTH) GBM_TRY(ensure_copy_stream(c));
  GBM_TRY(ensure_events(c, nch + 2));
  GBM_TRY(ensure(c.Xt, c.dev, (bytes ? 1 : 2) * sh.stream * npad * 8));
  GBM_TRY(ensure_locus_stats(c, pl));
  GBM_TRY(ensure(c.errs, c.dev, nch * 4));
  if (bytes) GBM_TRY(ensure(c.D8, c.dev, pl * n));
  int64_t wsb = 0;
  GBM_TRY(ensure_chunked_grm(c, n, sched, &wsb));
  GBM_HIP_TRY(hipMemsetAsync(c.q.p, 0, 8, s));
  GBM_HIP_TRY(hipMemsetAsync(c.errs.p, 0, nch * 4, s));
  if (pr.src == Source::SYNTH)
    GBM_TRY(gbm_dev_synth_dosage_i8((int8_t*)c.D8.p, n, pl, n, pr.seed, sh.j0, s));
  else
    GBM_TRY(stream_upload(pr, sh, sched, 0));
  for (int64_t k = 0; k < nch; k++) {
    double* Zb = nullptr;
    GBM_TRY(stream_standardize(pr, sh, sched, k, (int64_t*)c.q.p, &Zb));
    GBM_TRY(add_chunk_grm(c, Zb, sched[k].second, n, k, wsb, (int32_t*)c.errs.p + k));
    if (pr.src == Source::F64) GBM_HIP_TRY(hipEventRecord(c.ev[nch + k % 2], s));
    // queued behind chunk k's work (a pageable copy blocks this thread while the device computes)
    if (pr.src != Source::SYNTH && k + 1 < nch) GBM_TRY(stream_upload(pr, sh, sched, k + 1));
  }
  std::vector<int32_t> errs(nch, 0);
  GBM_HIP_TRY(hipMemcpyAsync(errs.data(), c.errs.p, nch * 4, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipMemcpyAsync(&sh.q_host, c.q.p, 8, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  for (int64_t k = 0; k < nch; k++)
    if (errs[k] < 0)
      return fail(GBM_E_HIP, "GRM in-order carry accumulation (streamed chunk " + std::to_string(k) +
                                 "): an inter-workgroup wait timed out (G is invalid)");
  return GBM_OK;
}

// Marker effects of a streamed shard into B (nt x p) and msum: from the resident dosages in one
// pass (z rebuilt in registers), or chunk by chunk from re-uploaded fp64 rows (standardised again:
// the same bits; kept count into a scratch cell).
int stream_effects_shard(const Problem& pr, Shard& sh, int64_t nt, double inv_q) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, npad = npad_of(n), pl = sh.p;
  hipStream_t s = c.stream.s;
  if (pr.src != Source::F64 || sh.exact) {  // resident dosage bytes (an exact shard of fp64 X holds D8 = 2x)
    const int ploidy = pr.src == Source::I8 ? pr.ploidy : 2;
    GBM_TRY(launch_marker_rows_i8((const int8_t*)c.D8.p, n, pl, n, ploidy, (const double*)c.A.p, npad, nt, inv_q,
                                  nullptr, (const double*)c.mean.p, (const double*)c.sd.p, (const int32_t*)c.keep.p,
                                  (double*)c.B.p, pl, s));
  } else {
    const Sched sched = shard_schedule(pr, pl, sh.stream);
    const int64_t nch = (int64_t)sched.size();
    GBM_TRY(ensure(c.q2, c.dev, 8));
    GBM_TRY(stream_upload(pr, sh, sched, 0));
    for (int64_t k = 0; k < nch; k++) {
      const int64_t j = sched[k].first, pc = sched[k].second;
      double* Zb = nullptr;
      GBM_TRY(stream_standardize(pr, sh, sched, k, (int64_t*)c.q2.p, &Zb));
      GBM_TRY(launch_marker_rows(Zb, npad, pc, n, (const double*)c.A.p, npad, nt, inv_q, nullptr,
                                 (const double*)c.sd.p + j, (const int32_t*)c.keep.p + j, (double*)c.B.p + j, pl, s));
      GBM_HIP_TRY(hipEventRecord(c.ev[nch + k % 2], s));
      if (k + 1 < nch) GBM_TRY(stream_upload(pr, sh, sched, k + 1));
    }
  }
  return launch_weighted_sum((const double*)c.mean.p, (const double*)c.B.p, pl, pl, nt, (double*)c.msum.p, s);
}

// ---- GRM mode of a call (include/gbm.h GBM_GRM_*) -------------------------------------------------------
// The exact-integer GRM (grm_exact.hip) of a dosage shard: the dosages stay resident as
// bytes (uploaded, converted from fp64 X on the device, or generated there), their GRM is computed exactly by
// int8 digit GEMMs, and the marker effects re-read them (stream_effects_shard). No fp64 genotype rows are
// formed. grm_mode exact / auto picks it per call; GBM_GRM (fp64 | exact | auto) only supplies the mode of
// calls that pass GBM_GRM_DEFAULT.

// fp64 host X of a shard → dosage bytes D8 = 2x on the device (chunks of loci through two fp64 staging
// buffers, the upload of chunk k + 1 beside the conversion of chunk k). Returns kNotDosage when some 2x is not
// exactly 0, 1 or 2 — with early_exit (grm_mode auto) already after the first chunk, so data that is not
// dosage-valued costs one chunk's upload before the fp64 path takes over.
int dosage_upload_shard(const Problem& pr, Shard& sh, bool early_exit) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  GBM_TRY(ensure_copy_stream(c));
  const int64_t chunk = std::max<int64_t>(256, std::min<int64_t>((pl + 7) / 8, ((int64_t)1 << 30) / (n * 8)));
  const Sched sched = chunk_schedule(pl, std::min(chunk, pl), false);
  const int64_t nch = (int64_t)sched.size();
  GBM_TRY(ensure_events(c, nch + 2));
  GBM_TRY(ensure(c.Xt, c.dev, 2 * std::min(chunk, pl) * n * 8));
  GBM_TRY(ensure(c.D8, c.dev, pl * n));
  GBM_TRY(ensure(c.errs, c.dev, 4));
  GBM_HIP_TRY(hipMemsetAsync(c.errs.p, 0, 4, s));
  int32_t bad = 0;
  for (int64_t k = 0; k < nch; k++) {
    const int64_t j = sched[k].first, pc = sched[k].second;
    double* buf = (double*)c.Xt.p + (k % 2) * std::min(chunk, pl) * n;
    if (k >= 2) GBM_HIP_TRY(hipStreamWaitEvent(c.copy.s, c.ev[nch + k % 2], 0));
    GBM_HIP_TRY(hipMemcpy2DAsync(buf, n * 8, pr.X + (sh.j0 + j) * pr.ld, pr.ld * 8, n * 8, pc, hipMemcpyHostToDevice,
                                 c.copy.s));
    GBM_HIP_TRY(hipEventRecord(c.ev[k], c.copy.s));
    GBM_HIP_TRY(hipStreamWaitEvent(s, c.ev[k], 0));
    GBM_TRY(launch_dosage_from_f64(buf, n, n, pc, (int8_t*)c.D8.p + j * n, n, (int32_t*)c.errs.p, s));
    GBM_HIP_TRY(hipEventRecord(c.ev[nch + k % 2], s));
    if (k == 0 && early_exit && nch > 1) {
      GBM_HIP_TRY(hipMemcpyAsync(&bad, c.errs.p, 4, hipMemcpyDeviceToHost, s));
      GBM_HIP_TRY(hipStreamSynchronize(s));
      if (bad) break;
    }
  }
  GBM_HIP_TRY(hipMemcpyAsync(&bad, c.errs.p, 4, hipMemcpyDeviceToHost, s));
  GBM_HIP_TRY(hipStreamSynchronize(s));
  GBM_HIP_TRY(hipStreamSynchronize(c.copy.s));  // no upload still writes a staging buffer
  if (bad) return kNotDosage;
  sh.d8_ready = true;
  return GBM_OK;
}

// fp64 host X of a shard → dosage bytes D8 = 2x, packed on the HOST (GBM_HOST_PACK, default 1; packed_upload):
// chunks of ≈ 16 MB of bytes each (GBM_PACK_CHUNK loci for tests) through a ring of 4 pinned slots and 4 events,
// nothing queued behind the copies. C2: 250 MB cross PCIe instead of 2 GB of fp64.
int host_pack_upload_shard(const Problem& pr, Shard& sh, int threads) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  const int64_t pc = std::max<int64_t>(1, std::min<int64_t>(pl, knob_i64("GBM_PACK_CHUNK", ((int64_t)16 << 20) / n)));
  GBM_TRY(ensure(c.D8, c.dev, pl * n));
  GBM_TRY(packed_upload(pr, sh, chunk_schedule(pl, pc, false), 4, 4, threads, nullptr));
  sh.d8_ready = true;
  return GBM_OK;
}

// check_bytes (grm_mode auto on int8 input): bytes outside {0, 1, 2} return kNotDosage instead of the
// exact kernels' GBM_E_ARG, so that the call falls back to the fp64 path
int exact_grm_shard(const Problem& pr, Shard& sh, bool check_bytes) {
  FitCtx& c = sh.x();
  const int64_t n = pr.n, gdim = gdim_of(n), pl = sh.p;
  GBM_HIP_TRY(hipSetDevice(c.dev));
  hipStream_t s = c.stream.s;
  GBM_TRY(ensure(c.D8, c.dev, pl * n));
  GBM_TRY(ensure_locus_stats(c, pl));
  GBM_TRY(ensure(c.G, c.dev, gdim * gdim * 8));
  const int64_t wsb = gbm_dev_grm_exact_workspace(n, pl);
  GBM_TRY(ensure(c.wsg, c.dev, wsb));
  if (!sh.d8_ready) {
    if (pr.src == Source::SYNTH)
      GBM_TRY(gbm_dev_synth_dosage_i8((int8_t*)c.D8.p, n, pl, n, pr.seed, sh.j0, s));
    else if (pr.src == Source::I8)
      GBM_HIP_TRY(hipMemcpy2DAsync(c.D8.p, n, pr.D + sh.j0 * pr.ld, pr.ld, n, pl, hipMemcpyHostToDevice, s));
    else
      return fail(GBM_E_ARG, "exact GRM: fp64 genotypes not converted to dosages");
  }
  if (check_bytes) {
    int32_t bad = 0;
    GBM_TRY(ensure(c.errs, c.dev, 4));
    GBM_HIP_TRY(hipMemsetAsync(c.errs.p, 0, 4, s));
    GBM_TRY(launch_dosage_check_i8((const int8_t*)c.D8.p, n, n, pl, (int32_t*)c.errs.p, s));
    GBM_HIP_TRY(hipMemcpyAsync(&bad, c.errs.p, 4, hipMemcpyDeviceToHost, s));
    GBM_HIP_TRY(hipStreamSynchronize(s));
    if (bad) return kNotDosage;
  }
  GBM_HIP_TRY(hipMemsetAsync(c.q.p, 0, 8, s));
  GBM_TRY(launch_grm_exact((const int8_t*)c.D8.p, n, pl, n, 2, (double*)c.G.p, gdim, (double*)c.mean.p,
                           (double*)c.sd.p, (int32_t*)c.keep.p, (int64_t*)c.q.p, 0, c.wsg.p, wsb, nullptr, s));
  GBM_HIP_TRY(hipMemcpyAsync(&sh.q_host, c.q.p, 8, hipMemcpyDeviceToHost, s));
  return grm_exact_status(c.wsg.p, n, pl, s);  // syncs the stream
}

}  // namespace gbm
