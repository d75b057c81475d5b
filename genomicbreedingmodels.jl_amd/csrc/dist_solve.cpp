// What the shard leaders of a C-ABI call do together (fit_ctx.h): the sum of the partial GRMs
// (device-side for shards on one device, RCCL all-reduce across devices, device copies between
// leaders that share one) and the Cholesky solve factored across the leaders. RCCL communicators
// are created once per device set and reused.
#include <rccl/rccl.h>

#include <atomic>

#include "fit_ctx.h"

namespace gbm {

// ---- RCCL communicators, one set per distinct device list, created once ----------------------

// successful RCCL collectives so far (gbm_debug_rccl_calls: tests check that the RCCL path ran)
static std::atomic<int64_t> g_rccl_allreduce{0}, g_rccl_allgather{0};

void rccl_call_counts(int64_t* allreduce, int64_t* allgather) {
  if (allreduce) *allreduce = g_rccl_allreduce.load();
  if (allgather) *allgather = g_rccl_allgather.load();
}

namespace {

struct CommSet {
  std::vector<ncclComm_t> comms;
  std::mutex mu;  // one collective at a time on a communicator (same op order on every device)
};

int comm_set(const std::vector<int>& devs, CommSet** out) {
  static std::mutex mu;
  static auto* cache = new std::map<std::vector<int>, std::unique_ptr<CommSet>>;  // never destroyed
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache->find(devs);
  if (it == cache->end()) {
    auto cs = std::make_unique<CommSet>();
    cs->comms.resize(devs.size());
    ncclResult_t r = ncclCommInitAll(cs->comms.data(), (int)devs.size(), devs.data());
    if (r != ncclSuccess) return fail(GBM_E_RCCL, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
    it = cache->emplace(devs, std::move(cs)).first;
  }
  *out = it->second.get();
  return GBM_OK;
}

// copy = true: the contexts' copy streams (the distributed factorisation's area exchange)
int sync_all(Shards& shards, const std::vector<int>& which, bool copy = false) {
  for (int k : which) {
    FitCtx& c = shards[k]->x();
    GBM_HIP_TRY(hipSetDevice(c.dev));
    GBM_HIP_TRY(hipStreamSynchronize(copy ? c.copy.s : c.stream.s));
  }
  return GBM_OK;
}

// All-reduce by copies (leaders sharing a device, GBM_SHARD_LEADERS=each): the packed partials
// summed in leader order on the first leader (the order of the same-device sum), then copied back.
int copy_allreduce(Shards& shards, const std::vector<int>& leaders, int64_t psz) {
  GBM_TRY(sync_all(shards, leaders));
  FitCtx& c0 = shards[leaders[0]]->x();
  GBM_HIP_TRY(hipSetDevice(c0.dev));
  GBM_TRY(ensure(c0.tmp, c0.dev, psz * 8));
  for (size_t k = 1; k < leaders.size(); k++) {
    FitCtx& ck = shards[leaders[k]]->x();
    GBM_TRY(copy_dd(c0, c0.tmp.p, ck, ck.packed.p, psz * 8));
    GBM_TRY(launch_add_inplace((double*)c0.packed.p, (const double*)c0.tmp.p, psz, c0.stream.s));
  }
  GBM_TRY(sync_all(shards, {leaders[0]}));
  for (size_t k = 1; k < leaders.size(); k++) {
    FitCtx& ck = shards[leaders[k]]->x();
    GBM_TRY(copy_dd(ck, ck.packed.p, c0, c0.packed.p, psz * 8));
  }
  return GBM_OK;
}

// All-gather of the leaders' strip packs (cnt doubles each) into every leader's `gathered`, in
// leader (= rank) order: RCCL across distinct devices, device copies when leaders share one.
// area = true: the area buffers (astrip -> agathered) on the copy streams.
// on_copy: the strip buffers on the copy streams (the look-ahead's row exchange).
int allgather_strips(Shards& shards, const std::vector<int>& leaders, CommSet* cs, int64_t cnt, bool area = false,
                     bool on_copy = false) {
  auto src = [&](FitCtx& c) { return area ? c.astrip.p : c.strip.p; };
  auto dst = [&](FitCtx& c) { return (double*)(area ? c.agathered.p : c.gathered.p); };
  const bool cp = area || on_copy;
  if (cs) {
    ncclResult_t r = ncclGroupStart();
    for (size_t k = 0; k < leaders.size() && r == ncclSuccess; k++) {
      FitCtx& c = shards[leaders[k]]->x();
      r = ncclAllGather(src(c), dst(c), (size_t)cnt, ncclDouble, cs->comms[k], cp ? c.copy.s : c.stream.s);
    }
    ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      return fail(GBM_E_RCCL, std::string("ncclAllGather(Cholesky strip): ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    g_rccl_allgather.fetch_add(1);
    return GBM_OK;
  }
  GBM_TRY(sync_all(shards, leaders, cp));  // every pack is complete
  for (int d : leaders) {
    FitCtx& cd = shards[d]->x();
    for (size_t r = 0; r < leaders.size(); r++) {
      FitCtx& cr = shards[leaders[r]]->x();
      GBM_TRY(copy_dd(cd, dst(cd) + r * cnt, cr, src(cr), cnt * 8, cp ? cd.copy.s : cd.stream.s));
    }
  }
  return sync_all(shards, leaders, cp);  // no copy still reads a pack the next step overwrites
}

}  // namespace

// Copy bytes from one context's buffer to another's on dst's stream (same device or peer).
int copy_dd(FitCtx& dst, void* d, const FitCtx& src, const void* s, int64_t bytes, hipStream_t on) {
  GBM_HIP_TRY(hipSetDevice(dst.dev));
  if (!on) on = dst.stream.s;
  if (dst.dev == src.dev)
    GBM_HIP_TRY(hipMemcpyAsync(d, s, (size_t)bytes, hipMemcpyDeviceToDevice, on));
  else
    GBM_HIP_TRY(hipMemcpyPeerAsync(d, dst.dev, s, src.dev, (size_t)bytes, on));
  return GBM_OK;
}

// GBM_FORCE_RCCL=1 (a test hook): the collectives of a fit run even with one device
// leader — the partial-GRM all-reduce and the Cholesky strip all-gathers (from n >= GBM_DIST_SOLVE_MIN_N)
// execute on a 1-rank RCCL communicator (ncclCommInitAll over the one device) with the real payloads,
// so the RCCL path runs on a one-GPU box. A sum or gather over one rank is the identity: same bits.
bool force_rccl() { return knob_i64("GBM_FORCE_RCCL", 0) != 0; }

// Sum the partial GRMs of all shards into each device leader's G: the upper 128-tiles packed
// contiguously (half the bytes of G's rows); shards on one device added there in shard order,
// then the leaders all-reduced over RCCL (xGMI), then unpacked.
int allreduce_grm(Shards& shards, int64_t n) {
  const bool force = force_rccl();
  if (shards.size() < 2 && !force) return GBM_OK;
  const int64_t gdim = gdim_of(n), psz = gbm_dev_grm_packed_size(n);
  for (auto& sh : shards) {
    FitCtx& c = sh->x();
    GBM_HIP_TRY(hipSetDevice(c.dev));
    GBM_TRY(ensure(c.packed, c.dev, psz * 8));
    GBM_TRY(gbm_dev_grm_pack((const double*)c.G.p, gdim, n, (double*)c.packed.p, c.stream.s));
  }
  std::vector<int> leaders, devs;
  shard_leaders(shards, leaders, devs);
  for (size_t k = 0; k < shards.size(); k++) {
    Shard& sh = *shards[k];
    if (sh.leader == (int)k) continue;
    FitCtx& lc = shards[sh.leader]->x();
    GBM_HIP_TRY(hipSetDevice(lc.dev));
    GBM_HIP_TRY(hipStreamSynchronize(sh.x().stream.s));
    GBM_TRY(launch_add_inplace((double*)lc.packed.p, (const double*)sh.x().packed.p, psz, lc.stream.s));
  }
  std::vector<int> sorted = devs;
  std::sort(sorted.begin(), sorted.end());
  const bool shared_dev = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
  if (leaders.size() > 1 && shared_dev) {
    GBM_TRY(copy_allreduce(shards, leaders, psz));
  } else if (leaders.size() > 1 || force) {
    CommSet* cs = nullptr;
    GBM_TRY(comm_set(devs, &cs));
    std::lock_guard<std::mutex> lock(cs->mu);
    int rc = GBM_OK;
    ncclResult_t r = ncclGroupStart();
    for (size_t k = 0; k < leaders.size() && r == ncclSuccess; k++) {
      FitCtx& c = shards[leaders[k]]->x();
      r = ncclAllReduce(c.packed.p, c.packed.p, (size_t)psz, ncclDouble, ncclSum, cs->comms[k], c.stream.s);
    }
    ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      rc = fail(GBM_E_RCCL, std::string("ncclAllReduce(partial GRM): ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    else
      g_rccl_allreduce.fetch_add(1);
    for (int k : leaders) {  // complete the collective while holding the communicator
      FitCtx& c = shards[k]->x();
      (void)hipSetDevice(c.dev);
      if (hipStreamSynchronize(c.stream.s) != hipSuccess && rc == GBM_OK) rc = fail(GBM_E_HIP, "stream sync after all-reduce");
    }
    if (rc != GBM_OK) return rc;
  }
  for (int k : leaders) {
    FitCtx& c = shards[k]->x();
    GBM_HIP_TRY(hipSetDevice(c.dev));
    GBM_TRY(gbm_dev_grm_unpack((const double*)c.packed.p, n, (double*)c.G.p, gdim, c.stream.s));
  }
  return GBM_OK;
}

// GBLUP solve of V = G/q + λI factored across the device leaders (each holding the summed G): the
// C-ABI counterpart of gbm.sharded.chol_distributed. Per panel group, the leaders
// all-gather the group's diagonal area (after an earlier distributed group: its columns were updated
// by their owners) and factor its first block, every leader runs the group's panels and row updates
// on its own 128-column tiles (plus the area and the right-hand sides), the group's solved rows are
// all-gathered (each leader then holds them at every column, with their lower copy), and the
// trailing update runs on the leader's own tiles and the right-hand sides. Once the
// trailing matrix is small (GBM_DIST_TAIL_ROWS, default 8192) every remaining row is gathered once
// and the tail and the back substitution run on every leader. Bit-identical to the redundant
// launch-per-panel solve (the same kernels compute every tile from the same operands). Replaces the
// per-device pinv/Cholesky of V (reference src/gwas.jl:472,595) at multi-GPU scale.
int solve_distributed(Shards& shards, const std::vector<int>& leaders, const std::vector<int>& ldevs, int64_t n,
                      double inv_q, double lambda, int64_t nrhs) {
  const int64_t npad = npad_of(n), gdim = gdim_of(n), nb = npad / kCholNB;
  const int R = (int)leaders.size();
  const int64_t tail_rows = knob_i64("GBM_DIST_TAIL_ROWS", 8192);
  std::vector<int> sorted = ldevs;
  std::sort(sorted.begin(), sorted.end());
  CommSet* cs = nullptr;
  if (std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end()) GBM_TRY(comm_set(ldevs, &cs));
  std::unique_lock<std::mutex> lock;
  if (cs) lock = std::unique_lock<std::mutex>(cs->mu);  // this solve's collectives in one order on every device
  auto each = [&](auto&& fn) -> int {
    for (int r = 0; r < R; r++) {
      FitCtx& c = shards[leaders[r]]->x();
      GBM_HIP_TRY(hipSetDevice(c.dev));
      GBM_TRY(fn(r, c));
    }
    return GBM_OK;
  };
  auto distributable = [&](int64_t kb) {  // (a group reaching the end is the dataflow tail, GBM_CHOL_TAIL_FLOW)
    const int64_t g = gbm_dev_chol_group_size(n, kb);
    return gdim - kCholNB * kb > tail_rows && g >= 2 && g < nb - kb && (kCholNB * kb) % 128 == 0;
  };
  // rows [64 kb, 64 (kb + rows64)) of every leader's own tiles, all-gathered. kRows: final U rows
  // (their lower copy completed too); kRest: the trailing matrix's remaining rows (the tail switch);
  // kArea: the square diagonal area of a group only
  enum { kRows, kRest, kArea };
  // on_copy (kRows only): on the copy streams — the look-ahead's row exchange of the next group, beside the
  // trailing update on the main streams (the strip buffers are then free of main-stream work: the sizes
  // do not grow from group to group, and the tail's kRest exchange comes after a join)
  auto exchange = [&](int64_t kb, int64_t rows64, int what, bool on_copy = false) -> int {
    const int64_t cnt = what == kArea ? gbm_dev_chol_area_doubles(n, kb, rows64, R)
                                      : gbm_dev_chol_strip_doubles(n, kb, rows64, R);
    GBM_TRY(each([&](int r, FitCtx& c) {
      GBM_TRY(ensure(c.strip, c.dev, cnt * 8));
      GBM_TRY(ensure(c.gathered, c.dev, R * cnt * 8));
      const hipStream_t s = on_copy ? c.copy.s : c.stream.s;
      if (what == kArea)
        return gbm_dev_chol_area_pack((const double*)c.G.p, gdim, n, kb, rows64, r, R, (double*)c.strip.p, s);
      return gbm_dev_chol_strip_pack((const double*)c.G.p, gdim, n, kb, rows64, r, R, (double*)c.strip.p, s);
    }));
    GBM_TRY(allgather_strips(shards, leaders, cs, cnt, false, on_copy));
    return each([&](int r, FitCtx& c) {
      const double* gathered = (const double*)c.gathered.p;
      if (what == kRows)
        return gbm_dev_chol_strip_unpack_rows((double*)c.G.p, gdim, n, kb, rows64, r, R, gathered,
                                              on_copy ? c.copy.s : c.stream.s);
      if (what == kArea) {
        GBM_TRY(gbm_dev_chol_area_unpack((double*)c.G.p, gdim, n, kb, rows64, R, gathered, c.stream.s));
      } else {
        GBM_TRY(gbm_dev_chol_strip_unpack((double*)c.G.p, gdim, n, kb, rows64, R, gathered, c.stream.s));
      }
      return gbm_dev_chol_factor_diag((double*)c.G.p, gdim, n, kb, (int32_t*)c.info.p, c.wss.p, c.wss.cap, c.stream.s);
    });
  };
  // V only on the columns each leader reads before an exchange overwrites them, when the factorisation
  // distributes from the first group on
  const bool dist0 = R > 1 && distributable(0);
  GBM_TRY(each([&](int r, FitCtx& c) {
    return gbm_dev_chol_prepare_cols((double*)c.G.p, gdim, n, inv_q, nullptr, lambda, (const double*)c.Y.p, npad,
                                     nrhs, dist0 ? r : 0, dist0 ? R : 1, (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                                     c.stream.s);
  }));
  if (R == 1) {
    // one leader (GBM_FORCE_RCCL): the redundant solve, each distributable group's final rows passed
    // through the 1-rank all-gather between its panels and its trailing update (an identity exchange
    // with the real payload; same bits as gbm_dev_gblup_solve's launch-per-panel path)
    FitCtx& c = shards[leaders[0]]->x();
    for (int64_t kb = 0; kb < nb;) {
      const int64_t g = gbm_dev_chol_group_size(n, kb);
      if (distributable(kb)) {
        GBM_TRY(gbm_dev_chol_group_panels((double*)c.G.p, gdim, n, kb, 0, 1, (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                                          c.stream.s));
        GBM_TRY(exchange(kb, g, kRows));
        GBM_TRY(gbm_dev_chol_group_update((double*)c.G.p, gdim, n, kb, 0, 1, (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                                          c.stream.s));
      } else {
        GBM_TRY(gbm_dev_chol_group((double*)c.G.p, gdim, n, kb, 0, 1, (int32_t*)c.info.p, c.wss.p, c.wss.cap, c.stream.s));
      }
      kb += g;
    }
    GBM_TRY(gbm_dev_chol_finish((double*)c.G.p, gdim, n, (const double*)c.Y.p, npad, nrhs, lambda, (double*)c.A.p,
                                (double*)c.gebv.p, npad, (double*)c.mu.p, (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                                c.stream.s));
    return cs ? sync_all(shards, leaders) : GBM_OK;
  }
  // GBM_DIST_OVERLAP (default 1): the next group's area is updated and all-gathered on the copy streams
  // while the rest of the trailing update runs (same kernels, same tiles: same bits)
  const bool overlap = knob_i64("GBM_DIST_OVERLAP", 1) != 0;
  // GBM_DIST_LOOKAHEAD (with overlap): the next group's rows are updated first, then its panels and row
  // exchange run on the copy streams beside the rest of the trailing update. Default 1 for the device-copy
  // exchanges (the one-GPU rehearsal, tested bit-identical); default 0 over real RCCL (cs != nullptr) until a
  // multi-GPU run has shown the look-ahead's stream/communicator interleaving bit-identical there
  const bool lookahead = overlap && knob_i64("GBM_DIST_LOOKAHEAD", cs ? 0 : 1) != 0;
  if (overlap)
    GBM_TRY(each([&](int, FitCtx& c) -> int {
      GBM_TRY(ensure_copy_stream(c));
      if (!c.ev_area) GBM_HIP_TRY(hipEventCreateWithFlags(&c.ev_area, hipEventDisableTiming));
      if (!c.ev_upd) GBM_HIP_TRY(hipEventCreateWithFlags(&c.ev_upd, hipEventDisableTiming));
      return GBM_OK;
    }));
  auto update = [&](int64_t kb, int64_t lo, int64_t hi) {
    return each([&](int r, FitCtx& c) {
      return gbm_dev_chol_group_update_cols((double*)c.G.p, gdim, n, kb, r, R, lo, hi, (int32_t*)c.info.p, c.wss.p,
                                            c.wss.cap, c.stream.s);
    });
  };
  // the update of the columns [lo, hi) (the next group's area: about one tile column per rank, a few
  // workgroups one K = 64 g tile long) on the copy streams, beside the rest of the update on the main ones
  auto area_update_async = [&](int64_t kb, int64_t lo, int64_t hi) {
    return each([&](int r, FitCtx& c) -> int {
      GBM_HIP_TRY(hipEventRecord(c.ev_upd, c.stream.s));  // after the group's rows arrived
      GBM_HIP_TRY(hipStreamWaitEvent(c.copy.s, c.ev_upd, 0));
      return gbm_dev_chol_group_update_cols((double*)c.G.p, gdim, n, kb, r, R, lo, hi, (int32_t*)c.info.p, c.wss.p,
                                            c.wss.cap, c.copy.s);
    });
  };
  // the area exchange of the group at kb on the copy streams (after area_update_async); ends with ev_area,
  // which the group's panels wait for
  auto area_async = [&](int64_t kb, int64_t g) -> int {
    const int64_t cnt = gbm_dev_chol_area_doubles(n, kb, g, R);  // non-increasing over the groups
    GBM_TRY(each([&](int r, FitCtx& c) -> int {
      GBM_TRY(ensure(c.astrip, c.dev, cnt * 8));
      GBM_TRY(ensure(c.agathered, c.dev, R * cnt * 8));
      return gbm_dev_chol_area_pack((const double*)c.G.p, gdim, n, kb, g, r, R, (double*)c.astrip.p, c.copy.s);
    }));
    GBM_TRY(allgather_strips(shards, leaders, cs, cnt, true));
    return each([&](int, FitCtx& c) -> int {
      GBM_TRY(gbm_dev_chol_area_unpack((double*)c.G.p, gdim, n, kb, g, R, (const double*)c.agathered.p, c.copy.s));
      GBM_TRY(gbm_dev_chol_factor_diag((double*)c.G.p, gdim, n, kb, (int32_t*)c.info.p, c.wss.p, c.wss.cap, c.copy.s));
      GBM_HIP_TRY(hipEventRecord(c.ev_area, c.copy.s));
      return GBM_OK;
    });
  };
  bool dist = R > 1 && distributable(0), stale = false;  // stale: a distributed update skipped other ranks' tiles
  bool area_pending = false;                    // the current group's area is being exchanged (overlap)
  bool ahead = false;                           // (look-ahead) the current group's panels and rows: copy streams
  for (int64_t kb = 0; kb < nb;) {
    const int64_t g = gbm_dev_chol_group_size(n, kb);
    if (!dist) {
      GBM_TRY(each([&](int, FitCtx& c) {
        return gbm_dev_chol_group((double*)c.G.p, gdim, n, kb, 0, 1, (int32_t*)c.info.p, c.wss.p, c.wss.cap, c.stream.s);
      }));
      kb += g;
      continue;
    }
    if (area_pending) {
      GBM_TRY(each([&](int, FitCtx& c) -> int {
        GBM_HIP_TRY(hipStreamWaitEvent(c.stream.s, c.ev_area, 0));
        return GBM_OK;
      }));
      area_pending = false;
    } else if (stale) {
      GBM_TRY(exchange(kb, g, kArea));
    }
    auto panels = [&](int64_t k, bool on_copy) {
      return each([&](int r, FitCtx& c) {
        return gbm_dev_chol_group_panels((double*)c.G.p, gdim, n, k, r, R, (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                                         on_copy ? c.copy.s : c.stream.s);
      });
    };
    if (!ahead) {
      GBM_TRY(panels(kb, false));
      GBM_TRY(exchange(kb, g, kRows));
    }
    ahead = false;
    const int64_t k1 = kb + g;
    const bool next_dist = k1 < nb && distributable(k1);
    if (overlap && next_dist) {
      const int64_t g1 = gbm_dev_chol_group_size(n, k1);
      const int64_t area_hi = kCholNB * (k1 + g1);
      if (lookahead) {
        // on the copy streams: the next group's rows of every kept column (its area among them: one launch),
        // the area exchange, the next group's panels and row exchange — beside the rest of the update on
        // the main streams (the rows from area_hi on: disjoint tiles)
        auto tiles = [&](int64_t r_lo, int64_t r_hi, int64_t c_lo, bool on_copy) {
          return each([&](int r, FitCtx& c) -> int {
            if (on_copy) {
              GBM_HIP_TRY(hipEventRecord(c.ev_upd, c.stream.s));  // after the group's rows arrived
              GBM_HIP_TRY(hipStreamWaitEvent(c.copy.s, c.ev_upd, 0));
            }
            return gbm_dev_chol_group_update_tiles((double*)c.G.p, gdim, n, kb, r, R, r_lo, r_hi, c_lo, gdim,
                                                   (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                                                   on_copy ? c.copy.s : c.stream.s);
          });
        };
        GBM_TRY(tiles(kCholNB * k1, area_hi, kCholNB * k1, true));
        GBM_TRY(area_async(k1, g1));
        GBM_TRY(panels(k1, true));
        GBM_TRY(exchange(k1, g1, kRows, true));
        GBM_TRY(each([&](int, FitCtx& c) -> int {
          GBM_HIP_TRY(hipEventRecord(c.ev_area, c.copy.s));  // the next group waits for all of it
          return GBM_OK;
        }));
        GBM_TRY(tiles(area_hi, gdim, area_hi, false));
        ahead = true;
      } else {
        GBM_TRY(area_update_async(kb, kCholNB * k1, area_hi));  // the next group's area, on the copy streams
        GBM_TRY(update(kb, area_hi, gdim));  // the rest (and the right-hand sides) beside it and its exchange
        GBM_TRY(area_async(k1, g1));
      }
      area_pending = true;
    } else {
      GBM_TRY(update(kb, kCholNB * k1, gdim));
    }
    stale = true;
    kb = k1;
    if (kb >= nb) break;
    dist = next_dist;
    if (!dist) GBM_TRY(exchange(kb, nb - kb, kRest));  // the tail: every remaining row, once
  }
  GBM_TRY(each([&](int, FitCtx& c) {
    return gbm_dev_chol_finish((double*)c.G.p, gdim, n, (const double*)c.Y.p, npad, nrhs, lambda, (double*)c.A.p,
                               (double*)c.gebv.p, npad, (double*)c.mu.p, (int32_t*)c.info.p, c.wss.p, c.wss.cap,
                               c.stream.s);
  }));
  // the solve's collectives complete while this call still holds the communicators (as in
  // allreduce_grm): another call's collectives on the same device set come strictly after
  return cs ? sync_all(shards, leaders) : GBM_OK;
}

}  // namespace gbm
