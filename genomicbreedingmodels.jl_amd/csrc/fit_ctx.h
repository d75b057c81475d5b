// The pooled fit contexts and the SNP-column shards of a C-ABI call, and what capi.cpp (entry points,
// run_fit), shard_grm.cpp (a shard's genotypes -> its partial GRM, streamed effects) and
// dist_solve.cpp (RCCL, copy collectives, the distributed Cholesky) share. Not part of the ABI.
//
// Re-entrant, as cvmultithread! requires (reference src/cross_validation.jl:159): a call leases
// one pooled fit context per shard (its own stream and buffers) and returns it afterwards; the
// contexts' buffers only grow, so repeated calls of one shape allocate no device memory.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gbm_internal.h"
#include "host_util.h"

namespace gbm {

// ---- pooled fit contexts -----------------------------------------------------------------------

struct FitCtx {
  int dev = 0;
  Stream stream;
  Stream copy;                   // host -> device copies of the pipelined upload (created on first use)
  std::vector<hipEvent_t> ev;    // one per upload chunk
  DevBuf Xt, D8, mean, sd, keep, q, G, Gc, wsg, Y, A, gebv, mu, info, wss, B, msum, packed, out, part;
  DevBuf tmp, strip, gathered;   // copy exchanges; the distributed factorisation's strip all-gather
  DevBuf errs, q2;               // streamed fit: per-chunk carry error cells; scratch kept count
  DevBuf astrip, agathered;      // the distributed factorisation's area all-gather (on the copy stream)
  hipEvent_t ev_area = nullptr, ev_upd = nullptr;  // area exchange done / next area updated
  HostPinned pack;               // host-pack staging ring (fp64 host X packed to dosage bytes)
  ~FitCtx() {
    (void)hipSetDevice(dev);
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    if (ev_area) (void)hipEventDestroy(ev_area);
    if (ev_upd) (void)hipEventDestroy(ev_upd);
  }
};

inline CtxPool<FitCtx>& pool() { return CtxPool<FitCtx>::instance(); }

// One SNP-column shard [j0, j0 + p) on a leased context.
struct Shard {
  std::unique_ptr<FitCtx> c;
  int64_t j0 = 0, p = 0, q_host = 0;
  int64_t stream = 0;  // loci per chunk of the loci-streamed mode (plan_streaming); 0: resident
  bool exact = false;  // the exact-integer GRM of the resident dosages (grm_exact.hip, grm_mode exact / auto)
  bool d8_ready = false;  // fp64 X already converted into the dosage bytes D8 (dosage_upload_shard)
  int leader = -1;  // index of the shard that holds this device's summed GRM (itself if first)
  ~Shard() {
    if (c) pool().release(std::move(c));
  }
  FitCtx& x() { return *c; }
};
using Shards = std::vector<std::unique_ptr<Shard>>;

enum class Source { F64, I8, SYNTH };

struct Problem {
  Source src;
  const double* X;
  const int8_t* D;
  int ploidy;
  int64_t n, p, ld;
  uint64_t seed = 0;  // Source::SYNTH: genotypes generated on each device
};

constexpr int kNotDosage = 1;  // internal: the genotypes are not diploid dosages (auto falls back to fp64)

// GBM_SHARD_LEADERS=each: every shard keeps its own full G and is a rank of its own in the GRM sum
// and the distributed factorisation, its exchanges done by device copies. That is the one-GPU
// rehearsal of the multi-device path (devices = [0, 0, ...]; RCCL cannot put two ranks on one
// device). Default: one leader per device, RCCL between the leaders.
inline bool each_shard_leads() {
  const char* e = ::gbm::knob("GBM_SHARD_LEADERS");
  return e && strcmp(e, "each") == 0;
}

// Contiguous SNP-column blocks, one per listed device; leader = first shard on each device.
inline int make_shards(const std::vector<int>& devs, int64_t p, Shards& shards) {
  const int nd = (int)std::min<int64_t>((int64_t)devs.size(), p);
  const int64_t per = (p + nd - 1) / nd;
  const bool each = each_shard_leads();
  for (int k = 0; k < nd; k++) {
    const int64_t j0 = k * per;
    if (j0 >= p) break;
    auto sh = std::make_unique<Shard>();
    GBM_TRY(pool().acquire(devs[k], sh->c));
    sh->j0 = j0;
    sh->p = std::min(per, p - j0);
    for (size_t m = 0; m < shards.size() && !each; m++)
      if (shards[m]->x().dev == devs[k]) {
        sh->leader = shards[m]->leader;
        break;
      }
    if (sh->leader < 0) sh->leader = (int)shards.size();
    shards.push_back(std::move(sh));
  }
  return GBM_OK;
}

// The leaders (shard indices, in shard order = rank order) and their devices.
inline void shard_leaders(Shards& shards, std::vector<int>& leaders, std::vector<int>& ldevs) {
  for (size_t k = 0; k < shards.size(); k++)
    if (shards[k]->leader == (int)k) {
      leaders.push_back((int)k);
      ldevs.push_back(shards[k]->x().dev);
    }
}

// Runs fn(shard) for every shard at once, one host thread per shard (shard 0 on the calling
// thread): each device (and each shard sharing a device) uploads, standardises and builds its
// partial GRM side by side with the others. A pageable hipMemcpy blocks its calling thread until
// the copy is done, and each shard's final stream sync waits only for its own work, so driving the
// shards from one thread would run them back to back. Every shard's device work is the same as
// when run alone (fixed summation orders), so results do not depend on the interleaving. The
// lowest-numbered failing shard's code and message become the call's (the thread-local error of
// the worker is carried over to the caller).
template <class Fn>
int parallel_shards(Shards& shards, Fn&& fn) {
  const size_t m = shards.size();
  const char* e = ::gbm::knob("GBM_SHARD_THREADS");  // "0": one shard after the other (A/B, tests)
  if (m == 1 || (e && strcmp(e, "0") == 0)) {
    for (size_t k = 0; k < m; k++) GBM_TRY(fn(k, *shards[k]));
    return GBM_OK;
  }
  std::vector<int> rc(m, GBM_OK);
  std::vector<std::string> msg(m);
  auto run = [&](size_t k) {
    rc[k] = fn(k, *shards[k]);
    if (rc[k] != GBM_OK) msg[k] = last_error();
  };
  std::vector<std::thread> th;
  th.reserve(m - 1);
  for (size_t k = 1; k < m; k++) {
    try {
      th.emplace_back(run, k);
    } catch (...) {  // no thread available: run this shard on the calling thread
      run(k);
    }
  }
  run(0);
  for (auto& t : th) t.join();
  // a real error (negative code) of any shard takes priority over an internal status (kNotDosage > 0) of a
  // lower-numbered one: a fall-back must never hide a HIP/RCCL/OOM failure
  for (size_t k = 0; k < m; k++)
    if (rc[k] < 0) return fail(rc[k], msg[k]);
  for (size_t k = 0; k < m; k++)
    if (rc[k] != GBM_OK) return fail(rc[k], msg[k]);
  return GBM_OK;
}

// ---- shard_grm.cpp: a shard's genotypes -> its partial GRM; the streamed marker effects ----------
int ensure_copy_stream(FitCtx& c);
int64_t host_chunk(int64_t p);
int prepare_shard(const Problem& pr, Shard& sh, bool center_only = false, bool sync = true);
int grm_shard(const Problem& pr, Shard& sh);
int prepare_grm_shard(const Problem& pr, Shard& sh);
int upload_grm_pipelined(const Problem& pr, Shard& sh, int64_t chunk);
int upload_grm_pipelined_packed(const Problem& pr, Shard& sh, int64_t chunk, int threads);
int plan_streaming(const Problem& pr, Shards& shards, bool reml);
int stream_grm_shard(const Problem& pr, Shard& sh);
int dosage_upload_shard(const Problem& pr, Shard& sh, bool early_exit);
int host_pack_upload_shard(const Problem& pr, Shard& sh, int threads);
int exact_grm_shard(const Problem& pr, Shard& sh, bool check_bytes = false);
int stream_effects_shard(const Problem& pr, Shard& sh, int64_t nt, double inv_q);

// ---- dist_solve.cpp: collectives over the shard leaders, the distributed Cholesky ----------------
int copy_dd(FitCtx& dst, void* d, const FitCtx& src, const void* s, int64_t bytes, hipStream_t on = nullptr);
bool force_rccl();
int allreduce_grm(Shards& shards, int64_t n);
int solve_distributed(Shards& shards, const std::vector<int>& leaders, const std::vector<int>& ldevs, int64_t n,
                      double inv_q, double lambda, int64_t nrhs);
void rccl_call_counts(int64_t* allreduce, int64_t* allgather);

}  // namespace gbm
