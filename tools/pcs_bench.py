#!/usr/bin/env python
"""Timing of the principal components of a session's cached GRM (GenotypeSession.pcs) on synthetic genotypes, by
default at the C2 shape (n = 5 000 x p = 50 000), against the host path it replaces in gwasols (download of the
n x n GRM + gbm.gwas.pc1_of_grm).

How it measures: each pcs configuration (kind "grm" with k = 4, kind "reference" with k = 1) runs `--warmup` times
first (the first call also builds and caches the GRM), then `--reps` times; each figure is the median with its range
(min-max) of the host wall-clock around the (synchronous) session call, with the iteration count beside it. The block
product (gbm_dev_rows_times_sym, 32 rows) and the symmetric fill are timed with device events on a K built by the
same kernels through the stream-ordered C ABI (HipShardStages); the product's byte bound is npad²·8 B over the
6.3 TB/s a streaming kernel reaches on one MI355X (8 TB/s on the data sheet). The host path is timed once: the
device-to-host copy of K, then pc1_of_grm; |cos| between its vector and the device's PC1 is reported.

Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomicbreedingmodels.jl_amd"))

import numpy as np  # noqa: E402

HBM_STREAM_TBS = 6.3


def med(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--p", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=5000)
    ap.add_argument("--product-reps", type=int, default=50)
    ap.add_argument("--no-host", action="store_true", help="skip the host path (an n x n eigh)")
    a = ap.parse_args()

    import torch

    import gbm
    from gbm import _lib
    from gbm.gwas import pc1_of_grm
    from gbm.sharded import HipShardStages

    n, p = a.n, a.p
    idx = np.arange(n)
    res = {"tool": "pcs_bench", "n": n, "p": p, "tol": a.tol, "reps": a.reps, "warmup": a.warmup}

    # ---- pcs through the session ------------------------------------------------------------------------------
    pc1 = None
    with gbm.GenotypeSession.synthetic(a.seed, n, p) as s:
        for kind, k in (("grm", 4), ("reference", 1)):
            ms = []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    out = s.pcs(idx, k, kind=kind, tol=a.tol, max_iter=a.max_iter)
                t1 = time.perf_counter()
                if r >= a.warmup:
                    ms.append((t1 - t0) * 1e3)
            res[f"pcs_{kind}_k{k}"] = {"ms": med(ms), "iters": out["iters"], "converged": out["converged"],
                                       "max_resid": float(out["resid"].max()),
                                       "ms_per_iter": round(statistics.median(ms) / out["iters"], 4),
                                       "values_over_trace": [float(v) for v in out["values"] / out["trace"]]}
            if kind == "reference":
                pc1 = out["vectors"][:, 0].copy()
        res["session_stats"] = list(s.stats())

    # ---- the kernels on their own, and the host path on the same K ------------------------------------------------
    lib = gbm.load_library()
    st = HipShardStages(n, p, nrhs=1, lambda_=1.0, device=0)
    st.generate(a.seed, 0)
    st.standardize()
    st.grm_syrk()
    st.grm_reduce()
    torch.cuda.synchronize()
    q = int(st.q.item())
    npad = st.npad
    pv = lambda t: ctypes.c_void_p(t.data_ptr())
    K = torch.zeros((npad, npad), dtype=torch.float64, device=st.dev)
    Q = torch.zeros((32, npad), dtype=torch.float64, device=st.dev)
    Q[:, :n] = torch.from_numpy(np.random.default_rng(a.seed).standard_normal((32, n))).to(st.dev)
    Y = torch.empty_like(Q)
    wsb = lib.gbm_dev_rows_times_sym_workspace(n, 32)
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=st.dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # µs

    def fill():
        _lib.check(lib.gbm_dev_grm_symmetrize(pv(st.G), st.gdim, n, 1.0 / q, pv(K), npad, st._stream()),
                   "gbm_dev_grm_symmetrize")

    def product():
        _lib.check(lib.gbm_dev_rows_times_sym(pv(K), npad, n, pv(Q), npad, 32, pv(Y), npad, pv(ws), wsb, st._stream()),
                   "gbm_dev_rows_times_sym")

    fills = [timed(fill) for _ in range(a.warmup + a.reps)][a.warmup:]
    prods = [timed(product) for _ in range(5 + a.product_reps)][5:]
    err = float((Y - Q @ K).abs().max() / (Q @ K).abs().max())
    bound_us = npad * npad * 8 / (HBM_STREAM_TBS * 1e12) * 1e6
    res.update({"symmetrize_us": med(fills), "product_us": med(prods), "product_byte_bound_us": round(bound_us, 1),
                "product_fraction_of_byte_bound": round(bound_us / statistics.median(prods), 3),
                "product_splits_partial_mb": round(wsb / 1e6, 1), "product_max_rel_diff_vs_torch": err})

    if not a.no_host:
        t0 = time.perf_counter()
        Kh = K[:n, :n].cpu().numpy()
        t1 = time.perf_counter()
        v = pc1_of_grm(Kh)
        t2 = time.perf_counter()
        res.update({"host_download_ms": round((t1 - t0) * 1e3, 1), "host_pc1_of_grm_ms": round((t2 - t1) * 1e3, 1),
                    "host_path_ms": round((t2 - t0) * 1e3, 1),
                    "abs_cos_device_vs_host_pc1": abs(float(pc1 @ v)) / float(np.linalg.norm(v))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
