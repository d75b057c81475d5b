#!/usr/bin/env python
"""Timing of the mixed-model GWAS scan (GenotypeSession.gwas) on synthetic genotypes, by default at the C2
shape (n = 5 000 x p = 50 000), with its split into solve, whitening and statistics.

How it measures: everything runs `--warmup` times first (the first scan also builds and caches the GRM), then
`--reps` times; each figure is the median with its range (min-max). The whole scan is host wall-clock around
the (synchronous) session call. The solve and the whitening are timed with device events on the same kernels
driven through the stream-ordered C ABI (HipShardStages: gbm_dev_gblup_solve, then gbm_dev_whiten_rows on
copies of the standardised rows in the session's default chunks; the chunk copies are timed on their own). The
statistics pass is timed as the OLS scan, which runs the same statistics kernel once over all rows without solve
or whitening (it includes the result download); `rest_ms` is what is left of the whole scan after solve, chunk
copies and whitening. As a yardstick, torch.linalg.solve_triangular (rocBLAS trsm) solves X·U = R on the same
factor U (assembled dense from the factored blocks) and the same chunks; the largest relative difference between
the two results is reported. The whitening rate is n²p / t against the 78.6 TF/s fp64 matrix peak of one MI355X.

Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomicbreedingmodels.jl_amd"))

import numpy as np  # noqa: E402

PEAK_FP64_TFLOPS = 78.6


def med(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--p", type=int, default=50000)
    ap.add_argument("--kc", type=int, default=0, help="extra covariates beside the intercept (0-7)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--chunk", type=int, default=0, help="loci per chunk (default: the session's own choice)")
    ap.add_argument("--no-trsm", action="store_true", help="skip the rocBLAS yardstick")
    a = ap.parse_args()

    import torch

    import gbm
    from gbm import _lib
    from gbm.sharded import HipShardStages

    n, p, lam = a.n, a.p, 1.0
    rng = np.random.default_rng(a.seed)
    y = rng.standard_normal(n)
    C = rng.standard_normal((n, a.kc)) if a.kc else None
    idx = np.arange(n)
    if a.chunk:
        _lib.debug_set("GBM_GWAS_CHUNK", min(p, a.chunk))

    # ---- the whole scan through the session ---------------------------------------------------------------
    scan, ols = [], []
    with gbm.GenotypeSession.synthetic(a.seed, n, p) as s:
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            out = s.gwas(idx, y, covariates=C, model="mlm", sigma2=(lam, 1.0))
            t1 = time.perf_counter()
            s.gwas(idx, y, covariates=C, model="ols")
            t2 = time.perf_counter()
            if r >= a.warmup:
                scan.append((t1 - t0) * 1e3)
                ols.append((t2 - t1) * 1e3)
        tested = out["tested"]

    # ---- the pieces on the same kernels -----------------------------------------------------------------------
    lib = gbm.load_library()
    st = HipShardStages(n, p, nrhs=a.kc + 1, lambda_=lam, device=0)
    st.generate(a.seed, 0)
    st.Y.zero_()
    st.Y[a.kc, :n].copy_(torch.from_numpy(y))
    if a.kc:
        st.Y[:a.kc, :n].copy_(torch.from_numpy(np.ascontiguousarray(C.T)))
    st.standardize()
    st.grm_syrk()
    st.grm_reduce()
    torch.cuda.synchronize()
    G0 = st.G[: st.npad].clone()
    npad = st.npad
    # the session's default chunk (csrc/session_gwas.cpp gwas_chunk): one 64-row strip per compute unit, balanced
    ncu = torch.cuda.get_device_properties(st.dev).multi_processor_count
    strips = (p + 63) // 64
    cap = max(1, (768 << 20) // (npad * 8 * 64))
    if cap >= ncu:
        cap = cap // ncu * ncu
    nchunks = (strips + cap - 1) // cap
    chunk = min(p, (strips + nchunks - 1) // nchunks * 64)
    if a.chunk:
        chunk = min(p, a.chunk)
    W = torch.empty((chunk, npad), dtype=torch.float64, device=st.dev)
    pv = lambda t: ctypes.c_void_p(t.data_ptr())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def whiten(rows):
        _lib.check(lib.gbm_dev_whiten_rows(pv(st.G), st.gdim, n, pv(st.ws_solve), pv(W), npad, rows, st._stream()),
                   "gbm_dev_whiten_rows")

    solve, wh, cp, trsm = [], [], [], []
    U = None
    maxdiff = 0.0
    for r in range(a.warmup + a.reps):
        st.G[:npad].copy_(G0)
        torch.cuda.synchronize()
        t_solve = timed(st.solve)
        assert int(st.info.item()) == 0
        if U is None and not a.no_trsm:
            # the dense factor: off-diagonal blocks from G's upper part, diagonal blocks from the workspace (Ld)
            U = torch.triu(st.G[:npad, :npad]).clone()
            Ld = st.ws_solve[: npad * 64 * 8].view(torch.float64).view(npad // 64, 64, 64)
            for k in range(npad // 64):
                U[k * 64:(k + 1) * 64, k * 64:(k + 1) * 64] = Ld[k]
        t_wh = t_cp = t_tr = 0.0
        for j0 in range(0, p, chunk):
            rows = min(chunk, p - j0)
            t_cp += timed(lambda: W[:rows].copy_(st.Z[j0:j0 + rows]))
            t_wh += timed(lambda: whiten(rows))
            if U is not None:
                ref = [None]

                def tr():
                    ref[0] = torch.linalg.solve_triangular(U, st.Z[j0:j0 + rows], upper=True, left=False)
                t_tr += timed(tr)
                if r == 0:
                    maxdiff = max(maxdiff, float((W[:rows] - ref[0]).abs().max() / ref[0].abs().max()))
                del ref
        if r >= a.warmup:
            solve.append(t_solve)
            wh.append(t_wh)
            cp.append(t_cp)
            if U is not None:
                trsm.append(t_tr)

    flops = float(n) * float(n) * float(p)
    res = {
        "tool": "gwas_bench", "n": n, "p": p, "kc": a.kc, "reps": a.reps, "warmup": a.warmup, "tested": tested,
        "chunk_loci": chunk, "scan_ms": med(scan), "solve_ms": med(solve), "chunk_copy_ms": med(cp),
        "whiten_ms": med(wh), "stats_pass_ms_ols_scan": med(ols),
        "rest_ms": round(statistics.median(scan) - statistics.median(solve) - statistics.median(cp)
                         - statistics.median(wh), 3),
        "whiten_tflops": round(flops / (statistics.median(wh) * 1e-3) / 1e12, 2),
        "whiten_fraction_of_fp64_peak": round(flops / (statistics.median(wh) * 1e-3) / 1e12 / PEAK_FP64_TFLOPS, 3),
    }
    if trsm:
        res["rocblas_trsm_ms"] = med(trsm)
        res["whiten_over_trsm_time"] = round(statistics.median(wh) / statistics.median(trsm), 3)
        res["max_rel_diff_vs_trsm"] = maxdiff
    print(json.dumps(res))


if __name__ == "__main__":
    main()
