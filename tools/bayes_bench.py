"""ms per Gibbs iteration of BayesA, BayesB and BayesC (gbm_bayes_fit: one chain launch per
64-marker block) at the C4 shape (n = 10 000, p = 100 000), with byte and with fp64 genotype
storage, beside BRR's per-launch path (GBM_BRR_SWEEP=0) on the same box in the same run. The
per-iteration cost is constant, so two fits of different lengths separate it from the setup
(upload, column statistics, Gram blocks). ``--response ordinal`` times gbm_bayes_fit_ordinal instead, on the
same phenotype cut into K = 4 classes at its quartiles (``--response gaussian,ordinal``: both in one run,
the ratio of the two slopes is the ordinal steps' overhead). Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomicbreedingmodels.jl_amd"))


def per_iteration(fit, lo, hi):
    """(ms per iteration, seconds of the short fit, seconds of the long fit, last result)."""
    sec = {}
    for iters in (lo, hi):
        t0 = time.perf_counter()
        out = fit(iters)
        sec[iters] = time.perf_counter() - t0
    return (sec[hi] - sec[lo]) / (hi - lo) * 1e3, sec[lo], sec[hi], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--p", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=150, help="iterations of the long fit (the short one runs a fifth)")
    ap.add_argument("--models", default="BRR,BayesA,BayesB,BayesC")
    ap.add_argument("--storages", default="bytes,fp64")
    ap.add_argument("--response", default="gaussian", help="gaussian, ordinal or both (comma-separated)")
    args = ap.parse_args()
    import gbm
    from gbm import _lib, synth as S
    X = S.genotypes(4242, args.n, args.p)
    y = S.qtl_phenotypes(4242, args.n, args.p, ntraits=1)[:, 0]
    lo, hi = max(2, args.iters // 5), args.iters
    cls = np.searchsorted(np.quantile(y, [0.25, 0.5, 0.75]), y).astype(np.float64)  # K = 4
    _lib.debug_set("GBM_BRR_SWEEP", "0")  # BRR: one launch per block, the schedule the chain launches compare with
    for storage in args.storages.split(","):
        _lib.debug_set("GBM_BRR_I8", None if storage == "bytes" else "0")
        for model, response in ((m, r) for m in args.models.split(",") for r in args.response.split(",")):
            if response == "ordinal":
                if model == "BRR":
                    continue  # no ordinal response
                fit = lambda it, m=model: gbm.bayes_ordinal_arrays(m, X, cls, n_iter=it, n_burnin=it // 2, thin=1)
            elif model == "BRR":
                fit = lambda it: gbm.brr_arrays(X, y, n_iter=it, n_burnin=it // 2, thin=1)
            else:
                fit = lambda it, m=model: gbm.bayes_arrays(m, X, y, n_iter=it, n_burnin=it // 2, thin=1)
            fit(2)  # warm-up: the pooled context's buffers
            ms, s_lo, s_hi, out = per_iteration(fit, lo, hi)
            launches = -(-args.p // (128 if model == "BRR" and storage == "bytes" else 64))
            row = {"bench": "Gibbs iteration", "model": model, "response": response, "storage": storage, "n": args.n, "p": args.p,
                   "iters": [lo, hi], "seconds": [s_lo, s_hi], "ms_per_iter": ms,
                   "block_launches_per_iter": launches, "us_per_block_launch": ms * 1e3 / launches,
                   "cor": float(np.corrcoef(out[1], y)[0, 1])}
            if model != "BRR":
                row["pi"] = float(out[2][2])
                row["mean_pip"] = float(out[3].mean())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
