"""ms per Gibbs iteration of BayesA, BayesB and BayesC (gbm_bayes_fit: one chain launch per
64-marker block) at the C4 shape (n = 10 000, p = 100 000), with byte and with fp64 genotype
storage, beside BRR's per-launch path (GBM_BRR_SWEEP=0) on the same box in the same run. The
per-iteration cost is constant, so two fits of different lengths separate it from the setup
(upload, column statistics, Gram blocks). ``--response ordinal`` times gbm_bayes_fit_ordinal instead, on the
same phenotype cut into K = 4 classes at its quartiles (``--response gaussian,ordinal``: both in one run,
the ratio of the two slopes is the ordinal steps' overhead). ``--chains 1,4,8,24,32`` times gbm_bayes_fit_multi
with that many chains instead (the models of ``--models`` in turn, one phenotype column and seed per chain) and
adds the ms per chain-iteration; ``--multi-wg 1`` / ``--multi-wg 4`` force one / four chains per workgroup row
(GBM_BAYES_MULTI_WG) for the comparison of the two mappings. ``--folds F`` times a cross-validation's F folds
(fold of individual i: i mod F) x the models of ``--models`` two ways: F gbm_bayes_fit_multi calls, one per fold on
its training rows, and one gbm_bayes_fit_multi_rows call over all rows with a training set per fold; it reports
the per-iteration slope and the setup (the short fit's time less its iterations) of each. ``--repeats R`` repeats
every measurement (the run-to-run spread). Prints one JSON line per measurement."""
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
    ap.add_argument("--chains", default="", help="chain counts of gbm_bayes_fit_multi (comma-separated); empty: none")
    ap.add_argument("--multi-wg", type=int, default=0, choices=(0, 1, 4),
                    help="chains per workgroup row of a multi fit (0: the library's choice)")
    ap.add_argument("--folds", type=int, default=0, help="folds of the cross-validation comparison; 0: none")
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    import gbm
    from gbm import _lib, synth as S
    X = S.genotypes(4242, args.n, args.p)
    chains = [int(t) for t in args.chains.split(",") if t]
    Y = S.qtl_phenotypes(4242, args.n, args.p, ntraits=max(chains + [1]))
    y = np.ascontiguousarray(Y[:, 0])
    lo, hi = max(2, args.iters // 5), args.iters
    cls = np.searchsorted(np.quantile(y, [0.25, 0.5, 0.75]), y).astype(np.float64)  # K = 4
    _lib.debug_set("GBM_BRR_SWEEP", "0")  # BRR: one launch per block, the schedule the chain launches compare with
    for storage in args.storages.split(","):
        _lib.debug_set("GBM_BRR_I8", None if storage == "bytes" else "0")
        if args.folds:
            fold_rows(gbm, _lib, args, X, y, storage, lo, hi)
            continue
        if chains:
            multi_rows(gbm, _lib, args, chains, X, Y, storage, lo, hi)
            continue
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
            for rep in range(args.repeats):
                ms, s_lo, s_hi, out = per_iteration(fit, lo, hi)
                launches = -(-args.p // (128 if model == "BRR" and storage == "bytes" else 64))
                row = {"bench": "Gibbs iteration", "model": model, "response": response, "storage": storage,
                       "n": args.n, "p": args.p, "iters": [lo, hi], "seconds": [s_lo, s_hi], "ms_per_iter": ms,
                       "block_launches_per_iter": launches, "us_per_block_launch": ms * 1e3 / launches,
                       "cor": float(np.corrcoef(out[1], y)[0, 1])}
                if model != "BRR":
                    row["pi"] = float(out[2][2])
                    row["mean_pip"] = float(out[3].mean())
                print(json.dumps(row), flush=True)


def multi_rows(gbm, _lib, args, chains, X, Y, storage, lo, hi):
    """gbm_bayes_fit_multi at every chain count: the slope per iteration and per chain-iteration."""
    names = [m for m in args.models.split(",") if m != "BRR"]
    _lib.debug_set("GBM_BAYES_MULTI_WG", str(args.multi_wg) if args.multi_wg else None)
    for T in chains:
        models = [names[c % len(names)] for c in range(T)]
        Yt = np.asfortranarray(Y[:, :T])
        fit = lambda it: gbm.bayes_multi_arrays(models, X, Yt, n_iter=it, n_burnin=it // 2, thin=1,
                                                seeds=[42 + c for c in range(T)])
        fit(2)  # warm-up: the pooled context's buffers
        for rep in range(args.repeats):
            ms, s_lo, s_hi, out = per_iteration(fit, lo, hi)
            launches = -(-args.p // 64)
            print(json.dumps({"bench": "Gibbs iteration, multi", "chains": T, "chains_per_workgroup": args.multi_wg,
                              "models": sorted(set(models)), "storage": storage, "n": args.n, "p": args.p,
                              "iters": [lo, hi], "seconds": [s_lo, s_hi], "ms_per_iter": ms,
                              "ms_per_chain_iter": ms / T, "block_launches_per_iter": launches,
                              "us_per_block_launch": ms * 1e3 / launches,
                              "cor": float(np.corrcoef(out[1][:, 0], Yt[:, 0])[0, 1])}), flush=True)


def fold_rows(gbm, _lib, args, X, y, storage, lo, hi):
    """F folds x the models: a gbm_bayes_fit_multi call per fold on its training rows against one
    gbm_bayes_fit_multi_rows call on all rows. The folds' predictions of the two paths are compared."""
    names = [m for m in args.models.split(",") if m != "BRR"]
    F, M = args.folds, len(names)
    fold = np.arange(args.n) % F
    seeds = [42 + c for c in range(M)]
    row = {"folds": F, "models": names, "storage": storage, "n": args.n, "p": args.p, "iters": [lo, hi]}

    def slope(fit):
        ms, s_lo, s_hi, out = per_iteration(fit, lo, hi)
        return {"seconds": [s_lo, s_hi], "ms_per_iter": ms, "setup_seconds": s_lo - ms * 1e-3 * lo,
                "ms_per_fold_model_iter": ms / (F * M)}, out

    # one multi call per fold on X[train] (gathering the rows is the caller's cost today and is timed apart)
    t0 = time.perf_counter()
    parts = [(np.asfortranarray(X[fold != f]), np.asfortranarray(np.tile(y[fold != f, None], (1, M)))) for f in range(F)]
    gather = time.perf_counter() - t0
    _lib.debug_set("GBM_BAYES_MULTI_WG", None)

    def per_fold(it):
        return [gbm.bayes_multi_arrays(names, Xf, Yf, n_iter=it, n_burnin=it // 2, thin=1, seeds=seeds)
                for Xf, Yf in parts]

    per_fold(2)  # warm-up: the pooled context's buffers
    held = None
    for rep in range(args.repeats):
        fig, outs = slope(per_fold)
        held = [outs[f][0] for f in range(F)]  # b_hat per fold
        print(json.dumps(dict(row, bench="CV folds, a multi fit per fold", calls=F, chains_per_call=M,
                              gather_seconds=gather, **fig)), flush=True)
    del parts
    sets = np.stack([fold != f for f in range(F)])
    set_of = [f for f in range(F) for _ in range(M)]
    Yr = np.asfortranarray(np.tile(y[:, None], (1, F * M)))
    for wg in ((1, 4) if not args.multi_wg else (args.multi_wg,)):
        _lib.debug_set("GBM_BAYES_MULTI_WG", str(wg))
        fit = lambda it: gbm.bayes_multi_rows_arrays(names * F, X, Yr, sets, set_of, n_iter=it, n_burnin=it // 2,
                                                     thin=1, seeds=seeds * F)
        fit(2)
        for rep in range(args.repeats):
            fig, out = slope(fit)
            worst = max(float(np.abs(out[0][:, f * M + m] - held[f][:, m]).max() / np.abs(held[f][:, m]).max())
                        for f in range(F) for m in range(M))
            cor = float(np.corrcoef(out[1][fold == 0, 0], y[fold == 0])[0, 1])
            print(json.dumps(dict(row, bench="CV folds, one rows fit", calls=1, chains_per_call=F * M,
                                  chains_per_workgroup=wg, b_hat_rel_diff_from_per_fold=worst,
                                  held_out_cor_fold0=cor, **fig)), flush=True)
    _lib.debug_set("GBM_BAYES_MULTI_WG", None)


if __name__ == "__main__":
    main()
