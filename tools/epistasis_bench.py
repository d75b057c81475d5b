"""Seconds of one epistasis pair scan (GenotypeSession.pair_scan / gbm_session_pair_scan, K = 1000) per binary
operation on device-generated sessions at n = 5000 entries and l = 2000 and l = 10 000 loci: 2 warm-up runs, then
the median of 5, with the pair-rows per second (l² pairs x n rows over that time; the call includes the gather,
the selection and the candidates' way back).

    python tools/epistasis_bench.py                       # both shapes, mult / addnorm / raise
    python tools/epistasis_bench.py --shapes 5000x2000    # one shape

ε = 1e-3 (the synthetic genotypes are dosages/2; src/transformation.jl's default ε on dosages puts product
features next to the rank boundary). Prints one JSON line per operation and shape."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomicbreedingmodels.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000x2000,5000x10000")
    ap.add_argument("--ops", default="mult,addnorm,raise")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import gbm
    from gbm import synth as S
    for shape in args.shapes.split(","):
        n, l = (int(v) for v in shape.split("x"))
        y = S.qtl_phenotypes(4242, n, l, ntraits=1)[:, 0]
        idx = np.arange(n)
        with gbm.GenotypeSession.synthetic(4242, n, l) as s:
            for op in args.ops.split(","):
                times = []
                for r in range(args.warmup + args.runs):
                    t0 = time.perf_counter()
                    res = s.pair_scan(idx, y, op, eps=1e-3, k=1000)
                    if r >= args.warmup:
                        times.append(time.perf_counter() - t0)
                med = statistics.median(times)
                print(json.dumps({"bench": "epistasis pair scan", "op": op, "n": n, "l": l, "k": 1000,
                                  "seconds_median": med, "seconds_min": min(times), "seconds_max": max(times),
                                  "pair_rows_per_second": l * l * n / med, "tested": res["tested"],
                                  "degenerate": res["degenerate"], "n_top": int(res["index"].size)}), flush=True)


if __name__ == "__main__":
    main()
