"""Seconds of one full lasso path fit (gbm_session_enet_path: 100 λ down to 0.01 λ_max, tol = 1e-7, glmnet's
early stop) on device-generated sessions at C1 (200 x 1000) and C4 (10 000 x 100 000), and where they go.

    python tools/lasso_bench.py                    # wall times: training-set preparation, λ_max, the path
    python tools/lasso_bench.py --profile          # the same fit once more under rocprofv3 --kernel-trace --stats

--profile starts a child process of this tool under rocprofv3 (a run of its own) and sums its kernel trace into
the split of the path call: passes (enet_chain_kernel, enet_dots0_kernel, enet_reduce_kernel), screens
(marker_effects_kernel and its weighted sum), gathers plus Grams (enet_gather / gram / prep / x2), and what is
left of the call's wall time: the host synchronisations (one per pass, one per screen, one per λ) and launch
gaps. It also gives µs per enet_chain_kernel launch. Prints one JSON line per measurement."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomicbreedingmodels.jl_amd"))

SHAPES = {"C1": (200, 1000), "C4": (10000, 100000)}
GROUPS = {"passes": ("enet_chain_kernel", "enet_dots0_kernel", "enet_reduce_kernel"),
          "screens": ("marker_effects_kernel", "weighted_sum"),
          "gathers_grams": ("enet_gather_kernel", "enet_gram_kernel", "enet_prep_kernel", "enet_x2_kernel")}


def fit(name, alpha, tol):
    import gbm
    from gbm import synth as S
    n, p = SHAPES[name]
    y = S.qtl_phenotypes(4242, n, p, ntraits=1)[:, 0]
    idx = np.arange(n)
    row = {"bench": "lasso path", "config": name, "n": n, "p": p, "alpha": alpha, "tol": tol}
    with gbm.GenotypeSession.synthetic(4242, n, p) as s:
        t0 = time.perf_counter()
        s.ridge_path(idx, y, [1e6])  # centres the training rows and builds their kernel (which the lasso does not read)
        row["seconds_training_set_and_one_ridge_solve"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        lmax = s.ridge_lambda_max(idx, y) * 1e-3 / max(alpha, 1e-3)
        row["seconds_lambda_max"] = time.perf_counter() - t0
        lam = lmax * 0.01 ** (np.arange(100) / 99)
        s.enet_path(idx, y, lam[:2], alpha=alpha, tol=tol)  # warm-up: the session's buffers
        t0 = time.perf_counter()
        r = s.enet_path(idx, y, lam, alpha=alpha, tol=tol)
        row["seconds_path"] = time.perf_counter() - t0
    row.update({"nl_done": r["nl_done"], "passes": int(r["passes"].sum()), "nnz_last": int(r["nnz"][-1]),
                "dev_ratio_last": float(r["dev_ratio"][-1]), "warning": r["warning"]})
    return row


def kernel_totals(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    tot = {}
    for r in csv.DictReader(open(files[0])):
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        c = tot.setdefault(r["Kernel_Name"], [0, 0])
        c[0] += 1
        c[1] += ns
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C4")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--tol", type=float, default=1e-7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(fit(args.child, args.alpha, args.tol)), flush=True)
        return
    for name in args.configs.split(","):
        if not args.profile:
            print(json.dumps(fit(name, args.alpha, args.tol)), flush=True)
            continue
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, "--alpha", str(args.alpha), "--tol",
                   str(args.tol)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                sys.exit(f"rocprofv3 run failed ({out.returncode}):\n{out.stderr[-2000:]}")
            row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
            tot = kernel_totals(d)
        row["bench"] = "lasso path (under rocprofv3)"
        split = {}
        for g, names in GROUPS.items():
            split[g] = sum(ns for k, (c, ns) in tot.items() if any(nm in k for nm in names)) * 1e-9
        # the warm-up call and λ_max run the same kernels: a small share (2 of 100 λ, one screen)
        row["kernel_seconds"] = split
        row["kernels"] = {re.search(r"(enet_\w+|marker_effects_kernel)", k).group(1): {"calls": c, "us_per_call": ns / c * 1e-3}
                          for k, (c, ns) in sorted(tot.items()) if re.search(r"enet_\w+|marker_effects_kernel", k)}
        row["seconds_path_outside_kernels"] = row["seconds_path"] - sum(split.values())
        chain = [(c, ns) for k, (c, ns) in tot.items() if "enet_chain_kernel" in k]
        if chain:
            row["chain_launches"] = chain[0][0]
            row["us_per_chain_launch"] = chain[0][1] / chain[0][0] * 1e-3
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
