"""Digest of everything a session's entries return along one sequence of training sets, for builds compared side by
side (GBM_LIBGBM=...): one sha-256 per entry and session kind. The sequence is the one tests/test_gpu_session_reuse.py
checks against fresh sessions (it imports STEPS, open_session and run_step from here): one session on n = 300,
p = 700 goes through all 300 entries (npad 384), 257 (the same pitch), 120 (npad 128) and all 300 again, with 1, 3, 1
and 3 traits, first on host genotypes with the fp64 GRM, then on a synthetic session with grm_mode exact."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomicbreedingmodels.jl_amd"))
import numpy as np  # noqa: E402

N, P = 300, 700
KINDS = ("host-fp64", "synthetic-exact")
GWAS_CHUNK = 64  # GBM_GWAS_CHUNK of the sequence: 11 chunks of the 700 loci
_rng = np.random.default_rng(20261021)
X = _rng.integers(0, 3, size=(N, P)) / 2.0  # dosages / 2
YALL = X[:, ::9] @ _rng.standard_normal((X[:, ::9].shape[1], 3)) + 2.0 * _rng.standard_normal((N, 3))
COV = _rng.standard_normal((N, 2))
LOCI = np.arange(0, P, 5)[:130]
# (training entries, traits)
STEPS = (
    (np.arange(N), 1),
    (np.sort(_rng.choice(N, 257, replace=False)), 3),
    (np.sort(_rng.choice(N, 120, replace=False)), 1),
    (np.arange(N), 3),
)


def open_session(kind):
    from gbm.session import GenotypeSession
    if kind == "host-fp64":
        return GenotypeSession(X).set_grm("fp64")
    return GenotypeSession.synthetic(4242, N, P).set_grm("exact")


def run_step(s, idx, ntraits):
    """Every entry once on the training set idx: {entry: [arrays]} (GBM_GWAS_CHUNK = GWAS_CHUNK is the caller's)."""
    Y, y, ev = YALL[idx, :ntraits], YALL[idx, 0], np.arange(1, N, 7)
    out = {}
    b, yp, mu, q = s.gblup(idx, Y, 0.7)
    out["gblup_fit"] = [b, yp, mu, np.int64(q)]
    out["predict"] = [s.predict(ev, b)]
    r = s.reml(idx, y)
    out["reml"] = [np.array([r["lambda"], r["sigma2_e"], r["sigma2_u"], r["objective"]])]
    out["reml_objective"] = [s.reml_objective(idx, y, [0.5, 0.2], [0.5, 0.9])]
    lmax = s.ridge_lambda_max(idx, y)
    out["ridge_lambda_max"] = [np.float64(lmax)]
    out["ridge_path"] = list(s.ridge_path(idx, y, lmax * np.array([1e-2, 1e-3, 1e-4]), idx_eval=ev))
    alpha = 0.9
    e = s.enet_path(idx, y, lmax * 1e-3 / alpha * np.array([0.6, 0.3, 0.15]), alpha=alpha, idx_eval=ev)
    assert e["warning"] is None, e["warning"]
    out["enet_path"] = [e[k] for k in ("b_path", "dev_ratio", "passes", "nnz", "pred")]
    g = s.gwas(idx, y, covariates=COV[idx], model="mlm")
    out["gwas_mlm"] = [g["z"], g["b"], np.array([g["sigma2_e"], g["sigma2_u"]]), np.int64(g["tested"])]
    g = s.gwas(idx, y, model="ols")
    out["gwas_ols"] = [g["z"], g["b"], np.int64(g["tested"])]
    for kind, k in (("grm", 3), ("reference", 2)):
        c = s.pcs(idx, k, kind=kind)
        assert c["converged"]
        out["pcs_" + kind] = [c["vectors"], c["values"], np.float64(c["trace"]), c["resid"], np.int64(c["iters"])]
    for op in ("mult", "square"):  # binary: three panels of 64, 64 and 2 i-rows; unary: one row
        c = s.pair_scan(idx, y, op, loci=LOCI, k=50, panel_rows=64)
        out["pair_scan_" + op] = [c["index"], c["beta"], np.int64(c["tested"]), np.int64(c["degenerate"])]
    return out


def main():
    from gbm import _lib
    lib = os.path.basename(os.environ.get("GBM_LIBGBM", "libgbm.so"))
    _lib.debug_set("GBM_GWAS_CHUNK", str(GWAS_CHUNK))
    for kind in KINDS:
        h = {}
        with open_session(kind) as s:
            for idx, ntraits in STEPS:
                for entry, arrays in run_step(s, idx, ntraits).items():
                    for a in arrays:
                        h.setdefault(entry, hashlib.sha256()).update(np.ascontiguousarray(a).tobytes())
        for entry, d in h.items():
            print(f"{lib} {kind} {entry} {d.hexdigest()[:16]}", flush=True)


if __name__ == "__main__":
    main()
