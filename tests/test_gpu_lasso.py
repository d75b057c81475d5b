"""Lasso / elastic-net path on the device (gbm_session_enet_path, csrc/enet.hip) against the numpy
restatement of the same schedule (tests/lasso_ref.py) and R-glmnet known answers. tests/test_lasso.py asserts,
on the restatement alone, the conditions these cases rest on (active-list sizes, screening margins, the early
stop firing)."""
import numpy as np
import pytest

import gbm
import lasso_ref
from test_lasso import NL, RATIO, early_stop_case, r_cases, synth

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_r_glmnet_cases_one_lambda_each():
    """One-block active sets: R's answers to the 5e-6 of test_lasso.py, the loop at tol = 1e-14 to 1e-9."""
    worst_r, worst_l, m = 0.0, 0.0, 0
    for X, y, alpha, lam, ref in r_cases():
        n = X.shape[0]
        with gbm.GenotypeSession(X) as s:
            r = s.enet_path(np.arange(n), y, [lam], alpha=alpha, tol=1e-14, early_stop=False)
        lp = lasso_ref.enet_path(X, y, [lam], alpha=alpha, tol=1e-14)
        b, bl = r["b_path"][:, 0], lp["b_path"][:, 0]
        worst_r = max(worst_r, np.abs(b[1:] - ref).max())
        worst_l = max(worst_l, np.abs(b[1:] - bl[1:]).max() / max(1.0, np.abs(bl[1:]).max()))
        assert r["warning"] is None and r["nl_done"] == 1
        assert abs(b[0] - bl[0]) < 1e-9
        assert r["nnz"][0] == lp["nnz"][0]
        m += 1
    print(f"worst vs R {worst_r:.3e}, vs loop {worst_l:.3e}")
    assert m == 54
    assert worst_r < 5e-6
    assert worst_l <= 1e-9


@pytest.mark.parametrize("name,alpha", [("p>n", 1.0), ("p>n", 0.5), ("n>p", 1.0), ("n>p", 0.5)])
def test_synthetic_paths_two_certificates(name, alpha):
    """25 λ down to 0.03 λ_max at tol = 1e-16, early stop off: (1) coefficients against the loop within 10 x
    the loop's own convergence error max|B(tol) − B(tol/100)| (the factor is the margin for the device
    stopping one pass earlier or later); (2) the KKT residual of the device's b, recomputed here in fp64,
    within 10 x the loop's residual at the same tol. CPU measurements: convergence errors 8.1e-7 / 2.2e-7
    relative at (150, 600) for alpha = 1 / 0.5 and 2.9e-9 / 3.6e-9 at (1100, 300); KKT residuals 4.9e-7 /
    2.2e-7 and 7.3e-8 / 5.2e-8."""
    X, y = synth(name)
    n = X.shape[0]
    lam = lasso_ref.lambda_path(X, y, alpha, NL, RATIO)
    tol = 1e-16
    with gbm.GenotypeSession(X) as s:
        r = s.enet_path(np.arange(n), y, lam, alpha=alpha, tol=tol, early_stop=False)
    lp = lasso_ref.enet_path(X, y, lam, alpha=alpha, tol=tol)
    lp2 = lasso_ref.enet_path(X, y, lam, alpha=alpha, tol=tol / 100)
    assert r["warning"] is None and r["nl_done"] == NL
    B, Bl, Bl2 = r["b_path"][1:], lp["b_path"][1:], lp2["b_path"][1:]
    conv = np.abs(Bl - Bl2).max()
    err = np.abs(B - Bl).max()
    kkt_dev = max(lasso_ref.kkt_residual(X, y, lam[k], alpha, B[:, k]) for k in range(NL))
    kkt_loop = max(lasso_ref.kkt_residual(X, y, lam[k], alpha, Bl[:, k]) for k in range(NL))
    scale = np.abs(Bl2).max()
    print(f"{name} alpha={alpha}: |B - loop| = {err / scale:.3e} rel, loop convergence error = {conv / scale:.3e} rel, "
          f"KKT device = {kkt_dev:.3e}, KKT loop = {kkt_loop:.3e}, passes device/loop = {r['passes'].sum()}/"
          f"{lp['passes'].sum()}, nnz = {r['nnz'][-1]}")
    assert err <= 10 * conv
    assert kkt_dev <= 10 * kkt_loop
    assert rel(r["b_path"][0], lp["b_path"][0]) <= 10 * conv / scale + 1e-12
    assert np.abs(r["dev_ratio"] - lp["dev_ratio"]).max() < 1e-6


@pytest.mark.parametrize("seed,n,p,k", [(71, 300, 96, 64), (71, 300, 96, 65), (63, 256, 100, 10), (64, 257, 100, 10)])
def test_edge_shapes_planted_support(seed, n, p, k):
    """An active list of exactly one full block and of one block plus one marker; exactly one chunk workgroup
    of individuals and one chunk plus one individual. tol = 1e-14: a converged fit, compared to the loop at
    1e-9 relative (the bound of the R cases, which are converged fits too)."""
    X, y, S = lasso_ref.planted(seed, n, p, k)
    Xc = X - X.mean(axis=0)
    lmax = np.abs(Xc.T @ (y - y.mean())).max() / n
    lam = lmax * np.array([1.5, 0.1])
    lp = lasso_ref.enet_path(X, y, lam, alpha=1.0, tol=1e-14)
    assert lp["nactive"][-1] == k and lp["margin"] > 1e-9  # the stated count, on the loop
    assert np.array_equal(np.flatnonzero(lp["b_path"][1:, -1]), S)
    with gbm.GenotypeSession(X) as s:
        r = s.enet_path(np.arange(n), y, lam, alpha=1.0, tol=1e-14, early_stop=False)
    assert np.array_equal(np.flatnonzero(r["b_path"][1:, -1]), S)
    assert list(r["nnz"]) == [0, k]
    # a λ above λ_max: all-zero slopes, a0 = ȳ, no pass
    assert not r["b_path"][1:, 0].any() and abs(r["b_path"][0, 0] - y.mean()) < 1e-12 * abs(y.mean())
    assert r["passes"][0] == 0 and abs(r["dev_ratio"][0]) < 1e-12
    assert rel(r["b_path"][:, 1], lp["b_path"][:, 1]) <= 1e-9
    assert abs(r["dev_ratio"][1] - lp["dev_ratio"][1]) < 1e-9


def test_zero_variance_column_stays_zero():
    """A constant column carries the largest raw |xᵀy| of its neighbours (its centred column is 0): never
    admitted, b = 0 (glmnet's ju = 0)."""
    X, y, S = lasso_ref.planted(63, 256, 100, 10)
    j = int(S[3]) + 1 if int(S[3]) + 1 not in S else int(S[3]) - 1
    X = X.copy()
    X[:, j] = 1.0
    assert np.abs(X[:, j] @ y) > np.abs(X[:, [j - 1, j + 1]].T @ y).max()
    Xc = X - X.mean(axis=0)
    lam = np.abs(Xc.T @ (y - y.mean())).max() / 256 * np.array([1.0, 0.1, 0.001])
    lp = lasso_ref.enet_path(X, y, lam, alpha=0.5, tol=1e-14)
    with gbm.GenotypeSession(X) as s:
        r = s.enet_path(np.arange(256), y, lam, alpha=0.5, tol=1e-14, early_stop=False)
    assert (r["b_path"][1 + j] == 0.0).all()
    assert list(r["nnz"]) == list(lp["nnz"]) and r["nnz"][-1] == 10  # the planted support, the constant column out
    assert rel(r["b_path"], lp["b_path"]) <= 1e-9


def test_early_stop_matches_loop():
    X, y = early_stop_case()
    lam = lasso_ref.lambda_path(X, y, 1.0, 100, 1e-4)
    lp = lasso_ref.enet_path(X, y, lam, alpha=1.0, tol=1e-12, dev_max=0.999, fdev=1e-5)
    assert 5 <= lp["nl_done"] < 100
    with gbm.GenotypeSession(X) as s:
        r = s.enet_path(np.arange(40), y, lam, alpha=1.0, tol=1e-12)
        full = s.enet_path(np.arange(40), y, lam[:lp["nl_done"] + 3], alpha=1.0, tol=1e-12, early_stop=False)
    assert r["nl_done"] == lp["nl_done"]
    assert np.array_equal(r["lambdas"], lp["lambdas"])
    assert np.abs(r["dev_ratio"] - lp["dev_ratio"]).max() < 1e-9
    assert r["b_path"].shape == (121, lp["nl_done"])
    assert full["nl_done"] == lp["nl_done"] + 3  # the rule off: every λ is solved
    assert np.array_equal(full["b_path"][:, :r["nl_done"]], r["b_path"])


def test_idx_eval_predictions_and_subset_rows():
    X, y = synth("p>n")
    tr, ho = np.arange(0, 150, 2), np.arange(1, 150, 2)
    lam = lasso_ref.lambda_path(X[tr], y[tr], 1.0, 6, 0.2)
    with gbm.GenotypeSession(X) as s:
        r = s.enet_path(tr, y[tr], lam, tol=1e-12, idx_eval=ho, early_stop=False)
    lp = lasso_ref.enet_path(X[tr], y[tr], lam, tol=1e-12)
    want = r["b_path"][0][None, :] + X[ho] @ r["b_path"][1:]
    assert rel(r["pred"], want) < 1e-12
    assert rel(r["b_path"], lp["b_path"]) < 1e-8


def test_argument_refusals():
    X, y = synth("p>n")
    idx = np.arange(150)
    with gbm.GenotypeSession(X) as s:
        for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")), dict(tol=0.0), dict(max_passes=0)):
            with pytest.raises(gbm.ArgumentError):
                s.enet_path(idx, y, [0.1], **kw)
        for lam in ([0.1, 0.2], [0.1, 0.0], [float("inf")], [-1.0]):
            with pytest.raises(gbm.ArgumentError):
                s.enet_path(idx, y, lam)
        with pytest.raises(gbm.ArgumentError):
            s.enet_path(np.array([3, 2, 1]), y[:3], [0.1])
        with pytest.raises(gbm.ArgumentError):
            s.enet_path(idx, y, [0.1], idx_eval=[150])
        with pytest.raises(gbm.GBMError):
            s.enet_path(idx, np.ones(150), [0.1])
        # max_passes reached: GBM_OK with a warning (the BRR fallback convention)
        lam = lasso_ref.lambda_path(X, y, 1.0, 3, 0.1)
        r = s.enet_path(idx, y, lam, tol=1e-16, max_passes=2, early_stop=False)
        assert r["warning"] is not None and r["warning"].startswith("warning:") and r["passes"].max() == 2
        assert s.enet_path(idx, y, lam, tol=1e-7, early_stop=False)["warning"] is None
    # the active set is capped at min(p, 2 npad) packed rows: alpha small and λ tiny on n = 20 needs more
    Xw = synth("n>p")[0][:20]
    yw = synth("n>p")[1][:20]
    with gbm.GenotypeSession(Xw) as s:
        lmax = s.ridge_lambda_max(np.arange(20), yw) * 1e-3 / 0.01
        with pytest.raises(gbm.ArgumentError, match="cap"):
            s.enet_path(np.arange(20), yw, [lmax * 1e-3], alpha=0.01, early_stop=False)


def test_two_runs_bit_identical_and_ridge_cache_hit():
    X, y = synth("n>p")
    idx = np.arange(1100)
    lam = lasso_ref.lambda_path(X, y, 0.5, 8, 0.1)
    with gbm.GenotypeSession(X) as s:
        rl = s.ridge_lambda_max(idx, y)
        ridge0 = s.ridge_path(idx, y, [rl * 0.01])
        assert s.stats() == (1, 1)
        a = s.enet_path(idx, y, lam, alpha=0.5, tol=1e-10, early_stop=False)
        assert s.stats() == (1, 2)  # the lasso path on the same rows: a cache hit
        b = s.enet_path(idx, y, lam, alpha=0.5, tol=1e-10, early_stop=False)
        ridge1 = s.ridge_path(idx, y, [rl * 0.01])
        assert s.stats() == (1, 4)
    for key in ("b_path", "dev_ratio", "passes", "nnz"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(ridge0, ridge1)  # the cached Z and kernel are not written by the lasso path
    with gbm.GenotypeSession(X) as s:  # and on a fresh session: the same bits again
        c = s.enet_path(idx, y, lam, alpha=0.5, tol=1e-10, early_stop=False)
    assert np.array_equal(a["b_path"], c["b_path"])


def test_enet_path_cv_matches_loop():
    """20 λ down to 0.1 λ_max at tol = 1e-10 on both sides, the same folds. The bound is 10 x the loop's own
    convergence error |cv(tol) − cv(tol/100)|, as in test_synthetic_paths_two_certificates."""
    X, y = synth("p>n")
    folds = gbm.glmnet_folds(150, 10, np.random.default_rng(5))
    kw = dict(nlambda=20, lambda_min_ratio=0.1)
    ref = lasso_ref.enet_path_cv(X, y, folds, tol=1e-10, **kw)
    ref2 = lasso_ref.enet_path_cv(X, y, folds, tol=1e-12, **kw)
    got = gbm.enet_path_cv(X, y, alpha=1.0, seed=5, tol=1e-10, **kw)
    assert got["lambda"].size == ref["lambda"].size and rel(got["lambda"], ref["lambda"]) < 1e-12
    conv_b = np.abs(ref["betas"] - ref2["betas"]).max()
    conv_a = np.abs(ref["a0"] - ref2["a0"]).max()
    conv_l = np.abs(ref["meanloss"] - ref2["meanloss"]).max()
    print(f"betas: {np.abs(got['betas'] - ref['betas']).max():.3e} (loop convergence {conv_b:.3e}); meanloss: "
          f"{np.abs(got['meanloss'] - ref['meanloss']).max():.3e} (loop convergence {conv_l:.3e})")
    assert np.abs(got["betas"] - ref["betas"]).max() <= 10 * conv_b
    assert np.abs(got["a0"] - ref["a0"]).max() <= 10 * conv_a
    assert np.abs(got["meanloss"] - ref["meanloss"]).max() <= 10 * conv_l


def test_lasso_model_function():
    """reference lasso's defaults (100 λ, tol = 1e-7) against the loop with the same folds and the same
    selection. At 1e-7 a pass more or less moves the coefficients: the bound is 10 x the loop's own convergence
    error over the whole full-data path, max|B(tol) − B(tol/100)|."""
    X, y = synth("p>n")
    ent = [f"e{i}" for i in range(150)]
    g = gbm.Genomes(ent, ["p"] * 150, [f"l{j}" for j in range(600)], X)
    ph = gbm.Phenomes(ent, ["p"] * 150, ["t"], y[:, None])
    fit = gbm.lasso(genomes=g, phenomes=ph, seed=5)
    assert fit.model == "lasso" and fit.checkdims()
    folds = gbm.glmnet_folds(150, 10, np.random.default_rng(5))
    ref = lasso_ref.enet_path_cv(X, y, folds)
    b_ref = gbm.lasso_select(ref["a0"], ref["betas"], ref["meanloss"])
    fine = lasso_ref.enet_path(X, y, ref["lambda"], tol=1e-9)["b_path"]
    conv = np.abs(fine - np.vstack([ref["a0"], ref["betas"]])).max()
    print(f"|b_hat - loop| = {np.abs(fit.b_hat - b_ref).max():.3e}, loop convergence error {conv:.3e}")
    assert np.abs(fit.b_hat - b_ref).max() <= 10 * conv
    assert fit.metrics["cor"] > 0.5  # the reference doctest (src/linear.jl:298)
