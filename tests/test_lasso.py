"""Lasso / elastic-net path of reference ``lasso`` (GLMNet alpha = 1; src/linear.jl:302-378), CPU side: the
numpy restatement of the device schedule (tests/lasso_ref.py) against R-glmnet known answers
(tests/golden/enet/glmnet_enet_r.npz), the selection quirks, the ABI export, and the conditions the GPU cases of
tests/test_gpu_lasso.py rest on, asserted on the restatement alone. glmnet divides the user λ by the
population sd of y in the L2 term, so the y-scaled cases pin that σ_y factor:
glmnet(X, c·y, c·λ) = c·glmnet(X, y, λ)."""
import os
import re
import subprocess

import numpy as np
import pytest

import gbm
import lasso_ref
import oracle
from gbm import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enet", "glmnet_enet_r.npz")
# the two synthetic shapes of the GPU tests: (seed of X, n, p, seed of y)
SHAPES = {"p>n": (43, 150, 600, 44), "n>p": (47, 1100, 300, 48)}
NL, RATIO = 25, 0.03


def r_cases():
    z = np.load(GOLD)
    data = z["data"]
    for c in z["cases"]:
        n, p, alpha, lam = int(c[0]), int(c[1]), float(c[2]), float(c[3])
        y = data[:n, 0] - data[:n, 0].mean()
        y /= y.std(ddof=1)
        X = data[:n, 1:p + 1] - data[:n, 1:p + 1].mean(axis=0)
        X /= X.std(axis=0, ddof=1)
        yield X, y, alpha, lam, c[4:4 + p]


def synth(name):
    sx, n, p, sy = SHAPES[name]
    X = oracle.synth_genotypes(sx, n, p)
    return X, oracle.synth_phenotypes(X, sy)[:, 0]


def test_loop_matches_r_glmnet():
    """R's own convergence (thresh 1e-7) and printed digits bound the agreement: 2.03e-6 worst measured for a
    converged coordinate descent, bounded at 5e-6."""
    m, worst = 0, 0.0
    for X, y, alpha, lam, ref in r_cases():
        for c in (1.0, 10.0, 0.1):  # σ_y ≠ 1: the same R answers, scaled
            r = lasso_ref.enet_path(X, c * y, [c * lam], alpha=alpha, tol=1e-14)
            err = np.abs(r["b_path"][1:, 0] / c - ref).max()
            worst = max(worst, err)
            assert err < 5e-6, (alpha, lam, c, r["b_path"][:, 0], ref)
            assert abs(r["b_path"][0, 0]) < 1e-12 * c
        m += 1
    print(f"worst |b - R| = {worst:.3e}")
    assert m == 54


def test_lasso_select_quirks():
    a0 = np.array([10.0, 20.0, 30.0, 40.0])
    betas = np.array([[0.0, 1.0, 2.0, 0.0], [0.0, 3.0, 5.0, 0.0]])
    loss = np.array([0.1, 0.3, 0.2, 0.4])  # sorted: 0, 2, 1, 3
    # λ #1 has zero slopes (variance < 1e-10): skipped; the next by loss is λ #3 (idx 2) with ITS intercept
    # a0[idx_sort][1] = a0[2] (src/linear.jl:354,358) — ridge's double permutation would give a0[1]
    assert np.array_equal(gbm.lasso_select(a0, betas, loss), [30.0, 2.0, 5.0])
    assert np.array_equal(gbm.ridge_select(a0, betas, loss), [20.0, 2.0, 5.0])
    # no last-λ clause: the best λ is taken when it has slope variance, even if it is the last on the path
    last = np.array([[0.0, 1.0, 2.0, 4.0], [0.0, 3.0, 5.0, 9.0]])
    assert np.array_equal(gbm.lasso_select(a0, last, np.array([0.4, 0.3, 0.2, 0.1])), [40.0, 4.0, 9.0])
    # equal slopes have no variance; a path without any slope variance is where the reference indexes past the end
    flat = np.array([[0.0, 1.0], [0.0, 1.0]])
    with pytest.raises(gbm.GBMError, match="slope variance"):
        gbm.lasso_select(np.array([1.0, 2.0]), flat, np.array([0.1, 0.2]))


def test_library_exports_enet_path():
    assert "gbm_session_enet_path" in _lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "gbm_session_enet_path" in set(re.findall(r" T (gbm_[a-z0-9_]+)", out))
    lib = gbm.load_library()
    assert hasattr(lib, "gbm_session_enet_path") and lib.gbm_version() == 212
    # argument checks come before any device use
    lam = np.array([1.0])
    b = np.zeros(4)
    y = np.arange(3.0)
    assert lib.gbm_session_enet_path(None, None, 3, _lib.ptr(y), 1.0, _lib.ptr(lam), 1, 1e-7, 10, 0.999, 1e-5,
                                     _lib.ptr(b), None, 0, None, None, None, None, None) == _lib.GBM_E_ARG


@pytest.mark.parametrize("name,alpha,floor", [("p>n", 0.5, 129), ("p>n", 1.0, 65), ("n>p", 1.0, 65), ("n>p", 0.5, 65)])
def test_gpu_case_conditions(name, alpha, floor):
    """What the GPU cases rest on: the active list crosses the block counts they are meant to exercise (three
    blocks at (150, 600) for alpha = 0.5, two otherwise; (1100, 300) has five chunk workgroups) and no
    screening decision after the first λ lies within 1e-9·thr of its threshold (so rounding cannot move an
    admission). Measured: active lists of 146 / 126 at (150, 600) for alpha = 0.5 / 1 and 124 / 123 at
    (1100, 300); smallest margin 6.2e-6."""
    X, y = synth(name)
    assert (X.shape[0] + 255) // 256 == {"p>n": 1, "n>p": 5}[name]
    lam = lasso_ref.lambda_path(X, y, alpha, NL, RATIO)
    r = lasso_ref.enet_path(X, y, lam, alpha=alpha, tol=1e-16)
    print(name, alpha, "active", r["nactive"][-1], "margin", r["margin"])
    assert not r["hit"] and r["nl_done"] == NL
    assert r["nactive"][-1] >= floor
    assert r["margin"] > 1e-9


def test_early_stop_case_fires_before_the_end():
    """The p > n case of the GPU early-stop test saturates: glmnet's rule ends the 100-λ path early."""
    X, y = early_stop_case()
    lam = lasso_ref.lambda_path(X, y, 1.0, 100, 1e-4)
    r = lasso_ref.enet_path(X, y, lam, alpha=1.0, tol=1e-7, dev_max=0.999, fdev=1e-5)
    print("early stop at", r["nl_done"], "dev", r["dev_ratio"][-1])
    assert 5 <= r["nl_done"] < 100
    assert r["dev_ratio"][-1] > 0.999 or r["dev_ratio"][-1] - r["dev_ratio"][-2] < 1e-5 * r["dev_ratio"][-1]


def early_stop_case():
    """40 x 120 with a sparse exact signal: the lasso fits y almost perfectly well before λ_max·1e-4."""
    X = oracle.synth_genotypes(51, 40, 120)
    b = np.zeros(120)
    b[[3, 17, 40, 77, 101]] = [2.0, -1.5, 1.0, 3.0, -2.5]
    return X, 1.0 + X @ b
