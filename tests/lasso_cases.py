"""Inputs, cached loop results and the shared comparison of the elastic-net path's edge tests
(tests/test_lasso_cases.py on the CPU, tests/test_gpu_lasso_edges.py on the device): an admission of 17
blocks over two individual slices, 65 chunk workgroups, the one-slice / two-slice boundary, a list that fills
its cap of 70, collinear columns, columns constant within the training rows only, shapes down to (2, 1),
max_passes, and the inputs of the homogeneity and buffer-reuse tests.

tests/lasso_ref.py restates the device schedule, so where no decision of the loop (a screen, a stop) lies
within rounding of its threshold the device takes the same passes and differs from the loop by rounding
alone: `same_schedule` asserts equal pass counts and 1e-9. One decision is a tie by construction: a path from
lasso_ref.lambda_path starts at λ_max itself, where the marker that defines λ_max has |g_j| = thr up to the
rounding of the sums (the loop's `margin` leaves the first λ out for that reason). Admitted there, it gets
b ~ 1e-17 and one pass, and it stands first in the list from then on; not admitted, it joins at the next λ
in index order. Both are the stated schedule, so `loops` gives the loop on either side of such a tie and the
device has to match one of the two in full. Every array is built once and is read-only. Not a test module."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import lasso_ref
import oracle

# tol of a case that is not a converged fit (1e-14, 1e-16): the first of 1e-6 (`blocks17` only), 1e-7, 3e-8, 1e-8,
# 3e-7 at which the loop's stop margin passes STOP_MARGIN; 1e-7 does for all of them
STOP_MARGIN = 1e-6  # no pass's dmax within this (relative) of tol σ_y²: rounding (~1e-13) cannot move a stop
SCREEN_MARGIN = 1e-9  # tests/test_lasso.py's: no screened |g_j| within this of thr
TIE = 1e-9  # a first-λ screen closer than this is taken on both sides (lasso_ref.enet_path's `tie`)
BOUND = 1e-9  # device against loop at equal pass counts, the bound of the converged cases of test_gpu_lasso.py
BB, IW = 64, 256  # csrc/enet.hip: markers per block, individuals per chunk workgroup


class Case(NamedTuple):
    X: np.ndarray  # the session's genotypes
    idx: np.ndarray  # training rows (sorted)
    y: np.ndarray  # training phenotypes, one per row of idx
    lam: np.ndarray
    alpha: float
    tol: float
    max_passes: int = 1_000_000
    support: Optional[np.ndarray] = None  # planted designs: the columns the lasso must select


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _lmax(X, y, alpha):
    return lasso_ref.lambda_path(X, y, alpha, 2, 1.0)[0]


def _synth(sx, n, p, sy):
    X = oracle.synth_genotypes(sx, n, p)
    return X, oracle.synth_phenotypes(X, sy)[:, 0]


def _whole(X, y, lam, alpha, tol, **kw):
    X = np.asfortranarray(X)
    return Case(_frozen(X), _frozen(np.arange(X.shape[0])), _frozen(np.array(y)), _frozen(np.array(lam)), alpha, tol, **kw)


def _planted(seed, n, p, k):
    X, y, S = lasso_ref.planted(seed, n, p, k)
    return _whole(X, y, _lmax(X, y, 1.0) * np.array([1.5, 0.1]), 1.0, 1e-14, support=_frozen(S))


def _blocks17():
    X, y = _synth(91, 520, 1100, 92)
    return _whole(X, y, _lmax(X, y, 0.05) * np.array([1.5, 0.002]), 0.05, 1e-6)


def _allactive():
    X, y = _synth(93, 300, 70, 94)
    return _whole(X, y, lasso_ref.lambda_path(X, y, 0.5, 6, 1e-4), 0.5, 1e-14)


def _collinear():
    X = oracle.synth_genotypes(95, 200, 90).copy()
    X[:, 40] = X[:, 7]
    X[:, 80] = X[:, 7]
    X[:, 41] = 1.0 - X[:, 7]
    b = np.zeros(90)
    b[[7, 20, 55]] = [2.0, -1.0, 1.5]
    y = 1.0 + X @ b + 0.1 * np.random.default_rng(96).standard_normal(200)
    return _whole(X, y, lasso_ref.lambda_path(X, y, 0.5, 8, 0.01), 0.5, 1e-7)


CONST_COLS = (10, 300)  # of `const-train`: 0.5 and 0.3 on the even rows, varying on the odd ones


def _const_train():
    X, y = _synth(43, 150, 600, 44)  # test_lasso.SHAPES["p>n"]
    X = X.copy()
    tr = np.arange(0, 150, 2)
    X[tr, CONST_COLS[0]] = 0.5
    X[tr, CONST_COLS[1]] = 0.3
    lam = _lmax(X[tr], y[tr], 0.5) * np.array([1.5, 0.5, 0.2, 0.08])
    return Case(_frozen(np.asfortranarray(X)), _frozen(tr), _frozen(y[tr].copy()), _frozen(lam), 0.5, 1e-7)


def _tiny(n, p):
    X = oracle.synth_genotypes(97, n, p).copy()
    X[0, :] = 0.0
    X[1, :] = 1.0
    y = oracle.synth_phenotypes(X, 98)[:, 0]
    return _whole(X, y, lasso_ref.lambda_path(X, y, 1.0, 4, 0.05), 1.0, 1e-7)


def _max_passes():
    X, y = _synth(43, 150, 600, 44)  # the case of test_gpu_lasso.test_argument_refusals
    return _whole(X, y, lasso_ref.lambda_path(X, y, 1.0, 3, 0.1), 1.0, 1e-16, max_passes=2)


SLICE_SEEDS = {512: 71, 513: 72}  # planted(seed, n, 100, 65): the loop admits exactly the planted 65
TINY = ((2, 1), (5, 1), (3, 5))

BUILDERS = {"blocks17": _blocks17, "chunks65": lambda: _planted(81, 16400, 72, 66),
            "slice512": lambda: _planted(SLICE_SEEDS[512], 512, 100, 65),
            "slice513": lambda: _planted(SLICE_SEEDS[513], 513, 100, 65), "allactive": _allactive,
            "collinear": _collinear, "const-train": _const_train, "max-passes": _max_passes,
            **{f"tiny-{n}x{p}": functools.partial(_tiny, n, p) for n, p in TINY}}
SAME_SCHEDULE = tuple(BUILDERS)  # every case here goes through `same_schedule`


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def loop(name, tie=0.0):
    """lasso_ref.enet_path on the case's training rows, with its tol, alpha, λ and max_passes."""
    c = case(name)
    return lasso_ref.enet_path(c.X[c.idx], c.y, c.lam, alpha=c.alpha, tol=c.tol, max_passes=c.max_passes, tie=tie)


def loops(name):
    """The loop results the device may match: the plain loop where no screen of the first λ is within TIE of
    its threshold, else the loop with the tie not admitted and admitted."""
    if loop(name)["margin0"] > TIE:
        return (loop(name),)
    return loop(name, TIE), loop(name, -TIE)


def device(session, c, **kw):
    return session.enet_path(c.idx, c.y, c.lam, alpha=c.alpha, tol=c.tol, max_passes=c.max_passes, early_stop=False, **kw)


def gram_slices(n):
    """(S, slice) of launch_enet_gram: slices of individuals per Gram block and their length."""
    S = min(32, max(1, (n + 511) // 512))
    per = -(-n // S)
    return S, -(-per // BB) * BB if S > 1 else n


def cap(n, p):
    """Rows of the packed active set (session_linear.cpp): min(p, 2 npad), npad = n rounded up to 128."""
    return min(p, 2 * (-(-n // 128) * 128))


def support(B):
    """The admitted set at every λ as far as the slopes B (p, nl) show it: (j, k) with |b_jk| > 1e-12 max|B|
    (the device does not return its list; collinear columns leave 5e-15 where an exact zero belongs and a tie
    at λ_max leaves 1e-17, on the loop too)."""
    return np.argwhere(np.abs(B) > 1e-12 * np.abs(B).max())


def same_schedule(c, r, lps):
    """Device result r against the loop results lps (`loops`) at the same tol, alpha, λ and max_passes: the
    passes of one of them at every λ, and against that one the same admitted set and coefficients (intercept
    included) and deviance ratios within 1e-9. Returns (the loop result matched,
    max|b_dev − b_loop| / max(1, max|b_loop|))."""
    match = [lp for lp in lps if np.array_equal(r["passes"], lp["passes"])]
    assert match, (r["passes"], [lp["passes"] for lp in lps])
    lp = match[0]
    assert r["nl_done"] == lp["nl_done"] == c.lam.size
    B, Bl = r["b_path"], lp["b_path"]
    assert B.shape == Bl.shape == (c.X.shape[1] + 1, c.lam.size)
    assert np.array_equal(support(B[1:]), support(Bl[1:]))
    err = np.abs(B - Bl).max() / max(1.0, np.abs(Bl).max())
    dev = np.abs(r["dev_ratio"] - lp["dev_ratio"]).max()
    print(f"passes {r['passes'].tolist()} (of {len(lps)} loop schedules), |b - loop| = {err:.3e}, |dev_ratio - loop| = {dev:.3e}")
    assert err <= BOUND
    assert dev < BOUND
    return lp, err
