"""The elastic-net path's own edges on the device (gbm_session_enet_path, csrc/enet.hip): more than 16 Gram
blocks in one admission with sliced individuals and a later admission that starts at block 16, more than 64
chunk workgroups, the one-slice / two-slice boundary, a list that fills a cap that is no multiple of 64,
collinear columns, columns constant within the training rows only, shapes down to (2, 1), max_passes, exact
power-of-two homogeneity in y, and buffer reuse across calls of different shape on one session.

tests/lasso_ref.py restates the device schedule and tests/test_lasso_cases.py asserts that no decision of the
loop on these inputs lies near its threshold, so the device takes the same passes and differs by rounding
alone: lasso_cases.same_schedule asserts equal pass counts, the same admitted set and 1e-9 on the coefficients
and deviance ratios. A path that starts at λ_max itself has a tie at its first screen; there the device must
match the loop on one side of the tie or the other, in full (lasso_cases.loops)."""
import time

import numpy as np
import pytest

import gbm
import lasso_ref
from test_lasso import synth

import lasso_cases as lc

pytestmark = pytest.mark.gpu

KEYS = ("b_path", "dev_ratio", "passes", "nnz")


def run(name, **kw):
    c = lc.case(name)
    with gbm.GenotypeSession(c.X) as s:
        r = lc.device(s, c, **kw)
    return c, r


def test_17_blocks_in_one_admission_sliced_gram():
    """`blocks17`: launch_enet_gram's 16-block loop takes two trips with S = 2, then starts at block 16. Beside
    the same-schedule comparison, a certificate that does not depend on the schedule: the KKT residual of the
    device's b, recomputed here in fp64, within 10 x the loop's at the same tol."""
    c, r = run("blocks17")
    assert r["warning"] is None
    lp, _ = lc.same_schedule(c, r, lc.loops("blocks17"))
    kkt_dev = lasso_ref.kkt_residual(c.X, c.y, c.lam[1], c.alpha, r["b_path"][1:, 1])
    kkt_loop = lasso_ref.kkt_residual(c.X, c.y, c.lam[1], c.alpha, lp["b_path"][1:, 1])
    print(f"KKT device {kkt_dev:.3e}, loop {kkt_loop:.3e}")
    assert kkt_dev <= 10 * kkt_loop


def test_65_chunks():
    """`chunks65`, n = 16400: the chain's partial-sum reader takes its second trip, the next-block partial
    writer runs with C = 65, the Gram with 32 slices of which three are empty. n > 16384 is the smallest
    shape that reaches these lines; the session also builds the 16400² training kernel (over 72 loci). Session
    and path together: 0.13 s on an MI355X, printed here."""
    t0 = time.perf_counter()
    c, r = run("chunks65")
    print(f"n = 16400 session + path: {time.perf_counter() - t0:.2f} s")
    assert r["warning"] is None
    assert np.array_equal(np.flatnonzero(r["b_path"][1:, -1]), c.support)
    assert list(r["nnz"]) == [0, 66]
    lc.same_schedule(c, r, lc.loops("chunks65"))


@pytest.mark.parametrize("n", [512, 513])
def test_slice_boundary(n):
    """One Gram slice at n = 512, two of 320 at n = 513, as test_gpu_lasso.test_edge_shapes_planted_support."""
    c, r = run(f"slice{n}")
    y = c.y
    assert np.array_equal(np.flatnonzero(r["b_path"][1:, -1]), c.support)
    assert list(r["nnz"]) == [0, 65]
    assert not r["b_path"][1:, 0].any() and abs(r["b_path"][0, 0] - y.mean()) < 1e-12 * abs(y.mean())
    assert r["passes"][0] == 0 and abs(r["dev_ratio"][0]) < 1e-12
    lc.same_schedule(c, r, lc.loops(f"slice{n}"))


def test_every_marker_active_at_a_cap_of_70():
    """`allactive`: the list reaches 70 = p = cap (A + cnt == cap is no cap error), one block and six markers."""
    c, r = run("allactive")
    assert r["warning"] is None
    lc.same_schedule(c, r, lc.loops("allactive"))
    assert r["nnz"][-1] == 70


def test_collinear_columns():
    """`collinear`: three copies of a column and its complement; no nnz comparison (lasso_cases.support)."""
    c, r = run("collinear")
    lc.same_schedule(c, r, lc.loops("collinear"))


def test_constant_within_the_training_rows_only():
    """`const-train`: two columns constant on the training rows (0.5 and the non-dyadic 0.3) stay at b = 0 at
    every λ; they vary on the held-out rows, whose predictions are a0 + X b all the same."""
    c = lc.case("const-train")
    ho = np.setdiff1d(np.arange(c.X.shape[0]), c.idx)
    with gbm.GenotypeSession(c.X) as s:
        r = lc.device(s, c, idx_eval=ho)
    lc.same_schedule(c, r, lc.loops("const-train"))
    for j in lc.CONST_COLS:
        assert np.all(r["b_path"][1 + j] == 0.0)
    want = r["b_path"][0][None, :] + c.X[ho] @ r["b_path"][1:]
    assert np.abs(r["pred"] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("n,p", lc.TINY)
def test_tiny_shapes(n, p):
    c, r = run(f"tiny-{n}x{p}")
    assert r["warning"] is None
    lc.same_schedule(c, r, lc.loops(f"tiny-{n}x{p}"))


@pytest.mark.parametrize("e", [10, -10])
def test_power_of_two_homogeneity(e):
    """The path for (c y, c λ), c = 2^±10, is c times the path for (y, λ) bit for bit, with the same passes,
    nnz and deviance ratios: thr scales by c, tol σ_y² by c², l2 = nλ(1−α)/σ_y not at all, and a power of
    two scales every product, sum, reciprocal and square root exactly. An absolute constant in a kernel or a
    misplaced σ_y would break it."""
    X, y = synth("p>n")
    idx = np.arange(X.shape[0])
    lam = lasso_ref.lambda_path(X, y, 0.5, 6, 0.03)
    c = 2.0 ** e
    with gbm.GenotypeSession(X) as s:
        base = s.enet_path(idx, y, lam, alpha=0.5, tol=1e-10, early_stop=False)
        scaled = s.enet_path(idx, c * y, c * lam, alpha=0.5, tol=1e-10, early_stop=False)
    assert base["passes"].sum() > 50 and base["nnz"][-1] > 64
    assert np.array_equal(scaled["passes"], base["passes"]) and np.array_equal(scaled["nnz"], base["nnz"])
    assert np.array_equal(scaled["dev_ratio"], base["dev_ratio"])
    assert np.array_equal(scaled["b_path"], c * base["b_path"])


def test_max_passes_against_the_loop():
    """`max-passes`: two passes per λ on both sides, a λ that hits the limit not rescreened; the warning names
    the first λ the loop could not finish."""
    c, r = run("max-passes")
    lp, _ = lc.same_schedule(c, r, lc.loops("max-passes"))
    assert r["warning"] is not None and r["warning"].startswith("warning:")
    assert f"first at lambda number {lp['first_hit'] + 1} " in r["warning"]


def test_reuse_across_shapes_on_one_session():
    """The session's en* buffers only grow and the Gram blocks are never cleared: calls of 1100, 40, 600 and
    again 1100 rows on one session each give the bits of the same call on a fresh session (tol = 1e-10, four λ
    down to 0.02 λ_max)."""
    X, y = synth("n>p")
    rng = np.random.default_rng(7)
    rows = [np.arange(1100), np.sort(rng.choice(1100, 40, replace=False)), np.sort(rng.choice(1100, 600, replace=False)),
            np.arange(1100)]
    alphas = [0.5, 1.0, 0.5, 0.5]
    calls = []
    for idx, alpha in zip(rows, alphas):
        lam = lasso_ref.lambda_path(X[idx], y[idx], alpha, 2, 1.0)[0] * np.array([1.5, 0.2, 0.05, 0.02])
        calls.append(dict(idx=idx, y=y[idx], lambdas=lam, alpha=alpha, tol=1e-10, early_stop=False))
    with gbm.GenotypeSession(X) as s:
        shared = [s.enet_path(**kw) for kw in calls]
    # the loop's lists end at 192, 131 and 214 markers: 3, 3 and 4 blocks, the last call under the 600-row call's blocks
    assert shared[0]["nnz"][-1] > 128 and shared[1]["nnz"][-1] > 30 and shared[2]["nnz"][-1] > 128
    for kw, got in zip(calls[:3], shared):
        with gbm.GenotypeSession(X) as s:
            fresh = s.enet_path(**kw)
        for key in KEYS:
            assert np.array_equal(got[key], fresh[key]), (kw["idx"].size, key)
    for key in KEYS:
        assert np.array_equal(shared[0][key], shared[3][key]), key
