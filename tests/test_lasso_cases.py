"""The conditions that tests/test_gpu_lasso_edges.py rests on, asserted on the numpy loop alone
(lasso_ref.enet_path on the inputs of tests/lasso_cases.py): no stopping decision within 1e-6 of tol σ_y² and
no screening decision within 1e-9 of its threshold but the tie of a path that starts at λ_max itself, which is
taken on both sides (lasso_cases.loops), so that the device takes the loop's passes; and the block, chunk and slice counts each case is there to reach in csrc/enet.hip."""
import numpy as np
import pytest

import lasso_ref

import lasso_cases as lc


TIED = ("allactive", "collinear", "max-passes", "tiny-2x1", "tiny-5x1", "tiny-3x5")  # λ₁ = λ_max itself


@pytest.mark.parametrize("name", lc.SAME_SCHEDULE)
def test_no_decision_near_its_threshold(name):
    """Measured: the smallest stop margin is 1.4e-2 (`blocks17`), the smallest screening margin 1.1e-4
    (`const-train`). `max-passes` never comes near tol = 1e-16 (stop margin 4e12). The cases whose path
    starts at λ_max have their first screen within 5e-16 of its threshold (exactly on it in four of the six):
    a tie, taken on both sides, with no other marker within 1e-9 of either shifted threshold."""
    lps = lc.loops(name)
    assert len(lps) == (2 if name in TIED else 1)
    for lp in lps:
        print(name, "stop_margin", lp["stop_margin"], "margin", lp["margin"], "margin0", lp["margin0"], "passes", list(lp["passes"]))
        assert lp["nl_done"] == lc.case(name).lam.size
        assert lp["stop_margin"] > lc.STOP_MARGIN
        assert lp["margin"] > lc.SCREEN_MARGIN
        assert lp["margin0"] > 0.99 * lc.TIE
        assert lp["hit"] == (name == "max-passes")
        assert np.isfinite(lp["b_path"]).all() and np.isfinite(lp["dev_ratio"]).all()
    if name in TIED:  # the two sides differ in the first λ's passes, so a device result matches one at most
        assert lc.loop(name)["margin0"] < 1e-12
        assert lps[0]["passes"][0] == 0 and lps[1]["passes"][0] >= 1
        assert lps[0]["admits"][0][0] >= 1 and lps[1]["admits"][0][0] == 0


def test_tie_parameter_leaves_the_plain_loop_alone():
    """tie = 0 is the loop as it was, bit for bit (thr·(1 + 0) = thr); away from a tie, ±1e-9 changes nothing."""
    c = lc.case("const-train")
    X, kw = c.X[c.idx], dict(alpha=c.alpha, tol=c.tol)
    a, b, d = (lasso_ref.enet_path(X, c.y, c.lam, tie=t, **kw) for t in (0.0, lc.TIE, -lc.TIE))
    for key in ("b_path", "dev_ratio", "passes", "nnz"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], d[key])
    assert a["admits"] == b["admits"] == d["admits"] and a["margin0"] > 0.3


def test_stop_margin_is_the_closest_pass():
    """stop_margin on a one-marker fit worked by hand: x = (−½, ½), e = (−d, d), so g = d, the first pass
    moves b by δ = (d − thr)/x2 with x2 = ½ and dmax = x2 δ²/n; the second moves nothing (dmax = 0,
    margin 1)."""
    X, y = np.array([[0.0], [1.0]]), np.array([1.0, 3.0])
    lam, tol = 0.25, 1e-3
    lp = lasso_ref.enet_path(X, y, [lam], alpha=1.0, tol=tol)
    delta = (1.0 - 2 * lam) / 0.5
    dmax, t = 0.5 * delta * delta / 2, tol * 1.0
    assert list(lp["passes"]) == [2] and lp["admits"] == [(0, 0, 1)]
    assert lp["stop_margin"] == min(abs(dmax - t) / t, 1.0) == 1.0
    lp = lasso_ref.enet_path(X, y, [lam], alpha=1.0, tol=0.4)  # dmax = 0.25 < 0.4: one pass, margin 0.375
    assert list(lp["passes"]) == [1] and abs(lp["stop_margin"] - 0.375) < 1e-15


def test_blocks17_admits_17_blocks_then_starts_at_block_16():
    """(520, 1100), alpha = 0.05: the first screen at λ₂ admits 1074 markers (17 blocks from block 0: two trips
    of launch_enet_gram's 16-block loop, two slices of individuals), the next 14 more (blk0 = 16 with S = 2
    and the workspace of the trip before), the last 1; 43 passes at tol = 1e-6."""
    c, lp = lc.case("blocks17"), lc.loop("blocks17")
    n, p = c.X.shape
    print(lp["admits"], list(lp["passes"]))
    assert lc.gram_slices(n) == (2, 320)
    assert list(lp["nactive"])[0] == 0
    k, before, cnt = lp["admits"][0]
    assert (k, before) == (1, 0) and cnt >= 1025  # more than 16 blocks in one call
    k, before, cnt2 = lp["admits"][1]
    assert before // lc.BB == 16 and -(-(before + cnt2) // lc.BB) - 16 >= 1  # a call that starts at block 16
    assert lp["nactive"][-1] <= lc.cap(n, p) == 1100


def test_chunks65_shape():
    """n = 16400: 65 chunk workgroups (the partial-sum reader's second trip), two blocks (the next-block
    partial writer runs with C = 65), 32 Gram slices of 576 individuals of which three start past n."""
    c, lp = lc.case("chunks65"), lc.loop("chunks65")
    n = c.X.shape[0]
    assert -(-n // lc.IW) == 65
    S, sl = lc.gram_slices(n)
    assert (S, sl) == (32, 576) and sum(y * sl >= n for y in range(S)) == 3
    assert list(lp["nactive"]) == [0, 66] and list(lp["nnz"]) == [0, 66] and list(lp["passes"]) == [0, 6]
    assert np.array_equal(np.flatnonzero(lp["b_path"][1:, -1]), c.support)
    assert lp["margin"] > 0.8


@pytest.mark.parametrize("n,S,sl", [(512, 1, 512), (513, 2, 320)])
def test_slice_boundary_shapes(n, S, sl):
    """One slice at n = 512, two of 320 at n = 513; the loop admits exactly the planted 65 (two blocks).
    Seed 71 at n = 513 admits a 66th marker; seed 72 is the first that does not."""
    c, lp = lc.case(f"slice{n}"), lc.loop(f"slice{n}")
    assert c.X.shape == (n, 100) and lc.gram_slices(n) == (S, sl)
    assert lp["nactive"][-1] == 65 and list(lp["nnz"]) == [0, 65]
    assert np.array_equal(np.flatnonzero(lp["b_path"][1:, -1]), c.support)


def test_allactive_fills_its_cap():
    c, lp = lc.case("allactive"), lc.loop("allactive")
    n, p = c.X.shape
    assert lc.cap(n, p) == p == 70 and p % lc.BB != 0
    assert list(lp["nactive"]) == [1, 1, 44, 69, 70, 70]
    assert sorted(lp["active"]) == list(range(70))


def test_collinear_columns():
    """Columns 40 and 80 copy column 7 and column 41 is its complement: after centring, x₄₁ = −x₇. The ridge
    term makes the minimiser unique and splits the effect evenly: ±0.4901 at the last λ when converged; at
    tol = 1e-7 the four are within 0.02 of it. The loop leaves 5e-15 where a collinear column's exact zero
    belongs, so nnz is not compared on these inputs."""
    c, lp = lc.case("collinear"), lc.loop("collinear")
    X = c.X
    assert np.array_equal(X[:, 40], X[:, 7]) and np.array_equal(X[:, 80], X[:, 7]) and np.array_equal(X[:, 41], 1.0 - X[:, 7])
    assert X[:, 7].std() > 0
    b = lp["b_path"][1:, -1]
    assert np.abs(b[[7, 40, 80]] - 0.4901).max() < 0.02 and abs(b[41] + 0.4901) < 0.02
    fine = lasso_ref.enet_path(X, c.y, c.lam, alpha=c.alpha, tol=1e-14)["b_path"][1:, -1]
    assert np.abs(np.abs(fine[[7, 40, 80, 41]]) - 0.4901).max() < 5e-4


def test_const_train_columns():
    """Two columns constant on the training rows and varying on the others: centred on the training rows they
    are 0 (0.5) or rounding noise (0.3: x2 = 1.5e-29), never past the threshold, b = 0 at every λ."""
    c, lp = lc.case("const-train"), lc.loop("const-train")
    ho = np.setdiff1d(np.arange(c.X.shape[0]), c.idx)
    for j, v in zip(lc.CONST_COLS, (0.5, 0.3)):
        assert np.all(c.X[c.idx, j] == v) and c.X[ho, j].std() > 0
        assert np.all(lp["b_path"][1 + j] == 0.0)
    assert lp["nactive"][-1] > lc.BB  # two blocks by the last λ (measured 100)


@pytest.mark.parametrize("n,p", lc.TINY)
def test_tiny_shapes_run(n, p):
    c, lp = lc.case(f"tiny-{n}x{p}"), lc.loop(f"tiny-{n}x{p}")
    assert c.X.shape == (n, p) and c.lam.size == 4
    assert np.all(c.X[0] == 0.0) and np.all(c.X[1] == 1.0)
    assert lp["nnz"][-1] >= 1 and lp["dev_ratio"][-1] > 0.1


def test_max_passes_case_hits_at_the_second_lambda():
    """On either side of the tie at λ₁ the second λ is the first to hit the limit and is not rescreened once it has; with
    the tie admitted its two passes go to that one marker (the second moves nothing, so it converges at the
    limit) and the nine that the rescreen then adds get no pass: b = 0."""
    plain, admitted = lc.loops("max-passes")
    assert plain["hit"] and plain["first_hit"] == 1 and list(plain["passes"]) == [0, 2, 2]
    assert plain["admits"] == [(1, 0, 14)]
    assert admitted["hit"] and admitted["first_hit"] == 1 and list(admitted["passes"]) == [1, 2, 2]
    assert admitted["admits"] == [(0, 0, 1), (1, 1, 9)] and list(admitted["nnz"]) == [0, 1, 10]
