"""Several BayesA / BayesB / BayesC chains over one genotype matrix, each on its own training rows (libgbm
``gbm_bayes_fit_multi_rows``; ``gbm.bayes_multi_rows_arrays``; ``cvbulk(..., bayes_folds=True)``): the folds of a
cross-validation as chains of one pass. A chain's residual is exactly 0.0 at its held-out rows, so every sum over
individuals adds exact zeros there in the kernels' fixed order. That gives two exact contracts: one set of all rows
has the bits of ``gbm_bayes_fit_multi``, and a set that keeps the first n_c rows has the bits of the single fit on
those rows (b_hat, var, pip). Interleaved sets are compared with the literal loop on the chain's rows alone at the
suite's 1e-9 (their indicator margins: tests/test_bayes_rows.py). Every fit runs with byte and fp64 genotype
storage and with four chains and one chain per workgroup row forced, the four results equal bit for bit.
Shapes (csrc/bayes_abc.hip bayes_chain_kernel): chunk workgroups of 256 rows, blocks of 64 markers, workgroup rows
of 4 chains; (300, 150) has two chunk workgroups and blocks of 64, 64 and 22. Inputs and helpers:
tests/bayes_rows_cases.py, tests/bayes_multi_cases.py, tests/gibbs_cases.py."""
import ctypes

import numpy as np
import pytest

import gbm

import bayes_multi_cases as mc
import bayes_rows_cases as rc
import gibbs_cases as gc

pytestmark = pytest.mark.gpu


def rows_stats():
    calls, chains = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert gbm.load_library().gbm_debug_bayes_rows_stats(ctypes.byref(calls), ctypes.byref(chains)) == 0
    return calls.value, chains.value


def _dosage_case(n, p, T, sets, set_of):
    X, Y = mc.inputs("dosage", n, p)
    return rc._case(X, Y[:, :T], sets, set_of, [mc.model_of(c) for c in range(T)], [mc.seed_of(c) for c in range(T)])


# ---- 1. all rows: the bits of gbm_bayes_fit_multi ------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5])
def test_gpu_one_set_of_all_rows_has_the_bits_of_the_multi_fit(gbm_env, T):
    cs = _dosage_case(300, 150, T, np.ones((1, 300), dtype=bool), [0] * T)
    outs = rc.fit_all_ways(gbm_env, cs)
    assert [a.shape for a in outs] == [(151, T), (300, T), (3, T), (150, T)]
    mc.assert_same_bits(outs, mc.multi("dosage", 300, 150, T, gc.DEFAULT), "rows vs multi")


# ---- 2. tail hold-out: the bits of the single fit on the first n_c rows --------------------------------------
@pytest.mark.parametrize("n_c", [256, 257, 200])
def test_gpu_tail_hold_out_has_the_bits_of_the_fit_on_the_prefix(gbm_env, n_c):
    """Trailing zeros add exactly in every fixed-order sum (column statistics, Gram tiles, the chunk partials, μ,
    the variance partials), so b_hat, var and pip equal gbm.bayes_arrays on X[:n_c], y[:n_c] bit for bit; y_pred's
    chunking depends on n, so y_pred[:n_c] agrees to 1e-12 of its maximum. Y is NaN at the held-out rows."""
    T = 3
    X, Y = mc.inputs("dosage", 300, 150)
    Yn = np.array(Y[:, :T])
    Yn[n_c:] = np.nan
    cs = _dosage_case(300, 150, T, (np.arange(300) < n_c)[None, :], [0] * T)
    b_hat, y_pred, var, pip = rc.fit_all_ways(gbm_env, cs, Y=Yn)
    n_iter, n_burnin, thin = gc.DEFAULT
    gbm_env.setenv("GBM_BRR_I8", "1")
    for c in range(T):
        want = gbm.bayes_arrays(mc.model_of(c), X[:n_c], Y[:n_c, c], n_iter=n_iter, n_burnin=n_burnin, thin=thin,
                                seed=mc.seed_of(c))
        for name, a, b in (("b_hat", b_hat[:, c], want[0]), ("var", var[:, c], want[2]), ("pip", pip[:, c], want[3])):
            assert np.array_equal(a, b), (n_c, c, name, float(np.abs(a - b).max()))
        err = np.abs(y_pred[:n_c, c] - want[1]).max() / np.abs(want[1]).max()
        print("n_c", n_c, "chain", c, "y_pred rel", float(f"{err:.3g}"))
        assert err < 1e-12, (n_c, c, err)
        held = b_hat[0, c] + X[n_c:] @ b_hat[1:, c]
        assert rc.rel(y_pred[n_c:, c], held) < 1e-12, (n_c, c)


# ---- 3, 5, 6. interleaved folds, chunk edges and degenerate columns against the literal loop -----------------
@pytest.mark.parametrize("name", rc.LOOP_CASES)
def test_gpu_chains_on_their_rows_follow_the_literal_loop(gbm_env, name):
    """mod5 / random5: 15 chains, 5 fold sets x models A, B, C (set_of = c // 3), folds i % 5 and a seeded draw with
    replacement. chunk_out: n = 600 with rows 256 .. 511 held out (a whole chunk workgroup contributes zeros).
    three_rows: n_c = 3 at (300, 65). four_by_one: (4, 1), one row held out. degenerate: a marker that is zero on
    the training rows only and one that is constant there (the held-out prediction uses its drawn effect).
    Every chain within 1e-9 of bayes_abc_ref.bayes_gibbs on X[S_c], y[S_c] (b_hat, var, pip, y_pred at S_c); y_pred
    at the held-out rows within 1e-12 of b_hat[0] + X b_hat[1:]. Measured worst on an MI355X: 1.1e-15 against the
    loop (random5's b_hat; four_by_one's var 1.09e-15), 6.2e-16 at the held-out rows."""
    outs = rc.fit_all_ways(gbm_env, rc.case(name))
    worst = rc.worst_against_loop(name, outs)
    print(name, {k: float(f"{v:.3g}") for k, v in worst.items()})
    for k in rc.OUTPUTS:
        assert worst[k] < 1e-9, (name, k, worst[k])
    assert worst["held_out"] < 1e-12, (name, worst["held_out"])


def test_gpu_degenerate_marker_predicts_with_its_drawn_effect(gbm_env):
    """The marker that is zero on every training row has x2 = 0: its effect is a draw from its prior, not zero, and
    enters the held-out rows' prediction (compared above); here that BayesA's (always included) is in fact
    non-zero and moves the held-out prediction."""
    cs = rc.case("degenerate")
    b_hat, y_pred, _, _ = rc.fit(cs)
    assert cs["models"][0] == "BayesA" and b_hat[1 + 3, 0] != 0.0
    held = ~cs["sets"][0]
    without = b_hat[0, 0] + np.delete(cs["X"][held], 3, axis=1) @ np.delete(b_hat[1:, 0], 3)
    assert np.abs(y_pred[held, 0] - without).max() > 1e-3 * np.abs(y_pred[held, 0]).max()


def test_gpu_a_set_without_marker_variance_is_refused_by_name():
    """Every marker constant on the rows of set 1 (they vary on the held-out rows only): MSx = 0 there, GBM_E_DATA
    naming the set; set 0 (all rows) alone is fitted."""
    X = np.full((40, 5), 0.5)
    X[30:] = np.random.default_rng(3).integers(0, 3, (10, 5)) / 2
    Y = np.random.default_rng(4).standard_normal((40, 2))
    sets = np.ones((2, 40), dtype=bool)
    sets[1, 30:] = False
    kw = dict(n_iter=6, n_burnin=2, thin=1)
    with pytest.raises(gbm.GBMError, match="set 1: the markers have no variance") as err:
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesC"], X, Y, sets, [0, 1], **kw)
    assert err.value.code == gbm._lib.GBM_E_DATA
    b_hat = gbm.bayes_multi_rows_arrays(["BayesA", "BayesC"], X, Y, sets[:1], [0, 0], **kw)[0]
    assert np.isfinite(b_hat).all()


# ---- 4. workgroup-row edges ----------------------------------------------------------------------------------
def _distinct_sets(n, T):
    """T different training sets: set s holds out the rows i with i % (T + 1) == s."""
    return np.stack([np.arange(n) % (T + 1) != s for s in range(T)])


@pytest.mark.parametrize("n,p,T,shared", [(300, 150, 5, False), (300, 150, 4, False), (300, 150, 4, True),
                                          (77, 130, 32, False)],
                         ids=["T5-five-sets", "T4-four-sets", "T4-one-set", "T32-32-sets"])
def test_gpu_a_chain_does_not_depend_on_its_row_mates(gbm_env, n, p, T, shared):
    """T = 5 with five sets: the second workgroup row holds one chain and three empty slots. T = 4 with four sets in
    one workgroup: every wave loads the Gram column of its own set; with one shared set they load the same. T = 32
    with 32 sets at (77, 130): eight full rows, every mask bit in use. Each chain equals, bit for bit, the same
    chain run alone with its set (T = 1), so neither its slot, its neighbours' sets nor the set's index matter."""
    sets = _distinct_sets(n, 1 if shared else T)
    cs = _dosage_case(n, p, T, sets, [0] * T if shared else list(range(T)))
    outs = rc.fit_all_ways(gbm_env, cs)
    for c in sorted({0, 3, T - 1}):
        alone = rc.fit(cs, models=cs["models"][c:c + 1], Y=cs["Y"][:, c:c + 1], seeds=cs["seeds"][c:c + 1],
                       sets=cs["sets"][cs["set_of"][c]][None, :], set_of=(0,))
        mc.assert_same_bits(mc.chain(outs, c), mc.chain(alone, 0), ("chain", c, "alone"))
    assert not np.array_equal(outs[0][:, 0], outs[0][:, 1])


# ---- 7. the pooled context -----------------------------------------------------------------------------------
def test_gpu_pooled_context_across_fits(gbm_env):
    """A rows fit, then a plain multi fit, a single fit and a smaller rows fit on the pooled context, then the first
    again: unchanged bits, and no allocation (its buffers and its captured iteration are the first's). The plain
    fits in between keep their own bits; BRR's path statistics are untouched."""
    lib = gbm.load_library()
    path, fb = ctypes.c_int(-1), ctypes.c_int64(0)

    def brr_stats():
        lib.gbm_debug_brr_stats(ctypes.byref(path), ctypes.byref(fb))
        return path.value, fb.value

    gbm_env.setenv("GBM_BAYES_MULTI_WG", "4")
    stats = brr_stats()
    cs = rc.case("mod5")
    first = rc.fit(cs)
    multi = mc.multi("dosage", 300, 150, 5, gc.DEFAULT)
    for c in range(5):
        mc.assert_same_bits(mc.chain(multi, c), mc.single("dosage", 300, 150, c, gc.DEFAULT, "bytes"), ("multi", c))
    X, Y = mc.inputs("dosage", 300, 150)
    one = gbm.bayes_arrays(mc.model_of(2), X, Y[:, 2], n_iter=9, n_burnin=2, thin=1, seed=mc.seed_of(2))
    mc.assert_same_bits(one, mc.chain(multi, 2), "single fit after the rows fit")
    small = _dosage_case(200, 64, 2, _distinct_sets(200, 2), [0, 1])
    small_first = rc.fit(small)
    a0 = lib.gbm_device_allocations()
    last = rc.fit(cs)
    assert lib.gbm_device_allocations() == a0
    mc.assert_same_bits(first, last, "first vs last")
    mc.assert_same_bits(rc.fit(small), small_first, "small again")
    assert lib.gbm_device_allocations() == a0
    assert brr_stats() == stats


# ---- 8. cross-validation -------------------------------------------------------------------------------------
def test_gpu_cvbulk_runs_a_traits_folds_as_one_pass():
    """cvbulk over (bayesa, bayesb, bayesc), 3 folds, on 60 entries x 90 loci with two traits and a missing phenotype:
    with bayes_folds one rows call per trait carrying 9 chains, and every CV within 1e-9 of the bayes_folds=False
    result (b_hat, y_pred, validation_y_pred, relative to their maxima), with equal entries, populations, folds and
    validation_y_true. With bayes_folds=False the result is today's, bit for bit (no rows call)."""
    kw = rc.cv_kwargs()
    c0 = rows_stats()
    plain, notes0 = gbm.cvbulk(**kw)
    explicit, _ = gbm.cvbulk(bayes_folds=False, **kw)
    assert rows_stats() == c0
    assert all(mc.same_cv(a, b) for a, b in zip(plain, explicit))
    folds, notes = gbm.cvbulk(bayes_folds=True, **kw)
    assert rows_stats() == (c0[0] + 2, c0[1] + 18)
    assert notes == notes0 == [] and len(folds) == len(plain) == 18
    worst = dict(b_hat=0.0, y_pred=0.0, validation_y_pred=0.0)
    for a, b in zip(folds, plain):
        assert (a.replication, a.fold, a.fit.model, a.fit.trait) == (b.replication, b.fold, b.fit.model, b.fit.trait)
        assert a.fit.entries == b.fit.entries and a.fit.populations == b.fit.populations
        assert a.fit.b_hat_labels == b.fit.b_hat_labels and np.array_equal(a.fit.y_true, b.fit.y_true)
        assert a.validation_entries == b.validation_entries and a.validation_populations == b.validation_populations
        assert np.array_equal(a.validation_y_true, b.validation_y_true)
        assert a.checkdims() and set(a.metrics) == set(b.metrics) and set(a.fit.metrics) == set(b.fit.metrics)
        for k, u, v in (("b_hat", a.fit.b_hat, b.fit.b_hat), ("y_pred", a.fit.y_pred, b.fit.y_pred),
                        ("validation_y_pred", a.validation_y_pred, b.validation_y_pred)):
            worst[k] = max(worst[k], rc.rel(u, v))
    print({k: float(f"{v:.3g}") for k, v in worst.items()})
    for k, v in worst.items():
        assert v < 1e-9, (k, v)
