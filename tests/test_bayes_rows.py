"""CPU side of the multi-chain BayesA/B/C fit with a training set per chain (libgbm ``gbm_bayes_fit_multi_rows``,
``gbm.bayes_multi_rows_arrays``, ``cvmultithread(..., bayes_folds=True)``): every refusal comes back as GBM_E_ARG
before any device call with the chain or the set named; the grouping of the folds with the fit and the validation
stubbed (keys, shared sets, the split at 32 chains, error recording, jobs that share with nobody); and the
precondition of the device tests' loop comparisons: no indicator draw of a loop reference lies within 1e-6 of its
threshold. The device tests: tests/test_gpu_bayes_rows.py."""
import ctypes
import functools

import numpy as np
import pytest

import gbm
from gbm import _lib
from gbm import cv as gcv

import bayes_multi_cases as mc
import bayes_rows_cases as rc

E = _lib.GBM_E_ARG


def _rc(T=3, n=20, p=30, nsets=2, set_of=None, rows=None, ldrows=None, null=(), y_nan=None, y_const=None, n_iter=10,
        n_burnin=2, thin=1, ldy=None, models=None, **priors):
    """gbm_bayes_fit_multi_rows on valid arguments with the named ones replaced. Set 0 holds rows 0 .. 14, set 1
    rows 5 .. 19; chain c trains on set c % 2. ``y_nan`` / ``y_const``: (chain, rows)."""
    Tn = max(T, 1)
    X = np.asfortranarray(np.random.default_rng(0).random((n, p)))
    Y = np.asfortranarray(np.random.default_rng(1).random((n, Tn)))
    if rows is None:
        rows = np.zeros((max(nsets, 2), n), dtype=np.uint8)
        rows[0, :15] = 1
        rows[1, 5:] = 1
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if y_nan is not None:
        Y[y_nan[1], y_nan[0]] = np.nan
    if y_const is not None:
        Y[y_const[1], y_const[0]] = 1.0
    arr = {"models": np.array(models if models is not None else [1 + c % 3 for c in range(Tn)], dtype=np.intc),
           "r2": np.full(Tn, 0.5), "df0": np.full(Tn, 5.0), "prob_in": np.full(Tn, 0.5), "counts": np.full(Tn, 10.0),
           "seeds": np.arange(Tn, dtype=np.uint64), "X": X, "Y": Y, "rows": rows,
           "set_of": np.array(set_of if set_of is not None else [c % 2 for c in range(Tn)], dtype=np.intc),
           "b_hat": np.zeros((p + 1, Tn), order="F"), "y_pred": np.zeros((n, Tn), order="F"),
           "var": np.zeros((3, Tn), order="F"), "pip": np.zeros((p, Tn), order="F")}
    for name, (c, v) in priors.items():
        arr[name][c] = v
    a = {k: (None if k in null else _lib.ptr(v)) for k, v in arr.items()}
    return gbm.load_library().gbm_bayes_fit_multi_rows(
        T, a["models"], a["X"], n, p, n, a["Y"], n if ldy is None else ldy, nsets, a["rows"],
        rows.shape[1] if ldrows is None else ldrows, a["set_of"], n_iter, n_burnin, thin, a["r2"], a["df0"],
        a["prob_in"], a["counts"], a["seeds"], 0, a["b_hat"], p + 1, a["y_pred"], n, a["var"], a["pip"], p)


def _rows_stats():
    calls, chains = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert gbm.load_library().gbm_debug_bayes_rows_stats(ctypes.byref(calls), ctypes.byref(chains)) == 0
    return calls.value, chains.value


def test_arguments_are_refused_before_device_use():
    assert "gbm_bayes_fit_multi_rows" in _lib.EXPORTS and "gbm_debug_bayes_rows_stats" in _lib.EXPORTS
    before = _rows_stats()
    # gbm_bayes_fit_multi's own refusals
    for T in (0, -1, 33):
        assert _rc(T=T) == E and "nchains" in _lib.last_error()
    for name in ("models", "X", "Y", "r2", "df0", "prob_in", "counts", "seeds", "b_hat"):
        assert _rc(null=(name,)) == E and "required" in _lib.last_error(), name
    assert _rc(ldy=19) == E and "pitch" in _lib.last_error()
    for c in (0, 2):
        m = [1, 2, 3]
        m[c] = 4
        assert _rc(models=m) == E and f"chain {c}: model" in _lib.last_error()
        assert _rc(prob_in=(c, 1.0)) == E and f"chain {c}: bad prior" in _lib.last_error()
        assert _rc(r2=(c, 1.0)) == E and f"chain {c}: bad arguments" in _lib.last_error()
    assert _rc(thin=0) == E
    assert _rc(n_iter=4, n_burnin=4) == E and "no post-burn-in sample" in _lib.last_error()
    assert _rc(n_iter=(1 << 23) + 1) == E
    # the sets
    for nsets in (0, -1, 4):
        assert _rc(nsets=nsets) == E and "nsets" in _lib.last_error(), nsets
    for name in ("rows", "set_of"):
        assert _rc(null=(name,)) == E and "rows and set_of are required" in _lib.last_error()
    assert _rc(ldrows=19) == E and "ldrows" in _lib.last_error()
    for c, bad in ((0, -1), (1, 2), (2, 7)):
        so = [0, 1, 0]
        so[c] = bad
        assert _rc(set_of=so) == E and f"chain {c}: set_of" in _lib.last_error()
    few = np.zeros((2, 20), dtype=np.uint8)
    few[0, :15] = 1
    few[1, [3, 9]] = 1
    assert _rc(rows=few) == E and "set 1 has fewer than 3 rows" in _lib.last_error()
    byte = few.copy()
    byte[1, :10] = 1
    byte[0, 4] = 2
    assert _rc(rows=byte) == E and "set 0 has a byte other than 0 or 1" in _lib.last_error()
    # phenotypes: a non-finite value counts only inside the chain's set (chain 1 trains on rows 5 .. 19)
    assert _rc(y_nan=(1, 7)) == E and "chain 1: phenotype" in _lib.last_error()
    assert _rc(y_nan=(0, 3)) == E and "chain 0: phenotype" in _lib.last_error()
    assert _rc(y_const=(1, slice(5, 20))) == _lib.GBM_E_DATA and "chain 1: very low" in _lib.last_error()
    assert _rows_stats() == before
    if gbm.device_count() == 0:  # held-out NaN passes the checks: the call gets as far as asking for a device
        assert _rc(y_nan=(1, 2)) == _lib.GBM_E_NODEV
        assert _rows_stats() == (0, 0)


def test_python_arguments():
    X = np.random.default_rng(0).random((20, 30))
    Y = np.random.default_rng(1).random((20, 2))
    sets = np.ones((1, 20), dtype=bool)
    with pytest.raises(gbm.ArgumentError, match="BayesD"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesD"], X, Y, sets, [0, 0])
    with pytest.raises(gbm.ArgumentError, match="1 to 32"):
        gbm.bayes_multi_rows_arrays(["BayesA"] * 33, X, np.zeros((20, 33)), sets, [0] * 33)
    with pytest.raises(gbm.ArgumentError, match="one column"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesB"], X, Y[:, :1], sets, [0, 0])
    with pytest.raises(gbm.ArgumentError, match="boolean or uint8"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesB"], X, Y, np.ones((1, 20)), [0, 0])
    with pytest.raises(gbm.ArgumentError, match="boolean or uint8"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesB"], X, Y, np.ones((1, 19), dtype=bool), [0, 0])
    with pytest.raises(gbm.ArgumentError, match="one set index per chain"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesB"], X, Y, sets, [0])
    with pytest.raises(gbm.ArgumentError, match="chain 1: set_of"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesB"], X, Y, sets, [0, 1])
    with pytest.raises(gbm.ArgumentError, match="set 0 has fewer than 3 rows"):
        gbm.bayes_multi_rows_arrays(["BayesA", "BayesB"], X, Y, np.zeros((1, 20), dtype=np.uint8), [0, 0])


# ---- the precondition of the loop comparisons on the device -------------------------------------------------
@pytest.mark.parametrize("name", rc.LOOP_CASES)
def test_loop_references_keep_their_indicator_margins(name):
    """Every (chain, training rows) that tests/test_gpu_bayes_rows.py compares with the loop at 1e-9: no indicator
    draw of the loop lies within 1e-6 of its threshold (an fp64 rounding difference cannot flip it)."""
    cs = rc.case(name)
    for c, m in enumerate(cs["models"]):
        margin = rc.loop_reference(name, c)["margin"]
        assert m == "BayesA" or margin > 1e-6, (name, c, m, margin)


def test_cross_validation_loops_keep_their_indicator_margins():
    margins = rc.cv_margins()
    assert len(margins) == 18
    for key, margin in margins.items():
        assert key[2] == "BayesA" or margin > 1e-6, (key, margin)


# ---- farming by folds, the fit and the validation stubbed -----------------------------------------------------
def _jobs(models, g, ph, n_folds=3):
    return gbm.cvbulk_setup(genomes=g, phenomes=ph, models=models, n_replications=1, n_folds=n_folds)


def _all_loci(mv, p=90):
    return [(i, m, list(range(p))) for i, m in enumerate(mv)]


def test_fold_grouping_keys_and_shared_sets():
    """The jobs of a trait that share the loci and the schedule are one group whatever their fold; the three models
    of a fold share one set, which is the fold's training rows with a finite phenotype; another schedule or a
    loci subset is a group of its own, and a job that is alone in its group goes to the one-model path."""
    g, ph = mc.panel()
    short = functools.partial(gbm.bayesb, n_iter=9)
    cvs, _, mv = _jobs((gbm.bayesa, gbm.bayesb, gbm.bayesc, short), g, ph)
    assert len(cvs) == 24
    parts, single = gcv._bayes_fold_groups(_all_loci(mv), cvs, g, ph)
    assert single == []
    got = sorted(([ch[0] for ch in part[0]], part[2], part[4:]) for part in parts)
    want = []
    for t in (0, 1):  # per trait: the 9 default-schedule jobs of its folds, and the 3 short ones
        i0 = 12 * t
        want.append(([i0 + 4 * f + m for f in range(3) for m in range(3)], [f for f in range(3) for _ in range(3)],
                     (1500, 500)))
        want.append(([i0 + 4 * f + 3 for f in range(3)], [0, 1, 2], (9, 500)))
    assert got == sorted(want)
    Y = np.asarray(ph.phenotypes)
    for chains, sets, set_of, loci, _, _ in parts:
        assert loci == list(range(90)) and len(sets) == 3
        for (i, name, trait, rows), s in zip(chains, set_of):
            assert name == gcv._bayes_chain(mv[i])[0] and ph.traits[trait] == cvs[i].fit.trait
            assert [g.entries[r] for r in rows] == [e for e in cvs[i].fit.entries
                                                    if np.isfinite(Y[g.entries.index(e), trait])]
            want_set = np.zeros(60, dtype=bool)
            want_set[rows] = True
            assert np.array_equal(sets[s], want_set) and np.isfinite(Y[sets[s], trait]).all()
    # trait t2 has a missing phenotype at entry 7: it is in no set of t2, and in two of the three sets of t1
    t2 = [part for part in parts if part[0][0][2] == 1 and len(part[0]) == 9][0]
    t1 = [part for part in parts if part[0][0][2] == 0 and len(part[0]) == 9][0]
    assert not any(s[7] for s in t2[1]) and sum(bool(s[7]) for s in t1[1]) == 2
    # a loci subset and a lone schedule: jobs that share with nobody keep the one-model path
    jobs = _all_loci(mv)[:12]
    jobs[1] = (1, mv[1], list(range(10, 80)))
    jobs[3] = (3, functools.partial(gbm.bayesb, n_iter=7), list(range(90)))
    parts, single = gcv._bayes_fold_groups(jobs, cvs, g, ph)
    assert sorted(i for i, _, _ in single) == [1, 3] and single[0][2] in (list(range(10, 80)), list(range(90)))
    assert sorted(len(part[0]) for part in parts) == [2, 8]


def test_fold_groups_split_at_32_chains_keeping_a_set_together():
    g, ph = mc.panel()
    models = tuple([gbm.bayesa, gbm.bayesb, gbm.bayesc] * 4)  # 12 chains per fold, 3 folds per trait
    cvs, _, mv = _jobs(models, g, ph)
    cvs, mv = cvs[:36], mv[:36]  # trait t1
    parts, single = gcv._bayes_fold_groups(_all_loci(mv), cvs, g, ph)
    assert single == []
    assert [[ch[0] for ch in part[0]] for part in parts] == [list(range(24)), list(range(24, 36))]
    assert [part[2] for part in parts] == [[0] * 12 + [1] * 12, [0] * 12] and [len(part[1]) for part in parts] == [2, 1]
    # one set with more chains than a call holds fills calls of its own
    cvs40, mv40 = [cvs[0]] * 40, [mv[0]] * 40
    parts, _ = gcv._bayes_fold_groups(_all_loci(mv40), cvs40, g, ph)
    assert [len(part[0]) for part in parts] == [32, 8] and all(len(part[1]) == 1 for part in parts)


def test_cvmultithread_routes_folds_and_records_errors(monkeypatch, capsys):
    """With bayes_folds the jobs of a trait go to one rows fit (stubbed) over all entries; each job's Fit holds its
    own rows of the call's columns and is validated (stubbed); the unshared job keeps its own model call; a
    group's error is recorded for each of its jobs. Without bayes_folds the rows fit is never called."""
    g, ph = mc.panel()
    seen, called = [], []

    def other_model(**kw):
        called.append(kw["idx_trait"])
        raise gbm.GBMError("other path")

    def fake_rows(models, X, Y, sets, set_of, *, n_iter, n_burnin):
        seen.append((tuple(models), X.shape, Y.shape, np.asarray(sets).shape, tuple(set_of), n_iter, n_burnin))
        if np.isnan(Y[7, 0]):  # trait t2's column
            raise gbm.ArgumentError("trait two fails")
        T = len(models)
        b_hat = np.arange(91.0)[:, None] + 1000.0 * np.arange(T)
        y_pred = np.arange(60.0)[:, None] + 100.0 * np.arange(T)
        return b_hat, y_pred, np.zeros((3, T)), np.zeros((90, T))

    def fake_validate(fit, genomes, phenomes, *, idx_validation, replication, fold):
        if fit.model == "bayesc":
            raise gbm.GBMError("validation fails")
        return ("cv", fit, len(idx_validation), replication, fold)

    monkeypatch.setattr(gbm.bayes, "bayes_multi_rows_arrays", fake_rows)
    monkeypatch.setattr(gcv, "validate", fake_validate)
    models = (gbm.bayesa, gbm.bayesc, other_model)
    cvs, _, mv = _jobs(models, g, ph, n_folds=2)
    assert len(cvs) == 12
    placeholders = list(cvs)
    gbm.cvmultithread(cvs, genomes=g, phenomes=ph, models_vector=mv, verbose=True, devices=[0], bayes_folds=True)
    errors = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Warning")]
    four = ("BayesA", "BayesC", "BayesA", "BayesC")
    assert seen == [(four, (60, 90), (60, 4), (2, 60), (0, 0, 1, 1), 1500, 500)] * 2
    assert called == [1, 1, 2, 2]
    pos = {e: k for k, e in enumerate(g.entries)}
    for c, i in enumerate((0, 3)):  # the BayesA jobs of trait t1: chains 0 and 2 of the call
        tag, fit, nv, rep, fold = cvs[i]
        p0 = placeholders[i]
        rows = np.array([pos[e] for e in p0.fit.entries])
        assert tag == "cv" and (nv, rep, fold) == (len(p0.validation_entries), p0.replication, p0.fold)
        assert fit.model == "bayesa" and fit.trait == "t1" and fit.entries == p0.fit.entries
        assert fit.populations == p0.fit.populations and fit.b_hat_labels == p0.fit.b_hat_labels
        assert np.array_equal(fit.y_pred, rows + 200.0 * c) and np.array_equal(fit.b_hat, np.arange(91.0) + 2000.0 * c)
        assert np.array_equal(fit.y_true, np.asarray(ph.phenotypes)[rows, 0]) and fit.checkdims()
        assert set(fit.metrics) == set(gbm.metrics(fit.y_true, fit.y_pred))
    assert all(cvs[i] is placeholders[i] for i in (1, 2, 4, 5, 6, 7, 8, 9, 10, 11))
    assert sorted(errors) == sorted(
        [f"Warning: model fitting error in cross-validation job {k}: {msg}" for k, msg in
         ((2, "validation fails"), (5, "validation fails"), (3, "other path"), (6, "other path"), (9, "other path"),
          (12, "other path"), (7, "trait two fails"), (8, "trait two fails"), (10, "trait two fails"),
          (11, "trait two fails"))])
    # off by default: the rows fit is not reached
    seen.clear()
    monkeypatch.setattr(gbm.bayes, "bayes_multi_pairs", lambda *a, **k: (_ for _ in ()).throw(gbm.GBMError("multi")))
    cvs2, _, mv2 = _jobs((gbm.bayesa, gbm.bayesc), g, ph, n_folds=2)
    gbm.cvmultithread(cvs2, genomes=g, phenomes=ph, models_vector=mv2, devices=[0])
    assert seen == []
