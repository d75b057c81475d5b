"""CPU side of the multi-chain BayesA/B/C fit (libgbm ``gbm_bayes_fit_multi``, ``gbm.bayes_multi_arrays``, the
grouping of ``gbm.cvmultithread``): every refusal comes back as GBM_E_ARG before any device call, with the chain
named where a chain's own argument is at fault; and the farming's grouping keys, its split at 32 chains and its
error recording, with the fit and the validation stubbed. The device tests: tests/test_gpu_bayes_multi.py."""
import ctypes
import functools

import numpy as np
import pytest

import gbm
from gbm import _lib
from gbm import cv as gcv

import bayes_multi_cases as mc

E = _lib.GBM_E_ARG


def _rc(T=3, n=20, p=30, models=None, n_iter=10, n_burnin=2, thin=1, ldy=None, ldb=None, ldp=None, ldpip=None,
        null=(), y_nan=None, y_const=None, **priors):
    """gbm_bayes_fit_multi on valid arguments with the named ones replaced; ``priors``: name -> (chain, value)."""
    X = np.asfortranarray(np.random.default_rng(0).random((n, p)))
    Y = np.asfortranarray(np.random.default_rng(1).random((n, max(T, 1))))
    if y_nan is not None:
        Y[4, y_nan] = np.nan
    if y_const is not None:
        Y[:, y_const] = 1.0
    Tn = max(T, 1)
    arr = {"models": np.array(models if models is not None else [1 + c % 3 for c in range(Tn)], dtype=np.intc),
           "r2": np.full(Tn, 0.5), "df0": np.full(Tn, 5.0), "prob_in": np.full(Tn, 0.5), "counts": np.full(Tn, 10.0),
           "seeds": np.arange(Tn, dtype=np.uint64), "X": X, "Y": Y, "b_hat": np.zeros((p + 1, Tn), order="F"),
           "y_pred": np.zeros((n, Tn), order="F"), "var": np.zeros((3, Tn), order="F"),
           "pip": np.zeros((p, Tn), order="F")}
    for name, (c, v) in priors.items():
        arr[name][c] = v
    a = {k: (None if k in null else _lib.ptr(v)) for k, v in arr.items()}
    lib = gbm.load_library()
    return lib.gbm_bayes_fit_multi(T, a["models"], a["X"], n, p, n, a["Y"], n if ldy is None else ldy, n_iter,
                                   n_burnin, thin, a["r2"], a["df0"], a["prob_in"], a["counts"], a["seeds"], 0,
                                   a["b_hat"], p + 1 if ldb is None else ldb, a["y_pred"], n if ldp is None else ldp,
                                   a["var"], a["pip"], p if ldpip is None else ldpip)


def test_arguments_are_refused_before_device_use():
    assert "gbm_bayes_fit_multi" in _lib.EXPORTS and "gbm_debug_bayes_multi_stats" in _lib.EXPORTS
    for T in (0, -1, 33):
        assert _rc(T=T) == E
        assert "nchains" in _lib.last_error()
    for name in ("models", "X", "Y", "r2", "df0", "prob_in", "counts", "seeds", "b_hat"):
        assert _rc(null=(name,)) == E, name
        assert "required" in _lib.last_error()
    for kw in (dict(ldy=19), dict(ldb=30), dict(ldp=19), dict(ldpip=29)):
        assert _rc(**kw) == E, kw
        assert "pitch" in _lib.last_error()
    assert _rc(ldp=0, ldpip=0, null=("y_pred", "pip")) != E  # pitches of outputs not asked for are not read
    # a chain's own model, priors and phenotypes: the chain is named (0-based)
    for c in (0, 2):
        for bad in (0, 4, -1):
            m = [1, 2, 3]
            m[c] = bad
            assert _rc(models=m) == E
            assert f"chain {c}: model" in _lib.last_error()
        for name, v in (("df0", 0.5), ("prob_in", 0.0), ("prob_in", 1.0), ("prob_in", 0.05), ("prob_in", 0.95),
                        ("counts", 1.5)):
            assert _rc(**{name: (c, v)}) == E, (c, name, v)
            assert f"chain {c}: bad prior" in _lib.last_error()
        assert _rc(r2=(c, 1.0)) == E and f"chain {c}: bad arguments" in _lib.last_error()
        assert _rc(y_nan=c) == E and f"chain {c}: phenotype" in _lib.last_error()
        assert _rc(y_const=c) == _lib.GBM_E_DATA and f"chain {c}: very low" in _lib.last_error()
    # the common schedule and shape (gbm_bayes_fit's checks)
    assert _rc(thin=0) == E
    assert _rc(n_iter=4, n_burnin=4) == E and "no post-burn-in sample" in _lib.last_error()
    assert _rc(n_iter=(1 << 23) + 1) == E
    assert _rc(n=2) == E
    calls, chains = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert gbm.load_library().gbm_debug_bayes_multi_stats(ctypes.byref(calls), ctypes.byref(chains)) == 0
    if gbm.device_count() == 0:  # (on a device other tests' fits count too)
        assert (calls.value, chains.value) == (0, 0)


def test_python_arguments():
    X = np.random.default_rng(0).random((20, 30))
    Y = np.random.default_rng(1).random((20, 2))
    with pytest.raises(gbm.ArgumentError, match="BayesD"):
        gbm.bayes_multi_arrays(["BayesA", "BayesD"], X, Y)
    with pytest.raises(gbm.ArgumentError, match="1 to 32"):
        gbm.bayes_multi_arrays(["BayesA"] * 33, X, np.zeros((20, 33)))
    with pytest.raises(gbm.ArgumentError, match="one column"):
        gbm.bayes_multi_arrays(["BayesA", "BayesB"], X, Y[:, :1])
    with pytest.raises(gbm.ArgumentError, match="one entry per chain"):
        gbm.bayes_multi_arrays(["BayesA", "BayesB"], X, Y, seeds=[1, 2, 3])
    with pytest.raises(gbm.ArgumentError, match="chain 1: bad prior"):
        gbm.bayes_multi_arrays(["BayesA", "BayesB"], X, Y, prob_in=[0.5, 1.5])


# ---- farming, the fit and the validation stubbed -----------------------------------------------------------
def _jobs(models, g, ph, n_folds=2):
    return gbm.cvbulk_setup(genomes=g, phenomes=ph, models=models, n_replications=1, n_folds=n_folds)


def test_bayes_model_callables_are_recognised():
    assert gcv._bayes_chain(gbm.bayesa) == ("BayesA", 1500, 500)
    assert gcv._bayes_chain(functools.partial(gbm.bayesc, n_iter=30)) == ("BayesC", 30, 500)
    assert gcv._bayes_chain(functools.partial(gbm.bayesb, n_burnin=7, n_iter=9)) == ("BayesB", 9, 7)
    assert gcv._bayes_chain(functools.partial(gbm.bayesb, verbose=True)) is None
    assert gcv._bayes_chain(functools.partial(gbm.bayesb, None)) is None
    assert gcv._bayes_chain(gbm.gblup) is None and gcv._bayes_chain(gbm.bayesian) is None
    assert gcv._bayes_chain(lambda **kw: None) is None


def test_grouping_keys():
    """Jobs share a fit when the training entries, the loci, the training rows after the missing-phenotype drop
    and the schedule are equal: the three models of a (trait, fold); not another fold, another trait (its own
    fold permutation), another n_iter or n_burnin, a loci subset, or a trait whose missing cell is in the set."""
    g, ph = mc.panel()
    short = functools.partial(gbm.bayesb, n_iter=9)
    models = (gbm.bayesa, gbm.bayesb, gbm.bayesc, short, functools.partial(gbm.bayesb, n_burnin=9))
    cvs, _, mv = _jobs(models, g, ph)
    assert len(cvs) == 20
    jobs = [(i, m, list(range(90))) for i, m in enumerate(mv)]
    parts, single = gcv._bayes_groups(jobs, cvs, g, ph)
    assert sorted([jb[0] for jb in part] for part in parts) == [[0, 1, 2], [5, 6, 7], [10, 11, 12], [15, 16, 17]]
    assert sorted(i for i, _, _ in single) == [3, 4, 8, 9, 13, 14, 18, 19]
    for part in parts:
        assert [jb[1] for jb in part] == ["BayesA", "BayesB", "BayesC"] and part[0][5:] == (1500, 500)
    # a loci subset: its own key
    jobs[1] = (1, mv[1], list(range(10, 80)))
    parts, single = gcv._bayes_groups(jobs, cvs, g, ph)
    assert [0, 2] in [[jb[0] for jb in part] for part in parts] and 1 in [i for i, _, _ in single]
    # the same entries for both traits, trait t2's missing cell among them: the rows after the drop differ
    cvs2, _, mv2 = _jobs((gbm.bayesa,), g, ph)
    assert [cv.fit.trait for cv in cvs2] == ["t1", "t1", "t2", "t2"]
    k = 0 if "e7" in cvs2[0].fit.entries else 1  # the fold of t1 that trains on e7
    cvs2, mv2 = [cvs2[k], cvs2[2]], [mv2[k], mv2[2]]
    cvs2[1].fit.entries = list(cvs2[0].fit.entries)
    assert "e7" in cvs2[0].fit.entries
    parts, single = gcv._bayes_groups([(0, mv2[0], list(range(90))), (1, mv2[1], list(range(90)))], cvs2, g, ph)
    assert parts == [] and len(single) == 2
    cvs2[1].fit.entries = [e for e in cvs2[0].fit.entries if e != "e7"]
    cvs2[0].fit.entries = list(cvs2[1].fit.entries)
    parts, single = gcv._bayes_groups([(0, mv2[0], list(range(90))), (1, mv2[1], list(range(90)))], cvs2, g, ph)
    assert [[jb[0] for jb in part] for part in parts] == [[0, 1]] and [jb[2] for jb in parts[0]] == [0, 1]


def test_groups_split_at_32_chains():
    g, ph = mc.panel()
    models = tuple([gbm.bayesa, gbm.bayesb, gbm.bayesc] * 14)  # 42 jobs on one training set
    cvs, _, mv = _jobs(models, g, ph)
    cvs, mv = cvs[:42], mv[:42]  # trait t1, fold 1
    parts, single = gcv._bayes_groups([(i, m, list(range(90))) for i, m in enumerate(mv)], cvs, g, ph)
    assert [len(part) for part in parts] == [32, 10] and single == []
    assert [jb[0] for part in parts for jb in part] == list(range(42))


def test_cvmultithread_routes_and_records_errors(monkeypatch, capsys):
    """cvmultithread hands each group to one multi fit (stubbed), validates per job (stubbed), leaves the unshared
    job to its own model call, and records a group's error for each of its jobs."""
    g, ph = mc.panel()
    seen, called = [], []

    def other_model(**kw):
        called.append(kw["idx_trait"])
        raise gbm.GBMError("other path")

    def fake_pairs(pairs, genomes, phenomes, idx_entries, idx_loci_alleles, n_iter, n_burnin, verbose=False):
        seen.append((tuple(pairs), len(idx_entries), len(idx_loci_alleles), n_iter, n_burnin))
        if pairs[0][1] == 2:
            raise gbm.ArgumentError("trait two fails")
        return [("fit", m, t) for m, t in pairs]

    def fake_validate(fit, genomes, phenomes, *, idx_validation, replication, fold):
        if fit[1] == "BayesC":
            raise gbm.GBMError("validation fails")
        return ("cv",) + fit[1:] + (len(idx_validation), replication, fold)

    monkeypatch.setattr(gbm.bayes, "bayes_multi_pairs", fake_pairs)
    monkeypatch.setattr(gcv, "validate", fake_validate)
    models = (gbm.bayesa, functools.partial(gbm.bayesb, n_iter=1500), gbm.bayesc, other_model)
    cvs, _, mv = _jobs(models, g, ph)
    assert len(cvs) == 16
    cvs, mv = cvs[0:4] + cvs[8:12], mv[0:4] + mv[8:12]  # fold 1 of t1 and of t2
    placeholders = list(cvs)
    gbm.cvmultithread(cvs, genomes=g, phenomes=ph, models_vector=mv, verbose=True, devices=[0])
    errors = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Warning")]
    n1, n2 = len(placeholders[0].fit.entries), len(placeholders[4].fit.entries)
    assert seen == [((("BayesA", 1), ("BayesB", 1), ("BayesC", 1)), n1, 90, 1500, 500),
                    ((("BayesA", 2), ("BayesB", 2), ("BayesC", 2)), n2, 90, 1500, 500)]
    assert called == [1, 2]
    nv = len(placeholders[0].validation_entries)
    assert cvs[0] == ("cv", "BayesA", 1, nv, "replication_1", "fold_1") and cvs[1][:3] == ("cv", "BayesB", 1)
    assert all(cvs[i] is placeholders[i] for i in (2, 3, 4, 5, 6, 7))
    assert sorted(errors) == sorted(
        [f"Warning: model fitting error in cross-validation job {k}: {msg}" for k, msg in
         ((3, "validation fails"), (4, "other path"), (5, "trait two fails"), (6, "trait two fails"),
          (7, "trait two fails"), (8, "other path"))])
