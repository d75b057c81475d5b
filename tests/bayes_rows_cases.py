"""Inputs and comparisons of the tests of the multi-chain BayesA/B/C fit with a training set per chain (libgbm
``gbm_bayes_fit_multi_rows``, ``gbm.bayes_multi_rows_arrays``, ``cvbulk(..., bayes_folds=True)``):
tests/test_gpu_bayes_rows.py on the device, tests/test_bayes_rows.py on the CPU. A case is a dict of the call's
arguments; its loop references (``bayes_abc_ref.bayes_gibbs`` on the chain's rows alone) are computed once and
shared. Not a test module."""
import functools

import numpy as np

import gbm
import oracle

import bayes_abc_ref
import bayes_multi_cases as mc
import gibbs_cases as gc

OUTPUTS = gc.OUTPUTS
ABC = ("BayesA", "BayesB", "BayesC")
CV_SCHEDULE = dict(n_iter=12, n_burnin=4)  # of the cross-validation case (thin = 5: the model functions' default)


def _case(X, Y, sets, set_of, models, seeds, schedule=gc.DEFAULT):
    sets = np.ascontiguousarray(np.asarray(sets, dtype=bool))
    X, Y = np.asfortranarray(X), np.asfortranarray(Y)
    for a in (X, Y, sets):
        a.setflags(write=False)
    return dict(X=X, Y=Y, sets=sets, set_of=tuple(int(s) for s in set_of), models=tuple(models), seeds=tuple(seeds),
                schedule=schedule)


def fold_sets(folds, n_folds):
    """The training sets of a fold assignment (values 1 .. n_folds): set s holds the rows outside fold s + 1."""
    return np.stack([folds != s + 1 for s in range(n_folds)])


def _folds15(folds):
    """5 sets x models A, B, C: 15 chains, set_of = c // 3, phenotype column and seed of slot c."""
    X, Y = mc.inputs("dosage", 300, 150)
    T = 15
    return _case(X, Y[:, :T], fold_sets(folds, 5), [c // 3 for c in range(T)], [ABC[c % 3] for c in range(T)],
                 [mc.seed_of(c) for c in range(T)])


def _degenerate():
    """(120, 70): marker 3 is zero on the training rows but not on the held-out ones, marker 66 (second block) is
    constant on the training rows; rows 5, 17, ... are held out."""
    n, p = 120, 70
    X = np.array(oracle.synth_genotypes(91, n, p))
    train = np.arange(n) % 6 != 5
    X[train, 3] = 0.0
    X[~train, 3] = 1.0
    X[train, 66] = 0.5
    X[~train, 66] = np.where(np.arange((~train).sum()) % 2 == 0, 0.0, 1.0)
    Y = oracle.synth_phenotypes(X, 92, ntraits=3)
    return _case(X, Y, train[None, :], [0, 0, 0], ABC, [11, 12, 13])


@functools.lru_cache(maxsize=None)
def case(name):
    """The cases that are compared with the literal loop (their indicator margins: tests/test_bayes_rows.py)."""
    if name == "mod5":
        return _folds15(np.arange(300) % 5 + 1)
    if name == "random5":  # with replacement, as gbm.fold_assignments draws it
        return _folds15(gbm.fold_assignments(300, 5, 1, 1, 42)[0, 0])
    if name == "chunk_out":  # n = 600, rows 256 .. 511 held out: a whole chunk workgroup contributes zeros
        X = oracle.synth_genotypes(95, 600, 70)
        Y = oracle.synth_phenotypes(X, 96, ntraits=3)
        keep = np.ones(600, dtype=bool)
        keep[256:512] = False
        return _case(X, Y, keep[None, :], [0, 0, 0], ABC, [21, 22, 23])
    if name == "three_rows":  # n_c = 3 at (300, 65)
        X = oracle.synth_genotypes(97, 300, 65)
        Y = oracle.synth_phenotypes(X, 98, ntraits=3)
        keep = np.zeros(300, dtype=bool)
        keep[[7, 255, 256]] = True
        return _case(X, Y, keep[None, :], [0, 0, 0], ABC, [31, 32, 33], (6, 2, 1))
    if name == "four_by_one":  # (4, 1) with one row held out
        X = np.array([[0.0], [0.5], [1.0], [0.5]])
        Y = np.array([[0.3, -0.2, 1.1], [1.4, 0.1, 0.2], [2.2, 0.9, -0.7], [9.0, 9.0, 9.0]])
        return _case(X, Y, [[True, True, True, False]], [0, 0, 0], ABC, [41, 42, 43], (6, 2, 1))
    if name == "degenerate":
        return _degenerate()
    raise KeyError(name)


LOOP_CASES = ("mod5", "random5", "chunk_out", "three_rows", "four_by_one", "degenerate")


@functools.lru_cache(maxsize=None)
def loop_reference(name, c):
    """``bayes_gibbs`` of chain c of a case on its training rows alone (read-only)."""
    cs = case(name)
    rows = cs["sets"][cs["set_of"][c]]
    n_iter, n_burnin, thin = cs["schedule"]
    r = bayes_abc_ref.bayes_gibbs(cs["models"][c], cs["X"][rows], cs["Y"][rows, c], n_iter=n_iter, n_burnin=n_burnin,
                                  thin=thin, seed=cs["seeds"][c])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def fit(cs, **over):
    """gbm.bayes_multi_rows_arrays of a case (``over`` replaces arguments)."""
    a = dict(cs, **over)
    n_iter, n_burnin, thin = a["schedule"]
    return gbm.bayes_multi_rows_arrays(a["models"], a["X"], a["Y"], a["sets"], a["set_of"], n_iter=n_iter,
                                       n_burnin=n_burnin, thin=thin, seeds=list(a["seeds"]))


WAYS = tuple((storage, per_row) for storage in ("bytes", "fp64") for per_row in ("4", "1"))


def fit_all_ways(gbm_env, cs, **over):
    """The fit with byte and with fp64 genotype storage (GBM_BRR_I8) and with four chains and one chain per
    workgroup row forced (GBM_BAYES_MULTI_WG): the four results are equal bit for bit; returns the first."""
    first = None
    for storage, per_row in WAYS:
        gbm_env.setenv("GBM_BRR_I8", "1" if storage == "bytes" else "0")
        gbm_env.setenv("GBM_BAYES_MULTI_WG", per_row)
        outs = fit(cs, **over)
        if first is None:
            first = outs
        else:
            mc.assert_same_bits(outs, first, (storage, per_row, "vs", WAYS[0]))
    return first


def rel(a, b):
    """``gibbs_cases.rel``, the largest difference relative to the reference's largest magnitude; the difference
    itself where the reference is all zeros (the PIP of a marker that is never included), never NaN."""
    a, b = np.asarray(a), np.asarray(b)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / (scale if scale > 0.0 else 1.0))


def worst_against_loop(name, outs):
    """Per output, the largest relative error (``rel``) of any chain of ``outs`` against its loop on the
    training rows (y_pred at those rows), and the largest relative difference of y_pred at the held-out rows from
    b_hat[0] + X b_hat[1:] there (0 when no row is held out)."""
    cs = case(name)
    b_hat, y_pred, var, pip = outs
    worst = dict.fromkeys(OUTPUTS + ("held_out",), 0.0)
    for c in range(len(cs["models"])):
        rows = cs["sets"][cs["set_of"][c]]
        ref = loop_reference(name, c)
        got = {"b_hat": b_hat[:, c], "y_pred": y_pred[rows, c], "var": var[:, c], "pip": pip[:, c]}
        for k in OUTPUTS:
            worst[k] = max(worst[k], rel(got[k], ref[k]))
        if not rows.all():
            want = b_hat[0, c] + cs["X"][~rows] @ b_hat[1:, c]
            worst["held_out"] = max(worst["held_out"], rel(y_pred[~rows, c], want))
    return worst


# ---- the cross-validation case --------------------------------------------------------------------------------
def cv_models():
    return tuple(functools.partial(f, **CV_SCHEDULE) for f in (gbm.bayesa, gbm.bayesb, gbm.bayesc))


def cv_kwargs():
    g, ph = mc.panel()
    return dict(genomes=g, phenomes=ph, models=cv_models(), n_replications=1, n_folds=3)


def cv_margins():
    """The loop's indicator margin of every (trait, fold, model) of the cross-validation case."""
    kw = cv_kwargs()
    g, ph = kw["genomes"], kw["phenomes"]
    cvs, _, mv = gbm.cvbulk_setup(**kw)
    X, Y = np.asarray(g.allele_frequencies), np.asarray(ph.phenotypes)
    out = {}
    for cv, model in zip(cvs, mv):
        rows = [g.entries.index(e) for e in cv.fit.entries]
        t = ph.traits.index(cv.fit.trait)
        name = {"bayesa": "BayesA", "bayesb": "BayesB", "bayesc": "BayesC"}[model.func.__name__]
        r = bayes_abc_ref.bayes_gibbs(name, X[rows], Y[rows, t], **CV_SCHEDULE)
        out[(cv.fit.trait, cv.fold, name)] = r["margin"]
    return out
