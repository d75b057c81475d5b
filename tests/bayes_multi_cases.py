"""Inputs and comparisons of the multi-chain BayesA/B/C tests (tests/test_gpu_bayes_multi.py on the device,
tests/test_bayes_multi.py on the CPU): the chains of a fit (model, phenotype column, seed per slot), the single
fits they are compared with (each run once per storage and shared), field-by-field equality of Fits and CVs,
and a small two-trait panel. Not a test module."""
import dataclasses
import functools

import numpy as np

import gbm
import oracle

import gibbs_cases as gc

OUTPUTS = gc.OUTPUTS  # b_hat, y_pred, var, pip
PATTERN = ("BayesA", "BayesB", "BayesC", "BayesB")  # of a workgroup's four slots; rotated from row to row
TMAX = 32


def model_of(c):
    return PATTERN[(c + c // 4) % 4]


def seed_of(c):
    return 1000 + 7 * c


@functools.lru_cache(maxsize=None)
def inputs(kind, n, p):
    """(X, Y) with 32 phenotype columns (a fit of T chains takes the first T), read-only. ``dosage``: k/2
    genotypes (byte storage by default); ``scaled``: X·0.3 + 0.05 (fp64 storage whatever GBM_BRR_I8 says);
    ``tiny``: gibbs_cases' n = 3, p = 1."""
    if kind == "tiny":
        X, y = gc.case("tiny")
        assert X.shape == (n, p)
        Y = y[:, None] + np.random.default_rng(5).standard_normal((n, TMAX))
    else:
        X = oracle.synth_genotypes(61 + p, n, p)
        if kind == "scaled":
            X = X * 0.3 + 0.05
        Y = oracle.synth_phenotypes(X, 62, ntraits=TMAX)
    X = np.asfortranarray(X)
    Y = np.asfortranarray(Y)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


_SINGLE = {}


def single(kind, n, p, c, schedule, storage):
    """gbm.bayes_arrays of chain c's (model, column, seed), run once per (input, chain, schedule, storage); the
    caller has the storage set (``storage`` only keys the cache)."""
    key = (kind, n, p, c, schedule, storage)
    if key not in _SINGLE:
        X, Y = inputs(kind, n, p)
        n_iter, n_burnin, thin = schedule
        _SINGLE[key] = gbm.bayes_arrays(model_of(c), X, Y[:, c], n_iter=n_iter, n_burnin=n_burnin, thin=thin,
                                        seed=seed_of(c))
    return _SINGLE[key]


def multi(kind, n, p, T, schedule):
    X, Y = inputs(kind, n, p)
    n_iter, n_burnin, thin = schedule
    return gbm.bayes_multi_arrays([model_of(c) for c in range(T)], X, Y[:, :T], n_iter=n_iter, n_burnin=n_burnin,
                                  thin=thin, seeds=[seed_of(c) for c in range(T)])


def chain(outs, c):
    """Chain c's (b_hat, y_pred, var, pip) of a multi fit's outputs."""
    return tuple(a[:, c] for a in outs)


def assert_same_bits(got, want, what):
    for name, a, b in zip(OUTPUTS, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name, float(np.abs(a - b).max()))


def same_fit(a, b):
    """Every field of two Fits equal, arrays bit for bit."""
    for f in dataclasses.fields(a):
        u, v = getattr(a, f.name), getattr(b, f.name)
        if isinstance(u, np.ndarray):
            if not (isinstance(v, np.ndarray) and u.shape == v.shape and np.array_equal(u, v)):
                return False
        elif isinstance(u, dict):
            if set(u) != set(v) or any(not np.array_equal(u[k], v[k], equal_nan=True) for k in u):
                return False
        elif u != v:
            return False
    return True


def same_cv(a, b):
    if not same_fit(a.fit, b.fit):
        return False
    if (a.replication, a.fold, a.validation_populations, a.validation_entries) != (
            b.replication, b.fold, b.validation_populations, b.validation_entries):
        return False
    if not (np.array_equal(a.validation_y_true, b.validation_y_true)
            and np.array_equal(a.validation_y_pred, b.validation_y_pred)):
        return False
    return set(a.metrics) == set(b.metrics) and all(
        np.array_equal(a.metrics[k], b.metrics[k], equal_nan=True) for k in a.metrics)


def panel(n=60, p=90, missing=((7, 1),)):
    """Genomes and Phenomes of n entries x p loci with two traits; ``missing``: (entry, trait) cells set to NaN."""
    X = oracle.synth_genotypes(83, n, p)
    Y = oracle.synth_phenotypes(X, 84, ntraits=2, qtl_frac=0.05)
    for i, t in missing:
        Y[i, t] = np.nan
    ent = [f"e{i}" for i in range(n)]
    g = gbm.Genomes(ent, ["pop"] * n, [f"l{j}" for j in range(p)], X)
    ph = gbm.Phenomes(list(ent), ["pop"] * n, ["t1", "t2"], Y)
    return g, ph
