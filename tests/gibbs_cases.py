"""Inputs and cached references of the Gibbs samplers' edge tests (tests/test_gibbs_cases.py on the
CPU, tests/test_gpu_gibbs_edges.py on the device): byte storage at scales 4 and 1, bytes >= 128, a
dyadic value that fits no byte, thinned schedules, degenerate columns, the smallest shapes the ABI
accepts, p > 4096 and the shapes at both edges of the BRR super-block sweep. The references are
the literal one-marker-at-a-time loops (oracle.brr_gibbs, bayes_abc_ref.bayes_gibbs). Every array
is built once and is read-only. Not a test module."""
import functools

import numpy as np

import oracle

import bayes_abc_ref

SAMPLERS = ("BRR", "BayesA", "BayesB", "BayesC")
SEED = 99  # of every fit
SWEEP_CUS = 256  # the sweep's shapes below (1009 / 1008, `over`) are those of a 256-CU device

DEFAULT = (9, 2, 1)  # (n_iter, n_burnin, thin)
SCHEDULES = {"tiny": (6, 2, 1), "wide48": (3, 1, 1), "wide1009": (3, 1, 1), "over": (3, 1, 1)}
# schedule -> the 1-based iterations whose state is sampled
THINNING = {(13, 4, 3): (6, 9, 12),  # nsum = 3
            (9, 4, 2): (6, 8),  # nsum = 2: iteration 4 is excluded by the strict i > n_burnin
            (7, 0, 7): (7,)}  # nsum = 1: the last state

# storage the device chooses by itself: the byte scale s (X·s stored as bytes), None for fp64
STORAGE = {"tetra": 4, "counts": 1, "overflow": None, "plain300": 2, "plain1009": 2, "plain1008": 2,
           "degenerate": 2, "tiny": 2, "tiny63": 2, "wide48": 2, "wide1009": 2, "counts1009": 1, "over": 2}
BRR_ONLY = ("plain1009", "plain1008", "wide1009", "counts1009", "over")
SAME_PATH = ("tetra", "counts", "overflow", "degenerate", "tiny", "tiny63", "wide48")  # all four samplers


def schedule_of(name):
    return SCHEDULES.get(name, DEFAULT)


def over_n(cus=SWEEP_CUS):
    """One individual more than the super-block sweep takes (48 per workgroup, <= 256 workgroups)."""
    return 48 * min(cus, SWEEP_CUS) + 1


def _build(name, cus):
    if name == "tetra":  # tetraploid k/4: bytes 0..4 at scale 4
        rng = np.random.default_rng(401)
        f = rng.uniform(0.05, 0.95, 130)
        return rng.binomial(4, f, (300, 130)) / 4.0
    if name in ("counts", "counts1009"):  # scale 1; 40 cells in [128, 255], one of them 255 (1009: on the sweep)
        n = 300 if name == "counts" else 1009
        rng = np.random.default_rng(402 if name == "counts" else 404)
        X = rng.poisson(1.5, (n, 130)).astype(np.float64)
        cells = rng.choice(X.size, 40, replace=False)
        vals = rng.integers(128, 256, 40)
        vals[0] = 255
        X.flat[cells] = vals
        return X
    if name == "overflow":  # dyadic, but 128.5·s fits a byte at no s in (2, 4, 1): fp64 storage
        rng = np.random.default_rng(403)
        X = oracle.synth_genotypes(191, 300, 130)
        X[rng.integers(300), rng.integers(130)] = 128.5
        return X
    if name == "plain300":
        return oracle.synth_genotypes(191, 300, 130)
    if name == "plain1009":  # the first shape of the sweep: 63 chunks of 16 and one of 1 individual
        return oracle.synth_genotypes(191, 1009, 130)
    if name == "plain1008":  # 63 chunks: 10 rows of a super-block each, more than the sweep's 8
        return oracle.synth_genotypes(191, 1008, 130)
    if name == "degenerate":
        X = oracle.synth_genotypes(191, 300, 130)
        X[:, 5] = 0.0  # x2 = 0 (a draw from the prior), in the first half-block
        X[:, 64] = 0.5  # constant, the first column of the second half-block
        X[:, 70] = X[:, 69]  # an exact duplicate pair: a singular Gram block
        X[:, 129] = 1.0  # constant, the last column of the ragged block
        return X
    if name == "tiny":  # n = 3, p = 1: the smallest the ABI accepts
        return np.array([[0.0], [0.5], [1.0]])
    if name == "tiny63":  # one block, one marker short of full
        return oracle.synth_genotypes(124, 17, 63)
    if name == "wide48":  # p > 4096: the strides of the column statistics and the quantiser
        return oracle.synth_genotypes(7, 48, 4200)
    if name == "wide1009":  # p > 4096 on the sweep: nsb = 9 super-blocks
        return oracle.synth_genotypes(7, 1009, 4200)
    if name == "over":
        return oracle.synth_genotypes(191, over_n(cus), 130)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, cus=SWEEP_CUS):
    """(X, y) of a named input, Fortran-ordered and read-only; ``cus`` matters to "over" alone."""
    X = np.asfortranarray(_build(name, cus), dtype=np.float64)
    if name == "tiny":
        y = np.array([0.3, -1.0, 2.0])
    else:
        y = oracle.synth_phenotypes(X, 62)[:, 0]
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def loop(sampler, X, y, schedule):
    """The literal loop of ``sampler`` as {b_hat, y_pred, var, pip, margin} (+ b_last, mu_last for BRR)."""
    n_iter, n_burnin, thin = schedule
    if sampler == "BRR":
        r = oracle.brr_gibbs(X, y, n_iter=n_iter, n_burnin=n_burnin, thin=thin, seed=SEED)
        return {"b_hat": r["b_hat"], "y_pred": r["y_pred"], "var": np.array([r["varE"], r["varB"]]), "pip": None,
                "margin": np.inf, "b_last": r["b_last"], "mu_last": r["mu_last"]}
    return bayes_abc_ref.bayes_gibbs(sampler, X, y, n_iter=n_iter, n_burnin=n_burnin, thin=thin, seed=SEED)


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference(sampler, name, schedule=None, cus=SWEEP_CUS):
    X, y = case(name, cus)
    return _freeze(loop(sampler, X, y, schedule or schedule_of(name)))


@functools.lru_cache(maxsize=None)
def permuted_reference(sampler, name, schedule=None, cus=SWEEP_CUS):
    """The loop on the individuals in another order (rows of X and of y): the same chain, since the
    random numbers are indexed by marker and iteration, summed in another order. y_pred is returned
    in the original order."""
    X, y = case(name, cus)
    perm = np.random.default_rng(77).permutation(X.shape[0])
    r = loop(sampler, np.asfortranarray(X[perm]), y[perm], schedule or schedule_of(name))
    y_pred = np.empty_like(r["y_pred"])
    y_pred[perm] = r["y_pred"]
    r["y_pred"] = y_pred
    return _freeze(r)


def path_cases():
    """Every (case, schedule, samplers) the device tests compare with the loop."""
    out = [(name, schedule_of(name), SAMPLERS) for name in SAME_PATH]
    out += [("plain300", s, SAMPLERS) for s in THINNING]
    out += [("plain300", DEFAULT, SAMPLERS)]  # the pooled-context test's fit A
    out += [("plain1009", s, ("BRR",)) for s in THINNING]
    out += [(name, schedule_of(name), ("BRR",)) for name in BRR_ONLY]
    return out


OUTPUTS = ("b_hat", "y_pred", "var", "pip")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
