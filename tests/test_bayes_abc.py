"""BayesA, BayesB and BayesC Gibbs samplers (libgbm ``gbm_bayes_fit``; ``gbm.bayesa`` / ``bayesb`` /
``bayesc``). BGLR is un-vendored and stochastic, so parity with BGLR itself is unpinned. Pinned
instead: the device sampler (64-marker blocks, a serial chain per block on the blocks' Gram
matrices) against the literal one-marker-at-a-time loop of tests/bayes_abc_ref.py on the same
counter-based random numbers (same sample path), a sparse-signal recovery check whose thresholds
are fixed on that loop, bit-reproducibility, the model functions, and that BRR is untouched."""
import ctypes
import threading

import numpy as np
import pytest

import gbm
import oracle
from gbm import _lib

import bayes_abc_ref as ref

MODELS = ("BayesA", "BayesB", "BayesC")
# (n, p, iters): tests/test_brr.py's same-path shapes (p mod 64 = 44, 2, 0) ...
BASE_SHAPES = [(100, 300, 12), (77, 130, 9), (200, 64, 7)]
# ... then five chunk workgroups with a last block of one marker; p = 65; non-dyadic genotypes
# (X·0.3 + 0.05: fp64 storage whatever GBM_BRR_I8 says)
EXTRA_SHAPES = [(1100, 129, 5, False), (300, 65, 5, False), (300, 200, 6, True)]
PATH_CASES = [(n, p, it, False) for n, p, it in BASE_SHAPES] + EXTRA_SHAPES
MARGIN = 1e-6  # |logOdds − logit(u)| above which device rounding (~1e-12) cannot flip an indicator


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


# ---- CPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["BayesB", "BayesC"])
@pytest.mark.parametrize("n,p,iters,scale", PATH_CASES)
def test_reference_indicator_margin(model, n, p, iters, scale):
    """No indicator draw of the reference loop is closer than 1e-6 to its threshold, so a same-path
    comparison cannot fail for a rounding-level difference in logOdds (measured: >= 4.7e-5, the
    smallest at BayesB (100, 300, 12))."""
    margin = ref.path_ref(model, n, p, iters, scale=scale)["margin"]
    print(model, (n, p, iters), "margin", margin)
    assert margin > MARGIN


def test_reference_bayesa_has_no_indicator():
    r = ref.path_ref("BayesA", 77, 130, 9)
    assert r["margin"] == np.inf and np.array_equal(r["pip"], np.ones(130)) and r["var"][2] == 0.5


@pytest.fixture(scope="module")
def sparse_reference():
    X, y, g, qtl = ref.sparse_case()
    return {m: ref.bayes_gibbs(m, X, y, **ref.SPARSE_FIT) for m in MODELS}


@pytest.mark.parametrize("model", MODELS)
def test_reference_recovers_sparse_signal(sparse_reference, model):
    """Eight QTL (±1) among 1000 markers, h² = 0.5, on the literal loop: fixes the thresholds of the
    device test below independently of the device code. Measured: BayesB PIP 0.92 at the QTL / 0.156
    elsewhere, cor(ŷ, g) 0.90; BayesC 0.94 / 0.017, 0.97; BayesA mean |b̂| 0.55 at the QTL / 0.021
    elsewhere, cor 0.84."""
    r = sparse_reference[model]
    ref.check_sparse(model, r["b_hat"], r["y_pred"], r["pip"])


def _fit_rc(model=2, n=20, p=30, n_iter=10, n_burnin=2, thin=1, r2=0.5, df0=5.0, prob_in=0.5, counts=10.0):
    X = np.asfortranarray(np.random.default_rng(0).random((n, p)))
    y = np.arange(float(n))
    b, yp = np.zeros(p + 1), np.zeros(n)
    lib = gbm.load_library()
    return lib.gbm_bayes_fit(model, _lib.ptr(X), n, p, n, _lib.ptr(y), n_iter, n_burnin, thin, r2, df0, prob_in,
                             counts, 1, 0, _lib.ptr(b), _lib.ptr(yp), None, None)


def test_arguments_are_refused_before_device_use():
    E = _lib.GBM_E_ARG
    for bad_model in (0, 4, -1):
        assert _fit_rc(model=bad_model) == E
        assert "model" in _lib.last_error()
    for model in (1, 2, 3):
        assert _fit_rc(model, df0=0.5) == E  # the per-marker χ²(df0 + 1) needs shape >= 1
        assert _fit_rc(model, prob_in=0.0) == E
        assert _fit_rc(model, prob_in=1.0) == E
        assert _fit_rc(model, prob_in=-0.2) == E
        assert _fit_rc(model, prob_in=0.05) == E  # counts·prob_in = 0.5
        assert _fit_rc(model, prob_in=0.95) == E  # counts·(1 − prob_in) = 0.5
        assert _fit_rc(model, counts=1.5) == E
        assert "prior" in _lib.last_error()
        # gbm_brr_fit's checks
        assert _fit_rc(model, r2=1.0) == E
        assert _fit_rc(model, thin=0) == E
        assert _fit_rc(model, n_iter=4, n_burnin=4) == E
        assert _fit_rc(model, n_iter=(1 << 23) + 1) == E  # the per-marker stream packs it into 23 bits
    X = np.random.default_rng(0).random((20, 30))
    with pytest.raises(gbm.ArgumentError):
        gbm.bayes_arrays("BayesD", X, np.arange(20.0))
    with pytest.raises(gbm.ArgumentError):
        gbm.bayes_arrays("BayesB", X, np.arange(20.0), prob_in=1.5)
    ent = [f"e{i}" for i in range(20)]
    g = gbm.Genomes(ent, ["p"] * 20, [f"l{j}" for j in range(30)], X)
    ph = gbm.Phenomes(ent, ["p"] * 20, ["t"], np.arange(20.0)[:, None])
    with pytest.raises(gbm.ArgumentError, match="bayesa"):
        gbm.bayesian("BayesA", genomes=g, phenomes=ph)


# ---- GPU ---------------------------------------------------------------------------------------
def _device_fit(model, n, p, iters, scale, **kw):
    X, y = ref.path_case(n, p, None, scale)
    return gbm.bayes_arrays(model, X, y, n_iter=iters, n_burnin=2, thin=1, seed=99, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n,p,iters,scale", PATH_CASES)
def test_gpu_same_sample_path_as_literal_loop(gbm_env, model, n, p, iters, scale):
    """b_hat, y_pred, var and pip follow the literal loop to 1e-9 (tests/test_brr.py's bound for the
    same comparison), with byte storage (the default where the genotypes are k/2) and with fp64
    storage (GBM_BRR_I8=0); the two storages agree to 1e-10. Measured on an MI355X: worst error
    2.0e-15 over every model, shape and output; the two storages bit-identical."""
    r = ref.path_ref(model, n, p, iters, scale=scale)
    assert model == "BayesA" or r["margin"] > MARGIN
    got = _device_fit(model, n, p, iters, scale)
    gbm_env.setenv("GBM_BRR_I8", "0")
    f64 = _device_fit(model, n, p, iters, scale)
    names = ("b_hat", "y_pred", "var", "pip")
    errs = {}
    for storage, out in (("bytes", got), ("fp64", f64)):
        for name, a in zip(names, out):
            errs[storage, name] = rel(a, r[name])
    errs["bytes vs fp64"] = max(rel(a, b) for a, b in zip(got, f64))
    print(model, (n, p, iters), {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert errs.pop("bytes vs fp64") < 1e-10
    for k, v in errs.items():
        assert v < 1e-9, (k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_recovers_sparse_signal(model):
    """The data and assertions of test_reference_recovers_sparse_signal on the device output."""
    X, y, g, qtl = ref.sparse_case()
    b_hat, y_pred, var, pip = gbm.bayes_arrays(model, X, y, **ref.SPARSE_FIT)
    ref.check_sparse(model, b_hat, y_pred, pip)
    if model == "BayesA":
        assert np.array_equal(pip, np.ones(X.shape[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_bit_reproducible_pooled_and_threaded(model):
    """Two identical fits give identical bytes; the second adds no device allocation (pooled
    context, captured iteration reused); four threads fitting different seeds at once give the
    bytes of the serial runs (every sum is combined in a fixed order, no atomics)."""
    lib = gbm.load_library()
    X, y = ref.path_case(700, 450, 301)
    kw = dict(n_iter=6, n_burnin=2, thin=1)
    first = gbm.bayes_arrays(model, X, y, seed=5, **kw)
    a0 = lib.gbm_device_allocations()
    again = gbm.bayes_arrays(model, X, y, seed=5, **kw)
    assert lib.gbm_device_allocations() == a0
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    seeds = (5, 6, 7, 8)
    serial = [gbm.bayes_arrays(model, X, y, seed=s, **kw) for s in seeds]
    assert not np.array_equal(serial[0][0], serial[1][0])
    out, errs = [None] * 4, []

    def run(k):
        try:
            out[k] = gbm.bayes_arrays(model, X, y, seed=seeds[k], **kw)
        except Exception as e:  # reported below
            errs.append(repr(e))

    th = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for a, b in zip(out, serial):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def _model_function_data():
    X = oracle.synth_genotypes(81, 150, 500)
    Y = oracle.synth_phenotypes(X, 82)
    ent = [f"e{i}" for i in range(150)]
    g = gbm.Genomes(ent, ["p"] * 150, [f"l{j}" for j in range(500)], X)
    ph = gbm.Phenomes(ent, ["p"] * 150, ["t"], Y)
    return g, ph


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bayesa", "bayesb", "bayesc"])
def test_gpu_model_functions(name):
    """tests/test_brr.py test_gpu_bayesian_model_function's setup; cor > 0.5 is the reference
    doctest's bound (src/linear.jl:436)."""
    g, ph = _model_function_data()
    fit = getattr(gbm, name)(genomes=g, phenomes=ph, n_iter=300, n_burnin=100)
    assert fit.model == name and fit.checkdims() and fit.metrics["cor"] > 0.5
    pred = gbm.predict(fit, g, list(range(1, 151)))
    assert np.abs(pred - fit.y_pred).max() < 1e-9 * np.abs(fit.y_pred).max()


def _brr_stats():
    lib = gbm.load_library()
    path, fb = ctypes.c_int(-1), ctypes.c_int64(0)
    lib.gbm_debug_brr_stats(ctypes.byref(path), ctypes.byref(fb))
    return path.value, fb.value


@pytest.mark.gpu
def test_gpu_brr_untouched_by_a_bayesc_fit():
    X, y = ref.path_case(700, 450, 301)
    before = gbm.brr_arrays(X, y, n_iter=6, n_burnin=2, thin=1, seed=5)
    stats = _brr_stats()
    gbm.bayes_arrays("BayesC", X, y, n_iter=6, n_burnin=2, thin=1, seed=5)
    assert _brr_stats() == stats
    after = gbm.brr_arrays(X, y, n_iter=6, n_burnin=2, thin=1, seed=5)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
