"""BayesA, BayesB and BayesC with an ordinal response (libgbm ``gbm_bayes_fit_ordinal``;
``gbm.bayes_ordinal_arrays``, ``gbm.bayesian(..., response_type="ordinal")``). BGLR is un-vendored and
stochastic, so parity with BGLR itself is unpinned. Pinned instead: the device sampler against the
literal loop of tests/ordinal_ref.py on the same counter-based random numbers (same sample path),
the restated AS241 against scipy, the identification of the thresholds, a sparse-signal recovery
check whose bounds are fixed on that loop, bit-reproducibility on the pooled context, and that the
Gaussian sampler is untouched."""
import ctypes
import math

import numpy as np
import pytest

import gbm
from gbm import _lib

import bayes_abc_ref as abc_ref
import ordinal_ref as ref

MODELS = ("BayesA", "BayesB", "BayesC")
KS = (2, 3, 5)
# (n, p, iters, scale): p mod 64 = 44, 2, 0; five chunk workgroups with a last block of one marker and
# classes that span the chunks; non-dyadic genotypes (fp64 storage whatever GBM_BRR_I8 says)
PATH_CASES = [(100, 300, 12, False), (77, 130, 9, False), (200, 64, 7, False), (1100, 129, 5, False),
              (300, 200, 6, True)]
THIN_CASE = dict(model="BayesB", n=300, p=130, K=3, iters=13, n_burnin=4, thin=3)
MARGIN = 1e-6  # tests/test_bayes_abc.py's: device rounding (~1e-12) cannot flip an indicator beyond it
NAMES = ("b_hat", "y_pred", "var", "pip", "thresholds", "probs")


def rel(a, b):
    """Largest difference relative to the largest reference value; absolute where the reference is all zero
    (the one threshold of two classes of equal size is Φ⁻¹(1/2) = 0 exactly)."""
    scale = np.abs(np.asarray(b)).max()
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (scale if scale > 0.0 else 1.0)


# ---- CPU ---------------------------------------------------------------------------------------
def test_as241_agrees_with_scipy():
    """The restated PPND16 against scipy.special.ndtri to 1e-15 relative from 1e-300 to 1 − 1e-16, through
    both tails and the central branch and at the branch points (measured: worst 7.5e-16, at p = 1e-179)."""
    from scipy.special import ndtri
    grid = np.concatenate([10.0 ** -np.arange(1.0, 301.0), np.linspace(0.001, 0.999, 1999),
                           1.0 - 10.0 ** -np.arange(1.0, 17.0), [0.075, 0.925, 0.0749999, 0.9250001]])
    worst = 0.0
    for p in grid:
        a, b = ref.ppnd16(float(p)), float(ndtri(float(p)))
        worst = max(worst, abs(a - b) / abs(b) if b != 0.0 else abs(a))
    print("worst relative error", worst)
    assert ref.ppnd16(0.5) == 0.0 and ref.ppnd16(0.0) == -math.inf and ref.ppnd16(1.0) == math.inf
    assert worst < 1e-15


def test_library_as241_has_the_restatement_coefficients():
    """csrc/gibbs_common.h's gibbs_ppnd16 and the restatement hold the same constants in the same order
    (the routines' own values, host and device, are held to an mpmath reference through gbm_debug_ordinal_math:
    tests/test_ordinal_cases.py, tests/test_gpu_ordinal_edges.py)."""
    import inspect
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "gibbs_common.h")).read()
    body = hdr[hdr.index("double gibbs_ppnd16"):hdr.index("// TN(m; a, b; u)")]
    number = r"(?<![\w.])\d+\.\d+(?:e-?\d+)?"
    mine = [float(v) for v in re.findall(number, body) if len(v) >= 14]  # the 45 coefficients, not 0.5, 1.6, …
    theirs = [float(v) for v in re.findall(number, inspect.getsource(ref.ppnd16)) if len(v) >= 14]
    assert len(mine) == 45 and mine == theirs


def test_truncated_normal_stays_in_its_interval():
    """TN(m; a, b; u) lies in [a, b] for intervals below, above and around the mean, half-open ones and ones
    so far out that Φ has no mass left in fp64 (then: the end nearer the mean); u → 0, 1 reach the ends."""
    for m, a, b in [(0.0, -1.0, 2.0), (0.3, 1.0, 2.5), (0.3, -2.5, -1.0), (1.0, -math.inf, 0.0), (-1.0, 0.5, math.inf),
                    (0.0, 9.0, 9.5), (0.0, 40.0, 41.0), (0.0, -41.0, -40.0), (50.0, -math.inf, 0.0)]:
        xs = [ref.truncnorm(m, a, b, u) for u in (2.0 ** -54, 0.01, 0.3, 0.5, 0.9, 1 - 2.0 ** -53)]
        assert all(a <= x <= b for x in xs), (m, a, b, xs)
        assert sorted(xs) in (xs, xs[::-1])  # monotone in u (falling after a reflection)
    assert ref.truncnorm(0.0, 40.0, 41.0, 0.7) == 40.0 and ref.truncnorm(0.0, -41.0, -40.0, 0.7) == -40.0


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n,p,iters,scale", PATH_CASES)
def test_reference_margin_gap_and_identification(model, K, n, p, iters, scale):
    """On every same-path case no indicator draw of the loop is within 1e-6 of its threshold and every
    threshold is drawn from an interval of positive length, so the device comparison cannot fail for a
    rounding-level difference; t_1 never moves, and with K = 2 no threshold does. Measured: smallest margin
    1.1e-4 (BayesC, (300, 200, 6) scaled, K = 3), smallest gap 3.9e-4 ((1100, 129, 5), K = 5)."""
    r = ref.ordinal_path_ref(model, n, p, iters, K, scale)
    print(model, K, (n, p, iters), "margin", r["margin"], "gap", r["gap"])
    assert model == "BayesA" or r["margin"] > MARGIN
    assert r["gap"] > 0.0
    assert (r["gap"] == math.inf) == (K == 2)
    assert r["t_end"][1] == r["t_start"][1]
    if K == 2:
        assert r["t_end"] == r["t_start"]
    assert all(a < b for a, b in zip(r["t_end"], r["t_end"][1:]))
    assert abs(r["thresholds"][0] - r["t_start"][1]) <= 1e-15 * max(1.0, abs(r["t_start"][1]))
    assert np.abs(r["probs"].sum(axis=1) - 1.0).max() < 1e-12 and r["var"][0] == 1.0


def test_reference_thinned_case_margin_and_gap():
    """The conditions above on the thinned case of the device test (measured: margin 5.0e-3, gap 4.1e-3); its
    means hold three samples."""
    c = THIN_CASE
    r = ref.ordinal_path_ref(c["model"], c["n"], c["p"], c["iters"], c["K"], False, c["n_burnin"], c["thin"])
    assert r["margin"] > MARGIN and r["gap"] > 0.0 and r["t_end"][1] == r["t_start"][1]
    full = ref.ordinal_path_ref(c["model"], c["n"], c["p"], c["iters"], c["K"], False, c["n_burnin"], 1)
    assert rel(r["thresholds"], full["thresholds"]) > 1e-6  # the gate matters


# Recovery figures measured on the literal loop (ordinal_ref.sparse_figures; SPARSE_FIT's schedule): the fit on
# the true classes, then the fit on the same classes permuted among the individuals (no signal).
SPARSE_MEASURED = {
    "BayesA": ({"cor": 0.8028, "thr_err": 0.1019}, {"cor": -0.0481, "thr_err": 0.1487}),
    "BayesB": ({"cor": 0.8417, "pip_qtl": 0.7297, "pip_rest": 0.2700, "thr_err": 0.1075},
               {"cor": -0.0319, "pip_qtl": 0.2578, "pip_rest": 0.2576, "thr_err": 0.1230}),
    "BayesC": ({"cor": 0.8720, "pip_qtl": 0.7016, "pip_rest": 0.1439, "thr_err": 0.1232},
               {"cor": -0.0477, "pip_qtl": 0.4328, "pip_rest": 0.4333, "thr_err": 0.1336}),
}


def check_sparse(model, y_pred, pip, thresholds):
    """The recovery assertions: every bound lies halfway between the loop's figure on the true classes and its
    figure on the permuted ones (SPARSE_MEASURED). BayesB's mean PIP away from the QTL has no bound: it does not
    tell the two fits apart (0.270 on the true classes, 0.258 on the permuted ones)."""
    f = ref.sparse_figures(y_pred, pip, thresholds)
    print(model, f)
    true, perm = SPARSE_MEASURED[model]
    half = {k: 0.5 * (true[k] + perm[k]) for k in true}
    assert f["cor"] >= half["cor"], (f, half)
    assert f["thr_err"] <= half["thr_err"], (f, half)
    if model != "BayesA":
        assert f["pip_qtl"] >= half["pip_qtl"], (f, half)
    if model == "BayesC":
        assert f["pip_rest"] <= half["pip_rest"], (f, half)
    return f


@pytest.fixture(scope="module")
def sparse_reference():
    X, cls, g, qtl = ref.sparse_ordinal_case()
    return {m: ref.ordinal_gibbs(m, X, cls, **abc_ref.SPARSE_FIT) for m in MODELS}


@pytest.mark.parametrize("model", MODELS)
def test_reference_recovers_sparse_ordinal_signal(sparse_reference, model):
    """Eight QTL (±1) among 1000 markers, h² = 0.5, the liability cut at −0.8, 0.1 and 1.0 standard deviations
    into four classes (57, 97, 103 and 43 individuals), on the literal loop: fixes the bounds of the device test
    independently of the device code. Measured on the true classes / on permuted classes: BayesA cor(ŷ, g)
    0.80 / −0.05, threshold error 0.102 / 0.149; BayesB cor 0.84 / −0.03, PIP at the QTL 0.73 / 0.26, elsewhere
    0.270 / 0.258, threshold error 0.107 / 0.123; BayesC cor 0.87 / −0.05, PIP 0.70 / 0.43 at the QTL, 0.144 /
    0.433 elsewhere, threshold error 0.123 / 0.134 (the classes' frequencies alone place the thresholds on the
    liability's scale, so the permuted fit is not far off them either)."""
    r = sparse_reference[model]
    f = check_sparse(model, r["y_pred"], r["pip"], r["thresholds"])
    for k, v in SPARSE_MEASURED[model][0].items():  # the table above is this loop's output
        assert abs(f[k] - v) < 1e-4, (k, f[k], v)


def _fit_rc(y=None, model=2, n=20, p=30, n_iter=10, n_burnin=2, thin=1, r2=0.5, df0=5.0, prob_in=0.5, counts=10.0,
            max_classes=32):
    X = np.asfortranarray(np.random.default_rng(0).random((n, p)))
    y = np.ascontiguousarray(np.arange(n) % 3 if y is None else y, dtype=np.float64)
    b, yp, cl, th = np.zeros(p + 1), np.zeros(n), np.zeros(64), np.zeros(64)
    K = ctypes.c_int64(0)
    lib = gbm.load_library()
    return lib.gbm_bayes_fit_ordinal(model, _lib.ptr(X), n, p, n, _lib.ptr(y), n_iter, n_burnin, thin, r2, df0, prob_in,
                                     counts, 1, 0, _lib.ptr(b), _lib.ptr(yp), None, None, max_classes,
                                     ctypes.addressof(K), _lib.ptr(cl), _lib.ptr(th), None, n)


def test_arguments_are_refused_before_device_use():
    E = _lib.GBM_E_ARG
    assert "gbm_bayes_fit_ordinal" in _lib.EXPORTS
    assert _fit_rc(y=np.ones(20)) == E  # K = 1
    assert "distinct" in _lib.last_error()
    assert _fit_rc(y=np.arange(40) % 33, n=40) == E  # K = 33
    assert _fit_rc(y=np.arange(20) % 4, max_classes=3) == E
    assert _fit_rc(y=np.r_[np.arange(19) % 3, np.nan]) == E
    for bad_model in (0, 4, -1):
        assert _fit_rc(model=bad_model) == E
        assert "model" in _lib.last_error()
    for model in (1, 2, 3):
        assert _fit_rc(model=model, df0=0.5) == E
        assert _fit_rc(model=model, prob_in=0.0) == E
        assert _fit_rc(model=model, prob_in=1.0) == E
        assert _fit_rc(model=model, prob_in=0.05) == E
        assert _fit_rc(model=model, counts=1.5) == E
        assert "prior" in _lib.last_error()
        assert _fit_rc(model=model, r2=1.0) == E
        assert _fit_rc(model=model, thin=0) == E
        assert _fit_rc(model=model, n_iter=4, n_burnin=4) == E
        assert _fit_rc(model=model, n_iter=(1 << 23) + 1) == E
    X = np.random.default_rng(0).random((20, 30))
    with pytest.raises(gbm.ArgumentError):
        gbm.bayes_ordinal_arrays("BayesD", X, np.arange(20.0) % 3)
    with pytest.raises(gbm.ArgumentError, match="distinct"):
        gbm.bayes_ordinal_arrays("BayesB", X, np.ones(20))
    with pytest.raises(gbm.ArgumentError, match="distinct"):
        gbm.bayes_ordinal_arrays("BayesB", np.random.default_rng(0).random((40, 30)), np.arange(40.0))


def _genomes_phenomes(X, y):
    n, p = X.shape
    ent = [f"e{i}" for i in range(n)]
    return (gbm.Genomes(ent, ["p"] * n, [f"l{j}" for j in range(p)], X),
            gbm.Phenomes(ent, ["p"] * n, ["t"], np.asarray(y, dtype=np.float64)[:, None]))


def test_bayesian_response_type_errors():
    """BRR has no ordinal response (the error names the three models that have), an unknown response type is
    refused, and the Gaussian refusals are the old ones."""
    g, ph = _genomes_phenomes(np.random.default_rng(0).random((20, 30)), np.arange(20) % 3)
    with pytest.raises(gbm.ArgumentError, match="BayesA.*BayesB.*BayesC"):
        gbm.bayesian("BRR", genomes=g, phenomes=ph, response_type="ordinal")
    with pytest.raises(gbm.ArgumentError, match="response_type"):
        gbm.bayesian("BRR", genomes=g, phenomes=ph, response_type="poisson")
    with pytest.raises(gbm.ArgumentError, match="response_type"):
        gbm.bayesian("BayesB", genomes=g, phenomes=ph, response_type="probit")
    with pytest.raises(gbm.ArgumentError, match="bayesa"):
        gbm.bayesian("BayesA", genomes=g, phenomes=ph)
    with pytest.raises(gbm.ArgumentError, match="not available"):
        gbm.bayesian("BayesD", genomes=g, phenomes=ph, response_type="gaussian")


# ---- GPU ---------------------------------------------------------------------------------------
def _device_fit(model, n, p, iters, K, scale, n_burnin=2, thin=1, **kw):
    X, cls = ref.ordinal_case(n, p, K, scale)
    return gbm.bayes_ordinal_arrays(model, X, cls, n_iter=iters, n_burnin=n_burnin, thin=thin, seed=99, **kw)


def _errors(out, r):
    b_hat, y_pred, var, pip, classes, thresholds, probs = out
    assert np.array_equal(classes, r["classes"])
    got = dict(zip(NAMES, (b_hat, y_pred, var, pip, thresholds, probs)))
    return {name: rel(got[name], r[name]) for name in NAMES}


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n,p,iters,scale", PATH_CASES)
def test_gpu_same_sample_path_as_literal_loop(gbm_env, model, K, n, p, iters, scale):
    """b_hat, y_pred, var, pip, the thresholds and the class probabilities follow the literal loop to 1e-9
    (tests/test_bayes_abc.py's and tests/test_brr.py's bound for the same comparison), with byte storage (the
    default where the genotypes are k/2) and with fp64 storage (GBM_BRR_I8=0); the two storages agree to
    1e-10. Measured on an MI355X: worst error 4.3e-15 over every model, shape, K and output (a class
    probability); the two storages bit-identical."""
    r = ref.ordinal_path_ref(model, n, p, iters, K, scale)
    assert (model == "BayesA" or r["margin"] > MARGIN) and r["gap"] > 0.0
    got = _device_fit(model, n, p, iters, K, scale)
    gbm_env.setenv("GBM_BRR_I8", "0")
    f64 = _device_fit(model, n, p, iters, K, scale)
    errs = {}
    for storage, out in (("bytes", got), ("fp64", f64)):
        for name, v in _errors(out, r).items():
            errs[storage, name] = v
    errs["bytes vs fp64"] = max(rel(a, b) for a, b in zip(got, f64))
    print(model, K, (n, p, iters), {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert got[2][0] == 1.0
    assert errs.pop("bytes vs fp64") < 1e-10
    for k, v in errs.items():
        assert v < 1e-9, (k, v)


@pytest.mark.gpu
def test_gpu_same_sample_path_thinned():
    """thin = 3 after a burn-in of 4: the gate of the thresholds' and the probabilities' running means away
    from thin = 1 (samples at iterations 6, 9 and 12 of 13)."""
    c = THIN_CASE
    r = ref.ordinal_path_ref(c["model"], c["n"], c["p"], c["iters"], c["K"], False, c["n_burnin"], c["thin"])
    assert r["margin"] > MARGIN and r["gap"] > 0.0
    out = _device_fit(c["model"], c["n"], c["p"], c["iters"], c["K"], False, c["n_burnin"], c["thin"])
    errs = _errors(out, r)
    print(c, {k: float(f"{v:.3g}") for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 1e-9, (k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_gpu_probabilities(K):
    """Every row of probs sums to 1 within 1e-12 and lies in [0, 1]; with two classes they are the loop's
    means of Φ(t_1 − ŷ) and Φ(−(t_1 − ŷ))."""
    n, p, iters = 1100, 129, 5
    out = _device_fit("BayesC", n, p, iters, K, False)
    probs = out[6]
    assert probs.shape == (n, K) and probs.min() >= 0.0 and probs.max() <= 1.0
    assert np.abs(probs.sum(axis=1) - 1.0).max() < 1e-12
    if K == 2:
        r = ref.ordinal_path_ref("BayesC", n, p, iters, K, False)
        assert rel(probs, r["phi_pm"]) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_recovers_sparse_ordinal_signal(model):
    """The data and assertions of test_reference_recovers_sparse_ordinal_signal on the device output."""
    X, cls, g, qtl = ref.sparse_ordinal_case()
    b_hat, y_pred, var, pip, classes, thresholds, probs = gbm.bayes_ordinal_arrays(model, X, cls, **abc_ref.SPARSE_FIT)
    check_sparse(model, y_pred, pip, thresholds)
    assert np.array_equal(classes, np.arange(4.0))
    # the most probable class is the observed one far more often than the largest class's share
    assert (probs.argmax(axis=1) == cls).mean() > np.bincount(cls.astype(int)).max() / len(cls)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_bit_reproducible_pooled_beside_the_gaussian_fit(model):
    """Two identical ordinal fits give identical bytes and the second adds no device allocation (pooled
    context, captured iteration reused); a Gaussian gbm_bayes_fit between two ordinal fits changes neither's
    bytes, and its own bytes are those of a run made before any ordinal fit of this shape."""
    lib = gbm.load_library()
    X, cls = ref.ordinal_case(700, 450, 3)
    yg = abc_ref.path_case(700, 450)[1]
    kw = dict(n_iter=6, n_burnin=2, thin=1, seed=5)
    gauss_before = gbm.bayes_arrays(model, X, yg, **kw)
    first = gbm.bayes_ordinal_arrays(model, X, cls, **kw)
    a0 = lib.gbm_device_allocations()
    again = gbm.bayes_ordinal_arrays(model, X, cls, **kw)
    assert lib.gbm_device_allocations() == a0
    assert _same(first, again)
    gauss_between = gbm.bayes_arrays(model, X, yg, **kw)
    third = gbm.bayes_ordinal_arrays(model, X, cls, **kw)
    assert lib.gbm_device_allocations() == a0
    assert _same(first, third)
    assert _same(gauss_before, gauss_between)
    assert not np.array_equal(first[0], gbm.bayes_ordinal_arrays(model, X, cls, **dict(kw, seed=6))[0])


@pytest.mark.gpu
def test_gpu_optional_outputs_may_be_null():
    """Without probs_out, and without thresholds_out, the call works and every other output keeps its bits."""
    n, p, K = 300, 130, 3
    X, cls = ref.ordinal_case(n, p, K)
    Xf = np.asfortranarray(X)
    full = gbm.bayes_ordinal_arrays("BayesB", X, cls, n_iter=8, n_burnin=2, thin=1, seed=7)
    noprob = gbm.bayes_ordinal_arrays("BayesB", X, cls, n_iter=8, n_burnin=2, thin=1, seed=7, probs=False)
    assert noprob[6] is None and _same(full[:6], noprob[:6])
    lib = gbm.load_library()
    b, yp, var, pip, cl = np.zeros(p + 1), np.zeros(n), np.zeros(3), np.zeros(p), np.zeros(K)
    pr = np.zeros((n + 3, K), order="F")  # a pitch above n
    nk = ctypes.c_int64(0)
    rc = lib.gbm_bayes_fit_ordinal(2, _lib.ptr(Xf), n, p, n, _lib.ptr(np.ascontiguousarray(cls)), 8, 2, 1, 0.5, 5.0, 0.5,
                                   10.0, 7, 0, _lib.ptr(b), _lib.ptr(yp), _lib.ptr(var), _lib.ptr(pip), K,
                                   ctypes.addressof(nk), _lib.ptr(cl), None, _lib.ptr(pr), n + 3)
    assert rc == 0 and nk.value == K
    assert _same(full[:5], (b, yp, var, pip, cl)) and np.array_equal(pr[:n], full[6]) and not pr[n:].any()


@pytest.mark.gpu
def test_gpu_bayesian_ordinal_response():
    """bayesian(..., response_type="ordinal"): y_true is the observed classes, y_pred the liability, which
    orders the classes (cor > 0.5 is the reference doctest's bound, src/bayes.jl:157), and predict reproduces it."""
    X, cls, g, qtl = ref.sparse_ordinal_case()
    gen, ph = _genomes_phenomes(X, cls)
    fit = gbm.bayesian("BayesC", genomes=gen, phenomes=ph, response_type="ordinal", n_iter=300, n_burnin=100)
    assert fit.model == "BayesC" and fit.checkdims() and np.array_equal(fit.y_true, cls)
    assert fit.metrics["cor"] > 0.5
    pred = gbm.predict(fit, gen, list(range(1, X.shape[0] + 1)))
    assert np.abs(pred - fit.y_pred).max() < 1e-9 * np.abs(fit.y_pred).max()
