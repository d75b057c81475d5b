"""The ordinal sampler on the device where tests/test_bayes_ordinal.py does not go (inputs, references and the
bounds' origin: tests/ordinal_cases.py, tests/test_ordinal_cases.py):

1. the device compilation of gibbs_phi, gibbs_ppnd16 and gibbs_truncnorm (gbm_debug_ordinal_math) against the
   mpmath reference on grids through both tails of AS241, reflected, half-open and far intervals, intervals
   without mass and the window where pa + u (pb − pa) rounds to 0 or 1;
2. ordinal_latent_kernel's and ordinal_threshold_kernel's edges against the literal loop on the same sample
   path: K = 32 (slots 62 / 63) and K = 31, chunks without a class (±∞ partials), a class of one member alone in
   the last chunk, n = 255 / 256 / 257, n = 3, labels that are not 0 … K − 1;
3. the pooled context across ordinal fits of other K, n and probs, with a Gaussian fit between them.

Bounds: the math 4 x the restatement's own error against mpmath; device against the loop 1e-9 relative on every
output, byte against fp64 storage 1e-10 (tests/test_bayes_ordinal.py's)."""
import numpy as np
import pytest

import gbm

import bayes_abc_ref as abc_ref
import ordinal_cases as oc
import ordinal_ref as ref

pytestmark = pytest.mark.gpu

LOOP, STORAGES, ROWSUM = 1e-9, 1e-10, 1e-12
MARGIN = 1e-6


# ---- 1. the device's Φ, Φ⁻¹ and TN ---------------------------------------------------------------
@pytest.fixture(scope="module")
def device_math():
    """One call per `what`: {what: (host values, device values)} on the grids followed by the exact-value points."""
    inputs = {0: oc.phi_grid(), 1: np.concatenate([oc.inv_grid(), oc.INV_POINTS]),
              2: np.concatenate([oc.tn_grid(), oc.no_mass_grid(), oc.window_grid()])}
    return {what: oc.library_math(what, a, device=True) for what, a in inputs.items()}


def test_gpu_math_against_mpmath(device_math):
    """The device's values within 4 x (c_Φ, c_inv, c_TN) of the mpmath reference, pointwise and normalised as
    those figures are (c_Φ = 1.55, c_inv = 7.27e-16, c_TN = 1.14e-15 for the restatement and for the host
    compilation); every TN draw finite and in its interval, the points left out of the error bound included.
    Measured on an MI355X: c_Φ = 2.46 (the device's erfc), c_inv = 6.06e-16, c_TN = 6.73e-16."""
    n_inv, n_tn = len(oc.inv_grid()), len(oc.tn_grid())
    dev = [device_math[0][1], device_math[1][1][:n_inv], device_math[2][1][:n_tn]]
    host = [device_math[0][0], device_math[1][0][:n_inv], device_math[2][0][:n_tn]]
    oc.check_math("host", *host)
    oc.check_math("device", *dev)


def test_gpu_math_exact_values_and_the_window(device_math):
    """On the device: Φ⁻¹(0) = −∞, Φ⁻¹(1/2) = 0, Φ⁻¹(1) = +∞; the no-mass intervals give 40, −40 and 0 at every u;
    every draw of the window (m = 37.6, 38, 38.4 above a half-open class's threshold, and the mirror image) and of
    the intervals where pa + u (pb − pa) rounds to 1 is finite and in [a, b]."""
    n_inv, n_tn, n_nm = len(oc.inv_grid()), len(oc.tn_grid()), len(oc.no_mass_grid())
    for label, k in (("host", 0), ("device", 1)):
        inv, tn = device_math[1][k], device_math[2][k]
        oc.check_exact_values(label, inv[n_inv:], tn[n_tn:n_tn + n_nm], tn[n_tn + n_nm:])


# ---- 2. the kernels' edges -----------------------------------------------------------------------
def _errors(out, r):
    assert np.array_equal(out[4], r["classes"])
    return {k: oc.rel(v, r[k]) for k, v in zip(oc.FIT_NAMES, out) if k != "classes"}


def _both_storages(gbm_env, name, model):
    got = oc.device_fit(name, model)
    gbm_env.setenv("GBM_BRR_I8", "0")
    f64 = oc.device_fit(name, model)
    gbm_env.delenv("GBM_BRR_I8")
    return got, f64


@pytest.mark.parametrize("name,model", [c for c in oc.fit_cases() if c[0] != "labels"])
def test_gpu_edge_fit_follows_the_literal_loop(gbm_env, name, model):
    """b_hat, y_pred, var, pip, classes, the thresholds and the probabilities of every edge fit follow the loop to
    1e-9, with byte storage and with GBM_BRR_I8=0; the two agree to 1e-10; the probabilities' rows sum to 1
    within 1e-12. Measured on an MI355X: worst error against the loop 1.5e-15 (`tiny2`, BayesA, y_pred; 1.4e-15 on
    `single257`), the two storages bit-identical, row sums within 5.6e-16; each case runs in 0.1 s or less."""
    r = oc.fit_reference(name, model)
    assert (model == "BayesA" or r["margin"] > MARGIN) and r["gap"] > 0.0
    got, f64 = _both_storages(gbm_env, name, model)
    errs = {(s, k): v for s, out in (("bytes", got), ("fp64", f64)) for k, v in _errors(out, r).items()}
    between = max(oc.rel(a, b) for a, b in zip(got, f64))
    rowsum = max(np.abs(out[6].sum(axis=1) - 1.0).max() for out in (got, f64))
    print(name, model, {f"{s} {k}": float(f"{v:.3g}") for (s, k), v in errs.items()},
          "bytes vs fp64", float(f"{between:.3g}"), "row sums", float(f"{rowsum:.3g}"))
    assert got[2][0] == 1.0 and f64[2][0] == 1.0
    assert between < STORAGES
    assert rowsum < ROWSUM
    for k, v in errs.items():
        assert v < LOOP, (k, v)


def test_gpu_class_labels_only_name_the_classes(gbm_env):
    """`n255` with the labels −2.5, 0 and 1e6 in place of 0, 1, 2: classes_out holds the sorted labels, and every
    other output has the bits of the fit on 0, 1, 2 (both storages); both follow the loop to 1e-9."""
    r = oc.fit_reference("labels", "BayesB")
    for plain, named in zip(_both_storages(gbm_env, "n255", "BayesB"), _both_storages(gbm_env, "labels", "BayesB")):
        assert np.array_equal(named[4], oc.LABELS) and np.array_equal(plain[4], [0.0, 1.0, 2.0])
        for k, a, b in zip(oc.FIT_NAMES, plain, named):
            assert k == "classes" or np.array_equal(a, b), k
        for k, v in _errors(named, r).items():
            assert v < LOOP, (k, v)


# ---- 3. the pooled context -------------------------------------------------------------------------
def _pool_calls():
    kw = dict(n_iter=5, n_burnin=2, thin=1, seed=oc.SEED)
    Xg, yg = abc_ref.path_case(1100, 129)
    X2, cls2 = ref.ordinal_case(1100, 129, 2)
    first = lambda: oc.device_fit("sorted1100", "BayesB")  # noqa: E731
    return [first,  # ordinal, 1100 x 129, K = 5, with probs
            lambda: oc.device_fit("k31_257", "BayesB", probs=False),  # smaller, K = 31, no probs
            lambda: gbm.bayes_arrays("BayesB", Xg, yg, **kw),  # Gaussian on the first shape
            lambda: gbm.bayes_ordinal_arrays("BayesB", X2, cls2, **kw),  # the first shape, K = 2
            first]


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


def test_gpu_pooled_context_across_ordinal_keys():
    """After gbm_release_device_cache(): an ordinal fit 1100 x 129 with K = 5 and probabilities; 257 x 130 with
    K = 31 and none (smaller buffers, no oprob); a Gaussian fit 1100 x 129; an ordinal fit 1100 x 129 with K = 2
    (the first fit's n and buffers, another K: a stale captured iteration or stale partial rows would show); the
    first again. Every one has the bits of the same call on a fresh context (made right after another release)."""
    lib = gbm.load_library()
    calls = _pool_calls()
    assert lib.gbm_release_device_cache() == 0
    pooled = [call() for call in calls]
    assert pooled[1][6] is None and pooled[3][6].shape == (1100, 2)
    assert _same(pooled[0], pooled[4])
    for i, call in enumerate(calls[:4]):
        assert lib.gbm_release_device_cache() == 0
        assert _same(pooled[i], call()), i
    r = oc.fit_reference("sorted1100", "BayesB")
    for k, v in _errors(pooled[4], r).items():
        assert v < LOOP, (k, v)
