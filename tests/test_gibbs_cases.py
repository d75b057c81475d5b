"""The conditions that tests/test_gpu_gibbs_edges.py rests on, asserted on the reference loops alone
(oracle.brr_gibbs, bayes_abc_ref.bayes_gibbs on the inputs of tests/gibbs_cases.py): no indicator
draw near its threshold, a rounding noise of the loops themselves far below the device bound, the
sample gate of the thinned schedules, and the argument refusals of the two fits."""
import numpy as np
import pytest

import gbm
from gbm import _lib

import gibbs_cases as gc

CASES = [(name, sched, sampler) for name, sched, samplers in gc.path_cases() for sampler in samplers]
MARGIN = 1e-6  # tests/test_bayes_abc.py's: device rounding (~1e-12) cannot flip an indicator beyond it
SENSITIVITY = 1e-11  # two orders under the device bound of 1e-9


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_inputs_are_what_the_device_tests_need():
    """Each input takes the storage it is meant to: X·s is whole and <= 255 at the first s of
    (2, 4, 1) only where gibbs_cases.STORAGE says so; `counts` holds bytes >= 128 and a 255."""
    for name, want in gc.STORAGE.items():
        X, y = gc.case(name)
        assert X.flags.f_contiguous and not X.flags.writeable and y.shape == (X.shape[0],)
        fits = [s for s in (2, 4, 1) if np.all(X * s == np.rint(X * s)) and (X * s).min() >= 0 and (X * s).max() <= 255]
        assert (fits[0] if fits else None) == want, (name, fits)
    X = gc.case("tetra")[0]
    assert set(np.unique(X * 4)) == {0, 1, 2, 3, 4}
    for name in ("counts", "counts1009"):
        X = gc.case(name)[0]
        assert (X >= 128).sum() == 40 and X.max() == 255
    X = gc.case("overflow")[0]
    assert (X == 128.5).sum() == 1 and np.all(X * 2 == np.rint(X * 2))  # dyadic, yet no byte
    X = gc.case("degenerate")[0]
    assert not X[:, 5].any() and np.all(X[:, 64] == 0.5) and np.all(X[:, 129] == 1.0)
    assert np.array_equal(X[:, 69], X[:, 70]) and X[:, 69].std() > 0
    assert gc.case("plain1009")[0].shape == (1009, 130) and gc.case("over")[0].shape == (12289, 130)
    assert gc.case("wide1009")[0].shape == (1009, 4200) and gc.case("tiny")[0].shape == (3, 1)


@pytest.mark.parametrize("name,sched,model", [c for c in CASES if c[2] in ("BayesB", "BayesC")], ids=_id)
def test_reference_indicator_margin(name, sched, model):
    """No indicator draw of the loop is within 1e-6 of its threshold (tests/test_bayes_abc.py's
    MARGIN), so the device's rounding cannot flip one. Measured: the smallest is 1.9e-4 (BayesB,
    `overflow`), the next 2.3e-4 (BayesC, `overflow`)."""
    margin = gc.reference(model, name, sched)["margin"]
    print(model, name, sched, "margin", margin)
    assert margin > MARGIN


@pytest.mark.parametrize("name,sched,sampler", CASES, ids=_id)
def test_reference_rounding_sensitivity(name, sched, sampler):
    """The loop on the individuals in another order is the same chain with other summation orders:
    every output agrees with the first order to 1e-11, which leaves two orders between the
    reference's own rounding noise and the device bound of 1e-9. Measured: at most 2.3e-15
    (BRR, `wide48`, y_pred); pip is bit-equal everywhere."""
    r, q = gc.reference(sampler, name, sched), gc.permuted_reference(sampler, name, sched)
    names = [k for k in gc.OUTPUTS if r[k] is not None]
    errs = {k: gc.rel(q[k], r[k]) for k in names}
    print(sampler, name, sched, {k: float(f"{v:.3g}") for k, v in errs.items()})
    for k, v in errs.items():
        assert v < SENSITIVITY, (k, v)


@pytest.mark.parametrize("sampler", gc.SAMPLERS)
@pytest.mark.parametrize("sched", list(gc.THINNING), ids=_id)
def test_reference_sample_gate(sampler, sched):
    """A thinned schedule's means are the plain means of the chain's states at the iterations the
    table of the schedule names (3, 2 and 1 samples): the state after iteration k is what the loop
    returns for (k, 0, k), the random numbers being indexed by iteration. For BRR that state is
    also checked against the loop's own b_last and mu_last."""
    X, y = gc.case("plain300")
    taken = gc.THINNING[sched]
    assert len(taken) == {(13, 4, 3): 3, (9, 4, 2): 2, (7, 0, 7): 1}[sched]
    states = [gc.loop(sampler, X, y, (k, 0, k)) for k in taken]
    if sampler == "BRR":
        for s in states:
            assert np.array_equal(s["b_hat"], np.concatenate([[s["mu_last"]], s["b_last"]]))
    r = gc.reference(sampler, "plain300", sched)
    for k in gc.OUTPUTS:
        if r[k] is None:
            continue
        mean = np.mean([s[k] for s in states], axis=0)
        if len(taken) == 1:
            assert np.array_equal(r[k], mean), k
        else:
            assert gc.rel(r[k], mean) < 1e-13, k
    if sampler == "BRR" and sched == (7, 0, 7):
        assert np.array_equal(r["b_hat"], np.concatenate([[r["mu_last"]], r["b_last"]]))


def test_a_schedule_without_a_sample_is_refused_before_device_use():
    """(n_iter, n_burnin, thin) = (5, 4, 3): no multiple of 3 lies in (4, 5]. Both fits refuse it
    while checking their arguments, as tests/test_bayes_abc.py's refusals."""
    X, y = gc.case("plain300")
    n, p = X.shape
    b, yp = np.zeros(p + 1), np.zeros(n)
    lib = gbm.load_library()
    rc = lib.gbm_brr_fit(_lib.ptr(X), n, p, n, _lib.ptr(y), 5, 4, 3, 0.5, 5.0, 1, 0, _lib.ptr(b), _lib.ptr(yp), None)
    assert rc == _lib.GBM_E_ARG and "no post-burn-in sample" in _lib.last_error()
    for model in (1, 2, 3):
        rc = lib.gbm_bayes_fit(model, _lib.ptr(X), n, p, n, _lib.ptr(y), 5, 4, 3, 0.5, 5.0, 0.5, 10.0, 1, 0,
                               _lib.ptr(b), _lib.ptr(yp), None, None)
        assert rc == _lib.GBM_E_ARG and "no post-burn-in sample" in _lib.last_error()
    with pytest.raises(gbm.ArgumentError):
        gbm.brr_arrays(X, y, n_iter=5, n_burnin=4, thin=3)
    with pytest.raises(gbm.ArgumentError):
        gbm.bayes_arrays("BayesB", X, y, n_iter=5, n_burnin=4, thin=3)
