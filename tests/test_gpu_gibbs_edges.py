"""The Gibbs samplers on the device (gbm_brr_fit, gbm_bayes_fit) against the literal loops on the
same sample path, where tests/test_brr.py and tests/test_bayes_abc.py do not go: thinned schedules
(the sample gate of brr_step_kernel, brr_step128_kernel, brr_sweep_la2_kernel, bayes_chain_kernel,
brr_var_kernel and bayes_final_kernel), byte storage at scales 4 and 1 with bytes >= 128, a dyadic
value that fits no byte, degenerate columns, n = 3 and p = 1, p > 4096, both edges of the BRR
super-block sweep, and the pooled context across fits of different keys. Inputs and references:
tests/gibbs_cases.py; what the bounds rest on: tests/test_gibbs_cases.py.

Bounds (tests/test_brr.py, tests/test_bayes_abc.py): device against the loop 1e-9 relative on every
output; byte storage against fp64 storage 1e-10; sweep against per-launch 1e-10."""
import ctypes

import numpy as np
import pytest

import gbm
from gbm import _lib

import gibbs_cases as gc

pytestmark = pytest.mark.gpu

LOOP, STORAGES, PATHS = 1e-9, 1e-10, 1e-10
_COLD = {}  # (sampler, case) -> the default-storage outputs of test_gpu_same_path, for the pooled-context test


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


def fit(sampler, name, schedule=None, cus=gc.SWEEP_CUS):
    """(b_hat, y_pred, var[, pip]) of one device fit of a named input."""
    X, y = gc.case(name, cus)
    n_iter, n_burnin, thin = schedule or gc.schedule_of(name)
    kw = dict(n_iter=n_iter, n_burnin=n_burnin, thin=thin, seed=gc.SEED)
    if sampler == "BRR":
        return gbm.brr_arrays(X, y, **kw)
    return gbm.bayes_arrays(sampler, X, y, **kw)


def errors(got, ref):
    return {k: gc.rel(a, ref[k]) for k, a in zip(gc.OUTPUTS, got)}


def report(what, errs):
    print(*what, {k: float(f"{v:.3g}") for k, v in errs.items()})


def check_against_loop(sampler, name, schedule, outs, cus=gc.SWEEP_CUS):
    """``outs``: label -> device outputs; every one within 1e-9 of the loop, printed first."""
    ref = gc.reference(sampler, name, schedule, cus)
    assert sampler in ("BRR", "BayesA") or ref["margin"] > 1e-6
    errs = {(label, k): v for label, got in outs.items() for k, v in errors(got, ref).items()}
    report((sampler, name, schedule or gc.schedule_of(name)), {f"{a} {k}": v for (a, k), v in errs.items()})
    for k, v in errs.items():
        assert v < LOOP, (k, v)
    return ref


def brr_path():
    lib = gbm.load_library()
    path, fb = ctypes.c_int(-1), ctypes.c_int64(0)
    lib.gbm_debug_brr_stats(ctypes.byref(path), ctypes.byref(fb))
    return path.value, fb.value


def brr_shape():
    lib = gbm.load_library()
    v = [ctypes.c_int(-1) for _ in range(5)]
    lib.gbm_debug_brr_shape(*[ctypes.byref(x) for x in v])
    return dict(zip(("C", "O", "R", "Ko", "Kn"), (x.value for x in v)))


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def needs_256_cus():
    cus = device_cus()
    if cus < gc.SWEEP_CUS:
        pytest.skip(f"the sweep's first shape is n = 1009 on >= 256 CUs only; this device has {cus}")


def both_storages(gbm_env, sampler, name, schedule=None):
    """The fit with the storage the device chooses and with fp64 storage; they agree to 1e-10."""
    got = fit(sampler, name, schedule)
    gbm_env.setenv("GBM_BRR_I8", "0")
    f64 = fit(sampler, name, schedule)
    gbm_env.delenv("GBM_BRR_I8")
    d = max(gc.rel(a, b) for a, b in zip(got, f64))
    print(sampler, name, "default storage vs fp64", float(f"{d:.3g}"))
    assert d < STORAGES
    return {"default": got, "fp64": f64}


# ---- 1. same path at the byte scales, the degenerate columns and the edge shapes --------------------
@pytest.mark.parametrize("sampler", gc.SAMPLERS)
@pytest.mark.parametrize("name", gc.SAME_PATH)
def test_gpu_same_path(gbm_env, sampler, name):
    """BRR and BayesA/B/C follow the loop to 1e-9 on b_hat, y_pred, var and pip, with the storage
    the device chooses (bytes at scale 4 for `tetra`, 1 for `counts` with bytes up to 255, 2
    elsewhere; fp64 for `overflow`) and with GBM_BRR_I8=0; the two agree to 1e-10. The duplicate
    pair of `degenerate` matches the loop marker by marker, and `counts`' y_pred is the numpy
    product of the returned b_hat (a cell unpacked as a signed byte would move it by orders).
    Measured on an MI355X: worst error against the loop 1.0e-14 (BRR, `wide48`, b_hat), 1.5e-15 on
    the 300 x 130 inputs; the two storages within 1.4e-15 for BRR and bit-identical for A/B/C."""
    outs = both_storages(gbm_env, sampler, name)
    _COLD[sampler, name] = outs["default"]
    ref = check_against_loop(sampler, name, None, outs)
    X, _ = gc.case(name)
    for label, got in outs.items():
        b_hat = got[0]
        if name == "degenerate":
            scale = np.abs(ref["b_hat"]).max()
            for j in (5, 64, 69, 70, 129):
                assert abs(b_hat[1 + j] - ref["b_hat"][1 + j]) < LOOP * scale, (label, j)
            assert abs(b_hat[1 + 70] - b_hat[1 + 69]) > 1e-6 * scale  # own random numbers each
        if name == "counts":
            assert gc.rel(b_hat[0] + X @ b_hat[1:], got[1]) < LOOP, label
            assert gc.rel(b_hat[0] + X @ b_hat[1:], ref["y_pred"]) < LOOP, label


# ---- 2. the sample gate --------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", gc.SAMPLERS)
@pytest.mark.parametrize("schedule", list(gc.THINNING), ids=_id)
def test_gpu_thinning(gbm_env, sampler, schedule):
    """(n_iter, n_burnin, thin) = (13, 4, 3), (9, 4, 2), (7, 0, 7) on `plain300` (the per-launch
    kernels), both storages: the running means follow the loop's, which samples iterations
    6, 9, 12; 6, 8 (not 4: the strict i > n_burnin); and 7 alone, where BRR's b_hat is the loop's
    last state. Measured on an MI355X: worst error against the loop 1.0e-15, the storages within
    5.8e-16."""
    outs = both_storages(gbm_env, sampler, "plain300", schedule)
    ref = check_against_loop(sampler, "plain300", schedule, outs)
    if sampler == "BRR" and schedule == (7, 0, 7):
        last = np.concatenate([[ref["mu_last"]], ref["b_last"]])
        for label, got in outs.items():
            assert gc.rel(got[0], last) < LOOP, label


@pytest.mark.parametrize("schedule", list(gc.THINNING), ids=_id)
def test_gpu_thinning_on_the_sweep(gbm_env, schedule):
    """The same schedules through brr_sweep_la2_kernel (n = 1009: path 4, no fall-back) and then
    through the per-launch byte path (GBM_BRR_SWEEP=0), each against the loop and against each
    other. Measured on an MI355X: worst error against the loop 1.0e-15, between the paths 1.0e-15."""
    needs_256_cus()
    _, fb0 = brr_path()
    sweep = fit("BRR", "plain1009", schedule)
    assert brr_path() == (4, fb0)
    gbm_env.setenv("GBM_BRR_SWEEP", "0")
    launches = fit("BRR", "plain1009", schedule)
    assert brr_path() == (0, fb0)
    ref = check_against_loop("BRR", "plain1009", schedule, {"sweep": sweep, "per-launch": launches})
    d = max(gc.rel(a, b) for a, b in zip(sweep, launches))
    print("sweep vs per-launch", float(f"{d:.3g}"))
    assert d < PATHS
    if schedule == (7, 0, 7):
        assert gc.rel(sweep[0], np.concatenate([[ref["mu_last"]], ref["b_last"]])) < LOOP


# ---- 3. the sweep's boundaries -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain1009", "wide1009", "counts1009"])
def test_gpu_sweep_first_shape(gbm_env, name):
    """n = 1009 is the first n the sweep takes on 256 CUs: 64 workgroups of 16 individuals (the last
    holds one) owning 8 rows of a super-block each; with p = 4200, nine super-blocks; with counts
    at scale 1, bytes >= 128 through the sweep's own unpacking. Path 4 without a fall-back, equal
    to the per-launch path to 1e-10 and to the loop to 1e-9. Measured on an MI355X: worst error
    against the loop 4.0e-15 (`wide1009`, y_pred), between the paths 1.6e-15."""
    needs_256_cus()
    _, fb0 = brr_path()
    sweep = fit("BRR", name)
    assert brr_path() == (4, fb0)
    shape = brr_shape()
    assert (shape["C"], shape["R"], shape["Ko"], shape["Kn"]) == (64, 8, 16, 16), shape
    gbm_env.setenv("GBM_BRR_SWEEP", "0")
    launches = fit("BRR", name)
    assert brr_path() == (0, fb0)
    check_against_loop("BRR", name, None, {"sweep": sweep, "per-launch": launches})
    d = max(gc.rel(a, b) for a, b in zip(sweep, launches))
    print("sweep vs per-launch", float(f"{d:.3g}"))
    assert d < PATHS


def test_gpu_sweep_first_excluded_shape():
    """n = 1008: 63 workgroups would own 10 rows each, more than the sweep's 8, so the per-launch
    byte path runs by itself (path 0, no fall-back counted). Measured on an MI355X: 6.1e-16."""
    needs_256_cus()
    _, fb0 = brr_path()
    got = fit("BRR", "plain1008")
    assert brr_path() == (0, fb0)
    check_against_loop("BRR", "plain1008", None, {"per-launch": got})


def test_gpu_one_past_the_sweep():
    """n = 48·min(CUs, 256) + 1: chunks of 48 individuals no longer cover the data, and the
    per-launch byte path runs with no knob set. Measured on an MI355X (n = 12 289): 7.2e-16."""
    cus = device_cus()
    _, fb0 = brr_path()
    got = fit("BRR", "over", cus=cus)
    assert brr_path() == (0, fb0)
    check_against_loop("BRR", "over", None, {"per-launch": got}, cus=cus)


# ---- 4. the pooled context across keys -------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["BRR", "BayesB"])
def test_gpu_pooled_context_across_keys(gbm_env, sampler):
    """Fit A (`plain300`); `tetra` (A's n, p and buffers, another byte scale: a stale captured
    iteration would run it at scale 2); A thinned; `wide48` (another shape); A again. The two A
    fits are equal bit for bit, and the `tetra` fit in the middle has the bytes of a `tetra` fit
    that did not follow A. Every fit is also within 1e-9 of the loop (measured on an MI355X:
    at most 1.0e-14, `wide48`)."""
    cold = _COLD.get((sampler, "tetra"))
    if cold is None:
        cold = fit(sampler, "tetra")
    a1 = fit(sampler, "plain300")
    tetra = fit(sampler, "tetra")
    thinned = fit(sampler, "plain300", (13, 4, 3))
    wide = fit(sampler, "wide48")
    a2 = fit(sampler, "plain300")
    for u, v in zip(a1, a2):
        assert np.array_equal(u, v)
    for u, v in zip(tetra, cold):
        assert np.array_equal(u, v)
    check_against_loop(sampler, "plain300", gc.DEFAULT, {"first": a1})
    check_against_loop(sampler, "tetra", None, {"after plain300": tetra})
    check_against_loop(sampler, "plain300", (13, 4, 3), {"thinned": thinned})
    check_against_loop(sampler, "wide48", None, {"wide48": wide})


# ---- markers without variance ------------------------------------------------------------------------
def test_gpu_constant_genotypes_are_refused():
    """Every cell 0.5: Σx²/n − Σ mean² is exactly 0, and both fits return GBM_E_DATA."""
    X = np.full((300, 130), 0.5, order="F")
    y = gc.case("plain300")[1]
    for call in (lambda: gbm.brr_arrays(X, y, n_iter=3, n_burnin=1, thin=1),
                 lambda: gbm.bayes_arrays("BayesA", X, y, n_iter=3, n_burnin=1, thin=1),
                 lambda: gbm.bayes_arrays("BayesB", X, y, n_iter=3, n_burnin=1, thin=1),
                 lambda: gbm.bayes_arrays("BayesC", X, y, n_iter=3, n_burnin=1, thin=1)):
        with pytest.raises(gbm.GBMError, match="no variance") as ei:
            call()
        assert ei.value.code == _lib.GBM_E_DATA
    # the context that refused serves the next fit
    check_against_loop("BRR", "plain300", gc.DEFAULT, {"after the refusal": fit("BRR", "plain300")})
