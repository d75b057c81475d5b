"""Drop-in device farming and the in-process multi-shard path of the C ABI (SURVEY.md §8b
Threading, §8e):

* explicit device lists with a repeated ordinal (devices=[0, 0]): SNP-column shards on one
  device, their packed partial GRMs added on the device, the b_hat shard offsets and the Σ m_j b_j
  assembly — against the oracle;
* devices=NULL under an unchanged cvmultithread!: each calling thread is given one device from
  GBM_DEVICES (round-robin by first call); eight threads at once are bit-identical to serial;
* pooled contexts: after a warm-up call, a call of the same shape makes no device allocation.
"""
import threading

import numpy as np
import pytest

import gbm
import oracle
from gbm import _lib

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
@pytest.mark.parametrize("n,p,t", [(333, 1777, 3), (1030, 2501, 1)])
def test_same_device_shards_match_oracle(devices, n, p, t):
    X = oracle.synth_genotypes(n + p, n, p)
    X[:, 5] = 0.5  # monomorphic locus inside shard 0
    Y = oracle.synth_phenotypes(X, 11, ntraits=t)
    b_hat, y_pred, mu, q = gbm.gblup_arrays(X, Y, lambda_=0.9, devices=devices)
    ref = oracle.gblup_fit(X, Y, 0.9)
    assert q == ref["q"]
    assert rel(y_pred, ref["y_pred"]) < 1e-9
    assert rel(mu, ref["mu"]) < 1e-9
    assert rel(b_hat, ref["b_hat"]) < 1e-6
    assert b_hat[1 + 5].tolist() == [0.0] * t
    G, qg = gbm.grm(X, devices=devices)
    Gr, qr = oracle.grm(X)
    assert qg == qr and rel(G, Gr) < 1e-12


@pytest.mark.parametrize("devices,n,lims,tail", [
    ([0, 0], 1500, ("0", "-1", "-1"), "256"),       # 4-panel groups, early switch to the redundant tail
    ([0, 0, 0], 1500, ("0", "-1", "-1"), "0"),      # 4-panel groups down to the 2-panel / single-panel tail
    ([0, 0, 0, 0], 3000, ("0", "0", "0"), "0"),     # 16, 8, 4, 2-panel groups, then single panels
    ([0, 0], 1030, ("0", "0", "0"), "512"),         # ragged n
])
def test_cabi_distributed_factorisation_bit_identical(gbm_env, devices, n, lims, tail):
    """gbm_gblup_fit with several device leaders factors V across them (solve_distributed in
    dist_solve.cpp: own-tile trailing updates, strip all-gathers, redundant tail). Rehearsed on one GPU
    with every shard its own leader (GBM_SHARD_LEADERS=each: copy all-reduce and copy all-gather
    in place of RCCL); bit-identical to the default path, where the shards' partial GRMs are summed
    on the device and one leader solves redundantly."""
    gbm_env.setenv("GBM_CHOL_G4_LIM", lims[0])
    gbm_env.setenv("GBM_CHOL_G8_LIM", lims[1])
    gbm_env.setenv("GBM_CHOL_G16_LIM", lims[2])
    gbm_env.setenv("GBM_UPD64_LIM", "128")
    gbm_env.setenv("GBM_CHOL_FLOW_MAX", "0")  # both sides on the launch-per-panel solve
    X = oracle.synth_genotypes(n + len(devices), n, 1900)
    Y = oracle.synth_phenotypes(X, 3, ntraits=2)
    ref = gbm.gblup_arrays(X, Y, lambda_=0.8, devices=devices)
    gbm_env.setenv("GBM_SHARD_LEADERS", "each")
    gbm_env.setenv("GBM_DIST_SOLVE_MIN_N", "0")
    gbm_env.setenv("GBM_DIST_TAIL_ROWS", tail)
    got = gbm.gblup_arrays(X, Y, lambda_=0.8, devices=devices)
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    fit = oracle.gblup_fit(X, Y, 0.8)
    assert rel(got[1], fit["y_pred"]) < 1e-9 and rel(got[0], fit["b_hat"]) < 1e-6
    G, qg = gbm.grm(X, devices=devices)  # the copy all-reduce of the GRM entry
    Gr, qr = oracle.grm(X)
    assert qg == qr and rel(G, Gr) < 1e-12


@pytest.mark.slow
def test_cabi_distributed_factorisation_default_thresholds():
    """The same at a size where the default thresholds choose the distributed solve themselves
    (n = 20 000 >= GBM_DIST_SOLVE_MIN_N = 16 384; 16- to 2-panel groups, the tail below 8 192
    rows): two device leaders (GBM_SHARD_LEADERS=each on one GPU) against one leader solving
    redundantly, bit for bit; genotypes generated on the device."""
    import os
    n, p = 20000, 6000
    rng = np.random.default_rng(7)
    Y = np.asfortranarray(rng.standard_normal((n, 2)))
    assert "GBM_DIST_SOLVE_MIN_N" not in os.environ
    ref = gbm.gblup_synthetic(99, n, p, Y, lambda_=0.5, devices=[0, 0])
    from gbm import _lib
    _lib.debug_set("GBM_SHARD_LEADERS", "each")
    try:
        got = gbm.gblup_synthetic(99, n, p, Y, lambda_=0.5, devices=[0, 0])
    finally:
        _lib.debug_set("GBM_SHARD_LEADERS", None)
        gbm.load_library().gbm_release_device_cache()
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    b_hat, y_pred, mu, q = got
    assert q == p and np.all(np.isfinite(y_pred))


def test_synthetic_fit_two_shards_one_device():
    n, p = 700, 3001
    X = oracle.synth_genotypes(4242, n, p)
    Y = oracle.synth_phenotypes(X, 5, ntraits=2)
    b1, y1, mu1, q1 = gbm.gblup_synthetic(4242, n, p, Y, devices=[0, 0])
    ref = oracle.gblup_fit(X, Y, 1.0)
    assert q1 == ref["q"] and rel(y1, ref["y_pred"]) < 1e-9 and rel(b1, ref["b_hat"]) < 1e-6


def test_no_device_allocation_after_warmup():
    lib = gbm.load_library()
    X = oracle.synth_genotypes(21, 1030, 2000)
    Y = oracle.synth_phenotypes(X, 22, ntraits=2)
    first = gbm.gblup_arrays(X, Y, lambda_=1.0)
    a0 = lib.gbm_device_allocations()
    for _ in range(3):
        again = gbm.gblup_arrays(X, Y, lambda_=1.0)
        assert np.array_equal(again[1], first[1]) and np.array_equal(again[0], first[0])
    gbm.gblup_arrays(X[:500], Y[:500], lambda_=1.0)  # smaller: fits the pooled buffers
    assert lib.gbm_device_allocations() == a0
    gbm.grm(X)
    a1 = lib.gbm_device_allocations()
    gbm.grm(X)
    assert lib.gbm_device_allocations() == a1
    _lib.check(lib.gbm_release_device_cache(), "release")
    gbm.gblup_arrays(X, Y, lambda_=1.0)
    assert lib.gbm_device_allocations() > a1  # the cache was really dropped


def test_gbm_devices_farming_eight_threads(gbm_env):
    """cvmultithread! calls the model from Threads.@threads with no devices argument: every
    thread takes its own slot of GBM_DEVICES. Eight threads on a one-GPU box (GBM_DEVICES lists
    device 0 eight times) give the serial results bit for bit, and once the pool holds a context
    per concurrent call, a round allocates nothing (each call leases a pooled context)."""
    gbm_env.setenv("GBM_DEVICES", ",".join(["0"] * 8))
    lib = gbm.load_library()
    lib.gbm_release_device_cache()
    X = oracle.synth_genotypes(5, 1030, 1400)
    cases = [oracle.synth_phenotypes(X, 300 + k, ntraits=2) for k in range(8)]
    serial = [gbm.gblup_arrays(X, Y, lambda_=0.7) for Y in cases]

    def round_of_threads():
        out, errs = [None] * 8, []

        def run(k):
            try:
                out[k] = gbm.gblup_arrays(X, cases[k], lambda_=0.7)
            except Exception as e:  # reported below
                errs.append(repr(e))

        th = [threading.Thread(target=run, args=(k,)) for k in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        return out

    # each round either allocates (a new context, or growing one last used for another shape) or
    # not; once eight contexts of this shape exist, no round of eight threads allocates
    quiet = False
    for _ in range(10):
        a0 = lib.gbm_device_allocations()
        for a, b in zip(round_of_threads(), serial):
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
        if lib.gbm_device_allocations() == a0:
            quiet = True
            break
    assert quiet


def test_gbm_devices_bad_ordinal_is_an_argument_error(gbm_env):
    gbm_env.setenv("GBM_DEVICES", "0,4096")
    X = oracle.synth_genotypes(1, 50, 100)
    with pytest.raises(gbm.ArgumentError):
        gbm.gblup_arrays(X, np.arange(50.0))


@pytest.mark.parametrize("chunk,carry", [(500, None), (1024, None), (1200, None), (1200, "1")])
def test_pipelined_host_upload_matches_oracle(gbm_env, chunk, carry):
    """gbm_gblup_fit with the host genotypes uploaded in loci chunks overlapped with the device
    work (GBM_HOST_CHUNK, re-read per call): chunk GRMs summed in order into G. Matches the oracle
    and the one-piece upload to rounding; the int8 entry (same chunks) stays bit-identical. Chunks
    after the first are added into G by the GRM itself (slab reduce, or range 0 of the in-order
    carry when GBM_GRM_CARRY=1); 1200 = 1200 + the halving tail 550 + 550."""
    if carry is None:
        gbm_env.delenv("GBM_GRM_CARRY", raising=False)  # the planner's choice (slabs here)
    else:
        gbm_env.setenv("GBM_GRM_CARRY", carry)
    n, p = 700, 2300
    X = oracle.synth_genotypes(31, n, p)
    Y = oracle.synth_phenotypes(X, 32, ntraits=2)
    gbm_env.setenv("GBM_HOST_CHUNK", str(chunk))
    b_hat, y_pred, mu, q = gbm.gblup_arrays(X, Y, lambda_=0.8)
    ref = oracle.gblup_fit(X, Y, 0.8)
    assert q == ref["q"]
    assert np.abs(y_pred - ref["y_pred"]).max() < 1e-9 * np.abs(ref["y_pred"]).max()
    assert np.abs(b_hat - ref["b_hat"]).max() < 1e-6 * np.abs(ref["b_hat"]).max()
    D = np.rint(X * 2).astype(np.int8)
    lib = gbm.load_library()
    nrhs = Y.shape[1]
    Yf = np.asfortranarray(Y)
    b2 = np.zeros((p + 1, nrhs), order="F")
    y2 = np.zeros((n, nrhs), order="F")
    mu2 = np.zeros(nrhs)
    q2 = np.zeros(1, dtype=np.int64)
    Df = np.asfortranarray(D)
    rc = lib.gbm_gblup_fit_dosage_i8(Df.ctypes.data, n, p, n, 2, Yf.ctypes.data, n, nrhs, 0.8, None, 0,
                                     b2.ctypes.data, y2.ctypes.data, mu2.ctypes.data, q2.ctypes.data)
    assert rc == 0, lib.gbm_last_error()
    assert np.array_equal(y2, y_pred) and np.array_equal(b2, b_hat)
    gbm_env.setenv("GBM_HOST_CHUNK", "0")
    b3, y3, mu3, q3 = gbm.gblup_arrays(X, Y, lambda_=0.8)
    assert q3 == q and np.abs(y3 - y_pred).max() < 1e-11 * np.abs(y3).max()


@pytest.mark.parametrize("devices,chunk,leaders", [
    ([0, 0], "500", None), ([0, 0, 0], "700", None), ([0, 0], "500", "each"), ([0, 0], "0", None)])
def test_multi_shard_fit_concurrent_equals_serial(gbm_env, devices, chunk, leaders):
    """The in-process multi-device fit drives every shard's upload, standardisation and partial GRM
    from its own host thread (fit_ctx.h parallel_shards; VERDICT r02 Missing #1): shard k+1's upload
    no longer waits for shard k's GRM. Same-device shards rehearse it on one GPU. Bit-identical to
    the one-after-the-other schedule (GBM_SHARD_THREADS=0) for the chunked host upload, the
    one-piece upload, both leader modes, the int8 entry and the GRM entries; matches the oracle."""
    gbm_env.setenv("GBM_HOST_CHUNK", chunk)
    if leaders:
        gbm_env.setenv("GBM_SHARD_LEADERS", leaders)
    n, p = 700, 2900
    X = oracle.synth_genotypes(77, n, p)
    X[:, 3] = 0.5
    Y = oracle.synth_phenotypes(X, 78, ntraits=2)
    D = np.asfortranarray(np.rint(X * 2).astype(np.int8))
    Yf = np.asfortranarray(Y)
    lib = gbm.load_library()

    def i8_fit():
        b = np.zeros((p + 1, 2), order="F")
        y = np.zeros((n, 2), order="F")
        mu = np.zeros(2)
        q = np.zeros(1, dtype=np.int64)
        dv, nd = _lib.devices_arg(devices)
        rc = lib.gbm_gblup_fit_dosage_i8(D.ctypes.data, n, p, n, 2, Yf.ctypes.data, n, 2, 0.8, dv, nd,
                                         b.ctypes.data, y.ctypes.data, mu.ctypes.data, q.ctypes.data)
        assert rc == 0, lib.gbm_last_error()
        return b, y

    runs = {}
    for mode in ("1", "0"):
        gbm_env.setenv("GBM_SHARD_THREADS", mode)
        runs[mode] = (gbm.gblup_arrays(X, Y, lambda_=0.8, devices=devices), i8_fit(),
                      gbm.grm(X, devices=devices), gbm.grm_ploidy_aware(X, ploidy=2, devices=devices))
    (fit, i8, grm, gpa), (fit0, i80, grm0, gpa0) = runs["1"], runs["0"]
    for a, b in zip(fit, fit0):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(i8, i80):
        assert np.array_equal(a, b)
    assert np.array_equal(grm[0], grm0[0]) and grm[1] == grm0[1]
    assert np.array_equal(gpa[0], gpa0[0])
    ref = oracle.gblup_fit(X, Y, 0.8)
    assert fit[3] == ref["q"] and rel(fit[1], ref["y_pred"]) < 1e-9 and rel(fit[0], ref["b_hat"]) < 1e-6
    Gr, qr = oracle.grm(X)
    assert grm[1] == qr and rel(grm[0], Gr) < 1e-12


def _oom_counts():
    import ctypes
    r, f = ctypes.c_int64(0), ctypes.c_int64(0)
    gbm.load_library().gbm_debug_oom_retries(ctypes.byref(r), ctypes.byref(f))
    return r.value, f.value


def test_oom_retry_frees_idle_gblup_and_brr_contexts(gbm_env):
    """An allocation that runs out of device memory frees the idle pooled contexts of its device —
    the BRR pool's as well as the GBLUP pool's — and is retried once; the fit then
    succeeds with the same results. GBM_TEST_OOM_ONCE=1 makes every allocation's first attempt fail."""
    lib = gbm.load_library()
    lib.gbm_release_device_cache()
    X = oracle.synth_genotypes(404, 300, 800)
    Y = oracle.synth_phenotypes(X, 405)
    ref = gbm.gblup_arrays(X, Y, devices=[0])
    gbm.brr_arrays(X, Y[:, 0], n_iter=4, n_burnin=1, thin=1, seed=3)  # leaves an idle BRR context
    r0, f0 = _oom_counts()
    gbm_env.setenv("GBM_TEST_OOM_ONCE", "1")
    X2 = oracle.synth_genotypes(406, 420, 1300)  # a larger shape: the leased context must grow
    Y2 = oracle.synth_phenotypes(X2, 407)
    got = gbm.gblup_arrays(X2, Y2, devices=[0])
    gbm_env.delenv("GBM_TEST_OOM_ONCE")
    r1, f1 = _oom_counts()
    assert r1 > r0 and f1 >= f0 + 1  # the idle BRR context was freed by a retry
    want = gbm.gblup_arrays(X2, Y2, devices=[0])
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    again = gbm.gblup_arrays(X, Y, devices=[0])
    for a, b in zip(again, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_reml_fit_multi_leader_rehearsal(gbm_env):
    """gbm_gblup_fit_reml over several device leaders at a size that takes the distributed
    factorisation (devices=[0, 0], every shard its own leader, GBM_DIST_SOLVE_MIN_N=0):
    λ is chosen on the first leader, the other leaders' G restored from its pristine copy, and the
    fit equals the single-device REML fit."""
    X = oracle.synth_genotypes(515, 700, 3000)
    Y = oracle.synth_phenotypes(X, 516, ntraits=2)
    ref = gbm.gblup_reml_arrays(X, Y, devices=[0])
    gbm_env.setenv("GBM_SHARD_LEADERS", "each")
    gbm_env.setenv("GBM_DIST_SOLVE_MIN_N", "0")
    got = gbm.gblup_reml_arrays(X, Y, devices=[0, 0])
    assert got[3] == ref[3]
    # the two G differ by the rounding of the shard sum: the λ searches agree to their tolerance
    assert np.abs(got[4]["lambda"] - ref[4]["lambda"]).max() < 1e-5 * np.abs(ref[4]["lambda"]).max()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert rel(got[1], ref[1]) < 1e-6 and rel(got[0], ref[0]) < 1e-5
