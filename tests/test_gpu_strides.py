"""Every host entry of the C ABI at a leading dimension larger than the row count (include/gbm.h: ldx, ldd,
ldy, ldg, ldb, ldo). A Julia caller passes `stride(X, 2)`, so a view into a larger parent array reaches these
paths; the Python wrappers always pass ld == n, and so did every test before this file.

Each input is embedded in a column-major parent with 5 or 64 extra rows per column (n = 333 is odd, so n + 5
leaves the columns only 8-byte aligned) whose padding rows hold a poison: NaN for fp64, the byte 77 (not a
dosage) for int8. Strided outputs are pre-filled with a sentinel that must survive in their padding rows.

For each call: the results equal the same call on the contiguous copy bit for bit (the stride changes only the
host side of a copy, so the device sees the same bytes, and these paths are bit-reproducible run to run), and
they match the oracle at the tolerances of test_gpu_parity.py."""
import numpy as np
import pytest

import oracle

import abi_direct as abi
from abi_direct import Mat, rel

pytestmark = pytest.mark.gpu

TOL_CONTRACT = 1e-6   # b_hat, relative to max |b|
TOL_TIGHT = 1e-9      # GEBVs, mu
TOL_G = 1e-12
N, P, T, LAM = 333, 1777, 3, 1.0
PADS = [5, 64]
FP64, EXACT = abi.MODES["fp64"], abi.MODES["exact"]

# name -> (knobs, devices). p = 1777: GBM_HOST_CHUNK = 500 gives the pipelined upload four chunks,
# GBM_STREAM_CHUNK = 500 the loci-streamed path four, GBM_PACK_CHUNK = 300 the host packer six (more than its ring)
CONFIGS = {
    "host_pack_1": ({"GBM_HOST_PACK": "1"}, None),
    "host_pack_0": ({"GBM_HOST_PACK": "0"}, None),
    "pack_threads_3": ({"GBM_PACK_THREADS": "3"}, None),
    "pack_threads_3_chunks": ({"GBM_PACK_THREADS": "3", "GBM_PACK_CHUNK": "300"}, None),
    "host_chunk_packed": ({"GBM_HOST_CHUNK": "500", "GBM_HOST_PACK": "1"}, None),
    "host_chunk_fp64": ({"GBM_HOST_CHUNK": "500", "GBM_HOST_PACK": "0"}, None),
    "streamed": ({"GBM_STREAM_CHUNK": "500"}, None),
    "two_shards": ({}, [0, 0]),
    "two_shards_host_chunk": ({"GBM_HOST_CHUNK": "500", "GBM_HOST_PACK": "0"}, [0, 0]),
}


@pytest.fixture(scope="module")
def data():
    X = oracle.synth_genotypes(7, N, P)
    Y = oracle.synth_phenotypes(X, 8, ntraits=T)
    Xr = np.asfortranarray(np.random.default_rng(70).random((N, P)))  # pooled allele frequencies: any real in [0, 1]
    return {"X": X, "Y": Y, "D": np.rint(2.0 * X).astype(np.int8), "ref": oracle.gblup_fit(X, Y, LAM),
            "Xr": Xr, "ref_r": oracle.gblup_fit(Xr, Y, LAM)}


def set_knobs(gbm_env, knobs):
    for name in ("GBM_HOST_PACK", "GBM_PACK_THREADS", "GBM_PACK_CHUNK", "GBM_HOST_CHUNK", "GBM_STREAM_CHUNK"):
        if name in knobs:
            gbm_env.setenv(name, knobs[name])
        else:
            gbm_env.delenv(name, raising=False)


def same_fit(a, b):
    """b_hat, y_pred, mu bit for bit; q and the GRM used."""
    return all(np.array_equal(a[k], b[k]) for k in range(3)) and a[3:] == b[3:]


def fit_matches(fit, ref):
    b, y, mu, q = fit[:4]
    assert q == ref["q"]
    assert rel(y, ref["y_pred"]) < TOL_TIGHT
    assert rel(mu, ref["mu"]) < TOL_TIGHT
    assert rel(b, ref["b_hat"]) < TOL_CONTRACT


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ["fp64", "exact", "auto"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_gblup_fit_ex_strided_x_and_y(gbm_env, data, config, mode, pad):
    knobs, devices = CONFIGS[config]
    set_knobs(gbm_env, knobs)
    flat = abi.gblup_fit_ex(Mat(data["X"]), Mat(data["Y"]), LAM, mode, devices)
    wide = abi.gblup_fit_ex(Mat(data["X"], pad), Mat(data["Y"], pad), LAM, mode, devices)
    assert wide[4] == (FP64 if mode == "fp64" else EXACT)
    assert same_fit(wide, flat)
    fit_matches(wide, data["ref"])


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ["fp64", "auto"])
@pytest.mark.parametrize("config", ["host_pack_1", "host_chunk_packed", "host_chunk_fp64", "two_shards_host_chunk"])
def test_gblup_fit_ex_strided_real_valued_x(gbm_env, data, config, mode, pad):
    """Uniform reals are no dosages: grm_mode fp64 tries the packed pipeline (GBM_HOST_CHUNK with GBM_HOST_PACK = 1)
    and leaves it at the first chunk for the fp64 upload; auto tries the host packer and falls back to the fp64
    path. Exact refuses them."""
    knobs, devices = CONFIGS[config]
    set_knobs(gbm_env, knobs)
    flat = abi.gblup_fit_ex(Mat(data["Xr"]), Mat(data["Y"]), LAM, mode, devices)
    wide = abi.gblup_fit_ex(Mat(data["Xr"], pad), Mat(data["Y"], pad), LAM, mode, devices)
    assert wide[4] == FP64
    assert same_fit(wide, flat)
    fit_matches(wide, data["ref_r"])
    assert abi.gblup_fit_ex(Mat(data["Xr"], pad), Mat(data["Y"], pad), LAM, "exact", devices, raw=True) == abi._lib.GBM_E_ARG


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ["fp64", "exact"])
@pytest.mark.parametrize("config", ["host_pack_1", "host_chunk_fp64", "streamed", "two_shards", "two_shards_host_chunk"])
def test_dosage_i8_fit_ex_strided(gbm_env, data, config, mode, pad):
    knobs, devices = CONFIGS[config]
    set_knobs(gbm_env, knobs)
    flat = abi.dosage_fit_ex(Mat(data["D"]), 2, Mat(data["Y"]), LAM, mode, devices)
    wide = abi.dosage_fit_ex(Mat(data["D"], pad), 2, Mat(data["Y"], pad), LAM, mode, devices)
    assert wide[4] == (FP64 if mode == "fp64" else EXACT)
    assert same_fit(wide, flat)
    fit_matches(wide, data["ref"])


@pytest.mark.parametrize("pad,mode", [(5, "fp64"), (64, "fp64"), (5, "exact")])
def test_reml_fit_ex_strided(data, pad, mode):
    """Strided X and Y; the entry reads trait t at Y + t*ldy for the REML search and for the fit."""
    X, Y = data["X"], data["Y"]
    flat = abi.reml_fit_ex(Mat(X), Mat(Y), mode)
    wide = abi.reml_fit_ex(Mat(X, pad), Mat(Y, pad), mode)
    for a, b in zip(wide, flat):
        assert np.array_equal(a, b)
    lam = wide[4]
    for t in range(T):
        ref = oracle.gblup_fit(X, Y[:, t], float(lam[t]))
        assert wide[3] == ref["q"]
        assert rel(wide[1][:, t], ref["y_pred"][:, 0]) < TOL_TIGHT
        assert rel(wide[2][t], ref["mu"][0]) < TOL_TIGHT
        assert rel(wide[0][:, t], ref["b_hat"][:, 0]) < TOL_CONTRACT


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_grm_strided_in_and_out(data, devices, pad):
    X = data["X"]
    Gf, qf = abi.grm(Mat(X), 0, devices)
    Gw, qw = abi.grm(Mat(X, pad), pad, devices)
    assert qw == qf == data["ref"]["q"]
    assert abi.padding_untouched(Gw, N)
    assert np.array_equal(Gw[:N], Gf)
    assert rel(Gw[:N], data["ref"]["G"]) < TOL_G
    assert np.array_equal(Gw[:N], Gw[:N].T)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_grm_ploidy_aware_strided_in_and_out(devices, pad):
    ploidy = 4
    X = np.round(np.random.default_rng(N + P).random((N, P)) ** 2 * ploidy) / ploidy
    X[:, 3] = 0.5
    Gf, denf = abi.grm_ploidy_aware(Mat(X), ploidy, 0, devices)
    Gw, denw = abi.grm_ploidy_aware(Mat(X, pad), ploidy, pad, devices)
    ref, den_ref = oracle.grm_ploidy_aware(X, ploidy)
    assert denw == denf and abs(denw - den_ref) <= 1e-12 * den_ref
    assert abi.padding_untouched(Gw, N)
    assert np.array_equal(Gw[:N], Gf)
    assert rel(Gw[:N], ref) < TOL_G


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("which", ["X", "Xr"])
def test_colstats_strided(data, which, pad):
    X = data[which].copy()
    X[:, 11] = 0.5  # a monomorphic column
    mf, sf, kf, qf = abi.colstats(Mat(X))
    mw, sw, kw, qw = abi.colstats(Mat(X, pad))
    assert qw == qf and np.array_equal(mw, mf) and np.array_equal(sw, sf) and np.array_equal(kw, kf)
    mr, sr, kr = oracle.colstats(X)
    assert qw == kr.sum() and np.array_equal(kw, kr) and not kw[11]
    assert rel(mw, mr) < 1e-14 and rel(sw[kw], sr[kr]) < 1e-13


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("which", ["X", "Xr"])
def test_predict_strided_x_b_and_out(data, which, pad):
    X = data[which]
    B = data["ref" if which == "X" else "ref_r"]["b_hat"]
    flat = abi.predict(Mat(X), Mat(B))
    wide = abi.predict(Mat(X, pad), Mat(B, pad), pad)
    assert abi.padding_untouched(wide, N)
    assert np.array_equal(wide[:N], flat)
    assert rel(wide[:N], oracle.predict_linear(X, B)) < TOL_TIGHT


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("source,grm", [("f64", "fp64"), ("f64", "exact"), ("i8", "fp64"), ("i8", "exact")])
def test_session_strided_create_fit_predict(data, source, grm, pad):
    """gbm_session_create (ldx) / gbm_session_create_dosage_i8 (ldd), gbm_session_gblup_fit (ldy) on a strict
    subset of the rows and gbm_session_predict (ldb, ldo) on the others."""
    X, Y = data["X"], data["Y"]
    rng = np.random.default_rng(5)
    train = np.sort(rng.choice(N, size=250, replace=False))
    val = np.setdiff1d(np.arange(N), train)
    src = data["D"] if source == "i8" else X
    ploidy = 2 if source == "i8" else None
    with abi.Session(Mat(src), ploidy, grm=grm) as s0, abi.Session(Mat(src, pad), ploidy, grm=grm) as s1:
        flat = s0.fit(train, Mat(Y[train]), LAM)
        wide = s1.fit(train, Mat(Y[train], pad), LAM)
        pf = s0.predict(val, Mat(flat[0]))
        pw = s1.predict(val, Mat(wide[0], pad), pad)
    assert same_fit(wide, flat)
    fit_matches(wide, oracle.gblup_fit(X[train], Y[train], LAM))
    assert abi.padding_untouched(pw, val.size)
    assert np.array_equal(pw[:val.size], pf)
    assert rel(pw[:val.size], oracle.predict_linear(X[val], wide[0])) < TOL_TIGHT


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("which", ["dosage", "real"])
def test_brr_fit_strided(which, pad):
    """gbm_brr_fit (ldx): the same sample path as the contiguous call (same seed), and as the oracle's sampler
    at the tolerance of test_brr.py. Dosages are stored as bytes on the device, reals as fp64."""
    n, p, iters = 203, 150, 6
    X = oracle.synth_genotypes(61, n, p) if which == "dosage" else np.random.default_rng(61).random((n, p))
    y = oracle.synth_phenotypes(X, 62)[:, 0]
    flat = abi.brr_fit(Mat(X), y, iters, 2, 1, 99)
    wide = abi.brr_fit(Mat(X, pad), y, iters, 2, 1, 99)
    for a, b in zip(wide, flat):
        assert np.array_equal(a, b)
    ref = oracle.brr_gibbs(X, y, n_iter=iters, n_burnin=2, thin=1, seed=99)
    assert rel(wide[0], ref["b_hat"]) < 1e-9 and rel(wide[1], ref["y_pred"]) < 1e-9
    assert abs(wide[2][0] - ref["varE"]) < 1e-9 * ref["varE"] and abs(wide[2][1] - ref["varB"]) < 1e-9 * ref["varB"]
