"""The GWAS scan's own edges on the default factorisation path (gbm_session_gwas, gwas_stats_kernel<K>,
gbm_dev_whiten_rows): every covariate count the statistics kernel is instantiated for, training sets at the
API minima and at every n mod 4, 18 column blocks, strips and chunks of 1, 63, 64 and 65 loci, more than
32 768 rows in one statistics launch, whitening with 1, 63, 64 and 65 rows in a buffer wider and longer than
the rows it whitens, and an int8 session. The inputs and references are those of tests/gwas_cases.py (their
own agreement and margins: tests/test_gwas_cases.py); the bound is tests/test_gpu_gwas.py's 1e-9 of max|z|
and of max|b|, dropped loci exactly 0."""
import ctypes
import functools

import numpy as np
import pytest

import gbm
import oracle
from gbm import _lib

import gwas_cases as gc

pytestmark = pytest.mark.gpu

TOL = 1e-9
TOL_WHITEN = 1e-10


def scan(s, name):
    c = gc.CASES[name]
    idx, _, y, C = gc.inputs(name)
    return s.gwas(idx, y, covariates=C, model=c.model, sigma2=c.s2)


def check(r, name):
    c = gc.CASES[name]
    z, b, _ = gc.reference(name)
    m = gc.compared(name)
    ez, eb = gc.rel(r["z"][m], z[m]), gc.rel(r["b"][m], b[m])
    print(f"{name}: z rel err {ez:.3e} b rel err {eb:.3e} tested {r['tested']}")
    assert ez < TOL and eb < TOL
    assert np.all(r["z"][~m] == 0.0) and np.all(r["b"][~m] == 0.0)
    assert r["tested"] == c.tested == int(m.sum())
    assert (r["sigma2_e"], r["sigma2_u"]) == (c.s2 if c.model == "mlm" else (None, None))


@pytest.fixture(scope="module")
def sessions():
    """One session per input, opened when first asked for."""
    open_ = {}

    def get(dname):
        if dname not in open_:
            open_[dname] = gbm.GenotypeSession(gc.data(dname)[0])
        return open_[dname]

    yield get
    for s in open_.values():
        s.close()


# ---- covariate counts -------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["mlm", "ols"])
@pytest.mark.parametrize("kc", [3, 4, 5, 6, 7])
def test_every_covariate_count(sessions, kc, model):
    """gwas_stats_kernel<K> for K = kc + 1 = 4 … 8; the mixed model reads a (kc + 2)² Schur block."""
    name = f"fix-kc{kc}-{model}"
    assert gc.CASES[name].kc == kc
    check(scan(sessions("fixture"), name), name)


def test_seven_covariates_at_a_small_lambda(sessions):
    assert gc.CASES["fix-kc7-small"].s2 == (1e-3, 1.0)
    check(scan(sessions("fixture"), "fix-kc7-small"), "fix-kc7-small")


def test_locus_in_the_span_of_two_covariates_is_dropped(sessions):
    name = "fix-span2"
    r = scan(sessions("fixture"), name)
    j = int(np.nonzero(gc.reference(name)[2])[0][gc.SPAN_LOCUS])
    assert not gc.compared(name)[j] and r["z"][j] == 0.0 and r["b"][j] == 0.0
    assert r["tested"] == gc.CASES["fix-kc3-mlm"].tested - 1
    check(r, name)  # every other locus against the reference


@pytest.mark.parametrize("model", ["mlm", "ols"])
def test_collinear_covariates_are_a_data_error(sessions, model):
    idx, _, y, C = gc.inputs("fix-kc3-mlm")
    for bad in (np.column_stack([C[:, 0], C[:, 1], C[:, 0] + C[:, 1]]), np.column_stack([C[:, 0], C[:, 0]]),
                np.column_stack([C[:, 0], np.full(idx.size, 2.0)])):  # a sum, a duplicate, the intercept again
        with pytest.raises(gbm.GBMError, match="collinear") as e:
            sessions("fixture").gwas(idx, y, covariates=bad, model=model, sigma2=gc.S2)
        assert e.value.code == _lib.GBM_E_DATA


# ---- training-set sizes -----------------------------------------------------------------------

@pytest.mark.parametrize("name", [k for k in gc.CASES if k.startswith("tiny-")])
def test_training_sets_at_the_api_minimum(sessions, name):
    """n_train = 3 (kc = 0) and n_train = kc + 3 = 10 (kc = 7): the smallest the scan accepts, one 128-wide tile
    that is almost all padding; n_train = 12 beside them."""
    c = gc.CASES[name]
    assert c.n_train in (3, 10, 12) and c.n_train >= c.kc + 3
    check(scan(sessions("tiny"), name), name)
    if c.n_train == c.kc + 3:
        idx, _, y, C = gc.inputs(name)
        with pytest.raises(gbm.ArgumentError, match="at least kc"):
            sessions("tiny").gwas(idx[1:], y[1:], covariates=None if C is None else C[1:], model=c.model, sigma2=c.s2)


@pytest.mark.parametrize("name", [k for k in gc.CASES if k.startswith("fix-n")])
def test_ragged_last_quad(sessions, name):
    """n_train = 130, 131, 257: n mod 4 = 2, 3, 1 through the statistics kernel's last, partial group of four."""
    assert gc.CASES[name].n_train % 4 in (1, 2, 3)
    check(scan(sessions("fixture"), name), name)


def test_eighteen_column_blocks(sessions):
    """n_train = 1100: the whitening sweep's two-register-set prefetch (m + 3 < k) at depth."""
    check(scan(sessions("n1100"), "n1100-kc7"), "n1100-kc7")


# ---- strips and chunks ------------------------------------------------------------------------

def test_chunks_of_one_strip_more_and_less(sessions, gbm_env):
    s, got = sessions("p130"), []
    for chunk in (1, 63, 64, 65, None):
        if chunk is None:
            gbm_env.delenv("GBM_GWAS_CHUNK")
        else:
            gbm_env.setenv("GBM_GWAS_CHUNK", str(chunk))
        got.append(scan(s, "p130"))
    check(got[-1], "p130")
    for r in got[:-1]:
        assert np.array_equal(r["z"], got[-1]["z"]) and np.array_equal(r["b"], got[-1]["b"])
        assert r["tested"] == got[-1]["tested"]


# ---- more than 32 768 rows in one statistics launch --------------------------------------------

@pytest.mark.parametrize("model", ["ols", "mlm"])
def test_grid_stride_loop_of_the_statistics_kernel(sessions, model):
    """p = 33 000 > 4 waves x 8192 workgroups: OLS is one launch over Z, the mixed model one chunk of 33 000
    (128 x 8 bytes a row: far under the 768 MB cap). Loci without variance on both sides of 32 768 return 0;
    row 32 768 itself, the first of the second sweep and the only one a stride of nwaves + 1 skips, is a tested
    locus."""
    name = f"long-{model}"
    r = scan(sessions("long"), name)
    flat = list(gc.FLAT)
    assert min(flat) < 32768 <= max(flat) and not r["z"][flat].any() and not r["b"][flat].any()
    assert gc.compared(name)[32767:32770].all()  # the first rows of the second sweep are tested loci
    check(r, name)
    m = gc.compared(name)
    assert np.all(r["z"][m] != 0.0)  # every tested locus was written, past row 32 767 too


# ---- whitening: row counts, strides, rows past the end -------------------------------------------

SENTINEL = 7.25


@functools.lru_cache(maxsize=None)
def factored(n, lam=0.6):
    """(stages after the solve, U) of the fixture's first n rows."""
    import torch

    from gbm.sharded import HipShardStages
    X, y = gc.data("fixture")
    X, y = np.asfortranarray(X[:n]), y[:n].copy()
    st = HipShardStages(n, X.shape[1], nrhs=1, lambda_=lam, device=0)
    st.upload_genotypes(X.copy())
    st.load_phenotypes(y)
    st.standardize()
    st.grm_syrk()
    st.grm_reduce()
    st.solve()
    torch.cuda.synchronize()
    assert int(st.info.item()) == 0
    K, _ = oracle.grm(X)
    return st, np.linalg.inv(np.linalg.cholesky(K + lam * np.eye(n)).T)


@pytest.mark.parametrize("n", [100, 333])
def test_whitening_row_counts_and_strides(n):
    """rows = 1, 63, 64, 65 at nb = 2 and nb = 6 column blocks, in a buffer of rows + 3 rows with ldr = npad + 2:
    the two extra columns and the rows past `rows` keep their sentinel, the padding columns stay 0, and a row's
    bits do not depend on the launch it fell into."""
    import torch
    st, Uinv = factored(n)
    npad, ldr = st.npad, st.npad + 2
    assert npad == {100: 128, 333: 384}[n]
    lib = gbm.load_library()
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())
    Rn = np.random.default_rng(9).standard_normal((65, n))
    first = None
    for rows in (65, 1, 63, 64):
        host = np.full((rows + 3, ldr), SENTINEL)
        host[:rows, :npad] = 0.0
        host[:rows, :n] = Rn[:rows]
        R = torch.from_numpy(host).to(st.dev)
        _lib.check(lib.gbm_dev_whiten_rows(p_(st.G), st.gdim, n, p_(st.ws_solve), p_(R), ldr, rows, st._stream()),
                   "gbm_dev_whiten_rows")
        torch.cuda.synchronize()
        got = R.cpu().numpy()
        err = gc.rel(got[:rows, :n], Rn[:rows] @ Uinv)
        print(f"whitening n={n} rows={rows} ldr={ldr}: rel err {err:.3e}")
        assert err < TOL_WHITEN
        assert np.all(got[:rows, n:npad] == 0.0)
        assert np.all(got[:, npad:] == SENTINEL) and np.all(got[rows:] == SENTINEL)
        if first is None:
            first = got[:65, :npad].copy()
        else:
            assert np.array_equal(got[:rows, :npad], first[:rows])


# ---- int8 session ------------------------------------------------------------------------------

def test_dosage_i8_session_scans_the_same_bits(sessions):
    """The int8 session in its default GRM mode against the f64 session on the same dosages, as
    test_session_dosage_i8_matches_f64 asserts for gblup."""
    name = "fix-kc3-mlm"
    ra = scan(sessions("fixture"), name)
    with gbm.GenotypeSession(dosage_i8=gc.dosage_i8(), ploidy=2) as s:
        rb = scan(s, name)
    assert np.array_equal(ra["z"], rb["z"]) and np.array_equal(ra["b"], rb["b"]) and ra["tested"] == rb["tested"]
    check(rb, name)
