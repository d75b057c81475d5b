"""Leading principal components of a session's cached GRM (GenotypeSession.pcs / gbm_session_pcs), and the two
device entries under it (gbm_dev_grm_symmetrize, gbm_dev_rows_times_sym), against numpy.

References: K_ref = ZZᵀ/q from numpy on the same rows (standardised as gwasprep does, src/gwas.jl:112-128) and, for
kind "reference", M_ref = K̃HK̃ᵀ in the literal form of gbm.gwas.pc1_of_grm. The eigenpair checks that hold whatever
the spectrum looks like (orthonormality, residual against M_ref, eigenvalues against eigvalsh, trace) are separated
from the eigenvector comparison, which is made only for pairs whose eigenvalue gap g (over λ₁) the test computes
and asserts to be >= 3e-3, with the bound |cos| >= 1 − (10·tol/g)²."""
import ctypes
import functools
import math
import os
import warnings

import numpy as np
import pytest

import gbm
import oracle
from gbm import _lib
from gbm.gwas import pc1_of_grm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ragged_333x1777_3traits.npz")
EPS = np.finfo(np.float64).eps
TOL = 1e-10


# ---- inputs and references (computed once, read-only) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    d = np.load(GOLDEN)
    D = np.asarray(d["dosage"], dtype=np.int8)
    X = np.asfortranarray(D.astype(np.float64) / float(d["ploidy"]))
    y = np.asarray(d["phenotypes"][:, 0], dtype=np.float64)
    for a in (D, X, y):
        a.setflags(write=False)
    return D, X, y


@functools.lru_cache(maxsize=None)
def four_populations():
    rng = np.random.default_rng(11)
    p = 1500
    f0 = rng.uniform(0.1, 0.9, p)
    rows = []
    for size in (100, 90, 70, 40):
        f = np.clip(f0 + 0.12 * rng.standard_normal(p), 0.02, 0.98)
        rows.append(rng.binomial(2, f, (size, p)) / 2.0)
    X = np.asfortranarray(np.vstack(rows))
    X.setflags(write=False)
    return X


def dataset(name):
    return golden()[1] if name == "golden" else four_populations()


def subset(name, n_train):
    n = dataset(name).shape[0]
    if n_train == n:
        return np.arange(n)
    return np.sort(np.random.default_rng(n_train).choice(n, n_train, replace=False))


def standardised(X):
    """gwasprep (src/gwas.jl:112-128): kept loci, standardised columns (ddof = 1)."""
    sd = X.std(axis=0, ddof=1)
    keep = sd > EPS
    return (X[:, keep] - X[:, keep].mean(axis=0)) / sd[keep]


@functools.lru_cache(maxsize=None)
def reference(name, n_train, kind):
    """(M_ref, eigenvalues descending, eigenvectors as columns in that order) of the rows subset(name, n_train)."""
    Z = standardised(dataset(name)[subset(name, n_train)])
    K = Z @ Z.T / Z.shape[1]
    if kind == "reference":  # pc1_of_grm's matrix
        Kt = (K - K.mean(axis=0)) / K.std(axis=0, ddof=1)
        Kc = Kt - Kt.mean(axis=1, keepdims=True)
        M = Kc @ Kc.T
    else:
        M = K
    w, V = np.linalg.eigh(M)
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    for a in (M, w, V):
        a.setflags(write=False)
    return M, w, V


def gaps(w, k):
    """g_i: the smaller neighbouring eigenvalue gap over λ₁, i < k."""
    return np.array([min(w[i - 1] - w[i] if i else np.inf, w[i] - w[i + 1]) / w[0] for i in range(k)])


def check_gap_free(r, ref, k, tol=TOL, max_iter=1000, label=""):
    M, w, _ = ref
    V, th = r["vectors"], r["values"]
    assert V.shape == (M.shape[0], k) and th.shape == (k,)
    bound = (tol + 1e-12) * w[0]
    e_orth = float(np.abs(V.T @ V - np.eye(k)).max())
    e_res = float(np.linalg.norm(M @ V - V * th, axis=0).max())
    e_val = float(np.abs(th - w[:k]).max())
    e_tr = abs(r["trace"] - np.trace(M)) / np.trace(M)
    print(f"{label}: iters {r['iters']}, ‖VᵀV − I‖ {e_orth:.2e}, residual {e_res:.2e}, |θ − λ| {e_val:.2e} "
          f"(bound {bound:.2e}), trace rel {e_tr:.2e}, resid reported {r['resid'].max():.2e}")
    assert e_orth <= 1e-12
    assert e_res <= bound
    assert e_val <= bound
    assert e_tr <= 1e-12
    assert r["converged"] and r["iters"] < max_iter and np.all(r["resid"] < tol)
    assert np.all(np.diff(th) <= 0)


def check_sign_rule(V):
    for i in range(V.shape[1]):
        at = int(np.argmax(np.abs(V[:, i])))  # the lowest index among ties
        assert V[at, i] > 0, (i, at, V[at, i])


def abs_cos(a, b):
    """|cos| of two vectors with exactly summed dot products: what is left is the rounding of each product, of the
    square root and of the division, under 4 ε in all (the allowance the comparisons below add; near well separated
    eigenvalues the bound (10·tol/g)² itself is below ε)."""
    return abs(math.fsum(a * b)) / math.sqrt(math.fsum(a * a) * math.fsum(b * b))


def check_vectors(r, ref, k, tol=TOL, label=""):
    _, w, Vref = ref
    g = gaps(w, k)
    assert np.all(g >= 3e-3), g
    V = r["vectors"]
    for i in range(k):
        c = abs_cos(V[:, i], Vref[:, i])
        need = 1.0 - (10.0 * tol / g[i]) ** 2
        print(f"{label} pair {i}: 1 − |cos| {1 - c:.2e}, gap {g[i]:.4f}, allowed {1 - need:.2e}")
        assert c >= need - 4 * EPS
    check_sign_rule(V)


@pytest.fixture(scope="module")
def sessions():
    opened = {}

    def get(name):
        if name not in opened:
            opened[name] = gbm.GenotypeSession(dataset(name))
        return opened[name]

    yield get
    for s in opened.values():
        s.close()


# ---- symmetric fill ------------------------------------------------------------------------------------------------
def defined_mask(gdim):
    """The elements of G that gbm_dev_grm defines: 128-tiles with tile-row <= tile-column, inside a diagonal tile the
    16-blocks with block-row <= block-column (the diagonal 16-blocks whole)."""
    i = np.arange(gdim)[:, None]
    j = np.arange(gdim)[None, :]
    return (i // 128 < j // 128) | ((i // 128 == j // 128) & (i // 16 <= j // 16))


def p_(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", [128, 129, 300])
def test_symmetric_fill_reads_only_defined_elements(n):
    import torch

    lib = gbm.load_library()
    npad, gdim = lib.gbm_dev_npad(n), lib.gbm_dev_gdim(n)
    A = np.random.default_rng(n).standard_normal((n, n))
    A = (A + A.T) / 2
    Gh = np.full((gdim, gdim), np.nan)
    ok = defined_mask(gdim)[:n, :n]
    Gh[:n, :n][ok] = A[ok]
    assert np.isnan(Gh[n:, :]).all() and np.isnan(Gh[:, n:]).all() and np.isnan(Gh[:n, :n][~ok]).all()
    G = torch.from_numpy(Gh).to("cuda:0")
    K = torch.full((npad, npad), float("nan"), dtype=torch.float64, device="cuda:0")
    scale = 1.0 / 7.0
    _lib.check(lib.gbm_dev_grm_symmetrize(p_(G), gdim, n, scale, p_(K), npad, None), "gbm_dev_grm_symmetrize")
    torch.cuda.synchronize()
    got = K.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(got[:n, :n], scale * A)
    assert np.array_equal(got, got.T)
    assert np.all(got[n:, :] == 0.0) and np.all(got[:, n:] == 0.0)


# ---- block product -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def product_case(n, rows=64):
    rng = np.random.default_rng(1000 + n)
    npad = (n + 127) // 128 * 128
    A = rng.standard_normal((n, n))
    K = np.zeros((npad, npad))
    K[:n, :n] = (A + A.T) / 2
    Qt = np.zeros((rows, npad))
    Qt[:, :n] = rng.standard_normal((rows, n))
    ref = Qt @ K
    for a in (K, Qt, ref):
        a.setflags(write=False)
    return K, Qt, ref


def run_product(Kd, n, Qt_rows):
    import torch

    lib = gbm.load_library()
    npad = Kd.shape[0]
    rows = Qt_rows.shape[0]
    Q = torch.tensor(Qt_rows, device="cuda:0")
    Y = torch.full((rows, npad), float("nan"), dtype=torch.float64, device="cuda:0")
    wsb = lib.gbm_dev_rows_times_sym_workspace(n, rows)
    ws = torch.empty(wsb // 8, dtype=torch.float64, device="cuda:0")
    _lib.check(lib.gbm_dev_rows_times_sym(p_(Kd), npad, n, p_(Q), npad, rows, p_(Y), npad, p_(ws), wsb, None),
               "gbm_dev_rows_times_sym")
    torch.cuda.synchronize()
    return Y.cpu().numpy()


# 128, 129, 300: one 64-row chunk per workgroup; 1100 and 2500: two and three chunks (the prefetched K rows)
@pytest.mark.parametrize("n", [128, 129, 300, 1100, 2500])
def test_block_product_against_numpy(n):
    import torch

    K, Qt, ref = product_case(n)
    Kd = torch.tensor(K, device="cuda:0")
    first = {}
    for rows in (16, 32, 48, 64):
        got = run_product(Kd, n, Qt[:rows])
        bound = 4 * n * EPS * np.abs(Qt[:rows]).max() * np.abs(K).max()
        err = float(np.abs(got - ref[:rows]).max())
        print(f"n={n} rows={rows}: max err {err:.2e}, bound {bound:.2e}")
        assert err <= bound
        assert np.all(got[:, n:] == 0.0)
        again = run_product(Kd, n, Qt[:rows])
        assert np.array_equal(got, again)  # two calls, the same bits
        first[rows] = got
    # a row's bits do not depend on the other rows of the call
    assert np.array_equal(first[32][:16], first[16])
    assert np.array_equal(first[48][:32], first[32])
    assert np.array_equal(first[64][:48], first[48])


# ---- eigenpairs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grm", "reference"])
@pytest.mark.parametrize("k", [1, 4, 16])
def test_golden_fixture_all_rows(sessions, kind, k):
    r = sessions("golden").pcs(np.arange(333), k, kind=kind, tol=TOL)
    ref = reference("golden", 333, kind)
    check_gap_free(r, ref, k, label=f"golden {kind} k={k}")
    check_sign_rule(r["vectors"])
    if kind == "grm" and k == 4:
        check_vectors(r, ref, 4, label="golden grm")


@pytest.mark.parametrize("kind", ["grm", "reference"])
@pytest.mark.parametrize("n_train", [128, 129, 257])  # no padding, almost all padding, a ragged third tile
def test_golden_fixture_row_subsets(sessions, n_train, kind):
    r = sessions("golden").pcs(subset("golden", n_train), 3, kind=kind, tol=TOL)
    check_gap_free(r, reference("golden", n_train, kind), 3, label=f"golden[{n_train}] {kind}")
    check_sign_rule(r["vectors"])


@pytest.mark.parametrize("kind", ["grm", "reference"])
@pytest.mark.parametrize("n_train", [300, 129, 257])
def test_four_populations_eigenvectors(sessions, n_train, kind):
    r = sessions("4pop").pcs(subset("4pop", n_train), 3, kind=kind, tol=TOL)
    ref = reference("4pop", n_train, kind)
    check_gap_free(r, ref, 3, label=f"4pop[{n_train}] {kind}")
    assert np.all(gaps(ref[1], 3) >= 0.13)
    check_vectors(r, ref, 3, label=f"4pop[{n_train}] {kind}")


def test_reference_pc1_against_pc1_of_grm(sessions):
    """Kind "reference", k = 1, against the host path's own function on K_ref."""
    Z = standardised(golden()[1])
    v_ref = pc1_of_grm(Z @ Z.T / Z.shape[1])
    _, w, _ = reference("golden", 333, "reference")
    g = gaps(w, 1)[0]
    assert g >= 3e-3
    r = sessions("golden").pcs(np.arange(333), 1, kind="reference", tol=TOL)
    c = abs_cos(r["vectors"][:, 0], v_ref)
    print(f"reference PC1: 1 − |cos| {1 - c:.2e}, gap of M {g:.4f}")
    assert c >= 1.0 - (10.0 * TOL / g) ** 2 - 4 * EPS
    check_sign_rule(r["vectors"])


# ---- cache and determinism -----------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_and_leave_the_cache_intact():
    _, X, y = golden()
    ALL = np.arange(333)
    with gbm.GenotypeSession(X) as s:
        b1, yp1, _, _ = s.gblup(ALL, y, 0.7)
        assert s.stats() == (1, 0)
        r1 = s.pcs(ALL, 4, kind="grm")
        r2 = s.pcs(ALL, 4, kind="grm")
        q1 = s.pcs(ALL, 2, kind="reference")
        q2 = s.pcs(ALL, 2, kind="reference")
        for a, b in ((r1, r2), (q1, q2)):
            for key in ("vectors", "values", "resid"):
                assert np.array_equal(a[key], b[key]), key
            assert a["trace"] == b["trace"] and a["iters"] == b["iters"]
        b2, yp2, _, _ = s.gblup(ALL, y, 0.7)
        assert np.array_equal(b1, b2) and np.array_equal(yp1, yp2)
        assert s.stats() == (1, 5)  # one build, then hits only
    with gbm.GenotypeSession(X) as s:  # pcs first: it builds, the fit hits
        s.pcs(ALL, 1)
        assert s.stats() == (1, 0)
        b3, yp3, _, _ = s.gblup(ALL, y, 0.7)
        assert s.stats() == (1, 1)
        assert np.array_equal(b1, b3) and np.array_equal(yp1, yp3)


def test_exact_grm_session():
    D, X, _ = golden()
    idx = np.arange(200)
    with gbm.GenotypeSession(dosage_i8=D, ploidy=2) as s:
        s.set_grm("exact")
        r = s.pcs(idx, 4, kind="grm", tol=TOL)
        r1 = s.pcs(idx, 2, kind="reference", tol=TOL)
        assert s.grm_used() == "exact"
    Z = standardised(X[idx])
    K = Z @ Z.T / Z.shape[1]
    w = np.linalg.eigvalsh(K)[::-1]
    check_gap_free(r, (K, w, None), 4, label="exact grm[200]")
    Kt = (K - K.mean(axis=0)) / K.std(axis=0, ddof=1)
    Kc = Kt - Kt.mean(axis=1, keepdims=True)
    M = Kc @ Kc.T
    check_gap_free(r1, (M, np.linalg.eigvalsh(M)[::-1], None), 2, label="exact reference[200]")


# ---- non-convergence -----------------------------------------------------------------------------------------------
def test_max_iter_returns_the_last_iterate_with_a_warning(sessions):
    s = sessions("golden")
    with pytest.warns(RuntimeWarning, match="max_iter = 2 reached"):
        r = s.pcs(np.arange(333), 3, kind="grm", tol=TOL, max_iter=2)
    assert r["converged"] is False and r["iters"] == 2
    assert r["resid"].max() > TOL
    assert np.isfinite(r["vectors"]).all() and np.isfinite(r["values"]).all() and np.isfinite(r["resid"]).all()
    assert np.isfinite(r["trace"])
    assert np.abs(np.linalg.norm(r["vectors"], axis=0) - 1.0).max() <= 1e-14
    with warnings.catch_warnings():  # a converged call afterwards is silent again
        warnings.simplefilter("error")
        assert s.pcs(np.arange(333), 1)["converged"]


# ---- integration ---------------------------------------------------------------------------------------------------
def test_gwas_n_pcs_against_numpy_eigenvectors(sessions):
    _, _, y = golden()
    ALL = np.arange(333)
    _, w, V = reference("golden", 333, "grm")
    g = gaps(w, 2).min()
    assert g >= 3e-3
    s = sessions("golden")
    got = s.gwas(ALL, y, model="ols", n_pcs=2)
    ref = s.gwas(ALL, y, covariates=V[:, :2], model="ols")
    bound = 100 * TOL / g
    for key in ("z", "b"):
        err = float(np.abs(got[key] - ref[key]).max() / np.abs(ref[key]).max())
        print(f"gwas n_pcs=2 {key}: rel err {err:.2e}, bound {bound:.2e}")
        assert err <= bound
    assert got["tested"] == ref["tested"]
    extra = np.random.default_rng(5).standard_normal((333, 1))
    got1 = s.gwas(ALL, y, covariates=extra, model="ols", n_pcs=1)
    ref1 = s.gwas(ALL, y, covariates=np.column_stack([extra, V[:, 0]]), model="ols")
    assert float(np.abs(got1["z"] - ref1["z"]).max() / np.abs(ref1["z"]).max()) <= bound
    again = s.gwas(ALL, y, model="ols")  # the default is the scan without principal components
    assert np.array_equal(again["z"], s.gwas(ALL, y, model="ols", n_pcs=0)["z"])


def test_gwasols_device_pc1_against_the_host_path():
    n, p = 240, 900
    X = oracle.synth_genotypes(77, n, p).copy()
    X[:, [10, 500]] = X[0, [10, 500]]  # two loci-alleles without variance
    rng = np.random.default_rng(3)
    sd = X.std(axis=0, ddof=1)
    qtl = np.argsort(sd)[-3:]
    y = ((X[:, qtl] - X[:, qtl].mean(axis=0)) / sd[qtl]) @ np.array([1.0, -1.0, 1.0]) + 0.5 * rng.standard_normal(n)
    ent = [f"e{i}" for i in range(n)]
    genomes = gbm.Genomes(ent, ["pop"] * n, [f"l{j}" for j in range(p)], X)
    phenomes = gbm.Phenomes(ent, ["pop"] * n, ["t1"], y[:, None])
    Z = standardised(X)
    K = Z @ Z.T / Z.shape[1]
    Kt = (K - K.mean(axis=0)) / K.std(axis=0, ddof=1)
    Kc = Kt - Kt.mean(axis=1, keepdims=True)
    g = gaps(np.linalg.eigvalsh(Kc @ Kc.T)[::-1], 1)[0]
    assert g >= 3e-3
    auto = gbm.gwasols(genomes=genomes, phenomes=phenomes)  # pc="auto"
    assert auto.metrics == {"pc1_on_device": 1.0, "grm_builds": 1.0}
    host = gbm.gwasols(genomes=genomes, phenomes=phenomes, pc="host")
    assert host.metrics == {"pc1_on_device": 0.0, "grm_builds": 2.0}
    bound = 100 * 1e-12 / g
    err = float(np.abs(auto.b_hat - host.b_hat).max() / np.abs(host.b_hat).max())
    print(f"gwasols auto vs host: rel err {err:.2e}, bound {bound:.2e}, gap of M {g:.4f}")
    assert auto.b_hat_labels == host.b_hat_labels and auto.model == host.model == "GWAS_OLS"
    assert err <= bound
    aware = gbm.gwasols(genomes=genomes, phenomes=phenomes, GRM_type="ploidy-aware")
    assert aware.metrics["pc1_on_device"] == 0.0 and len(aware.b_hat) == len(host.b_hat)


def _few_loci(n=80, p=20):
    X = np.random.default_rng(21).integers(0, 3, (n, p)) / 2.0
    y = np.random.default_rng(22).standard_normal(n)
    return np.asfortranarray(X), y


def test_pcs_reports_a_block_that_lost_rank():
    """n >= 64 entries with fewer than 32 polymorphic loci: rank K <= 20, so the 32-wide block cannot stay
    independent. The entry says so (GBM_E_DATA, code on the exception) for both kinds, and the session goes on
    working."""
    X, y = _few_loci()
    with gbm.GenotypeSession(X) as s:
        for kind in ("grm", "reference"):
            with pytest.raises(gbm.GBMError, match="lost rank") as e:
                s.pcs(np.arange(80), 1, kind=kind)
            assert e.value.code == _lib.GBM_E_DATA
        with pytest.raises(gbm.GBMError, match="lost rank"):
            s.gwas(np.arange(80), y, model="ols", n_pcs=1)
        assert s.gwas(np.arange(80), y, model="ols")["tested"] == 20
        assert s.stats()[0] == 1


def test_gwasols_auto_takes_the_host_path_when_the_block_loses_rank():
    """The default arguments on a small valid input (n = 80 >= 64, p = 20 < 32): the device attempt fails with
    'lost rank', and gwasols returns what pc="host" returns, bit for bit (the same host GRM, the same pc1_of_grm, the
    same scan)."""
    n, p = 80, 20
    X, y = _few_loci(n, p)
    ent = [f"e{i}" for i in range(n)]
    genomes = gbm.Genomes(ent, ["pop"] * n, [f"l{j}" for j in range(p)], X)
    phenomes = gbm.Phenomes(ent, ["pop"] * n, ["t1"], y[:, None])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the fallback is silent
        auto = gbm.gwasols(genomes=genomes, phenomes=phenomes)
    host = gbm.gwasols(genomes=genomes, phenomes=phenomes, pc="host")
    assert auto.metrics == {"pc1_on_device": 0.0, "grm_builds": 3.0}
    assert host.metrics == {"pc1_on_device": 0.0, "grm_builds": 2.0}
    assert auto.b_hat_labels == host.b_hat_labels and len(auto.b_hat) == p
    assert np.isfinite(host.b_hat).all() and np.abs(host.b_hat).max() > 0
    assert np.array_equal(auto.b_hat, host.b_hat)


def test_gwas_n_pcs_refuses_unconverged_components(sessions):
    _, _, y = golden()
    s = sessions("golden")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # an error, not a warning
        with pytest.raises(gbm.GBMError, match="did not converge in 2 iterations"):
            s.gwas(np.arange(333), y, model="ols", n_pcs=2, pcs_max_iter=2)
    with pytest.raises(gbm.ArgumentError, match="tol must be finite and > 0"):  # pcs_tol reaches pcs too
        s.gwas(np.arange(333), y, model="ols", n_pcs=2, pcs_tol=0.0)
