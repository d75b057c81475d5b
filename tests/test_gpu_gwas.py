"""Mixed-model and OLS GWAS scans (GenotypeSession.gwas, gbm.gwasreml / gbm.gwasols, gbm_dev_whiten_rows) against
a numpy restatement of the reference's literal per-marker forms:

  gwasreml (src/gwas.jl:591-599):  V_inv = pinv(σ²_u K + σ²_e I); X = [1, C, x_j];
      b = pinv(XᵀV⁻¹X)(XᵀV⁻¹y);  z_j = b[end] / sqrt(inv(XᵀV⁻¹X)[end])
  gwasols  (src/gwas.jl:241-245):  Vinv = pinv(XᵀX); b = Vinv Xᵀy; t_j = b[end] / sqrt(Vinv[end, end])

with x_j and y standardised as gwasprep does (src/gwas.jl:112-128) and K = ZZᵀ/q (the library's stated difference
from the reference's column-standardised K). The library computes the same numbers as a Schur complement on
whitened rows; the restatement does not. Tolerance: 1e-9 of max|z| and of max|b| (the project's GEBV parity
criterion); dropped loci are exactly 0."""
import ctypes
import functools
import os

import numpy as np
import pytest

import gbm
import oracle
from gbm import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ragged_333x1777_3traits.npz")
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def fixture():
    d = np.load(GOLDEN)
    D = np.asarray(d["dosage"], dtype=np.int8)
    X = np.asfortranarray(D.astype(np.float64) / float(d["ploidy"]))
    y = np.asarray(d["phenotypes"][:, 0], dtype=np.float64)
    for a in (D, X, y):
        a.setflags(write=False)
    return D, X, y


@functools.lru_cache(maxsize=None)
def covariates(n, kc, seed=5):
    C = np.random.default_rng(seed).standard_normal((n, kc))
    C.setflags(write=False)
    return C


def standardised(X, y):
    """gwasprep (src/gwas.jl:112-128): kept loci, standardised columns (ddof = 1) and y."""
    sd = X.std(axis=0, ddof=1)
    keep = sd > np.finfo(np.float64).eps
    Z = (X[:, keep] - X[:, keep].mean(axis=0)) / sd[keep]
    ys = (y - y.mean()) / y.std(ddof=1)
    return Z, ys, keep


def ref_scan(X, y, C, s2e=None, s2u=None):
    """(z, b, keep) over all loci by the literal per-marker forms; V = I (gwasols) when s2e is None."""
    Z, ys, keep = standardised(X, y)
    n, q = Z.shape
    X0 = np.ones((n, 1)) if C is None else np.column_stack([np.ones(n), C])
    k = X0.shape[1]
    if s2e is None:
        Vinv = np.eye(n)
    else:
        Vinv = np.linalg.pinv(s2u * (Z @ Z.T) / q + s2e * np.eye(n))
    VX0, Vy, VZ = Vinv @ X0, Vinv @ ys, Vinv @ Z
    M0, r0 = X0.T @ VX0, X0.T @ Vy
    z, b = np.zeros(X.shape[1]), np.zeros(X.shape[1])
    cols = np.nonzero(keep)[0]
    for jj, j in enumerate(cols):
        x, vx = Z[:, jj], VZ[:, jj]
        M = np.empty((k + 1, k + 1))
        M[:k, :k] = M0
        M[:k, k] = M[k, :k] = X0.T @ vx
        M[k, k] = x @ vx
        rhs = np.r_[r0, x @ Vy]
        bh = np.linalg.pinv(M) @ rhs
        with np.errstate(invalid="ignore"):  # (a locus in the covariates' span: M is singular, its z is not compared)
            z[j] = bh[-1] / np.sqrt(np.linalg.inv(M)[-1, -1])
        b[j] = bh[-1]
    return z, b, keep


@functools.lru_cache(maxsize=None)
def ref_mlm_full(s2e, s2u, kc):
    _, X, y = fixture()
    return ref_scan(X, y, covariates(333, kc) if kc else None, s2e, s2u)


def close(got, ref, what):
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{what}: rel err {err:.3e}")
    assert err < TOL, (what, err)


def check_scan(r, ref, label):
    z, b, keep = ref
    close(r["z"], z, label + " z")
    close(r["b"], b, label + " b")
    assert np.all(r["z"][~keep] == 0.0) and np.all(r["b"][~keep] == 0.0)
    assert r["tested"] == int(keep.sum())


@pytest.fixture(scope="module")
def session():
    _, X, _ = fixture()
    with gbm.GenotypeSession(X) as s:
        yield s


ALL = np.arange(333)


@pytest.mark.parametrize("s2", [(0.5, 0.5), (1e-3, 1.0)])
@pytest.mark.parametrize("kc", [0, 2])
def test_mixed_model_parity_and_chunk_independence(session, gbm_env, s2, kc):
    _, _, y = fixture()
    C = covariates(333, kc) if kc else None
    gbm_env.setenv("GBM_GWAS_CHUNK", "500")  # four chunks, the last of 277 loci (ragged strips)
    r = session.gwas(ALL, y, covariates=C, model="mlm", sigma2=s2)
    assert r["tested"] == 1774 and (r["sigma2_e"], r["sigma2_u"]) == s2
    check_scan(r, ref_mlm_full(s2[0], s2[1], kc), f"mlm s2={s2} kc={kc}")
    gbm_env.delenv("GBM_GWAS_CHUNK")
    r1 = session.gwas(ALL, y, covariates=C, model="mlm", sigma2=s2)  # the default chunk: one
    assert np.array_equal(r1["z"], r["z"]) and np.array_equal(r1["b"], r["b"]) and r1["tested"] == r["tested"]


@pytest.mark.parametrize("n_train", [128, 129, 200])  # no padding, almost all padding, two 128-tiles
def test_training_set_sizes_at_the_padding_edges(session, n_train):
    _, X, y = fixture()
    idx = np.sort(np.random.default_rng(n_train).choice(333, n_train, replace=False))
    C = covariates(333, 1)[idx]
    r = session.gwas(idx, y[idx], covariates=C, model="mlm", sigma2=(0.4, 0.7))
    check_scan(r, ref_scan(X[idx], y[idx], C, 0.4, 0.7), f"n_train={n_train}")


def test_reml_route_uses_the_null_model_estimates(session):
    _, _, y = fixture()
    est = session.reml(ALL, y)
    r = session.gwas(ALL, y, model="mlm", sigma2=None)
    assert r["sigma2_e"] == est["sigma2_e"] and r["sigma2_u"] == est["sigma2_u"]
    r2 = session.gwas(ALL, y, model="mlm", sigma2=(est["sigma2_e"], est["sigma2_u"]))
    assert np.array_equal(r["z"], r2["z"]) and np.array_equal(r["b"], r2["b"])
    assert r["tested"] == 1774 and np.abs(r["z"]).max() > 0


def test_ols_parity_and_covariate_sign(session):
    _, X, y = fixture()
    Z, _, _ = standardised(X, y)
    pc = np.linalg.eigh(Z @ Z.T / Z.shape[1])[1][:, -1]
    r = session.gwas(ALL, y, covariates=pc, model="ols")
    assert r["sigma2_e"] is None and r["sigma2_u"] is None
    check_scan(r, ref_scan(X, y, pc), "ols")
    rf = session.gwas(ALL, y, covariates=-pc, model="ols")
    assert np.array_equal(rf["z"], r["z"]) or np.abs(rf["z"] - r["z"]).max() <= 1e-12


def test_locus_in_the_covariate_span_is_dropped(session):
    _, X, y = fixture()
    Z, _, keep = standardised(X, y)
    cols = np.nonzero(keep)[0]
    j = int(cols[700])
    C = Z[:, 700].copy()
    r = session.gwas(ALL, y, covariates=C, model="mlm", sigma2=(0.5, 0.5))
    assert r["z"][j] == 0.0 and r["b"][j] == 0.0 and r["tested"] == 1773
    z, b, _ = ref_scan(X, y, C, 0.5, 0.5)
    others = np.ones(X.shape[1], dtype=bool)
    others[j] = False
    close(r["z"][others], z[others], "span z")
    close(r["b"][others], b[others], "span b")
    assert np.all(r["z"][~keep] == 0.0)


def test_scan_leaves_the_training_cache_intact():
    _, X, y = fixture()
    with gbm.GenotypeSession(X) as s:
        b1, yp1, _, _ = s.gblup(ALL, y, 0.7)
        assert s.stats() == (1, 0)
        r = s.gwas(ALL, y, covariates=covariates(333, 2), model="mlm", sigma2=(0.5, 0.5))
        assert r["tested"] == 1774
        b2, yp2, _, _ = s.gblup(ALL, y, 0.7)
        assert np.array_equal(b1, b2) and np.array_equal(yp1, yp2)
        builds, hits = s.stats()
        assert builds == 1 and hits >= 2


def test_exact_grm_session():
    D, _, y = fixture()
    with gbm.GenotypeSession(dosage_i8=D, ploidy=2) as s:
        s.set_grm("exact")
        r = s.gwas(ALL, y, model="mlm", sigma2=(0.5, 0.5))
        assert s.grm_used() == "exact"
    check_scan(r, ref_mlm_full(0.5, 0.5, 0), "exact GRM")


def test_whiten_rows_against_numpy_inverse():
    """gbm_dev_whiten_rows after a gbm_dev_gblup_solve at n = 333 (npad 384): 70 rows (a ragged second strip),
    R U⁻¹ with U from numpy's Cholesky of G/q + λI; the padding columns stay 0."""
    import torch

    from gbm.sharded import HipShardStages
    _, X, y = fixture()
    n, p, lam = 333, X.shape[1], 0.6
    st = HipShardStages(n, p, nrhs=1, lambda_=lam, device=0)
    st.upload_genotypes(X.copy())
    st.load_phenotypes(y.copy())
    st.standardize()
    st.grm_syrk()
    st.grm_reduce()
    st.solve()
    torch.cuda.synchronize()
    assert int(st.info.item()) == 0
    Rh = np.zeros((70, st.npad))
    Rh[:, :n] = np.random.default_rng(8).standard_normal((70, n))
    R = torch.from_numpy(Rh).to(st.dev)
    lib = gbm.load_library()
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.gbm_dev_whiten_rows(p_(st.G), st.gdim, n, p_(st.ws_solve), p_(R), st.npad, 70, st._stream()),
               "gbm_dev_whiten_rows")
    torch.cuda.synchronize()
    got = R.cpu().numpy()
    K, _ = oracle.grm(X)
    U = np.linalg.cholesky(K + lam * np.eye(n)).T
    ref = Rh[:, :n] @ np.linalg.inv(U)
    err = float(np.abs(got[:, :n] - ref).max() / np.abs(ref).max())
    print(f"whiten rows: rel err {err:.3e}")
    assert err < 1e-10
    assert np.all(got[:, n:] == 0.0)
    # a row's result does not depend on the launch it fell into: the last 6 rows alone
    R2 = torch.from_numpy(Rh[64:]).to(st.dev)
    _lib.check(lib.gbm_dev_whiten_rows(p_(st.G), st.gdim, n, p_(st.ws_solve), p_(R2), st.npad, 6, st._stream()),
               "gbm_dev_whiten_rows")
    torch.cuda.synchronize()
    assert np.array_equal(R2.cpu().numpy(), got[64:])


def test_model_functions_build_the_fit_and_find_a_qtl():
    n, p = 240, 900
    X = oracle.synth_genotypes(77, n, p).copy()
    X[:, [10, 500]] = X[0, [10, 500]]  # two loci-alleles without variance
    rng = np.random.default_rng(3)
    sd = X.std(axis=0, ddof=1)
    # three large QTL among the loci with the most variance (the reference doctest's qualitative check)
    qtl = np.argsort(sd)[-3:]
    g = ((X[:, qtl] - X[:, qtl].mean(axis=0)) / sd[qtl]) @ np.array([1.0, -1.0, 1.0])
    y = g + 0.5 * rng.standard_normal(n)
    ent = [f"e{i}" for i in range(n)]
    labels = [f"l{j}" for j in range(p)]
    genomes = gbm.Genomes(ent, ["pop"] * n, labels, X)
    phenomes = gbm.Phenomes(ent, ["pop"] * n, ["t1"], y[:, None])
    kept = [labels[j] for j in range(p) if sd[j] > np.finfo(np.float64).eps]
    assert len(kept) <= p - 2
    for fn, name in ((gbm.gwasreml, "GWAS_REML"), (gbm.gwasols, "GWAS_OLS")):
        fit = fn(genomes=genomes, phenomes=phenomes)
        assert fit.model == name and fit.trait == "t1" and fit.n == n and fit.l == len(kept)
        assert fit.b_hat_labels == kept and "intercept" not in fit.b_hat_labels
        assert len(fit.b_hat) == len(kept) and fit.entries == ent and fit.checkdims()
        top = fit.b_hat_labels[int(np.argmax(np.abs(fit.b_hat)))]
        assert top in {labels[j] for j in qtl}, (name, top)
    fit = gbm.gwasols(genomes=genomes, phenomes=phenomes, GRM_type="ploidy-aware")
    assert fit.model == "GWAS_OLS" and len(fit.b_hat) == len(kept)
