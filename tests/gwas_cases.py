"""Inputs and cached references of the GWAS scan's edge tests (tests/test_gwas_cases.py on the CPU,
tests/test_gpu_factor_readers.py and tests/test_gpu_gwas_edges.py on the device): every covariate count
the statistics kernel is instantiated for, training sets at the API minima and at every n mod 4, a
matrix of 18 column blocks, a session of 130 loci for the chunk sweep and one of 33 000 loci for the
statistics kernel's grid-stride loop.

Two references that share no step. ``literal`` is tests/test_gpu_gwas.py's ``ref_scan``: the
reference's per-marker ``pinv`` forms in float64. ``schur`` works in np.longdouble: a hand-written
Cholesky of V = σ²_u ZZᵀ/q + σ²_e I (none for OLS), [1, C], y and every locus whitened by forward
substitution, the covariates orthogonalised by twice-iterated Gram–Schmidt, and then
num = R_zᵀR_y, s = ΣR_z², z = num/√s, b = num/s for all loci at once. Every array is built once and
is read-only. Not a test module."""
import functools
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

import oracle

from test_gpu_gwas import ref_scan, standardised

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ragged_333x1777_3traits.npz")
LD = np.longdouble
S2 = (0.4, 0.7)  # (σ²_e, σ²_u) of the ordinary mixed-model cases: λ = 0.571
S2_SMALL = (1e-3, 1.0)  # λ = 10⁻³
FLAT = (5, 32760, 32775, 32999)  # loci of `long` without variance, on both sides of index 32 768 (itself tested)
SPAN_LOCUS = 700  # of the fixture's kept loci: the one `fix-span2` places in the covariates' span


class Case(NamedTuple):
    data: str  # the session's X and y (``data``)
    n_train: Optional[int]  # None: every row; else ``rows`` picks that many
    kc: int
    model: str  # "mlm" | "ols"
    s2: Optional[Tuple[float, float]]
    tested: int  # loci the scan tests: polymorphic in the rows and outside the covariates' span
    literal: bool = True  # False: the per-marker loop is too slow (33 000 loci), `schur` alone


def _cases():
    c = {"n1100-kc7": Case("n1100", None, 7, "mlm", S2, 200), "n1100-kc0": Case("n1100", None, 0, "mlm", S2, 200),
         "fix-kc7-small": Case("fixture", None, 7, "mlm", S2_SMALL, 1774),
         "fix-span2": Case("fixture", None, 3, "mlm", S2, 1773),
         "p130": Case("p130", None, 3, "mlm", S2, 130)}
    for model, s2 in (("mlm", S2), ("ols", None)):
        for kc in (3, 4, 5, 6, 7):
            c[f"fix-kc{kc}-{model}"] = Case("fixture", None, kc, model, s2, 1774)
        for m, tested in ((130, 1774), (131, 1774), (257, 1774)):
            c[f"fix-n{m}-{model}"] = Case("fixture", m, 2, model, s2, tested)
        for m, kc, tested in ((3, 0, 285), (10, 7, 386), (12, 7, 389)):
            c[f"tiny-n{m}-kc{kc}-{model}"] = Case("tiny", m, kc, model, s2, tested)
        c[f"long-{model}"] = Case("long", None, 2, model, s2, 32988, literal=False)  # FLAT and 8 more are flat
    return c


CASES = _cases()
READER_CASES = ("n1100-kc7", "n1100-kc0")
MINIMUM = tuple(k for k in CASES if k.startswith("tiny-n10-"))  # n_train = kc + 3
SPAN = {"fix-span2": (SPAN_LOCUS,)}  # case -> indices (among the kept loci) placed in the covariates' span


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def data(name):
    """(X, y) of a session, X Fortran-ordered; both read-only."""
    if name == "fixture":  # the ragged 333 x 1777 fixture of tests/test_gpu_gwas.py
        d = np.load(GOLDEN)
        X = np.asarray(d["dosage"], dtype=np.float64) / float(d["ploidy"])
        y = np.asarray(d["phenotypes"][:, 0], dtype=np.float64)
    else:
        seed, n, p = {"n1100": (1100, 1100, 200), "p130": (130, 64, 130), "tiny": (12, 12, 400),
                      "long": (33, 40, 33000)}[name]
        X = oracle.synth_genotypes(seed, n, p).copy()
        if name == "long":
            X[:, list(FLAT)] = X[0, list(FLAT)]
        y = oracle.synth_phenotypes(X, seed + 1)[:, 0]
    return _frozen(np.asfortranarray(X), y)


@functools.lru_cache(maxsize=None)
def dosage_i8():
    """The fixture's dosages as stored (int8, ploidy 2): data("fixture")[0] is exactly dosage / 2."""
    d = np.load(GOLDEN)
    assert int(d["ploidy"]) == 2
    return _frozen(np.asfortranarray(np.asarray(d["dosage"], dtype=np.int8)))


@functools.lru_cache(maxsize=None)
def rows(dname, n_train):
    """The training rows (sorted) of a case: all, or n_train of them drawn with a seed of their own."""
    n = data(dname)[0].shape[0]
    if n_train is None or n_train == n:
        return _frozen(np.arange(n))
    return _frozen(np.sort(np.random.default_rng(1000 + n_train).choice(n, n_train, replace=False)))


@functools.lru_cache(maxsize=None)
def _normal(n, kc, seed=5):
    return _frozen(np.random.default_rng(seed).standard_normal((n, kc)))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(idx, X[idx], y[idx], C or None) of a case; C (n_train, kc) Fortran-ordered."""
    c = CASES[name]
    X, y = data(c.data)
    idx = rows(c.data, c.n_train)
    Xt, yt = np.asfortranarray(X[idx]), y[idx].copy()
    C = None
    if c.kc:
        C = _normal(X.shape[0], c.kc)[idx].copy()
        if name in SPAN:  # the locus = 0.7 c_1 + 1.3 c_2: a combination of two covariates
            Z, _, _ = standardised(Xt, yt)
            C[:, 1] = (Z[:, SPAN[name][0]] - 0.7 * C[:, 0]) / 1.3
        C = np.asfortranarray(C)
        C.setflags(write=False)
    return idx, _frozen(Xt), _frozen(yt), C


@functools.lru_cache(maxsize=None)
def literal(name):
    """(z, b, keep) over all p loci by the per-marker pinv forms (test_gpu_gwas.ref_scan), float64."""
    c = CASES[name]
    assert c.literal, name
    _, X, y, C = inputs(name)
    s2e, s2u = c.s2 if c.model == "mlm" else (None, None)
    return _frozen(*ref_scan(X, y, C, s2e, s2u))


def cholesky_ld(V):
    """Lower L with V = LLᵀ, column by column in long double (no LAPACK)."""
    n = V.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        r = L[j, :j]
        L[j, j] = np.sqrt(V[j, j] - r @ r)
        if j + 1 < n:
            L[j + 1:, j] = (V[j + 1:, j] - L[j + 1:, :j] @ r) / L[j, j]
    return L


def forward_ld(L, B):
    """L⁻¹B by forward substitution, every column of B at once."""
    W = np.empty_like(B)
    for i in range(L.shape[0]):
        W[i] = (B[i] - L[i, :i] @ W[:i]) / L[i, i]
    return W


def _standardised_ld(X, y):
    X = X.astype(LD)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    sd = np.sqrt(((X - mean) ** 2).sum(axis=0) / (n - 1))
    keep = sd > np.finfo(np.float64).eps
    Z = (X[:, keep] - mean[keep]) / sd[keep]
    y = y.astype(LD)
    ym = y.sum() / n
    ys = (y - ym) / np.sqrt(((y - ym) ** 2).sum() / (n - 1))
    return Z, ys, keep


@functools.lru_cache(maxsize=None)
def _whitened(dname, n_train, s2):
    """(L or None, L⁻¹Z, L⁻¹y, keep) of a training set: shared by the cases that differ in covariates alone."""
    X, y = data(dname)
    idx = rows(dname, n_train)
    Z, ys, keep = _standardised_ld(X[idx], y[idx])
    if s2 is None:
        return None, Z, ys, keep
    n, q = Z.shape
    L = cholesky_ld(LD(s2[1]) * (Z @ Z.T) / q + LD(s2[0]) * np.eye(n, dtype=LD))
    W = forward_ld(L, np.column_stack([Z, ys]))
    return L, W[:, :q], W[:, q], keep


@functools.lru_cache(maxsize=None)
def schur(name):
    """(z, b, keep, ratio) over all p loci in long double, returned as float64: ratio = s_j/d_j (0 where not kept)."""
    c = CASES[name]
    _, X, _, C = inputs(name)
    L, Wz, wy, keep = _whitened(c.data, c.n_train, c.s2 if c.model == "mlm" else None)
    n = Wz.shape[0]
    X0 = np.ones((n, 1), dtype=LD) if C is None else np.column_stack([np.ones(n, dtype=LD), C.astype(LD)])
    if L is not None:
        X0 = forward_ld(L, X0)
    Q = np.zeros_like(X0)
    for k in range(X0.shape[1]):  # Gram–Schmidt, every projection twice
        v = X0[:, k].copy()
        for _ in range(2):
            v -= Q[:, :k] @ (Q[:, :k].T @ v)
        Q[:, k] = v / np.sqrt(v @ v)
    Rz, ry = Wz.copy(), wy.copy()
    for _ in range(2):
        Rz -= Q @ (Q.T @ Rz)
        ry -= Q @ (Q.T @ ry)
    num, s, d = Rz.T @ ry, (Rz * Rz).sum(axis=0), (Wz * Wz).sum(axis=0)
    p = X.shape[1]
    z, b, ratio = np.zeros(p), np.zeros(p), np.zeros(p)
    z[keep], b[keep], ratio[keep] = num / np.sqrt(s), num / s, s / d
    return _frozen(z, b, keep.copy(), ratio)


def reference(name):
    """(z, b, keep) the device is compared with: the literal forms, or `schur` where they are too slow."""
    return literal(name) if CASES[name].literal else schur(name)[:3]


def compared(name):
    """Mask over the p loci of those whose statistics are compared (kept and outside the covariates' span)."""
    keep = reference(name)[2]
    m = keep.copy()
    if name in SPAN:
        m[np.nonzero(keep)[0][list(SPAN[name])]] = False
    return m


def rel(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max())


@functools.lru_cache(maxsize=None)
def whitening(lam=0.6, nrows=129, seed=8):
    """(R (nrows, 1100), U) of the whitening tests at n = 1100: U upper with UᵀU = ZZᵀ/q + λI (numpy's Cholesky)."""
    X, _ = data("n1100")
    n = X.shape[0]
    K, _ = oracle.grm(X)
    U = np.linalg.cholesky(K + lam * np.eye(n)).T.copy()
    R = np.random.default_rng(seed).standard_normal((nrows, n))
    return _frozen(R, U)


@functools.lru_cache(maxsize=None)
def whitening_ref(lam=0.6, nrows=129, seed=8):
    R, U = whitening(lam, nrows, seed)
    return _frozen(R @ np.linalg.inv(U))
