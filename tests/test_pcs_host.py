"""Principal components of a session's GRM without a device: the binding list, the host Jacobi eigensolver
(gbm_debug_sym_eig) against numpy.linalg.eigh, and the argument validation of gbm_session_pcs,
gbm_dev_grm_symmetrize, gbm_dev_rows_times_sym and of the Python keywords n_pcs / pc."""
import ctypes

import numpy as np
import pytest

import gbm
from gbm import _lib

EPS = np.finfo(np.float64).eps
NEW = ("gbm_dev_grm_symmetrize", "gbm_dev_rows_times_sym", "gbm_dev_rows_times_sym_workspace", "gbm_session_pcs",
       "gbm_debug_sym_eig")


def test_new_symbols_are_bound():
    lib = gbm.load_library()
    assert lib.gbm_version() == 212  # additive
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert callable(getattr(gbm.GenotypeSession, "pcs"))
    assert (_lib.GBM_PCS_GRM, _lib.GBM_PCS_REFERENCE) == (0, 1)


def _sym_eig(A):
    lib = gbm.load_library()
    m = A.shape[0]
    A = np.ascontiguousarray(A, dtype=np.float64)
    w, V = np.zeros(m), np.zeros((m, m))
    _lib.check(lib.gbm_debug_sym_eig(_lib.ptr(A), m, _lib.ptr(w), _lib.ptr(V)), "gbm_debug_sym_eig")
    return w, V.T  # columns = eigenvectors


def _cases():
    rng = np.random.default_rng(17)
    out = []
    for m in (1, 2, 31, 32, 64):
        A = rng.standard_normal((m, m))
        out.append((f"random m={m}", (A + A.T) / 2))
    Qm, _ = np.linalg.qr(rng.standard_normal((12, 12)))
    out.append(("repeated eigenvalue", (Qm * np.array([3.0, 3.0, 3.0, 1.0, 1.0, -2.0, 0.5, 0.5, 0.0, 7.0, 7.0, 4.0])) @ Qm.T))
    out.append(("diagonal", np.diag(rng.standard_normal(9))))
    return out


@pytest.mark.parametrize("label,A", _cases(), ids=[c[0] for c in _cases()])
def test_sym_eig_against_numpy(label, A):
    A = (A + A.T) / 2
    w, V = _sym_eig(A)
    m = A.shape[0]
    bound = 64 * EPS * np.linalg.norm(A, 2)
    ref = np.linalg.eigvalsh(A)[::-1]
    e_val = float(np.abs(w - ref).max())
    e_res = float(np.linalg.norm(A @ V - V * w, 2))
    e_orth = float(np.abs(V.T @ V - np.eye(m)).max())
    print(f"{label}: |w - eigvalsh| {e_val:.2e}, ‖AV − VΛ‖ {e_res:.2e}, ‖VᵀV − I‖ {e_orth:.2e}, bound {bound:.2e}")
    assert np.all(np.diff(w) <= 0)  # descending
    assert e_val <= bound and e_res <= bound
    assert e_orth <= 64 * EPS


def test_sym_eig_rejects_bad_arguments():
    lib = gbm.load_library()
    A, w, V = np.eye(3), np.zeros(3), np.zeros((3, 3))
    E = _lib.GBM_E_ARG
    assert lib.gbm_debug_sym_eig(None, 3, _lib.ptr(w), _lib.ptr(V)) == E and "gbm_debug_sym_eig" in _lib.last_error()
    assert lib.gbm_debug_sym_eig(_lib.ptr(A), 0, _lib.ptr(w), _lib.ptr(V)) == E
    assert lib.gbm_debug_sym_eig(_lib.ptr(A), 65, _lib.ptr(w), _lib.ptr(V)) == E
    A[1, 2] = np.nan
    assert lib.gbm_debug_sym_eig(_lib.ptr(A), 3, _lib.ptr(w), _lib.ptr(V)) == E and "NaN" in _lib.last_error()


def _pcs(lib, n_train=100, kind=0, k=2, tol=1e-10, max_iter=10, vec=True, val=True, session=None):
    v, w = np.zeros((n_train if n_train > 0 else 1) * 16), np.zeros(16)
    return lib.gbm_session_pcs(session, None, n_train, kind, k, tol, max_iter, _lib.ptr(v) if vec else None,
                               _lib.ptr(w) if val else None, None, None, None)


def test_session_pcs_rejects_bad_arguments_with_a_message():
    lib = gbm.load_library()
    E = _lib.GBM_E_ARG
    for kind in (-1, 2):
        assert _pcs(lib, kind=kind) == E and "kind" in _lib.last_error()
    for k in (0, 17, -3):
        assert _pcs(lib, k=k) == E and "k must be in [1, 16]" in _lib.last_error()
    for n_train in (63, 1, 0):
        assert _pcs(lib, n_train=n_train) == E and "at least 64" in _lib.last_error()
    for tol in (0.0, -1e-3, float("inf"), float("nan")):
        assert _pcs(lib, tol=tol) == E and "tol" in _lib.last_error()
    for max_iter in (0, -5):
        assert _pcs(lib, max_iter=max_iter) == E and "max_iter" in _lib.last_error()
    assert _pcs(lib, vec=False) == E and "NULL" in _lib.last_error()
    assert _pcs(lib, val=False) == E and "NULL" in _lib.last_error()
    # everything valid gets as far as the NULL session (64 rows and k = 16 are the edges that pass)
    assert _pcs(lib, n_train=64, k=16, kind=1) == E and "session is NULL" in _lib.last_error()


def test_symmetrize_rejects_bad_arguments():
    lib = gbm.load_library()
    n = 300
    G, K = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)  # never dereferenced
    npad, gdim = lib.gbm_dev_npad(n), lib.gbm_dev_gdim(n)
    E = _lib.GBM_E_ARG
    assert lib.gbm_dev_grm_symmetrize(None, gdim, n, 1.0, K, npad, None) == E
    assert "gbm_dev_grm_symmetrize" in _lib.last_error()
    assert lib.gbm_dev_grm_symmetrize(G, gdim, n, 1.0, None, npad, None) == E
    assert lib.gbm_dev_grm_symmetrize(G, gdim, n, 1.0, G, gdim, None) == E          # in place
    assert lib.gbm_dev_grm_symmetrize(G, gdim, 0, 1.0, K, npad, None) == E
    assert lib.gbm_dev_grm_symmetrize(G, npad - 1, n, 1.0, K, npad, None) == E      # ldg < npad
    assert lib.gbm_dev_grm_symmetrize(G, gdim, n, 1.0, K, npad - 2, None) == E      # ldk < npad
    assert lib.gbm_dev_grm_symmetrize(G, gdim, n, 1.0, K, npad + 1, None) == E      # odd ldk
    assert lib.gbm_dev_grm_symmetrize(G, gdim, n, float("nan"), K, npad, None) == E
    assert lib.gbm_dev_grm_symmetrize(G, gdim, n, 1.0, ctypes.c_void_p((1 << 24) + 8), npad, None) == E  # alignment


def test_rows_times_sym_rejects_bad_arguments():
    lib = gbm.load_library()
    n = 300
    K, Q, Y, ws = (ctypes.c_void_p(a << 20) for a in (1, 16, 32, 48))  # never dereferenced
    npad = lib.gbm_dev_npad(n)
    wsb = lib.gbm_dev_rows_times_sym_workspace(n, 32)
    assert wsb >= 16 and lib.gbm_dev_rows_times_sym_workspace(n, 64) >= wsb
    assert lib.gbm_dev_rows_times_sym_workspace(0, 32) == 0
    E = _lib.GBM_E_ARG
    call = lib.gbm_dev_rows_times_sym
    for rows in (0, 8, 24, 80, -16):
        assert call(K, npad, n, Q, npad, rows, Y, npad, ws, 1 << 40, None) == E and "rows must be" in _lib.last_error()
    assert call(K, npad, 0, Q, npad, 32, Y, npad, ws, wsb, None) == E and "n must be" in _lib.last_error()
    assert call(None, npad, n, Q, npad, 32, Y, npad, ws, wsb, None) == E and "gbm_dev_rows_times_sym" in _lib.last_error()
    assert call(K, npad, n, None, npad, 32, Y, npad, ws, wsb, None) == E
    assert call(K, npad, n, Q, npad, 32, None, npad, ws, wsb, None) == E
    assert call(K, npad, n, Q, npad, 32, Q, npad, ws, wsb, None) == E               # in place
    assert call(K, npad - 2, n, Q, npad, 32, Y, npad, ws, wsb, None) == E           # ldk < npad
    assert call(K, npad, n, Q, npad + 1, 32, Y, npad, ws, wsb, None) == E           # odd ldq
    assert call(K, npad, n, Q, npad, 32, Y, npad - 2, ws, wsb, None) == E           # ldy < npad
    assert call(K, npad, n, ctypes.c_void_p((16 << 20) + 8), npad, 32, Y, npad, ws, wsb, None) == E  # alignment
    assert call(K, npad, n, Q, npad, 32, Y, npad, None, wsb, None) == E and "workspace" in _lib.last_error()
    assert call(K, npad, n, Q, npad, 32, Y, npad, ws, wsb - 8, None) == E and "workspace" in _lib.last_error()


def _bare_session(p=5):
    s = gbm.GenotypeSession.__new__(gbm.GenotypeSession)
    s.lib, s._h, s.p = gbm.load_library(), ctypes.c_void_p(), p
    return s


def test_python_argument_checks_of_pcs_and_n_pcs():
    """A session object without a device handle is enough: the Python checks raise first, and a call that passes
    them stops at the library's NULL-session check."""
    s = _bare_session()
    idx, y = np.arange(70), np.arange(70.0)
    with pytest.raises(gbm.ArgumentError, match="kind must be"):
        s.pcs(idx, 2, kind="pca")
    for k in (0, 17):
        with pytest.raises(gbm.ArgumentError, match=r"k must be in \[1, 16\]"):
            s.pcs(idx, k)
    with pytest.raises(gbm.ArgumentError, match="session is NULL"):
        s.pcs(idx, 2, kind="reference")
    with pytest.raises(gbm.ArgumentError, match="at least 64"):
        s.pcs(np.arange(10), 1)
    with pytest.raises(gbm.ArgumentError, match="n_pcs"):
        s.gwas(idx, y, model="ols", n_pcs=-1)
    with pytest.raises(gbm.ArgumentError, match="n_pcs"):
        s.gwas(idx, y, model="ols", n_pcs=8)
    with pytest.raises(gbm.ArgumentError, match="n_pcs"):
        s.gwas(idx, y, covariates=np.zeros((70, 5)), model="ols", n_pcs=3)  # 5 + 3 > 7
    with pytest.raises(gbm.ArgumentError, match="session is NULL"):
        s.gwas(idx, y, covariates=np.zeros((70, 5)), model="ols", n_pcs=2)  # 7 in all: reaches pcs


def test_library_errors_carry_their_return_code():
    """gwasols tells pcs' data error (its host path takes over) from every other failure by this code."""
    gbm.load_library()
    with pytest.raises(gbm.ArgumentError) as e:
        _lib.check(_lib.GBM_E_ARG, "x")
    assert e.value.code == _lib.GBM_E_ARG
    for rc in (_lib.GBM_E_DATA, _lib.GBM_E_HIP):
        with pytest.raises(gbm.GBMError) as e:
            _lib.check(rc, "x")
        assert e.value.code == rc


def test_gwasols_checks_pc_before_device_use():
    n, p = 12, 20
    X = np.random.default_rng(0).integers(0, 3, (n, p)) / 2.0
    ent = [f"e{i}" for i in range(n)]
    g = gbm.Genomes(ent, ["p"] * n, [f"l{j}" for j in range(p)], X)
    ph = gbm.Phenomes(ent, ["p"] * n, ["t1"], np.random.default_rng(1).standard_normal((n, 1)))
    with pytest.raises(gbm.ArgumentError, match="Unrecognised `pc`"):
        gbm.gwasols(genomes=g, phenomes=ph, pc="device")
