"""GWAS entry points without a device: argument validation of gbm_session_gwas and gbm_dev_whiten_rows, the
GRM_type checks of gbm.gwasreml / gbm.gwasols, and the binding list."""
import ctypes

import numpy as np
import pytest

import gbm
from gbm import _lib

NAN = float("nan")


def _gwas(lib, kc=0, model=0, s2e=0.5, s2u=0.5, session=None):
    y = np.arange(10.0)
    z = np.zeros(4)
    return lib.gbm_session_gwas(session, None, 10, _lib.ptr(y), None, 10, kc, model, s2e, s2u, _lib.ptr(z), None, None,
                                None)


def test_new_symbols_are_bound():
    assert "gbm_session_gwas" in _lib.EXPORTS and "gbm_dev_whiten_rows" in _lib.EXPORTS
    lib = gbm.load_library()
    assert lib.gbm_version() == 212
    assert hasattr(lib, "gbm_session_gwas") and hasattr(lib, "gbm_dev_whiten_rows")
    assert {"gwasreml", "gwasols"} <= set(gbm.__all__)


def test_session_gwas_rejects_bad_arguments_with_a_message():
    lib = gbm.load_library()
    E = _lib.GBM_E_ARG
    assert _gwas(lib) == E and "session is NULL" in _lib.last_error()
    for kc in (-1, 8):
        assert _gwas(lib, kc=kc) == E and "kc" in _lib.last_error()
    for model in (-1, 2):
        assert _gwas(lib, model=model) == E and "model" in _lib.last_error()
    for s2e, s2u in ((0.0, 0.5), (0.5, -1.0), (float("inf"), 0.5)):
        assert _gwas(lib, s2e=s2e, s2u=s2u) == E and "sigma2" in _lib.last_error()
    # NaN asks for the REML estimate, and OLS ignores the variances: both get as far as the NULL session
    assert _gwas(lib, s2e=NAN, s2u=NAN) == E and "session is NULL" in _lib.last_error()
    assert _gwas(lib, model=1, s2e=-1.0, s2u=0.0) == E and "session is NULL" in _lib.last_error()


def test_whiten_rows_rejects_bad_arguments():
    lib = gbm.load_library()
    n = 300
    G, ws, R = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21), ctypes.c_void_p(1 << 22)  # never dereferenced
    gdim, npad = lib.gbm_dev_gdim(n), lib.gbm_dev_npad(n)
    E = _lib.GBM_E_ARG
    assert lib.gbm_dev_whiten_rows(None, gdim, n, ws, R, npad, 4, None) == E
    assert "gbm_dev_whiten_rows" in _lib.last_error()
    assert lib.gbm_dev_whiten_rows(G, gdim, n, None, R, npad, 4, None) == E
    assert lib.gbm_dev_whiten_rows(G, gdim, n, ws, None, npad, 4, None) == E
    assert lib.gbm_dev_whiten_rows(G, gdim - 2, n, ws, R, npad, 4, None) == E   # ldg < gdim
    assert lib.gbm_dev_whiten_rows(G, gdim, n, ws, R, npad - 2, 4, None) == E   # ldr < npad
    assert lib.gbm_dev_whiten_rows(G, gdim, n, ws, R, npad + 1, 4, None) == E   # odd ldr
    assert lib.gbm_dev_whiten_rows(G, gdim, n, ws, R, npad, -1, None) == E
    assert lib.gbm_dev_whiten_rows(G, gdim, n, ws, ctypes.c_void_p((1 << 22) + 8), npad, 4, None) == E  # alignment
    assert lib.gbm_dev_whiten_rows(G, gdim, n, ws, R, npad, 0, None) == _lib.GBM_OK  # nothing to do


def _pair():
    n, p = 12, 20
    X = np.random.default_rng(0).integers(0, 3, (n, p)) / 2.0
    ent = [f"e{i}" for i in range(n)]
    g = gbm.Genomes(ent, ["p"] * n, [f"l{j}" for j in range(p)], X)
    ph = gbm.Phenomes(ent, ["p"] * n, ["t1"], np.random.default_rng(1).standard_normal((n, 1)))
    return g, ph


def test_grm_type_is_checked_before_device_use():
    g, ph = _pair()
    for fn in (gbm.gwasreml, gbm.gwasols):
        with pytest.raises(gbm.ArgumentError, match="Unrecognised `GRM_type`"):
            fn(genomes=g, phenomes=ph, GRM_type="complex")
    with pytest.raises(gbm.ArgumentError, match="simple GRM"):
        gbm.gwasreml(genomes=g, phenomes=ph, GRM_type="ploidy-aware")


def test_session_gwas_python_argument_checks():
    """GenotypeSession.gwas validates model, shapes and sigma2 on the host (a session object without a device
    handle is enough: nothing reaches the library)."""
    s = gbm.GenotypeSession.__new__(gbm.GenotypeSession)
    s.lib, s._h, s.p = gbm.load_library(), ctypes.c_void_p(), 5
    y = np.arange(6.0)
    with pytest.raises(gbm.ArgumentError, match="model must be"):
        s.gwas(np.arange(6), y, model="lmm")
    with pytest.raises(gbm.ArgumentError, match="one row per"):
        s.gwas(np.arange(6), y, covariates=np.zeros((5, 1)))
    with pytest.raises(gbm.ArgumentError, match="one value per"):
        s.gwas(np.arange(6), y[:5])
    with pytest.raises(gbm.ArgumentError, match="sigma2"):
        s.gwas(np.arange(6), y, sigma2=(NAN, 0.5))
    with pytest.raises(gbm.ArgumentError, match="session is NULL"):
        s.gwas(np.arange(6), y, sigma2=(0.5, 0.5))
