"""ctypes calls of the C ABI (include/gbm.h) with explicit leading dimensions, for the tests that the Python
wrappers cannot express: every wrapper passes ld == n (or p + 1). A plain helper module, no tests in it.

A `Mat` is a column-major matrix embedded in a larger parent (`pad` extra rows per column, filled with a
poison); pad = 0 is the contiguous copy. Outputs that take a leading dimension are returned as their whole
parent, pre-filled with SENTINEL, so a test can look at the padding rows too."""
import ctypes

import numpy as np

from gbm import _lib

SENTINEL = -7777.25
MODES = {"fp64": _lib.GBM_GRM_FP64, "exact": _lib.GBM_GRM_EXACT, "auto": _lib.GBM_GRM_AUTO}


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


class Mat:
    """A (n x k) as the top rows of a column-major (n + pad) x k parent whose other rows hold `poison`."""

    def __init__(self, A, pad=0, poison=None):
        A = np.asarray(A)
        if A.ndim == 1:
            A = A[:, None]
        self.n, self.k = A.shape
        self.ld = self.n + pad
        if poison is None:
            poison = np.nan if A.dtype.kind == "f" else 77
        self.parent = np.full((self.ld, self.k), poison, dtype=A.dtype, order="F")
        self.parent[:self.n] = A
        self.ptr = _lib.ptr(self.parent)


def out_parent(n, k, pad=0):
    return np.full((n + pad, k), SENTINEL, order="F")


def padding_untouched(parent, n):
    return bool(np.all(parent[n:] == SENTINEL))


def _outputs(n, p, t):
    return (np.zeros((p + 1, t), order="F"), np.zeros((n, t), order="F"), np.zeros(t), np.zeros(1, dtype=np.int64),
            ctypes.c_int(-1))


def gblup_fit_ex(X, Y, lam, mode, devices=None, nrhs=None, raw=False):
    """gbm_gblup_fit_ex on Mats. Returns (b_hat, y_pred, mu, q, grm_used); raw: the return code only."""
    lib = _lib.load()
    t = Y.k if nrhs is None else nrhs
    b, y, mu, q, used = _outputs(X.n, X.k, max(t, 1))
    dv, nd = _lib.devices_arg(devices)
    rc = lib.gbm_gblup_fit_ex(X.ptr, X.n, X.k, X.ld, Y.ptr, Y.ld, t, float(lam), dv, nd, MODES[mode], _lib.ptr(b),
                              _lib.ptr(y), _lib.ptr(mu), _lib.ptr(q), ctypes.byref(used))
    if raw:
        return rc
    _lib.check(rc, "gbm_gblup_fit_ex")
    return b, y, mu, int(q[0]), used.value


def dosage_fit_ex(D, ploidy, Y, lam, mode, devices=None):
    lib = _lib.load()
    b, y, mu, q, used = _outputs(D.n, D.k, Y.k)
    dv, nd = _lib.devices_arg(devices)
    rc = lib.gbm_gblup_fit_dosage_i8_ex(D.ptr, D.n, D.k, D.ld, int(ploidy), Y.ptr, Y.ld, Y.k, float(lam), dv, nd,
                                        MODES[mode], _lib.ptr(b), _lib.ptr(y), _lib.ptr(mu), _lib.ptr(q),
                                        ctypes.byref(used))
    _lib.check(rc, "gbm_gblup_fit_dosage_i8_ex")
    return b, y, mu, int(q[0]), used.value


def reml_fit_ex(X, Y, mode, devices=None):
    """gbm_gblup_fit_reml_ex. Returns (b_hat, y_pred, mu, q, lambda, sigma2_e, sigma2_u)."""
    lib = _lib.load()
    b, y, mu, q, used = _outputs(X.n, X.k, Y.k)
    lam, s2e, s2u = np.zeros(Y.k), np.zeros(Y.k), np.zeros(Y.k)
    dv, nd = _lib.devices_arg(devices)
    rc = lib.gbm_gblup_fit_reml_ex(X.ptr, X.n, X.k, X.ld, Y.ptr, Y.ld, Y.k, dv, nd, MODES[mode], _lib.ptr(b),
                                   _lib.ptr(y), _lib.ptr(mu), _lib.ptr(q), _lib.ptr(lam), _lib.ptr(s2e),
                                   _lib.ptr(s2u), ctypes.byref(used))
    _lib.check(rc, "gbm_gblup_fit_reml_ex")
    return b, y, mu, int(q[0]), lam, s2e, s2u


def grm(X, gpad=0, devices=None):
    """gbm_grm. Returns (the (n + gpad) x n parent of G_out, q)."""
    lib = _lib.load()
    G = out_parent(X.n, X.n, gpad)
    q = np.zeros(1, dtype=np.int64)
    dv, nd = _lib.devices_arg(devices)
    _lib.check(lib.gbm_grm(X.ptr, X.n, X.k, X.ld, dv, nd, _lib.ptr(G), X.n + gpad, _lib.ptr(q)), "gbm_grm")
    return G, int(q[0])


def grm_ploidy_aware(X, ploidy, gpad=0, devices=None):
    lib = _lib.load()
    G = out_parent(X.n, X.n, gpad)
    den = np.zeros(1)
    dv, nd = _lib.devices_arg(devices)
    _lib.check(lib.gbm_grm_ploidy_aware(X.ptr, X.n, X.k, X.ld, int(ploidy), dv, nd, _lib.ptr(G), X.n + gpad,
                                        _lib.ptr(den)), "gbm_grm_ploidy_aware")
    return G, float(den[0])


def colstats(X, device=0):
    lib = _lib.load()
    m, s = np.zeros(X.k), np.zeros(X.k)
    keep = np.zeros(X.k, dtype=np.uint8)
    q = np.zeros(1, dtype=np.int64)
    _lib.check(lib.gbm_colstats(X.ptr, X.n, X.k, X.ld, device, _lib.ptr(m), _lib.ptr(s), _lib.ptr(keep), _lib.ptr(q)),
               "gbm_colstats")
    return m, s, keep.astype(bool), int(q[0])


def predict(X, B, opad=0, device=0):
    """gbm_predict; B a Mat of (p + 1) x nrhs. Returns the (n + opad) x nrhs parent of out."""
    lib = _lib.load()
    out = out_parent(X.n, B.k, opad)
    _lib.check(lib.gbm_predict(X.ptr, X.n, X.k, X.ld, B.ptr, B.ld, B.k, device, _lib.ptr(out), X.n + opad),
               "gbm_predict")
    return out


class Session:
    """gbm_session_create / gbm_session_create_dosage_i8 on a Mat (ploidy given: int8 dosages)."""

    def __init__(self, X, ploidy=None, device=0, grm=None):
        self.lib = _lib.load()
        self.h = ctypes.c_void_p()
        self.n, self.p = X.n, X.k
        if ploidy is None:
            rc = self.lib.gbm_session_create(X.ptr, X.n, X.k, X.ld, device, ctypes.byref(self.h))
        else:
            rc = self.lib.gbm_session_create_dosage_i8(X.ptr, X.n, X.k, X.ld, int(ploidy), device, ctypes.byref(self.h))
        _lib.check(rc, "gbm_session_create")
        if grm is not None:
            _lib.check(self.lib.gbm_session_set_grm_mode(self.h, MODES[grm]), "gbm_session_set_grm_mode")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.h:
            self.lib.gbm_session_destroy(self.h)
            self.h = ctypes.c_void_p()

    def fit(self, idx, Y, lam, nrhs=None, raw=False):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        t = Y.k if nrhs is None else nrhs
        b, y, mu, q, _ = _outputs(idx.size, self.p, max(t, 1))
        rc = self.lib.gbm_session_gblup_fit(self.h, _lib.ptr(idx), idx.size, Y.ptr, Y.ld, t, float(lam), _lib.ptr(b),
                                            _lib.ptr(y), _lib.ptr(mu), _lib.ptr(q))
        if raw:
            return rc
        _lib.check(rc, "gbm_session_gblup_fit")
        return b, y, mu, int(q[0])

    def predict(self, idx, B, opad=0):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = out_parent(idx.size, B.k, opad)
        _lib.check(self.lib.gbm_session_predict(self.h, _lib.ptr(idx), idx.size, B.ptr, B.ld, B.k, _lib.ptr(out),
                                                idx.size + opad), "gbm_session_predict")
        return out


def brr_fit(X, y, n_iter, n_burnin, thin, seed, device=0):
    lib = _lib.load()
    y = np.ascontiguousarray(y, dtype=np.float64)
    b, yp, var = np.zeros(X.k + 1), np.zeros(X.n), np.zeros(2)
    rc = lib.gbm_brr_fit(X.ptr, X.n, X.k, X.ld, _lib.ptr(y), n_iter, n_burnin, thin, 0.5, 5.0, seed, device,
                         _lib.ptr(b), _lib.ptr(yp), _lib.ptr(var))
    _lib.check(rc, "gbm_brr_fit")
    return b, yp, var
