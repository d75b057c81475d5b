"""Device-resident genotype sessions (libgbm ``gbm_session_*``): the fold-farming runtime behind
``cvmultithread``/``cvbulk`` and the REML choice of λ (row 2).

X is uploaded once per device; each fit gathers its training rows on the device, and the
standardised training genotypes + GRM are cached per training set (reference
src/cross_validation.jl:159-186 refits everything per fold)."""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib
from ._lib import ArgumentError, GBMError


def _idx(idx) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
    if a.ndim != 1 or a.size == 0:
        raise ArgumentError("entry indices must be a non-empty 1-D array")
    return a


class GenotypeSession:
    """X (n entries x p loci-alleles, allele frequencies) resident on one device."""

    def __init__(self, X: np.ndarray | None = None, *, device: int = 0, dosage_i8: np.ndarray | None = None,
                 ploidy: int | None = None):
        self.lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.device = int(device)
        if dosage_i8 is not None:
            D = np.asfortranarray(np.asarray(dosage_i8, dtype=np.int8))
            self.n, self.p = D.shape
            if not ploidy or ploidy < 1:
                raise ArgumentError("ploidy must be >= 1 with int8 dosages")
            rc = self.lib.gbm_session_create_dosage_i8(_lib.ptr(D), self.n, self.p, self.n, int(ploidy), self.device,
                                                       ctypes.byref(self._h))
            _lib.check(rc, "gbm_session_create_dosage_i8")
        else:
            X = np.asfortranarray(np.asarray(X, dtype=np.float64))
            if X.ndim != 2:
                raise ArgumentError("X must be a 2-D (entries x loci-alleles) array")
            if not np.isfinite(X).all():
                raise ArgumentError("X has missing/NaN/Inf allele frequencies")
            self.n, self.p = X.shape
            rc = self.lib.gbm_session_create(_lib.ptr(X), self.n, self.p, self.n, self.device, ctypes.byref(self._h))
            _lib.check(rc, "gbm_session_create")

    @classmethod
    def synthetic(cls, seed: int, n: int, p: int, *, device: int = 0) -> "GenotypeSession":
        """Session over the counter-hash synthetic genotypes of loci 0..p-1, generated
        on the device (benchmark-scale configs without a host copy of X)."""
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.device = int(device)
        self.n, self.p = int(n), int(p)
        _lib.check(self.lib.gbm_session_create_synthetic(int(seed), self.n, self.p, self.device, ctypes.byref(self._h)),
                   "gbm_session_create_synthetic")
        return self

    # ---- lifetime -------------------------------------------------------------------------
    def close(self):
        if self._h:
            self.lib.gbm_session_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.close()
        except Exception:
            pass

    # ---- GRM arithmetic -----------------------------------------------------------------------
    def set_grm(self, grm):
        """GRM arithmetic of the training GRMs: None (the GBM_GRM variable, else fp64), "fp64", "exact" or
        "auto" (exact when the genotypes are diploid dosages/2; include/gbm.h gbm_session_set_grm_mode)."""
        _lib.check(self.lib.gbm_session_set_grm_mode(self._h, _lib.grm_mode(grm)), "gbm_session_set_grm_mode")
        return self

    def grm_used(self):
        """"fp64" or "exact": the GRM the cached training set was built with (None before the first fit)."""
        v = ctypes.c_int(-1)
        _lib.check(self.lib.gbm_session_grm_used(self._h, ctypes.byref(v)), "gbm_session_grm_used")
        return {_lib.GBM_GRM_FP64: "fp64", _lib.GBM_GRM_EXACT: "exact"}.get(v.value)

    # ---- model calls ----------------------------------------------------------------------
    def gblup(self, idx, Y, lambda_: float = 1.0):
        """GBLUP on rows ``idx`` (0-based, strictly increasing); Y (n_train,) or (n_train, t).
        Returns (b_hat (p+1, t), y_pred (n_train, t), mu (t,), q)."""
        idx = _idx(idx)
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        Y = np.asfortranarray(Y)
        m, t = Y.shape
        if m != idx.size:
            raise ArgumentError("Y rows must match the training indices")
        b_hat = np.zeros((self.p + 1, t), order="F")
        y_pred = np.zeros((m, t), order="F")
        mu = np.zeros(t)
        q = np.zeros(1, dtype=np.int64)
        rc = self.lib.gbm_session_gblup_fit(self._h, _lib.ptr(idx), m, _lib.ptr(Y), m, t, float(lambda_),
                                            _lib.ptr(b_hat), _lib.ptr(y_pred), _lib.ptr(mu), _lib.ptr(q))
        _lib.check(rc, "gbm_session_gblup_fit")
        return b_hat, y_pred, mu, int(q[0])

    def predict(self, idx, b_hat) -> np.ndarray:
        """b0 + X[idx, :] b for b_hat (p+1,) or (p+1, t); returns (n_val,) or (n_val, t)."""
        idx = _idx(idx)
        b = np.asarray(b_hat, dtype=np.float64)
        one = b.ndim == 1
        if one:
            b = b[:, None]
        b = np.asfortranarray(b)
        if b.shape[0] != self.p + 1:
            raise ArgumentError("b_hat must have p + 1 rows (intercept first)")
        t = b.shape[1]
        out = np.zeros((idx.size, t), order="F")
        rc = self.lib.gbm_session_predict(self._h, _lib.ptr(idx), idx.size, _lib.ptr(b), self.p + 1, t,
                                          _lib.ptr(out), idx.size)
        _lib.check(rc, "gbm_session_predict")
        return out[:, 0].copy() if one else out

    def reml_objective(self, idx, y, sigma2_e, sigma2_u) -> np.ndarray:
        """Reference loglikreml (src/gwas.jl:450-483) with X = 1 at the given (σ²_e, σ²_u) pairs."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        se = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma2_e, dtype=np.float64)))
        su = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma2_u, dtype=np.float64)))
        if se.shape != su.shape or y.shape != (idx.size,):
            raise ArgumentError("shape mismatch")
        out = np.zeros(se.size)
        rc = self.lib.gbm_session_reml_objective(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), _lib.ptr(se),
                                                 _lib.ptr(su), se.size, _lib.ptr(out))
        _lib.check(rc, "gbm_session_reml_objective")
        return out

    def reml(self, idx, y) -> dict:
        """REML λ = σ²_e/σ²_u for standardised y over the reference's box [eps, 1]² (src/gwas.jl:585)."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.shape != (idx.size,):
            raise ArgumentError("y must have one value per training index")
        v = np.zeros(4)
        p = [ctypes.c_void_p(v.ctypes.data + 8 * k) for k in range(4)]
        rc = self.lib.gbm_session_reml(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), *p)
        _lib.check(rc, "gbm_session_reml")
        return {"lambda": float(v[0]), "sigma2_e": float(v[1]), "sigma2_u": float(v[2]), "objective": float(v[3])}

    def pcs(self, idx, k: int = 1, kind: str = "grm", tol: float = 1e-10, max_iter: int = 1000) -> dict:
        """Leading ``k`` (<= 16) eigenpairs of the relationship matrix of rows ``idx`` (>= 64 of them), by block
        subspace iteration on the cached GRM (gbm_session_pcs). ``kind``: "grm" (K = ZZᵀ/q, the matrix of
        :meth:`gwas`) or "reference" (the PCA of the column-standardised K that reference gwasols takes its PC1
        from, src/gwas.jl:130, 234; :func:`gbm.gwas.pc1_of_grm`). Stops when every relative Ritz residual
        ‖Mv − θv‖/θ₁ is below ``tol``, or after ``max_iter`` iterations (then ``converged`` is False and a
        warning is issued). Returns dict(vectors (n_train, k) [unit columns, largest component positive], values
        (k,) descending, trace, resid (k,), iters, converged)."""
        idx = _idx(idx)
        try:
            kd = _lib.PCS_KINDS[kind]
        except (KeyError, TypeError):
            raise ArgumentError(f"kind must be 'grm' or 'reference', got {kind!r}") from None
        k = int(k)
        if not 1 <= k <= 16:
            raise ArgumentError("k must be in [1, 16]")
        vec = np.zeros((idx.size, k), order="F")
        val, res = np.zeros(k), np.zeros(k)
        tr = np.zeros(1)
        it = np.zeros(1, dtype=np.int64)
        rc = self.lib.gbm_session_pcs(self._h, _lib.ptr(idx), idx.size, kd, k, float(tol), int(max_iter), _lib.ptr(vec),
                                      _lib.ptr(val), _lib.ptr(tr), _lib.ptr(res), _lib.ptr(it))
        _lib.check(rc, "gbm_session_pcs")
        msg = _lib.last_error()
        converged = not msg.startswith("warning:")
        if not converged:
            warnings.warn(msg, RuntimeWarning, stacklevel=2)
        return {"vectors": vec, "values": val, "trace": float(tr[0]), "resid": res, "iters": int(it[0]),
                "converged": converged}

    def gwas(self, idx, y, covariates=None, model: str = "mlm", sigma2=None, n_pcs: int = 0, pcs_tol: float = 1e-10,
             pcs_max_iter: int = 1000) -> dict:
        """GWAS scan over all p loci on rows ``idx`` (gbm_session_gwas; reference gwasreml / gwasols,
        src/gwas.jl:591-599, 241-245). ``covariates``: (n_train,) or (n_train, kc <= 7) beside the intercept.
        ``n_pcs`` > 0 appends that many leading principal components of K = ZZᵀ/q (:meth:`pcs`, kind "grm") to
        the covariates (kc + n_pcs <= 7), computed with ``pcs_tol`` and ``pcs_max_iter``; the scan never runs on
        unconverged components: GBMError is raised when they do not converge, as it is by :meth:`pcs` itself when
        the block loses rank (fewer than 32 eigenvalues of K above rounding).
        ``model``: "mlm" (V = σ²_u ZZᵀ/q + σ²_e I on the cached GRM factor) or "ols" (V = I). ``sigma2``:
        (σ²_e, σ²_u) for "mlm", or None to estimate them once by the null-model REML of :meth:`reml`.
        Returns dict(z (p,), b (p,), sigma2_e, sigma2_u, tested); untested loci (not polymorphic in the rows, or in
        the covariates' span) have z = b = 0; sigma2_e/sigma2_u are None for "ols"."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.shape != (idx.size,):
            raise ArgumentError("y must have one value per training index")
        try:
            m = {"mlm": 0, "ols": 1}[model]
        except (KeyError, TypeError):
            raise ArgumentError(f"model must be 'mlm' or 'ols', got {model!r}") from None
        if covariates is None:
            C, kc = None, 0
        else:
            C = np.asarray(covariates, dtype=np.float64)
            if C.ndim == 1:
                C = C[:, None]
            if C.ndim != 2 or C.shape[0] != idx.size:
                raise ArgumentError("covariates must have one row per training index")
            C = np.asfortranarray(C)
            kc = C.shape[1]
        n_pcs = int(n_pcs)
        if n_pcs < 0 or (n_pcs > 0 and kc + n_pcs > 7):  # without PCs the library checks kc as before
            raise ArgumentError(f"n_pcs must be >= 0 with at most 7 covariates in all (got {kc} covariates + "
                                f"{n_pcs} principal components)")
        if sigma2 is None:
            s2e = s2u = float("nan")
        else:
            s2e, s2u = (float(v) for v in sigma2)
            if m == 0 and (np.isnan(s2e) or np.isnan(s2u)):
                raise ArgumentError("sigma2 must be a pair of positive numbers (None: estimate by REML)")
        if n_pcs > 0:
            with warnings.catch_warnings():  # not converged is an error here, not a warning
                warnings.simplefilter("ignore", RuntimeWarning)
                rp = self.pcs(idx, n_pcs, kind="grm", tol=pcs_tol, max_iter=pcs_max_iter)
            if not rp["converged"]:
                raise GBMError(f"gwas: the {n_pcs} principal components did not converge in {rp['iters']} iterations "
                               f"(largest relative residual {rp['resid'].max():.3g} against pcs_tol {pcs_tol:.3g}); "
                               "raise pcs_max_iter or pcs_tol, or pass covariates of your own")
            pcs = rp["vectors"]
            C = np.asfortranarray(pcs if C is None else np.column_stack([C, pcs]))
            kc += n_pcs
        z = np.zeros(self.p)
        b = np.zeros(self.p)
        used = np.zeros(2)
        tested = np.zeros(1, dtype=np.int64)
        rc = self.lib.gbm_session_gwas(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), _lib.ptr(C) if kc else None,
                                       idx.size, kc, m, s2e, s2u, _lib.ptr(z), _lib.ptr(b), _lib.ptr(used),
                                       _lib.ptr(tested))
        _lib.check(rc, "gbm_session_gwas")
        return {"z": z, "b": b, "sigma2_e": None if m else float(used[0]), "sigma2_u": None if m else float(used[1]),
                "tested": int(tested[0])}

    def pair_scan(self, idx, y, op, *, loci=None, eps: float = float(np.finfo(np.float64).eps), use_abs: bool = False,
                  var_threshold: float = 0.01, commutative: bool = False, k: int = 1000, panel_rows: int = 0,
                  full: bool = False) -> dict:
        """Epistasis feature scan on rows ``idx`` (gbm_session_pair_scan; reference transform1 / transform2,
        src/transformation.jl:130-468): the slope of y ~ [1, f] for f = op(x_i, x_j) over all ordered pairs of the
        loci ``loci`` (0-based, distinct; None: all p), or f = op(x_j) for the unary operations, with
        x = X[idx, loci] + ``eps`` (absolute values with ``use_abs``). ``op``: one of the names "mult", "addnorm",
        "raise", "square", "invoneplus", "log10epsdivlog10eps" or the function of that name in
        :mod:`gbm.transformation`. Loci with variance below ``var_threshold`` are skipped (slope 0), as are, with
        ``commutative``, the pairs j < i. Returns dict(index (the flat indices i·l + j, or j, of the at most ``k``
        largest |slope| > eps, descending, ties to the lower index), beta (their slopes), tested, degenerate
        (pairs whose feature is constant to rounding: slope 0, never selected) and, with ``full``, beta_full
        ((l, l) or (l,)), which needs every slope in one panel). ``panel_rows`` (a multiple of 64; 0: by a 256 MB
        budget) sets the i-rows per panel and does not change the result. A non-finite feature value raises
        ArgumentError with the reference's advice (a larger eps and/or use_abs)."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.shape != (idx.size,):
            raise ArgumentError("y must have one value per training index")
        name = op if isinstance(op, str) else getattr(op, "__name__", None)
        if name not in _lib.PAIR_OPS:
            raise ArgumentError(f"op must be one of {', '.join(_lib.PAIR_OPS)} (by name or as the function of "
                                f"gbm.transformation), got {op!r}: the scan has no CPU fallback for other functions")
        code = _lib.PAIR_OPS[name]
        unary = code >= 3
        if loci is None:
            lc, l = None, self.p
        else:
            lc = np.ascontiguousarray(np.asarray(loci, dtype=np.int64))
            if lc.ndim != 1 or lc.size == 0:
                raise ArgumentError("loci must be a non-empty 1-D array")
            l = lc.size
        k = int(k)
        nslopes = l if unary else l * l
        if not 1 <= k <= 65536 or k > nslopes:
            raise ArgumentError(f"k must be in [1, 65536] and at most the number of slopes ({nslopes}), got {k}")
        top_i = np.zeros(k, dtype=np.int64)
        top_b = np.zeros(k)
        meta = np.zeros(3, dtype=np.int64)
        mp = [ctypes.c_void_p(meta.ctypes.data + 8 * j) for j in range(3)]
        beta = np.zeros(nslopes) if full else None
        rc = self.lib.gbm_session_pair_scan(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), _lib.ptr(lc), l, code,
                                            float(eps), int(bool(use_abs)), float(var_threshold),
                                            int(bool(commutative)), int(panel_rows), k, _lib.ptr(top_i),
                                            _lib.ptr(top_b), mp[0], _lib.ptr(beta), mp[1], mp[2])
        if rc == _lib.GBM_E_DATA:
            raise ArgumentError(
                f"Cannot transform the allele frequencies using the function: `{name}`. Please consider adding a "
                f"larger `ϵ` (currently equal to {eps}) and/or using absolute values, i.e. use `use_abs=true` "
                f"(currently equal to {str(bool(use_abs)).lower()}). [{_lib.last_error()}]")
        _lib.check(rc, "gbm_session_pair_scan")
        nt = int(meta[0])
        out = {"index": top_i[:nt].copy(), "beta": top_b[:nt].copy(), "tested": int(meta[1]),
               "degenerate": int(meta[2])}
        if full:
            out["beta_full"] = beta if unary else beta.reshape(l, l)
        return out

    def ridge_lambda_max(self, idx, y) -> float:
        """glmnet's first λ for alpha = 0 on rows ``idx`` (standardize = false)."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        out = np.zeros(1)
        rc = self.lib.gbm_session_ridge_lambda_max(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), _lib.ptr(out))
        _lib.check(rc, "gbm_session_ridge_lambda_max")
        return float(out[0])

    def ridge_path(self, idx, y, lambdas, idx_eval=None):
        """Exact glmnet ridge solutions (alpha = 0, standardize = false, intercept) on rows ``idx``
        at each λ. Returns b_path (p+1, nl) [intercept first] and, with ``idx_eval``, the
        predictions (n_eval, nl)."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        lam = np.ascontiguousarray(np.atleast_1d(np.asarray(lambdas, dtype=np.float64)))
        b = np.zeros((self.p + 1, lam.size), order="F")
        if idx_eval is not None:
            ie = _idx(idx_eval)
            pred = np.zeros((ie.size, lam.size), order="F")
            rc = self.lib.gbm_session_ridge_path(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), _lib.ptr(lam),
                                                 lam.size, _lib.ptr(b), _lib.ptr(ie), ie.size, _lib.ptr(pred))
            _lib.check(rc, "gbm_session_ridge_path")
            return b, pred
        rc = self.lib.gbm_session_ridge_path(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), _lib.ptr(lam), lam.size,
                                             _lib.ptr(b), None, 0, None)
        _lib.check(rc, "gbm_session_ridge_path")
        return b

    def enet_path(self, idx, y, lambdas, alpha: float = 1.0, tol: float = 1e-7, max_passes: int = 1_000_000,
                  idx_eval=None, early_stop: bool = True) -> dict:
        """glmnet lasso / elastic-net solutions (alpha in (0, 1], standardize = false, intercept) on rows
        ``idx`` along the non-increasing ``lambdas``, by coordinate descent on the device
        (gbm_session_enet_path). ``early_stop``: glmnet's rule (dev_max = 0.999, fdev = 1e-5); off, every λ is
        solved. Returns dict(b_path (p+1, nl_done) [intercept first], lambdas (the λ kept), dev_ratio, passes,
        nnz, nl_done, warning (None or the library's message) and, with ``idx_eval``, pred (n_eval, nl_done))."""
        idx = _idx(idx)
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        lam = np.ascontiguousarray(np.atleast_1d(np.asarray(lambdas, dtype=np.float64)))
        nl = lam.size
        b = np.zeros((self.p + 1, nl), order="F")
        dev, passes, nnz, done = np.zeros(nl), np.zeros(nl, dtype=np.int64), np.zeros(nl, dtype=np.int64), np.zeros(1, dtype=np.int64)
        ie = _idx(idx_eval) if idx_eval is not None else None
        pred = np.zeros((ie.size, nl), order="F") if ie is not None else None
        dev_max, fdev = (0.999, 1e-5) if early_stop else (float("inf"), 0.0)
        rc = self.lib.gbm_session_enet_path(self._h, _lib.ptr(idx), idx.size, _lib.ptr(y), float(alpha), _lib.ptr(lam),
                                            nl, float(tol), int(max_passes), dev_max, fdev, _lib.ptr(b),
                                            _lib.ptr(ie), 0 if ie is None else ie.size, _lib.ptr(pred),
                                            _lib.ptr(done), _lib.ptr(dev), _lib.ptr(passes), _lib.ptr(nnz))
        _lib.check(rc, "gbm_session_enet_path")
        k = int(done[0])
        msg = _lib.last_error()
        out = {"b_path": b[:, :k], "lambdas": lam[:k], "dev_ratio": dev[:k], "passes": passes[:k], "nnz": nnz[:k],
               "nl_done": k, "warning": msg if msg.startswith("warning:") else None}
        if pred is not None:
            out["pred"] = pred[:, :k]
        return out

    def stats(self):
        """(GRM builds, GRM cache hits)."""
        v = np.zeros(2, dtype=np.int64)
        rc = self.lib.gbm_session_stats(self._h, ctypes.c_void_p(v.ctypes.data), ctypes.c_void_p(v.ctypes.data + 8))
        _lib.check(rc, "gbm_session_stats")
        return int(v[0]), int(v[1])
