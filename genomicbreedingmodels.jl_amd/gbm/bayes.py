"""``bayesian`` — mirror of reference src/bayes.jl:158-224 for ``bglr_model = "BRR"`` (Bayesian
ridge regression), with the Gibbs sampler on the GPU (libgbm ``gbm_brr_fit``) instead of an
Rscript/BGLR round trip (src/bayes.jl:28-105). SURVEY.md §8f row 3, config C4.

``bayesa``, ``bayesb``, ``bayesc`` — mirrors of the reference's model functions
(src/linear.jl:440-626) over the BayesA / BayesB / BayesC samplers of libgbm ``gbm_bayes_fit``.

``bayesian(m, ..., response_type="ordinal")`` and ``bayes_ordinal_arrays`` — the same three models with the
reference's ordinal response (the threshold model of libgbm ``gbm_bayes_fit_ordinal``)."""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib
from ._lib import ArgumentError, GBMError
from .metrics import metrics
from .prediction import extractxyetc
from .types import Fit, Genomes, Phenomes

SUPPORTED = ("BRR",)
BAYES_MODELS = {"BayesA": 1, "BayesB": 2, "BayesC": 3}  # include/gbm.h GBM_BAYES_*
RESPONSE_TYPES = ("gaussian", "ordinal")  # the reference's (src/bayes.jl:32)


def brr_arrays(X: np.ndarray, y: np.ndarray, *, n_iter: int = 1500, n_burnin: int = 500, thin: int = 5,
               r2: float = 0.5, df0: float = 5.0, seed: int = 42, device: int = 0):
    """Array-level BRR Gibbs sampler. Returns (b_hat (p+1,), y_pred (n,), [σ²_e, σ²_b] posterior means)."""
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    n, p = X.shape
    b_hat = np.zeros(p + 1)
    y_pred = np.zeros(n)
    var = np.zeros(2)
    lib = _lib.load()
    rc = lib.gbm_brr_fit(_lib.ptr(X), n, p, n, _lib.ptr(y), int(n_iter), int(n_burnin), int(thin), float(r2),
                         float(df0), int(seed) & 0xFFFFFFFFFFFFFFFF, int(device), _lib.ptr(b_hat), _lib.ptr(y_pred),
                         _lib.ptr(var))
    _lib.check(rc, "gbm_brr_fit")
    msg = _lib.last_error()
    if msg.startswith("warning"):  # the sweep timed out and the fit was re-run on the per-launch path
        warnings.warn(msg, RuntimeWarning, stacklevel=2)
    return b_hat, y_pred, var


def bayesian(bglr_model: str = "BRR", *, genomes: Genomes, phenomes: Phenomes, idx_entries=None,
             idx_loci_alleles=None, idx_trait: int = 1, response_type: str = "gaussian", n_burnin: int = 500,
             n_iter: int = 1500, verbose: bool = False, thin: int = 5, seed: int = 42, device: int = 0) -> Fit:
    """Bayesian genomic prediction, same signature and Fit assembly as the reference
    (src/bayes.jl:158-224). With the Gaussian response only the BRR model runs here; BayesA, BayesB
    and BayesC run through the model functions ``bayesa``, ``bayesb`` and ``bayesc``. With
    ``response_type="ordinal"`` (the threshold model, ``gbm_bayes_fit_ordinal``) the model is BayesA,
    BayesB or BayesC: ``y_true`` holds the observed classes and ``y_pred`` the liability μ̄ + X b̄
    (the reference's ``X * b_hat``)."""
    if response_type not in RESPONSE_TYPES:
        raise ArgumentError(f"response_type `{response_type}` is not one of {RESPONSE_TYPES}")
    if response_type == "ordinal":
        if bglr_model not in BAYES_MODELS:
            raise ArgumentError(f"bglr_model `{bglr_model}` has no ordinal response; supported with "
                                f"response_type = 'ordinal': {tuple(BAYES_MODELS)}")
        return _ordinal_fit(bglr_model, genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, n_iter, n_burnin,
                            thin, seed, device, verbose)
    if bglr_model not in SUPPORTED:
        hint = "; use gbm.bayesa, gbm.bayesb or gbm.bayesc for BayesA, BayesB, BayesC" if bglr_model in BAYES_MODELS else ""
        raise ArgumentError(f"bglr_model `{bglr_model}` is not available through bayesian(); supported: {SUPPORTED}{hint}")
    X, y, entries, populations, loci_alleles = extractxyetc(
        genomes, phenomes, idx_entries=idx_entries, idx_loci_alleles=idx_loci_alleles, idx_trait=idx_trait,
        add_intercept=False)
    fit = Fit(n=X.shape[0], l=X.shape[1] + 1)
    fit.model = bglr_model
    fit.b_hat_labels = ["intercept"] + list(loci_alleles)
    fit.trait = phenomes.traits[idx_trait - 1]
    fit.entries = entries
    fit.populations = populations
    fit.y_true = y
    b_hat, y_pred, var = brr_arrays(X, y, n_iter=n_iter, n_burnin=n_burnin, thin=thin, seed=seed, device=device)
    fit.b_hat = b_hat
    fit.y_pred = y_pred
    fit.metrics = metrics(y, y_pred)
    if verbose:
        print(fit.metrics, "posterior means: varE", var[0], "varB", var[1])
    if not fit.checkdims():
        raise GBMError("Error fitting " + fit.model + ".")
    return fit


def bayes_arrays(model: str, X: np.ndarray, y: np.ndarray, *, n_iter: int = 1500, n_burnin: int = 500, thin: int = 5,
                 r2: float = 0.5, df0: float = 5.0, prob_in: float = 0.5, counts: float = 10.0, seed: int = 42,
                 device: int = 0):
    """Array-level BayesA / BayesB / BayesC Gibbs sampler (``model`` one of "BayesA", "BayesB", "BayesC").
    Returns (b_hat (p+1,), y_pred (n,), [σ²_e, mean_j σ²_b_j, π] posterior means, pip (p,))."""
    if model not in BAYES_MODELS:
        raise ArgumentError(f"model `{model}` is not one of {tuple(BAYES_MODELS)}")
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    n, p = X.shape
    b_hat = np.zeros(p + 1)
    y_pred = np.zeros(n)
    var = np.zeros(3)
    pip = np.zeros(p)
    lib = _lib.load()
    rc = lib.gbm_bayes_fit(BAYES_MODELS[model], _lib.ptr(X), n, p, n, _lib.ptr(y), int(n_iter), int(n_burnin),
                           int(thin), float(r2), float(df0), float(prob_in), float(counts),
                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(device), _lib.ptr(b_hat), _lib.ptr(y_pred),
                           _lib.ptr(var), _lib.ptr(pip))
    _lib.check(rc, "gbm_bayes_fit")
    return b_hat, y_pred, var, pip


MAX_CHAINS = 32  # include/gbm.h GBM_BAYES_MAX_CHAINS


def _chain_arguments(models, r2, df0, prob_in, counts, seeds):
    """The per-chain arrays of a multi-chain call: model codes, priors and seeds (a scalar serves every chain)."""
    T = len(models)

    def per_chain(v, name, dtype=np.float64):
        a = np.asarray(v)
        if a.ndim == 0:
            return np.full(T, v, dtype=dtype)
        if a.shape != (T,):
            raise ArgumentError(f"`{name}` must be a scalar or have one entry per chain ({T}), got shape {a.shape}")
        return np.ascontiguousarray(a, dtype=dtype)

    mod = np.array([BAYES_MODELS[m] for m in models], dtype=np.intc)
    r2, df0 = per_chain(r2, "r2"), per_chain(df0, "df0")
    prob_in, counts = per_chain(prob_in, "prob_in"), per_chain(counts, "counts")
    seeds = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in per_chain(seeds, "seeds", object)], dtype=np.uint64)
    return mod, r2, df0, prob_in, counts, seeds


def bayes_multi_arrays(models, X: np.ndarray, Y: np.ndarray, *, n_iter: int = 1500, n_burnin: int = 500, thin: int = 5,
                       r2=0.5, df0=5.0, prob_in=0.5, counts=10.0, seeds=42, device: int = 0):
    """T = len(models) independent BayesA / BayesB / BayesC chains over one X in one pass (``gbm_bayes_fit_multi``):
    chain c has the model ``models[c]``, the phenotypes ``Y[:, c]`` and entry c of ``r2``, ``df0``, ``prob_in``,
    ``counts`` and ``seeds`` (a scalar serves every chain). Returns (b_hat (p+1, T), y_pred (n, T), var (3, T),
    pip (p, T)); column c has the bits of ``bayes_arrays(models[c], X, Y[:, c], ...)`` with the chain's arguments."""
    models = list(models)
    for m in models:
        if m not in BAYES_MODELS:
            raise ArgumentError(f"model `{m}` is not one of {tuple(BAYES_MODELS)}")
    T = len(models)
    if not 1 <= T <= MAX_CHAINS:
        raise ArgumentError(f"bayes_multi_arrays runs 1 to {MAX_CHAINS} chains per call, got {T}")
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    Y = np.asarray(Y, dtype=np.float64)
    n, p = X.shape
    if Y.ndim != 2 or Y.shape != (n, T):
        raise ArgumentError(f"Y must have one column of {n} phenotypes per chain, ({n}, {T}); got {Y.shape}")
    Y = np.asfortranarray(Y)
    mod, r2, df0, prob_in, counts, seeds = _chain_arguments(models, r2, df0, prob_in, counts, seeds)
    b_hat = np.zeros((p + 1, T), order="F")
    y_pred = np.zeros((n, T), order="F")
    var = np.zeros((3, T), order="F")
    pip = np.zeros((p, T), order="F")
    lib = _lib.load()
    rc = lib.gbm_bayes_fit_multi(T, _lib.ptr(mod), _lib.ptr(X), n, p, n, _lib.ptr(Y), n, int(n_iter), int(n_burnin),
                                 int(thin), _lib.ptr(r2), _lib.ptr(df0), _lib.ptr(prob_in), _lib.ptr(counts),
                                 _lib.ptr(seeds), int(device), _lib.ptr(b_hat), p + 1, _lib.ptr(y_pred), n,
                                 _lib.ptr(var), _lib.ptr(pip), p)
    _lib.check(rc, "gbm_bayes_fit_multi")
    return b_hat, y_pred, var, pip


def bayes_multi_rows_arrays(models, X: np.ndarray, Y: np.ndarray, sets, set_of, *, n_iter: int = 1500,
                            n_burnin: int = 500, thin: int = 5, r2=0.5, df0=5.0, prob_in=0.5, counts=10.0, seeds=42,
                            device: int = 0):
    """``bayes_multi_arrays`` with a training set per chain (``gbm_bayes_fit_multi_rows``): ``sets`` is an
    (nsets, n) boolean or uint8 array (1 = a training row) and chain c trains on ``sets[set_of[c]]``; ``Y[i, c]``
    is read only at the chain's training rows (it may be NaN elsewhere). Returns what ``bayes_multi_arrays``
    returns, ``y_pred`` over all n rows: at a chain's held-out rows it is the fold's prediction."""
    models = list(models)
    for m in models:
        if m not in BAYES_MODELS:
            raise ArgumentError(f"model `{m}` is not one of {tuple(BAYES_MODELS)}")
    T = len(models)
    if not 1 <= T <= MAX_CHAINS:
        raise ArgumentError(f"bayes_multi_rows_arrays runs 1 to {MAX_CHAINS} chains per call, got {T}")
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    Y = np.asarray(Y, dtype=np.float64)
    n, p = X.shape
    if Y.ndim != 2 or Y.shape != (n, T):
        raise ArgumentError(f"Y must have one column of {n} phenotypes per chain, ({n}, {T}); got {Y.shape}")
    Y = np.asfortranarray(Y)
    sets = np.asarray(sets)
    if sets.ndim != 2 or sets.shape[1] != n or sets.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise ArgumentError(f"sets must be a boolean or uint8 array of shape (nsets, {n}); got {sets.dtype} "
                            f"{sets.shape}")
    sets = np.ascontiguousarray(sets.view(np.uint8) if sets.dtype == bool else sets)
    set_of = np.asarray(set_of)
    if set_of.shape != (T,) or not np.issubdtype(set_of.dtype, np.integer):
        raise ArgumentError(f"set_of must hold one set index per chain ({T}), got shape {set_of.shape}")
    set_of = np.ascontiguousarray(set_of, dtype=np.intc)
    mod, r2, df0, prob_in, counts, seeds = _chain_arguments(models, r2, df0, prob_in, counts, seeds)
    b_hat = np.zeros((p + 1, T), order="F")
    y_pred = np.zeros((n, T), order="F")
    var = np.zeros((3, T), order="F")
    pip = np.zeros((p, T), order="F")
    lib = _lib.load()
    rc = lib.gbm_bayes_fit_multi_rows(T, _lib.ptr(mod), _lib.ptr(X), n, p, n, _lib.ptr(Y), n, sets.shape[0],
                                      _lib.ptr(sets), n, _lib.ptr(set_of), int(n_iter), int(n_burnin), int(thin),
                                      _lib.ptr(r2), _lib.ptr(df0), _lib.ptr(prob_in), _lib.ptr(counts),
                                      _lib.ptr(seeds), int(device), _lib.ptr(b_hat), p + 1, _lib.ptr(y_pred), n,
                                      _lib.ptr(var), _lib.ptr(pip), p)
    _lib.check(rc, "gbm_bayes_fit_multi_rows")
    return b_hat, y_pred, var, pip


def bayes_ordinal_arrays(model: str, X: np.ndarray, y: np.ndarray, *, n_iter: int = 1500, n_burnin: int = 500,
                         thin: int = 5, r2: float = 0.5, df0: float = 5.0, prob_in: float = 0.5, counts: float = 10.0,
                         seed: int = 42, device: int = 0, probs: bool = True):
    """Array-level BayesA / BayesB / BayesC Gibbs sampler with an ordinal response (the threshold model of
    ``gbm_bayes_fit_ordinal``): the classes are the sorted distinct values of ``y`` (2 to 32 of them).
    Returns (b_hat (p+1,), y_pred (n,) the liability μ̄ + X b̄, [1, mean_j σ²_b_j, π] posterior means, pip (p,),
    classes (K,), thresholds (K−1,) posterior means of the finite thresholds, probs (n, K) posterior means of
    P(class k | individual i), or None with ``probs=False``)."""
    if model not in BAYES_MODELS:
        raise ArgumentError(f"model `{model}` is not one of {tuple(BAYES_MODELS)}")
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    n, p = X.shape
    K = len(np.unique(y))
    b_hat = np.zeros(p + 1)
    y_pred = np.zeros(n)
    var = np.zeros(3)
    pip = np.zeros(p)
    classes = np.zeros(max(K, 1))
    thresholds = np.zeros(max(K - 1, 1))
    pr = np.zeros((n, K), order="F") if probs else None
    nclass = ctypes.c_int64(0)
    lib = _lib.load()
    rc = lib.gbm_bayes_fit_ordinal(BAYES_MODELS[model], _lib.ptr(X), n, p, n, _lib.ptr(y), int(n_iter), int(n_burnin),
                                   int(thin), float(r2), float(df0), float(prob_in), float(counts),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(device), _lib.ptr(b_hat), _lib.ptr(y_pred),
                                   _lib.ptr(var), _lib.ptr(pip), max(K, 1), ctypes.addressof(nclass),
                                   _lib.ptr(classes), _lib.ptr(thresholds), _lib.ptr(pr), n)
    _lib.check(rc, "gbm_bayes_fit_ordinal")
    return b_hat, y_pred, var, pip, classes[:nclass.value], thresholds[:nclass.value - 1], pr


def _ordinal_fit(model: str, genomes: Genomes, phenomes: Phenomes, idx_entries, idx_loci_alleles, idx_trait: int,
                 n_iter: int, n_burnin: int, thin: int, seed: int, device: int, verbose: bool) -> Fit:
    """Fit assembly of ``bayesian`` (src/bayes.jl:158-224) for the ordinal response."""
    X, y, entries, populations, loci_alleles = extractxyetc(
        genomes, phenomes, idx_entries=idx_entries, idx_loci_alleles=idx_loci_alleles, idx_trait=idx_trait,
        add_intercept=False)
    fit = Fit(n=X.shape[0], l=X.shape[1] + 1)
    fit.model = model
    fit.b_hat_labels = ["intercept"] + list(loci_alleles)
    fit.trait = phenomes.traits[idx_trait - 1]
    fit.entries = entries
    fit.populations = populations
    fit.y_true = y
    b_hat, y_pred, var, pip, classes, thresholds, _ = bayes_ordinal_arrays(
        model, X, y, n_iter=n_iter, n_burnin=n_burnin, thin=thin, seed=seed, device=device, probs=False)
    fit.b_hat = b_hat
    fit.y_pred = y_pred
    fit.metrics = metrics(y, y_pred)
    if verbose:
        print(fit.metrics, "classes", classes, "posterior means: thresholds", thresholds, "mean varB", var[1], "pi",
              var[2], "mean PIP", pip.mean())
    if not fit.checkdims():
        raise GBMError("Error fitting " + fit.model + ".")
    return fit


def _bayes_model_function(model: str, genomes: Genomes, phenomes: Phenomes, idx_entries, idx_loci_alleles,
                          idx_trait: int, n_iter: int, n_burnin: int, verbose: bool) -> Fit:
    """Fit assembly of ``bayesian`` (src/bayes.jl:158-224) for the three model functions."""
    X, y, entries, populations, loci_alleles = extractxyetc(
        genomes, phenomes, idx_entries=idx_entries, idx_loci_alleles=idx_loci_alleles, idx_trait=idx_trait,
        add_intercept=False)
    fit = Fit(n=X.shape[0], l=X.shape[1] + 1)
    fit.model = model.lower()
    fit.b_hat_labels = ["intercept"] + list(loci_alleles)
    fit.trait = phenomes.traits[idx_trait - 1]
    fit.entries = entries
    fit.populations = populations
    fit.y_true = y
    b_hat, y_pred, var, pip = bayes_arrays(model, X, y, n_iter=n_iter, n_burnin=n_burnin)
    fit.b_hat = b_hat
    fit.y_pred = y_pred
    fit.metrics = metrics(y, y_pred)
    if verbose:
        print(fit.metrics, "posterior means: varE", var[0], "mean varB", var[1], "pi", var[2], "mean PIP", pip.mean())
    if not fit.checkdims():
        raise GBMError("Error fitting " + fit.model + ".")
    return fit


def bayes_multi_pairs(pairs, genomes: Genomes, phenomes: Phenomes, idx_entries, idx_loci_alleles, n_iter: int,
                      n_burnin: int, verbose: bool = False):
    """One Fit per (model, 1-based trait) pair, each what ``bayesa`` / ``bayesb`` / ``bayesc`` returns for the
    same arguments, from multi-chain fits over one gathered X (32 chains per pass). The traits must have their
    finite phenotypes on the same entries (one training matrix serves every chain)."""
    pairs = [(m, int(t)) for m, t in pairs]
    for m, t in pairs:
        if m not in BAYES_MODELS:
            raise ArgumentError(f"model `{m}` is not one of {tuple(BAYES_MODELS)}")
        if not 1 <= t <= len(phenomes.traits):
            raise ArgumentError(f"idx_trait = {t} is out of bounds (1 to {len(phenomes.traits)}).")
    if not pairs:
        return []
    traits = list(dict.fromkeys(t for _, t in pairs))
    X, y0, entries, populations, loci_alleles = extractxyetc(
        genomes, phenomes, idx_entries=idx_entries, idx_loci_alleles=idx_loci_alleles, idx_trait=traits[0],
        add_intercept=False)
    rows = np.arange(len(genomes.entries)) if idx_entries is None else np.asarray(idx_entries, dtype=np.int64) - 1
    ys = {traits[0]: y0}
    keep0 = np.isfinite(np.asarray(phenomes.phenotypes[rows, traits[0] - 1], dtype=np.float64))
    for t in traits[1:]:  # extractxyetc's phenotype handling on the shared rows
        phi = np.asarray(phenomes.phenotypes[rows, t - 1], dtype=np.float64)
        if not np.array_equal(np.isfinite(phi), keep0):
            raise ArgumentError(f"traits `{phenomes.traits[traits[0] - 1]}` and `{phenomes.traits[t - 1]}` have their "
                                "missing phenotypes on different entries: chains of one pass share the training rows")
        y = phi[keep0]
        if y.var(ddof=1) < 1e-20:
            raise GBMError("Very low or zero variance in trait: `" + str(phenomes.traits[t - 1]) + "`.")
        ys[t] = y
    fits = []
    for c0 in range(0, len(pairs), MAX_CHAINS):
        chunk = pairs[c0:c0 + MAX_CHAINS]
        Y = np.column_stack([ys[t] for _, t in chunk])
        b_hat, y_pred, var, pip = bayes_multi_arrays([m for m, _ in chunk], X, Y, n_iter=n_iter, n_burnin=n_burnin)
        for c, (m, t) in enumerate(chunk):
            fit = Fit(n=X.shape[0], l=X.shape[1] + 1)
            fit.model = m.lower()
            fit.b_hat_labels = ["intercept"] + list(loci_alleles)
            fit.trait = phenomes.traits[t - 1]
            fit.entries = list(entries)
            fit.populations = list(populations)
            fit.y_true = ys[t].copy()
            fit.b_hat = np.ascontiguousarray(b_hat[:, c])
            fit.y_pred = np.ascontiguousarray(y_pred[:, c])
            fit.metrics = metrics(fit.y_true, fit.y_pred)
            if verbose:
                print(fit.metrics, "posterior means: varE", var[0, c], "mean varB", var[1, c], "pi", var[2, c],
                      "mean PIP", pip[:, c].mean())
            if not fit.checkdims():
                raise GBMError("Error fitting " + fit.model + ".")
            fits.append(fit)
    return fits


def bayes_multi(models, *, genomes: Genomes, phenomes: Phenomes, idx_entries=None, idx_loci_alleles=None,
                idx_traits=(1,), n_iter: int = 1500, n_burnin: int = 500, verbose: bool = False):
    """``bayesa`` / ``bayesb`` / ``bayesc`` for every (model, trait) of ``models`` ("BayesA", "BayesB", "BayesC") x
    ``idx_traits`` (1-based) on one training set, as chains of one pass over its genotypes. Returns the Fits in
    the order model-major, trait-minor; each equals the model function's Fit for the same arguments."""
    return bayes_multi_pairs([(m, t) for m in models for t in idx_traits], genomes, phenomes, idx_entries,
                             idx_loci_alleles, n_iter, n_burnin, verbose)


def bayesa(*, genomes: Genomes, phenomes: Phenomes, idx_entries=None, idx_loci_alleles=None, idx_trait: int = 1,
           n_iter: int = 1500, n_burnin: int = 500, verbose: bool = False) -> Fit:
    """BayesA (scaled-t marker effects), mirror of reference src/linear.jl:440-465."""
    return _bayes_model_function("BayesA", genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, n_iter,
                                 n_burnin, verbose)


def bayesb(*, genomes: Genomes, phenomes: Phenomes, idx_entries=None, idx_loci_alleles=None, idx_trait: int = 1,
           n_iter: int = 1500, n_burnin: int = 500, verbose: bool = False) -> Fit:
    """BayesB (point mass at zero + scaled-t slab), mirror of reference src/linear.jl:521-546."""
    return _bayes_model_function("BayesB", genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, n_iter,
                                 n_burnin, verbose)


def bayesc(*, genomes: Genomes, phenomes: Phenomes, idx_entries=None, idx_loci_alleles=None, idx_trait: int = 1,
           n_iter: int = 1500, n_burnin: int = 500, verbose: bool = False) -> Fit:
    """BayesC (point mass at zero + Gaussian slab), mirror of reference src/linear.jl:602-626."""
    return _bayes_model_function("BayesC", genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait, n_iter,
                                 n_burnin, verbose)
