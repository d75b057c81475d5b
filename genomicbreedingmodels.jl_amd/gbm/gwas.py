"""``gwasreml`` and ``gwasols`` — GPU counterparts of the reference's GWAS model functions
(src/gwas.jl:146-260 ``gwasols``, 485-620 ``gwasreml``), on :meth:`GenotypeSession.gwas`.

The Fit is assembled as ``gwasprep`` does (src/gwas.jl:93-141): loci-alleles without variance in the
selected entries are dropped, ``b_hat`` holds one statistic per kept locus-allele (no intercept entry) and
``b_hat_labels`` their labels.

Deliberate differences from the reference (include/gbm.h ``gbm_session_gwas``, DESIGN.md "GWAS scan"):
  * ``gwasreml`` estimates (σ²_e, σ²_u) once under the null model (P3D/EMMAX); the reference re-runs LBFGS for
    every marker;
  * the relationship matrix of the mixed model is K = ZZᵀ/q of the selected entries; the reference
    column-standardises K (which makes it non-symmetric);
  * the mixed model uses that simple GRM only: ``GRM_type="ploidy-aware"`` is refused by ``gwasreml`` and
    affects only the PC1 covariate of ``gwasols``.

``gwasols`` takes its PC1 covariate from the session's cached GRM on the device (:meth:`GenotypeSession.pcs`,
kind "reference": one GRM build, no n² download); ``pc="host"`` and the ploidy-aware GRM use the host
eigendecomposition :func:`pc1_of_grm`.
"""
from __future__ import annotations

import warnings

import numpy as np

from ._lib import GBM_E_DATA, ArgumentError, GBMError
from .arrays import grm, grm_ploidy_aware
from .prediction import extractxyetc
from .session import GenotypeSession
from .types import Fit, Genomes, Phenomes

GRM_TYPES = ("simple", "ploidy-aware")


def _check_grm_type(GRM_type):
    if GRM_type not in GRM_TYPES:
        raise ArgumentError("Unrecognised `GRM_type`. Please select from:\n\t‣ " + "\n\t‣ ".join(GRM_TYPES))


def _prep(genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait):
    """gwasprep's extraction (src/gwas.jl:93-115, 133-141): G, y, the kept loci-alleles and the empty Fit."""
    G, y, entries, populations, loci_alleles = extractxyetc(genomes, phenomes, idx_entries=idx_entries,
                                                            idx_loci_alleles=idx_loci_alleles, idx_trait=idx_trait,
                                                            add_intercept=False)
    if y.var(ddof=1) < np.finfo(np.float64).eps:
        raise ArgumentError("No variance in the trait: " + str(phenomes.traits[idx_trait - 1]) + ".")
    if not np.isfinite(G).all():
        raise ArgumentError("The allele frequencies of the selected entries have missing/NaN/Inf values.")
    v = G.std(axis=0, ddof=1)
    kept = np.nonzero(np.isfinite(v) & (v > np.finfo(np.float64).eps))[0]
    fit = Fit(n=G.shape[0], l=kept.size)
    fit.trait = phenomes.traits[idx_trait - 1]
    fit.b_hat_labels = [loci_alleles[j] for j in kept]
    fit.entries = entries
    fit.populations = populations
    fit.metrics = {"": 0.0}
    return G, y, kept, fit


def pc1_of_grm(K: np.ndarray) -> np.ndarray:
    """The covariate of reference gwasols (src/gwas.jl:130, 234): K's columns standardised (mean and sd over the
    rows, ddof = 1), then the first principal direction of a PCA that takes the columns as observations
    (MultivariateStats ``fit(PCA, K; maxoutdim=1).proj[:, 1]``). Its sign is arbitrary; the statistics do not
    depend on it."""
    K = np.asarray(K, dtype=np.float64)
    K = (K - K.mean(axis=0)) / K.std(axis=0, ddof=1)
    Kc = K - K.mean(axis=1, keepdims=True)
    w, V = np.linalg.eigh(Kc @ Kc.T)
    return V[:, -1].copy()


def _finish(fit: Fit, z: np.ndarray, kept: np.ndarray, model: str) -> Fit:
    fit.model = model
    fit.b_hat = np.asarray(z[kept], dtype=np.float64).copy()
    if not fit.checkdims():
        raise GBMError("Error performing GWAS (" + model + ").")
    return fit


def gwasreml(genomes: Genomes, phenomes: Phenomes, idx_entries=None, idx_loci_alleles=None, idx_trait: int = 1,
             GRM_type: str = "simple", verbose: bool = False, device: int = 0) -> Fit:
    """Mixed-model GWAS (reference gwasreml): z_j of X = [1, x_j] under V = σ²_u K + σ²_e I, with (σ²_e, σ²_u)
    from one null-model REML and K = ZZᵀ/q (see the module docstring for the differences)."""
    _check_grm_type(GRM_type)
    if GRM_type != "simple":
        raise ArgumentError("gwasreml: the mixed model runs on the simple GRM (ZZᵀ/q) only; GRM_type="
                            "\"ploidy-aware\" is not supported (it affects only gwasols' PC1 covariate)")
    G, y, kept, fit = _prep(genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait)
    with GenotypeSession(G, device=device) as s:
        r = s.gwas(np.arange(G.shape[0]), y, model="mlm", sigma2=None)
    fit.metrics = {"sigma2_e": r["sigma2_e"], "sigma2_u": r["sigma2_u"]}
    if verbose:
        print(f"GWAS via REML: {r['tested']} loci-alleles tested, sigma2_e={r['sigma2_e']:.4g} "
              f"sigma2_u={r['sigma2_u']:.4g}")
    return _finish(fit, r["z"], kept, "GWAS_REML")


PC_MODES = ("auto", "host")


def _device_pc1(s: GenotypeSession, rows: np.ndarray):
    """PC1 of the reference operator from the session's cached GRM, or None where the host path has to take over:
    the iteration did not converge, or the library reports GBM_E_DATA (a column of K without variance, or a block
    that lost rank: the operator has fewer than 32 eigenvalues above rounding, as with fewer than about 31
    polymorphic loci-alleles). Every other error is raised."""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            r = s.pcs(rows, 1, kind="reference", tol=1e-12)
    except GBMError as e:
        if getattr(e, "code", None) != GBM_E_DATA:
            raise
        return None
    return r["vectors"][:, 0] if r["converged"] else None


def gwasols(genomes: Genomes, phenomes: Phenomes, idx_entries=None, idx_loci_alleles=None, idx_trait: int = 1,
            GRM_type: str = "simple", verbose: bool = False, device: int = 0, pc: str = "auto") -> Fit:
    """OLS GWAS (reference gwasols): the t-like statistic of X = [1, PC1, x_j], PC1 from the (simple or
    ploidy-aware) GRM of the selected entries. ``pc="auto"``: for the simple GRM, PC1 comes from the scan's own
    session on the device (``pcs(..., kind="reference", tol=1e-12)``); the host path takes over when there are
    fewer than 64 entries, when the iteration does not converge, and when the library reports a data error (the
    block lost rank, e.g. fewer than about 31 polymorphic loci-alleles; a column of K without variance).
    ``pc="host"``: the GRM is downloaded and :func:`pc1_of_grm` runs on the host. The ploidy-aware GRM always takes
    the host path. The host path builds its GRM while no session is open (after a failed device attempt the
    session is closed first and a new one opened for the scan), so the n x n GRM never shares the device with a
    session's X, Z and two GRM copies.

    ``fit.metrics`` records the path: ``pc1_on_device`` (1.0 or 0.0) and ``grm_builds``, the GRMs built in all
    (the sessions' and the host path's own): 1 on the device path, 2 on the host path, 3 after a fallback."""
    _check_grm_type(GRM_type)
    if pc not in PC_MODES:
        raise ArgumentError("Unrecognised `pc`. Please select from:\n\t‣ " + "\n\t‣ ".join(PC_MODES))
    G, y, kept, fit = _prep(genomes, phenomes, idx_entries, idx_loci_alleles, idx_trait)
    rows = np.arange(G.shape[0])
    pc1, builds = None, 0
    s = GenotypeSession(G, device=device) if pc == "auto" and GRM_type == "simple" and G.shape[0] >= 64 else None
    try:
        if s is not None:
            pc1 = _device_pc1(s, rows)
        on_device = pc1 is not None
        if not on_device:
            if s is not None:
                builds += s.stats()[0]
                s.close()
                s = None
            K = (grm_ploidy_aware(G, devices=[device]) if GRM_type == "ploidy-aware" else grm(G, devices=[device]))[0]
            builds += 1
            pc1 = pc1_of_grm(K)
            del K
        if s is None:
            s = GenotypeSession(G, device=device)
        r = s.gwas(rows, y, covariates=pc1, model="ols")
        builds += s.stats()[0]
    finally:
        if s is not None:
            s.close()
    fit.metrics = {"pc1_on_device": float(on_device), "grm_builds": float(builds)}
    if verbose:
        print(f"GWAS via OLS using {GRM_type} GRM: {r['tested']} loci-alleles tested")
    return _finish(fit, r["z"], kept, "GWAS_OLS")
