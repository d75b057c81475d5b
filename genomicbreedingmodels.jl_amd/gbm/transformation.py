"""Epistasis feature engineering — mirrors of reference src/transformation.jl: the six named endofunctions,
``transform1``, ``transform2``, ``epistasisfeatures`` and ``reconstitutefeatures``.

The scan over all loci (pairs of loci) runs on the device (``GenotypeSession.pair_scan``); it knows the six
named operations only and there is no CPU fallback for another callable. The at most K selected columns are
materialised on the host by one helper (:func:`evaluate_feature`: numpy on X + ε, then the reference's snapping
of values within ε of 0 and 1), which ``reconstitutefeatures`` applies again at every level of a nested name, so
``epistasisfeatures`` → ``reconstitutefeatures`` is bitwise equal. (The reference's own ``reconstitutefeatures``
substitutes the frequencies into the name and ``eval``s it, without ε and without snapping.)

Difference from the reference: a pair whose feature is constant to rounding gets slope 0 here and is never
selected (include/gbm.h, gbm_session_pair_scan); the reference's pivoted QR returns a minimum-norm slope there."""
from __future__ import annotations

import numpy as np

from ._lib import ArgumentError, GBMError, PAIR_OPS
from .prediction import extractxyetc
from .session import GenotypeSession
from .types import Genomes, Phenomes

EPS = float(np.finfo(np.float64).eps)


# ---- the named endofunctions (src/transformation.jl:9-54) ---------------------------------------------------------
def square(x):
    return x * x


def invoneplus(x):
    return 1.0 / (1.0 + x)


def log10epsdivlog10eps(x):
    return np.log10(x + EPS) / np.log10(EPS)


def mult(x, y):
    return x * y


def addnorm(x, y):
    return (x + y) / 2.0


def raise_(x, y):
    return np.power(x, y)


raise_.__name__ = "raise"  # the reference's name (a keyword in Python)

UNARY = {"square": square, "invoneplus": invoneplus, "log10epsdivlog10eps": log10epsdivlog10eps}
BINARY = {"mult": mult, "addnorm": addnorm, "raise": raise_}
FUNCTIONS = {**UNARY, **BINARY}
assert set(FUNCTIONS) == set(PAIR_OPS)


def _named(f, table, arity: int) -> str:
    name = getattr(f, "__name__", None)
    if not callable(f) or table.get(name) is not f:
        raise ArgumentError(
            f"`{name if name else f!r}` is not one of the named {'single' if arity == 1 else 'two'}-argument "
            f"functions ({', '.join(table)}): the scan runs on the device, which has these operations only, and "
            "the package has no CPU fallback for another function")
    return name


def evaluate_feature(f, columns, eps: float = EPS) -> np.ndarray:
    """f over columns that already hold X + ε (and |·| when asked), then the reference's clean-up
    (src/transformation.jl:222-227, 456-460): |T| < ε → 0 and |T − 1| < ε → 1."""
    with np.errstate(all="ignore"):
        T = np.asarray(f(*columns), dtype=np.float64).copy()
    T[np.abs(T) < eps] = 0.0
    T[np.abs(T - 1.0) < eps] = 1.0
    return T


def _shifted(X, eps, use_abs):
    Xe = X + eps
    return np.abs(Xe) if use_abs else Xe


def _scan(X, y, name, eps, use_abs, var_threshold, commutative, k, device):
    n, l = X.shape
    nslopes = l if name in UNARY else l * l
    if k > nslopes:  # the reference's slice [1:n_new_features_per_transformation] throws a BoundsError
        raise ArgumentError(f"n_new_features_per_transformation = {k} is more than the {nslopes} slopes")
    if k < 1 or k > 65536:
        raise ArgumentError(f"n_new_features_per_transformation must be in [1, 65536], got {k}")
    if n < 3:
        raise ArgumentError("the scan needs at least 3 entries with phenotype data")
    with GenotypeSession(X, device=device) as s:
        return s.pair_scan(np.arange(n), y, name, eps=eps, use_abs=use_abs, var_threshold=var_threshold,
                           commutative=commutative, k=k)


def transform1(f, genomes: Genomes, phenomes: Phenomes, *, idx_trait: int = 1, idx_entries=None,
               idx_loci_alleles=None, n_new_features_per_transformation: int = 1000, eps: float = EPS,
               use_abs: bool = False, var_threshold: float = 0.01, verbose: bool = False, device: int = 0) -> Genomes:
    """Reference transform1 (src/transformation.jl:130-238; ``eps`` is its ϵ, ``var_threshold`` its σ²_threshold):
    the at most K loci whose f(x) has the largest |slope| on the trait, in rank order, named ``f(locus)``."""
    name = _named(f, UNARY, 1)
    X, y, entries, populations, loci_alleles = extractxyetc(genomes, phenomes, idx_entries=idx_entries,
                                                            idx_loci_alleles=idx_loci_alleles, idx_trait=idx_trait,
                                                            add_intercept=False)
    r = _scan(X, y, name, eps, use_abs, var_threshold, False, int(n_new_features_per_transformation), device)
    Xe = _shifted(X, eps, use_abs)
    idx = r["index"]
    T = evaluate_feature(f, (Xe[:, idx],), eps).reshape(X.shape[0], idx.size)
    out = Genomes(entries=entries, populations=populations,
                  loci_alleles=[f"{name}({loci_alleles[j]})" for j in idx], allele_frequencies=T)
    if not out.checkdims():
        raise GBMError("Error transforming each locus using the function `" + name + "`.")
    return out


def transform2(f, genomes: Genomes, phenomes: Phenomes, *, idx_trait: int = 1, idx_entries=None,
               idx_loci_alleles=None, n_new_features_per_transformation: int = 1000, eps: float = EPS,
               use_abs: bool = False, var_threshold: float = 0.01, commutative: bool = False, verbose: bool = False,
               device: int = 0) -> Genomes:
    """Reference transform2 (src/transformation.jl:319-468): the at most K ordered pairs of loci whose f(x_i, x_j)
    has the largest |slope| on the trait, in ascending flat index i·l + j, named ``f(locus_i,locus_j)``."""
    name = _named(f, BINARY, 2)
    X, y, entries, populations, loci_alleles = extractxyetc(genomes, phenomes, idx_entries=idx_entries,
                                                            idx_loci_alleles=idx_loci_alleles, idx_trait=idx_trait,
                                                            add_intercept=False)
    l = X.shape[1]
    r = _scan(X, y, name, eps, use_abs, var_threshold, commutative, int(n_new_features_per_transformation), device)
    Xe = _shifted(X, eps, use_abs)
    idx = np.sort(r["index"])
    ii, jj = idx // l, idx % l
    T = evaluate_feature(f, (Xe[:, ii], Xe[:, jj]), eps).reshape(X.shape[0], idx.size)
    out = Genomes(entries=entries, populations=populations,
                  loci_alleles=[f"{name}({loci_alleles[i]},{loci_alleles[j]})" for i, j in zip(ii, jj)],
                  allele_frequencies=T)
    if not out.checkdims():
        raise GBMError("Error transforming each locus using the function `" + name + "`.")
    return out


def epistasisfeatures(genomes: Genomes, phenomes: Phenomes, *, idx_trait: int = 1, idx_entries=None,
                      idx_loci_alleles=None, transformations1=(square, invoneplus, log10epsdivlog10eps),
                      transformations2=(mult, addnorm, raise_), n_new_features_per_transformation: int = 1000,
                      n_reps: int = 3, verbose: bool = False, device: int = 0) -> Genomes:
    """Reference epistasisfeatures (src/transformation.jl:540-668): ``n_reps`` rounds of every transformation on
    a Genomes that grows by the new features of each (one device session per transformation call)."""
    if not genomes.checkdims() and not phenomes.checkdims():
        raise ArgumentError("The Genomes and Phenomes structs are corrupted ☹.")
    if not genomes.checkdims():
        raise ArgumentError("The Genomes struct is corrupted ☹.")
    if not phenomes.checkdims():
        raise ArgumentError("The Phenomes struct is corrupted ☹.")
    if list(genomes.entries) != list(phenomes.entries):
        raise ArgumentError("The genomes and phenomes input need to have been merged to have consitent entries.")
    n_all, p_all = len(genomes.entries), len(genomes.loci_alleles)
    if idx_entries is None:
        idx_entries = np.arange(1, n_all + 1)
    else:
        idx_entries = np.asarray(idx_entries, dtype=np.int64)
        if idx_entries.size == 0 or idx_entries.min() < 1 or idx_entries.max() > n_all:
            raise ArgumentError(
                "The indexes of the entries, `idx_entries` are out of bounds. Expected range: from 1 to "
                f"{n_all} while the supplied range is from {idx_entries.min() if idx_entries.size else None} to "
                f"{idx_entries.max() if idx_entries.size else None}.")
    if idx_loci_alleles is None:
        idx_loci_alleles = np.arange(1, p_all + 1)
    else:
        idx_loci_alleles = np.asarray(idx_loci_alleles, dtype=np.int64)
        if idx_loci_alleles.size == 0 or idx_loci_alleles.min() < 1 or idx_loci_alleles.max() > p_all:
            raise ArgumentError(
                "The indexes of the loci_alleles, `idx_loci_alleles` are out of bounds. Expected range: from 1 to "
                f"{p_all} while the supplied range is from "
                f"{idx_loci_alleles.min() if idx_loci_alleles.size else None} to "
                f"{idx_loci_alleles.max() if idx_loci_alleles.size else None}.")
    if not 1 <= idx_trait <= len(phenomes.traits):
        raise ArgumentError(f"idx_trait = {idx_trait} is out of bounds (1 to {len(phenomes.traits)}).")
    for f in transformations1:
        _named(f, UNARY, 1)
    for f in transformations2:
        _named(f, BINARY, 2)
    rows, cols = idx_entries - 1, idx_loci_alleles - 1
    g = Genomes(entries=[genomes.entries[r] for r in rows], populations=[genomes.populations[r] for r in rows],
                loci_alleles=[genomes.loci_alleles[c] for c in cols],
                allele_frequencies=np.asarray(genomes.allele_frequencies, dtype=np.float64)[np.ix_(rows, cols)].copy())
    ph = Phenomes(entries=[phenomes.entries[r] for r in rows], populations=[phenomes.populations[r] for r in rows],
                  traits=[phenomes.traits[idx_trait - 1]],
                  phenotypes=np.asarray(phenomes.phenotypes, dtype=np.float64)[rows][:, [idx_trait - 1]].copy())
    for _ in range(int(n_reps)):
        for f in (*transformations1, *transformations2):
            tr = transform1 if f in tuple(transformations1) else transform2
            t = tr(f, g, ph, n_new_features_per_transformation=n_new_features_per_transformation, device=device)
            have = set(g.loci_alleles)
            new = []
            for c, nm in enumerate(t.loci_alleles):
                if nm not in have:
                    have.add(nm)
                    new.append(c)
            # a transformation drops the entries without a phenotype; the grown matrix keeps every entry
            if len(t.entries) != len(g.entries):
                raise GBMError("Error generating new features: entries without phenotype data (filter them first).")
            g.loci_alleles = list(g.loci_alleles) + [t.loci_alleles[c] for c in new]
            g.allele_frequencies = np.hstack([g.allele_frequencies, t.allele_frequencies[:, new]])
            if g.allele_frequencies.min() < 0.0 or abs(g.allele_frequencies.max() - 1.0) > 1e-12:
                raise GBMError("The function `" + f.__name__ + "` generates values outside the expected range of "
                               "zero to one. Please replace with an appropriate transforamtion function.")
    if not g.checkdims():
        raise GBMError("Error generating new features.")
    return g


# ---- names back to features -------------------------------------------------------------------------------------
def _split_top(inner: str) -> list:
    parts, depth, start = [], 0, 0
    for k, ch in enumerate(inner):
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth < 0:
                raise ArgumentError("unbalanced parentheses in the feature name")
        elif ch == "," and depth == 0:
            parts.append(inner[start:k])
            start = k + 1
    if depth != 0:
        raise ArgumentError("unbalanced parentheses in the feature name")
    parts.append(inner[start:])
    return parts


def parse_feature_name(name: str, known, leaf_ok: bool = True) -> tuple:
    """The tree of a nested feature name over the six function names: a leaf is a name in ``known`` (returned as
    the string), a node is (function name, [children]). ArgumentError for anything else. ``leaf_ok`` off: the
    name itself must be a node even when it is in ``known``."""
    if leaf_ok and name in known:
        return name
    k = name.find("(")
    if k <= 0 or not name.endswith(")"):
        raise ArgumentError(f"`{name}` is neither a known locus-allele name nor a feature name f(...)")
    fname = name[:k]
    if fname not in FUNCTIONS:
        raise ArgumentError(f"`{fname}` in `{name}` is not one of the named functions ({', '.join(FUNCTIONS)})")
    args = _split_top(name[k + 1:-1])
    if len(args) != (1 if fname in UNARY else 2):
        raise ArgumentError(f"`{fname}` takes {1 if fname in UNARY else 2} argument(s), `{name}` gives {len(args)}")
    return fname, [parse_feature_name(a, known) for a in args]


def reconstitutefeatures(genomes: Genomes, feature_names, *, eps: float = EPS, use_abs: bool = False,
                         verbose: bool = False) -> Genomes:
    """Reference reconstitutefeatures (src/transformation.jl:730-778): the features named by ``feature_names``
    (nested ``f(a)`` / ``f(a,b)`` over the six function names and the loci-alleles of ``genomes``), rebuilt by
    :func:`evaluate_feature` with the ε, the absolute values and the snapping that made them, at every level."""
    if not genomes.checkdims():
        raise ArgumentError("The Genomes struct is corrupted ☹.")
    pos = {nm: c for c, nm in enumerate(genomes.loci_alleles)}
    for nm in pos:
        if any(ch in nm for ch in "(),"):
            # a name with parentheses or a comma must itself be a feature over the other names
            try:
                parse_feature_name(nm, pos, leaf_ok=False)
            except ArgumentError:
                raise ArgumentError(f"the locus-allele name `{nm}` contains a parenthesis or a comma and is not a "
                                    "feature name: nested feature names cannot be told apart from it") from None
    X = np.asarray(genomes.allele_frequencies, dtype=np.float64)
    cache = {}

    def value(node):
        if isinstance(node, str):
            return X[:, pos[node]]
        key = repr(node)
        if key not in cache:
            fname, kids = node
            cache[key] = evaluate_feature(FUNCTIONS[fname], [_shifted(value(c), eps, use_abs) for c in kids], eps)
        return cache[key]

    names = list(feature_names)
    T = np.empty((X.shape[0], len(names)))
    for c, nm in enumerate(names):
        T[:, c] = value(parse_feature_name(nm, pos))
    out = Genomes(entries=list(genomes.entries), populations=list(genomes.populations), loci_alleles=names,
                  allele_frequencies=T)
    if not out.checkdims():
        raise GBMError("Error reconstituting features.")
    return out
