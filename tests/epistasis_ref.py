"""The epistasis feature scan of include/gbm.h (gbm_session_pair_scan) and the functions above it, as literal
numpy: reference transform1 / transform2 / epistasisfeatures (src/transformation.jl:130-668) restated with one
least-squares call per pair, beside the closed form the device uses (β = S_fy/S_ff with yc = y − ȳ,
S_fy = Σ f·yc, S_ff = Σ (f − f̄)²) in float64 and in long double.

Flat index of the pair (i, j) of l loci: i·l + j (0-based); a unary operation has l slopes, index j."""
import numpy as np

from gbm.transformation import evaluate_feature
from gbm.types import Genomes, Phenomes

EPS = float(np.finfo(np.float64).eps)

UNARY = ("square", "invoneplus", "log10epsdivlog10eps")
BINARY = ("mult", "addnorm", "raise")


def apply_op(op, a, b, dtype=np.float64):
    """f of the named operation on arrays of ``dtype`` (a is ignored by the unary operations)."""
    one, two, eps = dtype(1.0), dtype(2.0), dtype(EPS)
    with np.errstate(all="ignore"):
        if op == "mult":
            return a * b
        if op == "addnorm":
            return (a + b) / two
        if op == "raise":
            return np.power(a, b)
        if op == "square":
            return b * b
        if op == "invoneplus":
            return one / (one + b)
        if op == "log10epsdivlog10eps":
            return np.log10(b + eps) / np.log10(eps)
    raise ValueError(op)


def work_matrix(X, eps, use_abs=False):
    Xe = np.asarray(X, dtype=np.float64) + eps
    return np.abs(Xe) if use_abs else Xe


def skipped(Xe, var_threshold):
    return Xe.var(axis=0, ddof=1) < var_threshold


def tested_mask(Xe, op, var_threshold=0.01, commutative=False):
    """(l, l) (binary) or (l,) (unary): the pairs the reference's loop reaches ols with."""
    sk = skipped(Xe, var_threshold)
    if op in UNARY:
        return ~sk
    l = Xe.shape[1]
    m = ~sk[:, None] & ~sk[None, :]
    if commutative:
        m &= np.arange(l)[None, :] >= np.arange(l)[:, None]
    return m


def features(Xe, op, dtype=np.float64):
    """(l, l, n) (binary) or (l, n) (unary) feature values."""
    Z = np.asarray(Xe, dtype=dtype).T
    if op in UNARY:
        return apply_op(op, Z, Z, dtype)
    return apply_op(op, Z[:, None, :], Z[None, :, :], dtype)


def slopes_lstsq(Xe, y, op, var_threshold=0.01, commutative=False):
    """The literal loop: ols on [1, f] per tested pair (src/linear.jl:85, X \\ y), slope kept; 0 elsewhere."""
    mask = tested_mask(Xe, op, var_threshold, commutative)
    F = features(Xe, op)
    out = np.zeros(mask.shape)
    A = np.ones((Xe.shape[0], 2))
    for pos in zip(*np.nonzero(mask)):
        A[:, 1] = F[pos]
        out[pos] = np.linalg.lstsq(A, y, rcond=None)[0][1]
    return out


def closed_form(Xe, y, op, var_threshold=0.01, commutative=False, dtype=np.float64):
    """The closed form in ``dtype``: dict(beta, Sff, Sf2, Sfy, A = Σ|f − f̄||yc|, R = S_ff/Σf² (conditioning),
    ratio = n·S_ff/max(n, Σf²)² (the squared diagonal ratio of R in the QR of [1, f]), mask). beta is 0 off the
    mask; the other arrays hold the values of every pair."""
    mask = tested_mask(Xe, op, var_threshold, commutative)
    F = features(Xe, op, dtype)
    yv = np.asarray(y, dtype=dtype)
    n = dtype(len(yv))
    yc = yv - yv.sum() / n
    fbar = F.sum(axis=-1) / n
    D = F - fbar[..., None]
    with np.errstate(all="ignore"):
        Sff = (D * D).sum(axis=-1)
        Sf2 = (F * F).sum(axis=-1)
        Sfy = (F * yc).sum(axis=-1)
        A = (np.abs(D) * np.abs(yc)).sum(axis=-1)
        beta = np.where(mask, Sfy / np.where(Sff > 0, Sff, dtype(1.0)), dtype(0.0))
        R = Sff / Sf2
        ratio = n * Sff / np.maximum(n, Sf2) ** 2
    return {"beta": beta, "Sff": Sff, "Sf2": Sf2, "Sfy": Sfy, "A": A, "R": R, "ratio": ratio, "mask": mask}


DEGENERATE = (2.0 * EPS) ** 2  # the device's rule: ratio <= (2·eps)²


def error_ratio(beta, ld):
    """|β − β_ld| / (eps·(|β_ld|/√R + A/S_ff)) on the tested pairs (ld: closed_form(..., dtype=np.longdouble))."""
    m = ld["mask"]
    b = np.asarray(beta, dtype=np.longdouble)[m]
    bl, R, A, Sff = ld["beta"][m], ld["R"][m], ld["A"][m], ld["Sff"][m]
    return np.asarray(np.abs(b - bl) / (np.longdouble(EPS) * (np.abs(bl) / np.sqrt(R) + A / Sff)), dtype=np.float64)


def stable_topk(beta, k, eps):
    """sortperm(abs.(β), rev = true)[1:k] then the > ϵ filter (src/transformation.jl:420-428): flat indices."""
    b = np.asarray(beta, dtype=np.float64).ravel()
    if k > b.size:
        raise IndexError("k is more than the number of slopes")
    order = np.argsort(-np.abs(b), kind="stable")[:k]
    return order[np.abs(b[order]) > eps]


# ---- the functions above the scan ---------------------------------------------------------------------------------
def _xy(genomes, phenomes, idx_trait=1):
    X = np.asarray(genomes.allele_frequencies, dtype=np.float64)
    y = np.asarray(phenomes.phenotypes[:, idx_trait - 1], dtype=np.float64)
    return X, y


def transform1(f, genomes, phenomes, k=1000, eps=EPS, use_abs=False, var_threshold=0.01, slopes=slopes_lstsq):
    op = f.__name__
    X, y = _xy(genomes, phenomes)
    Xe = work_matrix(X, eps, use_abs)
    idx = stable_topk(slopes(Xe, y, op, var_threshold), k, eps)
    T = evaluate_feature(f, (Xe[:, idx],), eps).reshape(X.shape[0], idx.size)
    return Genomes(entries=list(genomes.entries), populations=list(genomes.populations),
                   loci_alleles=[f"{op}({genomes.loci_alleles[j]})" for j in idx], allele_frequencies=T)


def transform2(f, genomes, phenomes, k=1000, eps=EPS, use_abs=False, var_threshold=0.01, commutative=False,
               slopes=slopes_lstsq):
    op = f.__name__
    X, y = _xy(genomes, phenomes)
    l = X.shape[1]
    Xe = work_matrix(X, eps, use_abs)
    idx = np.sort(stable_topk(slopes(Xe, y, op, var_threshold, commutative), k, eps))
    names, cols = [], []
    for c in idx:
        i, j = c // l, c % l
        cols.append(evaluate_feature(f, (Xe[:, i], Xe[:, j]), eps))
        names.append(f"{op}({genomes.loci_alleles[i]},{genomes.loci_alleles[j]})")
    T = np.column_stack(cols) if cols else np.zeros((X.shape[0], 0))
    return Genomes(entries=list(genomes.entries), populations=list(genomes.populations), loci_alleles=names,
                   allele_frequencies=T)


def epistasisfeatures(genomes, phenomes, transformations1, transformations2, k=1000, n_reps=3,
                      slopes=slopes_lstsq):
    g = Genomes(entries=list(genomes.entries), populations=list(genomes.populations),
                loci_alleles=list(genomes.loci_alleles),
                allele_frequencies=np.array(genomes.allele_frequencies, dtype=np.float64))
    for _ in range(n_reps):
        for f in (*transformations1, *transformations2):
            t = (transform1 if f in transformations1 else transform2)(f, g, phenomes, k=k, slopes=slopes)
            new = []
            for c, nm in enumerate(t.loci_alleles):
                if nm not in g.loci_alleles and nm not in [t.loci_alleles[d] for d in new]:
                    new.append(c)
            g.loci_alleles = g.loci_alleles + [t.loci_alleles[c] for c in new]
            g.allele_frequencies = np.hstack([g.allele_frequencies, t.allele_frequencies[:, new]])
    return g


def slopes_closed64(Xe, y, op, var_threshold=0.01, commutative=False):
    """closed_form's float64 β with the device's degenerate rule (for the grown matrices of epistasisfeatures,
    where one lstsq per pair would take minutes)."""
    c = closed_form(Xe, y, op, var_threshold, commutative)
    return np.where(c["ratio"] <= DEGENERATE, 0.0, c["beta"])
