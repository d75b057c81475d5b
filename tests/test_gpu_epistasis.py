"""The epistasis feature scan on the device (GenotypeSession.pair_scan / gbm_session_pair_scan) and the functions
above it (gbm.transformation) against the numpy reference of epistasis_ref.py.

Shapes: n = 97 entries (no multiple of the 32-row chunk), l = 70 loci (one full 64-tile and a ragged 6), l = 130 for
the panels. Two data sets: allele frequencies round(beta(0.6, 0.6), 3) with ε = eps, and dosages binomial(2, f)/2
with ε = 1e-3 (with ε = eps on dosages, product features of scale ε sit next to the rank boundary: not tested).

Every comparison first asserts on the CPU what makes its input fair (conditions on the inputs, not measurements):
no tested pair within a factor 1e4 of the degenerate threshold (2·eps)², the float64 and long-double top-K sets
equal, the K-th value separated from the next by more than 100 pair tolerances.

The per-pair error against the long-double closed form is e = |β − β_ld| / (eps·(|β_ld|/√R + A/S_ff)), R = S_ff/Σf²,
A = Σ|f − f̄||yc|; the bound is max e <= 4·c_ref with c_ref the same maximum for numpy's float64 closed form and the
lstsq loop (computed here): the device differs from numpy in summation order and in the last ulp of pow and log10,
errors of the kind and size of numpy's own."""
import functools

import numpy as np
import pytest

import gbm
from gbm import transformation as tr

import epistasis_ref as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
N, L, K = 97, 70, 50
OPS = ref.UNARY + ref.BINARY
SKIP_CONST, SKIP_LOWVAR, DUP_A, DUP_B = 10, 20, 3, 66
DATA_EPS = {"continuous": EPS, "dosage": 1e-3}


# ---- inputs and references (computed once, read-only) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dataset(name, l=L):
    rng = np.random.default_rng(7)
    if name == "continuous":
        X = np.round(rng.beta(0.6, 0.6, (N, l)), 3)
    else:
        X = rng.binomial(2, rng.uniform(0.02, 0.98, l), (N, l)) / 2.0
    X[:, SKIP_CONST] = 0.5
    X[:, SKIP_LOWVAR] = np.where(np.arange(N) % 2 == 0, 0.43, 0.57)  # variance 0.0049 < 0.01
    X[:, DUP_B] = X[:, DUP_A]  # the same column in two tiles
    y = (1.0 + 0.8 * X[:, 1] - 0.6 * X[:, 5] + 0.5 * X[:, 30] + 1.2 * X[:, 7] * X[:, 40]
         + 0.4 * rng.standard_normal(N))
    X = np.asfortranarray(X)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def reference(name, op, rows=None, loci=None, l=L, eps=None, commutative=False):
    """dict: ld (long-double closed form), b64, loop (float64 β), c_ref, on the rows / loci subset."""
    X, y = dataset(name, l)
    r = np.arange(N) if rows is None else np.asarray(rows)
    c = np.arange(l) if loci is None else np.asarray(loci)
    Xe = ref.work_matrix(X[np.ix_(r, c)], DATA_EPS[name] if eps is None else eps)
    yy = y[r]
    ld = ref.closed_form(Xe, yy, op, commutative=commutative, dtype=np.longdouble)
    b64 = ref.closed_form(Xe, yy, op, commutative=commutative)["beta"]
    loop = ref.slopes_lstsq(Xe, yy, op, commutative=commutative)
    regular = ld["mask"] & (ld["ratio"] > 1e4 * ref.DEGENERATE)
    out = {"ld": ld, "b64": b64, "loop": loop, "regular": regular,
           "clear_degenerate": ld["mask"] & (ld["ratio"] < 1e-4 * ref.DEGENERATE)}
    sub = dict(ld, mask=regular)
    out["c_ref"] = max(ref.error_ratio(b64, sub).max(), ref.error_ratio(loop, sub).max())
    out["sub"] = sub
    return out


def guard_band(rf):
    """No tested pair within a factor 1e4 of the degenerate threshold."""
    ld = rf["ld"]
    assert (rf["regular"] | rf["clear_degenerate"])[ld["mask"]].all()


def expected_beta_ld(rf):
    return np.where(rf["regular"], rf["ld"]["beta"], np.longdouble(0.0))


def pair_tolerance(rf, flat):
    ld = rf["ld"]
    b, R, A, S = (np.asarray(ld[k]).ravel()[flat] for k in ("beta", "R", "A", "Sff"))
    return float(4.0 * rf["c_ref"] * EPS * (abs(b) / np.sqrt(R) + A / S))


def guard_topk(rf, k, eps):
    """The float64 and long-double top-k sets are equal, and the k-th |β| is more than 100 pair tolerances above
    the next smaller value (exact ties, as between (i, j) and (j, i) under mult, are settled by the index rule)."""
    bl = expected_beta_ld(rf)
    top_ld = ref.stable_topk(np.asarray(bl, dtype=np.float64), k, eps)
    b64 = np.where(rf["regular"], rf["b64"], 0.0)
    assert set(top_ld) == set(ref.stable_topk(b64, k, eps))
    a = np.abs(bl).ravel()
    kth = a[top_ld[-1]]
    below = a[a < kth]
    if len(top_ld) == k and below.size and below.max() > eps:
        nxt = int(np.argmax(np.where(a < kth, a, -1)))
        assert float(kth - a[nxt]) > 100.0 * max(pair_tolerance(rf, top_ld[-1]), pair_tolerance(rf, nxt))
    return top_ld


def scan(name, op, rows=None, loci=None, l=L, eps=None, session=None, **kw):
    X, y = dataset(name, l)
    r = np.arange(N) if rows is None else np.asarray(rows)
    e = DATA_EPS[name] if eps is None else eps
    kw.setdefault("k", K)
    if session is not None:
        return session.pair_scan(r, y[r], op, loci=loci, eps=e, **kw)
    with gbm.GenotypeSession(X) as s:
        return s.pair_scan(r, y[r], op, loci=loci, eps=e, **kw)


def check_full(res, rf, label):
    """beta_full against the long-double closed form: exact zeros off the regular pairs, the error bound on them."""
    guard_band(rf)
    bf = res["beta_full"]
    assert bf.shape == rf["ld"]["mask"].shape
    assert not bf[~rf["regular"]].any()
    assert res["tested"] == int(rf["ld"]["mask"].sum())
    assert res["degenerate"] == int(rf["clear_degenerate"].sum())
    e = ref.error_ratio(bf, rf["sub"]).max()
    print(f"{label}: max e = {e:.3f}, c_ref = {rf['c_ref']:.3f}, min R = {float(rf['ld']['R'][rf['regular']].min()):.3g}")
    assert e <= 4.0 * rf["c_ref"], (label, e, rf["c_ref"])


# ---- full β -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["continuous", "dosage"])
def test_full_beta_against_long_double(name, op):
    rf = reference(name, op)
    res = scan(name, op, full=True)
    check_full(res, rf, f"{name}/{op}")
    bf = res["beta_full"]
    if op in ref.BINARY:  # the skipped loci: exact zeros in their rows and columns
        for j in (SKIP_CONST, SKIP_LOWVAR):
            assert not bf[j, :].any() and not bf[:, j].any()
        assert name != "continuous" or res["tested"] == (L - 2) ** 2
    else:
        assert bf[SKIP_CONST] == 0.0 and bf[SKIP_LOWVAR] == 0.0
        assert name != "continuous" or res["tested"] == L - 2


# ---- determinism and position -------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ref.BINARY)
def test_bits_do_not_depend_on_the_call_or_the_position(op):
    X, _ = dataset("continuous")
    with gbm.GenotypeSession(X) as s:
        a = scan("continuous", op, session=s, full=True)
        b = scan("continuous", op, session=s, full=True)
    fa, fb = a["beta_full"], b["beta_full"]
    assert np.array_equal(fa.view(np.int64), fb.view(np.int64))
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["beta"].view(np.int64), b["beta"].view(np.int64))
    if op in ("mult", "addnorm"):
        assert np.array_equal(fa.view(np.int64), fa.T.copy().view(np.int64))
    # the duplicated column (tiles 0 and 1): equal rows and equal columns
    assert np.array_equal(fa[DUP_A, :].view(np.int64), fa[DUP_B, :].view(np.int64))
    assert np.array_equal(fa[:, DUP_A].copy().view(np.int64), fa[:, DUP_B].copy().view(np.int64))
    assert fa[DUP_A, :].any()


def test_top_k_tie_goes_to_the_lower_flat_index():
    res = scan("continuous", "mult", full=True, k=1)
    bf = res["beta_full"]
    i, j = divmod(int(res["index"][0]), L)
    # under mult the largest |β| is shared by (i, j) and (j, i), or by the duplicated column's pairs
    ties = np.flatnonzero(np.abs(bf).ravel() == abs(res["beta"][0]))
    assert ties.size >= 2 or i == j
    assert res["index"][0] == ties.min()


# ---- top-K --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("commutative", [False, True])
@pytest.mark.parametrize("op", ref.BINARY)
@pytest.mark.parametrize("name", ["continuous", "dosage"])
def test_top_k_follows_the_stable_rule(name, op, commutative):
    eps = DATA_EPS[name]
    rf = reference(name, op, commutative=commutative)
    guard_band(rf)
    full = scan(name, op, full=True, commutative=commutative)
    bf = full["beta_full"]
    if commutative:
        assert not bf[np.tril_indices(L, -1)].any()
    assert full["tested"] == int(rf["ld"]["mask"].sum())
    nzero = int((np.abs(bf) <= eps).sum())
    X, _ = dataset(name)
    with gbm.GenotypeSession(X) as s:
        for k in (1, K, L * L - nzero + 5):
            res = scan(name, op, session=s, k=k, commutative=commutative)
            want = ref.stable_topk(bf, k, eps)  # the reference's rule on the device's own slopes: exact
            assert np.array_equal(res["index"], want), k
            assert np.array_equal(res["beta"].view(np.int64), bf.ravel()[want].view(np.int64))
            if k > K:
                assert res["index"].size == L * L - nzero < k
    # and against the long-double slopes, where the guards make the set well defined
    top_ld = guard_topk(rf, K, eps)
    assert set(full["index"]) == set(top_ld)


@pytest.mark.parametrize("op", ref.UNARY)
def test_top_k_unary(op):
    rf = reference("continuous", op)
    full = scan("continuous", op, full=True, k=L)
    want = ref.stable_topk(full["beta_full"], L, EPS)
    assert np.array_equal(full["index"], want) and want.size == L - 2
    res = scan("continuous", op, k=7)
    assert np.array_equal(res["index"], want[:7])
    assert set(res["index"]) == set(guard_topk(rf, 7, EPS))


# ---- panels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["mult", "raise"])
def test_panels_do_not_change_the_result(op):
    l = 130
    X, _ = dataset("continuous", l)
    with gbm.GenotypeSession(X) as s:
        one = scan("continuous", op, l=l, session=s, full=True, k=300)
        want = ref.stable_topk(one["beta_full"], 300, EPS)
        assert np.array_equal(one["index"], want)
        for rows in (64, 128):
            many = scan("continuous", op, l=l, session=s, panel_rows=rows, k=300)
            assert np.array_equal(many["index"], one["index"])
            assert np.array_equal(many["beta"].view(np.int64), one["beta"].view(np.int64))
            assert (many["tested"], many["degenerate"]) == (one["tested"], one["degenerate"])
            with pytest.raises(gbm.ArgumentError, match="one panel"):
                scan("continuous", op, l=l, session=s, panel_rows=rows, full=True)
    rf = reference("continuous", op, l=l)
    check_full(one, rf, f"l=130/{op}")


# ---- subsets ------------------------------------------------------------------------------------------------------
ROWS80 = tuple(np.sort(np.random.default_rng(80).choice(N, 80, replace=False)))
ROWS33 = tuple(np.sort(np.random.default_rng(33).choice(N, 33, replace=False)))
ROWS3 = (4, 50, 90)
LOCI37 = tuple(np.random.default_rng(37).permutation(L)[:37])


@pytest.mark.parametrize("op", ["raise", "addnorm", "invoneplus"])
@pytest.mark.parametrize("rows, loci", [(ROWS80, None), (None, LOCI37), (ROWS33, LOCI37), (ROWS3, None)],
                         ids=["rows80", "loci37", "rows33-loci37", "rows3"])
def test_row_and_locus_subsets(op, rows, loci):
    rf = reference("continuous", op, rows=rows, loci=loci)
    res = scan("continuous", op, rows=rows, loci=None if loci is None else np.asarray(loci), full=True,
               k=5)
    check_full(res, rf, f"subset/{op}")
    assert np.array_equal(res["index"], ref.stable_topk(res["beta_full"], 5, EPS))


@pytest.mark.parametrize("op", ["mult", "square"])
def test_session_from_int8_dosages(op):
    X, y = dataset("dosage")
    D = np.asfortranarray(np.rint(2.0 * X).astype(np.int8))
    keep = [j for j in range(L) if j != SKIP_LOWVAR]  # 0.43 / 0.57 is no dosage
    assert np.array_equal(D[:, keep] / 2.0, X[:, keep])
    with gbm.GenotypeSession(dosage_i8=D, ploidy=2) as s:
        res = s.pair_scan(np.arange(N), y, op, loci=np.asarray(keep), eps=1e-3, full=True, k=K)
    rf = reference("dosage", op, loci=tuple(keep))
    check_full(res, rf, f"int8/{op}")
    with gbm.GenotypeSession(X) as s:
        same = s.pair_scan(np.arange(N), y, op, loci=np.asarray(keep), eps=1e-3, full=True, k=K)
    assert np.array_equal(res["beta_full"].view(np.int64), same["beta_full"].view(np.int64))


# ---- degenerate pairs ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_data():
    X, y = dataset("dosage")
    X = np.array(X)
    X[:, 12] = 1.0 - X[:, 11]  # addnorm(x11, x12) = 0.5 exactly
    X[:, 14] = np.where(X[:, 13] >= 0.5, 1.0, 0.0)
    X[:, 15] = 1.0 - X[:, 14]  # mult(x14, x15) = 0 exactly
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X, y


@pytest.mark.parametrize("op, planted", [("addnorm", (11, 12)), ("mult", (14, 15))])
def test_degenerate_pairs_get_zero_and_are_counted(op, planted):
    X, y = degenerate_data()
    Xe = ref.work_matrix(X, 0.0)
    ld = ref.closed_form(Xe, y, op, dtype=np.longdouble)
    regular = ld["mask"] & (ld["ratio"] > 1e4 * ref.DEGENERATE)
    clear = ld["mask"] & (ld["ratio"] < 1e-4 * ref.DEGENERATE)
    assert (regular | clear)[ld["mask"]].all()  # the guard band
    a, b = planted
    assert ld["mask"][a, b] and clear[a, b] and clear[b, a]
    with gbm.GenotypeSession(X) as s:
        res = s.pair_scan(np.arange(N), y, op, eps=0.0, full=True, k=L * L)
    bf = res["beta_full"]
    assert res["degenerate"] == int(clear.sum()) and res["tested"] == int(ld["mask"].sum())
    assert not bf[clear].any() and bf[regular].all()
    assert a * L + b not in res["index"] and b * L + a not in res["index"]
    assert np.array_equal(res["index"], ref.stable_topk(bf, L * L, 0.0))
    b64 = ref.closed_form(Xe, y, op)["beta"]
    sub = dict(ld, mask=regular)
    assert ref.error_ratio(bf, sub).max() <= 4.0 * max(ref.error_ratio(b64, sub).max(),
                                                       ref.error_ratio(ref.slopes_lstsq(Xe, y, op), sub).max())


# ---- errors -------------------------------------------------------------------------------------------------------
def test_errors():
    X, y = dataset("continuous")
    Xn = np.array(X)
    Xn[5, 8] = -0.3
    idx = np.arange(N)
    with gbm.GenotypeSession(Xn) as s:
        with pytest.raises(gbm.ArgumentError, match="use_abs=true"):
            s.pair_scan(idx, y, gbm.raise_, k=K)
        with pytest.raises(gbm.ArgumentError, match="use_abs=true"):
            s.pair_scan(idx, y, "log10epsdivlog10eps", k=K, eps=EPS)
        ok = s.pair_scan(idx, y, gbm.raise_, k=K, use_abs=True)
        assert ok["index"].size == K
        for bad in ("cube", np.multiply, lambda a, b: a * b, 7):
            with pytest.raises(gbm.ArgumentError, match="op must be one of"):
                s.pair_scan(idx, y, bad)
        for k in (0, 65537, L * L + 1):
            with pytest.raises(gbm.ArgumentError, match="k must be"):
                s.pair_scan(idx, y, "mult", k=k)
        with pytest.raises(gbm.ArgumentError, match="k must be"):
            s.pair_scan(idx, y, "square", k=L + 1)
        with pytest.raises(gbm.ArgumentError, match="strictly increasing"):
            s.pair_scan(idx[::-1], y, "mult", k=K)
        with pytest.raises(gbm.ArgumentError, match="out of range"):
            s.pair_scan(np.array([0, 1, N]), y[:3], "mult", k=K)
        with pytest.raises(gbm.ArgumentError, match="at least 3"):
            s.pair_scan(idx[:2], y[:2], "mult", k=K)
        with pytest.raises(gbm.ArgumentError, match="distinct"):
            s.pair_scan(idx, y, "mult", loci=[1, 2, 2], k=5)
        with pytest.raises(gbm.ArgumentError, match="out of range"):
            s.pair_scan(idx, y, "mult", loci=[1, 2, L], k=5)
        with pytest.raises(gbm.ArgumentError, match="multiple of 64"):
            s.pair_scan(idx, y, "mult", panel_rows=63, k=K)
        with pytest.raises(gbm.ArgumentError, match="binary"):
            s.pair_scan(idx, y, "square", commutative=True, k=5)
        with pytest.raises(gbm.ArgumentError, match="eps"):
            s.pair_scan(idx, y, "mult", eps=-1.0, k=5)
    g, p = population(X[:, :12], y)
    with pytest.raises(gbm.ArgumentError, match="not one of the named"):
        gbm.transform2(lambda a, b: a * b, g, p)


# ---- the Python layer ---------------------------------------------------------------------------------------------
def population(X, y):
    n, l = X.shape
    entries = [f"entry_{i + 1}" for i in range(n)]
    g = gbm.Genomes(entries=entries, populations=["pop"] * n,
                    loci_alleles=[f"chr{1 + j // 8}\t{100 * j + 1}\tA|T\tA" for j in range(l)],
                    allele_frequencies=np.array(X))
    p = gbm.Phenomes(entries=list(entries), populations=["pop"] * n, traits=["trait_1"],
                     phenotypes=np.array(y)[:, None])
    return g, p


@functools.lru_cache(maxsize=None)
def small_population():
    X, y = dataset("continuous")
    X = np.array(X[:, 24:48])  # 24 loci, none of the planted ones
    X[0, 0], X[1, 0] = 0.0, 1.0  # the range check of epistasisfeatures wants a maximum of 1
    y = y + 0.9 * X[:, 2] - 1.1 * X[:, 4] * X[:, 9]
    return X, y


def well_separated(beta, k, eps):
    """The top (k + 1) distinct |β| are more than 1e-9 apart (relative): the rank order is beyond rounding, whose
    scale on this data (R >= 1e-3, n = 97) is below 1e-12."""
    a = np.unique(np.abs(np.asarray(beta, dtype=np.float64)).ravel())[::-1]
    a = a[a > eps][: k + 1]
    return a.size < 2 or float((a[:-1] / a[1:]).min() - 1.0) > 1e-9


@pytest.mark.parametrize("f", [gbm.square, gbm.invoneplus, gbm.log10epsdivlog10eps, gbm.mult, gbm.addnorm, gbm.raise_],
                         ids=lambda f: f.__name__)
def test_transform_matches_the_literal_reference(f):
    X, y = small_population()
    g, p = population(X, y)
    unary = f.__name__ in ref.UNARY
    k = 6 if unary else 20
    assert well_separated(ref.slopes_lstsq(ref.work_matrix(X, EPS), y, f.__name__), k, EPS)
    if unary:
        got, want = gbm.transform1(f, g, p, n_new_features_per_transformation=k), ref.transform1(f, g, p, k=k)
    else:
        got, want = gbm.transform2(f, g, p, n_new_features_per_transformation=k), ref.transform2(f, g, p, k=k)
    assert got.loci_alleles == want.loci_alleles and len(got.loci_alleles) == k
    assert np.array_equal(got.allele_frequencies.view(np.int64), want.allele_frequencies.view(np.int64))
    assert got.entries == g.entries and got.checkdims()
    with pytest.raises(gbm.ArgumentError, match="more than the"):
        (gbm.transform1 if unary else gbm.transform2)(f, g, p, n_new_features_per_transformation=24 * 24 + 1)


def test_epistasisfeatures_and_reconstitution():
    X, y = small_population()
    g, p = population(X, y)
    t1, t2 = (gbm.square, gbm.invoneplus, gbm.log10epsdivlog10eps), (gbm.mult, gbm.addnorm, gbm.raise_)
    got = gbm.epistasisfeatures(g, p, n_new_features_per_transformation=20, n_reps=2)
    # the literal loop with the device's degenerate rule in its slopes (ref.slopes_closed64)
    want = ref.epistasisfeatures(g, p, t1, t2, k=20, n_reps=2, slopes=ref.slopes_closed64)
    assert got.loci_alleles == want.loci_alleles
    assert got.loci_alleles[:24] == g.loci_alleles and len(got.loci_alleles) > 24 + 60
    assert np.array_equal(got.allele_frequencies.view(np.int64), want.allele_frequencies.view(np.int64))
    assert any(nm.count("(") >= 2 for nm in got.loci_alleles)  # the second round builds on the first
    back = gbm.reconstitutefeatures(g, got.loci_alleles)
    assert back.loci_alleles == got.loci_alleles
    assert np.array_equal(back.allele_frequencies.view(np.int64), got.allele_frequencies.view(np.int64))


def test_scan_leaves_the_training_cache_alone():
    X, y = dataset("continuous")
    idx = np.asarray(ROWS80)
    with gbm.GenotypeSession(X) as s:
        b0, p0, mu0, q0 = s.gblup(idx, y[idx])
        builds, hits = s.stats()
        s.pair_scan(idx, y[idx], "mult", k=K)
        s.pair_scan(np.arange(N), y, "square", k=5)
        assert s.stats() == (builds, hits)
        b1, p1, mu1, q1 = s.gblup(idx, y[idx])
        assert s.stats() == (builds, hits + 1)
    assert q0 == q1 and np.array_equal(b0.view(np.int64), b1.view(np.int64))
    assert np.array_equal(p0.view(np.int64), p1.view(np.int64)) and np.array_equal(mu0.view(np.int64), mu1.view(np.int64))
