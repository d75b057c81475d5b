"""CPU tests of the epistasis feature layer (gbm.transformation) and of its numpy reference (epistasis_ref.py):
the three forms of the slope agree with each other, nested names parse and rebuild bitwise, and the argument
errors that need no device are raised. The device scan itself is tested in test_gpu_epistasis.py."""
import functools

import numpy as np
import pytest

import gbm
from gbm import _lib, transformation as tr

import epistasis_ref as ref

EPS = ref.EPS


@functools.lru_cache(maxsize=None)
def small():
    rng = np.random.default_rng(5)
    n, l = 41, 9
    X = np.round(rng.beta(0.6, 0.6, (n, l)), 3)
    X[:, 4] = 0.25  # a constant column: skipped
    y = 2.0 + X[:, 0] - 0.7 * X[:, 2] + 1.5 * X[:, 1] * X[:, 3] + 0.3 * rng.standard_normal(n)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def genomes_of(X, y):
    n, l = X.shape
    entries = [f"entry_{i + 1}" for i in range(n)]
    pops = ["pop"] * n
    g = gbm.Genomes(entries=entries, populations=pops,
                    loci_alleles=[f"chr1\t{j + 1}\tA|T\tA" for j in range(l)], allele_frequencies=np.array(X))
    p = gbm.Phenomes(entries=list(entries), populations=list(pops), traits=["trait_1"], phenotypes=np.array(y)[:, None])
    return g, p


def test_symbols_and_names():
    assert "gbm_session_pair_scan" in _lib.EXPORTS
    assert set(_lib.PAIR_OPS) == set(ref.UNARY) | set(ref.BINARY)
    assert [_lib.PAIR_OPS[k] for k in ("mult", "addnorm", "raise", "square", "invoneplus", "log10epsdivlog10eps")] == list(range(6))
    assert gbm.raise_.__name__ == "raise" and gbm.mult.__name__ == "mult"
    for f in (gbm.square, gbm.invoneplus, gbm.log10epsdivlog10eps):
        assert tr.UNARY[f.__name__] is f
    for f in (gbm.mult, gbm.addnorm, gbm.raise_):
        assert tr.BINARY[f.__name__] is f


def test_named_functions_match_the_reference_formulas():
    x = np.array([0.0, 0.25, 0.5, 1.0])
    y = np.array([1.0, 0.5, 0.25, 0.0])
    assert np.array_equal(gbm.square(x), x ** 2)
    assert np.array_equal(gbm.invoneplus(x), 1 / (1 + x))
    assert np.array_equal(gbm.log10epsdivlog10eps(x), np.log10(x + EPS) / np.log10(EPS))
    assert gbm.log10epsdivlog10eps(np.array([0.0]))[0] == 1.0
    assert np.array_equal(gbm.mult(x, y), x * y)
    assert np.array_equal(gbm.addnorm(x, y), (x + y) / 2)
    assert np.array_equal(gbm.raise_(x + 0.5, y), (x + 0.5) ** y)
    for name in ref.UNARY + ref.BINARY:
        assert np.array_equal(ref.apply_op(name, x + 0.5, y + 0.5), tr.FUNCTIONS[name](*([y + 0.5] if name in ref.UNARY else [x + 0.5, y + 0.5])))


@pytest.mark.parametrize("op", ref.UNARY + ref.BINARY)
def test_the_three_references_agree(op):
    X, y = small()
    Xe = ref.work_matrix(X, EPS)
    loop = ref.slopes_lstsq(Xe, y, op)
    c64 = ref.closed_form(Xe, y, op)
    cld = ref.closed_form(Xe, y, op, dtype=np.longdouble)
    m = cld["mask"]
    assert m.sum() == (8 if op in ref.UNARY else 64)  # the constant column is out
    assert not loop[~m].any() and not c64["beta"][~m].any()
    assert cld["ratio"][m].min() > 1e4 * ref.DEGENERATE
    # both float64 forms within a generous multiple of the rounding scale of the long-double one
    for b in (loop, c64["beta"]):
        assert ref.error_ratio(b, cld).max() < 64.0
    assert np.allclose(np.asarray(cld["R"][m], dtype=np.float64), c64["R"][m], rtol=1e-9)


def test_commutative_mask_and_stable_topk():
    X, y = small()
    Xe = ref.work_matrix(X, EPS)
    m = ref.tested_mask(Xe, "mult", commutative=True)
    assert m.sum() == 8 * 9 // 2 and not m[3, 2] and m[2, 3] and m[2, 2]
    b = np.array([0.5, -2.0, 2.0, 0.0, 1e-20, -0.5])
    assert list(ref.stable_topk(b, 3, EPS)) == [1, 2, 0]
    assert list(ref.stable_topk(b, 6, EPS)) == [1, 2, 0, 5]  # zeros and |β| <= ε drop out after the cut
    with pytest.raises(IndexError):
        ref.stable_topk(b, 7, EPS)


def test_evaluate_feature_snaps_to_zero_and_one():
    x = np.array([0.0, 1.0, 0.5]) + 1e-3
    T = tr.evaluate_feature(gbm.addnorm, (x, x - 0.0006), 1e-3)
    assert T[0] == 0.0 and T[1] == 1.0 and T[2] == (x[2] + (x[2] - 0.0006)) / 2.0
    # strict comparisons, as the reference's: a value exactly ε away stays
    T = tr.evaluate_feature(gbm.addnorm, (np.array([1.0 + EPS]), np.array([1.0 + EPS])), EPS)
    assert T[0] == 1.0 + EPS


def test_parse_nested_names():
    known = {"chr1\t1\tA|T\tA": 0, "chr1\t2\tA|T\tA": 1}
    a, b = known
    assert tr.parse_feature_name(a, known) == a
    assert tr.parse_feature_name(f"square({a})", known) == ("square", [a])
    t = tr.parse_feature_name(f"raise(mult({a},{b}),log10epsdivlog10eps(addnorm({b},{a})))", known)
    assert t == ("raise", [("mult", [a, b]), ("log10epsdivlog10eps", [("addnorm", [b, a])])])
    for bad in (f"cube({a})", f"mult({a})", f"square({a},{b})", f"square({a}", f"square({a}))", "square(nowhere)",
                f"mult({a},{b}) "):
        with pytest.raises(gbm.ArgumentError):
            tr.parse_feature_name(bad, known)


def test_reconstitute_round_trip_on_nested_names():
    X, y = small()
    g, _ = genomes_of(X, y)
    a, b, c = g.loci_alleles[:3]
    eps = 1e-3
    Xe = X + eps
    lvl1 = tr.evaluate_feature(gbm.mult, (Xe[:, 0], Xe[:, 1]), eps)
    lvl2 = tr.evaluate_feature(gbm.invoneplus, (lvl1 + eps,), eps)
    lvl3 = tr.evaluate_feature(gbm.raise_, (lvl2 + eps, Xe[:, 2]), eps)
    names = [f"mult({a},{b})", f"invoneplus(mult({a},{b}))", f"raise(invoneplus(mult({a},{b})),{c})", c]
    out = gbm.reconstitutefeatures(g, names, eps=eps)
    assert out.loci_alleles == names and out.entries == g.entries
    assert np.array_equal(out.allele_frequencies, np.column_stack([lvl1, lvl2, lvl3, X[:, 2]]))
    # a Genomes that already holds a feature column hands it back as it is
    g2 = gbm.Genomes(entries=g.entries, populations=g.populations, loci_alleles=g.loci_alleles + names[:1],
                     allele_frequencies=np.column_stack([X, lvl1]))
    out2 = gbm.reconstitutefeatures(g2, names[:2], eps=eps)
    assert np.array_equal(out2.allele_frequencies, np.column_stack([lvl1, lvl2]))
    # use_abs: the absolute value after the shift, at every level
    Xn = np.array(X)
    Xn[:, 0] = -Xn[:, 0]
    gn = gbm.Genomes(entries=g.entries, populations=g.populations, loci_alleles=g.loci_alleles, allele_frequencies=Xn)
    outn = gbm.reconstitutefeatures(gn, [f"raise({a},{b})"], eps=eps, use_abs=True)
    assert np.array_equal(outn.allele_frequencies[:, 0],
                          tr.evaluate_feature(gbm.raise_, (np.abs(Xn[:, 0] + eps), np.abs(Xn[:, 1] + eps)), eps))


def test_reconstitute_rejects_ambiguous_locus_names():
    X, y = small()
    g, _ = genomes_of(X, y)
    for bad in ("chr1\t1\tA(T\tA", "chr1\t1\tA,T\tA", "cube(x)"):
        gb = gbm.Genomes(entries=g.entries, populations=g.populations, loci_alleles=[bad] + g.loci_alleles[1:],
                         allele_frequencies=g.allele_frequencies)
        with pytest.raises(gbm.ArgumentError, match="parenthesis or a comma"):
            gbm.reconstitutefeatures(gb, [g.loci_alleles[1]])
    with pytest.raises(gbm.ArgumentError):
        gbm.reconstitutefeatures(g, ["square(unknown)"])


def test_argument_errors_before_any_device_work():
    X, y = small()
    g, p = genomes_of(X, y)
    with pytest.raises(gbm.ArgumentError, match="not one of the named"):
        gbm.transform1(lambda x: x ** 2, g, p)
    with pytest.raises(gbm.ArgumentError, match="not one of the named"):
        gbm.transform2(lambda a, b: a * b, g, p)
    with pytest.raises(gbm.ArgumentError, match="not one of the named"):
        gbm.transform1(gbm.mult, g, p)  # a binary function where a unary one belongs
    with pytest.raises(gbm.ArgumentError, match="not one of the named"):
        gbm.transform2(np.multiply, g, p)
    with pytest.raises(gbm.ArgumentError, match="more than the 9 slopes"):
        gbm.transform1(gbm.square, g, p, n_new_features_per_transformation=10)
    with pytest.raises(gbm.ArgumentError, match="more than the 81 slopes"):
        gbm.transform2(gbm.mult, g, p, n_new_features_per_transformation=82)
    with pytest.raises(gbm.ArgumentError, match="out of bounds"):
        gbm.transform2(gbm.mult, g, p, idx_loci_alleles=[0, 1])
    with pytest.raises(gbm.ArgumentError, match="out of bounds"):
        gbm.epistasisfeatures(g, p, idx_entries=[1, 2, 99])
    with pytest.raises(gbm.ArgumentError, match="not one of the named"):
        gbm.epistasisfeatures(g, p, transformations1=[np.sqrt])
    bad = gbm.Genomes(entries=g.entries[:-1], populations=g.populations, loci_alleles=g.loci_alleles,
                      allele_frequencies=g.allele_frequencies)
    with pytest.raises(gbm.ArgumentError, match="corrupted"):
        gbm.epistasisfeatures(bad, p)
