"""The conditions that tests/test_gpu_factor_readers.py and tests/test_gpu_gwas_edges.py rest on,
asserted on the references alone (tests/gwas_cases.py): the literal per-marker ``pinv`` forms and the
long-double Schur route agree far below the device bound of 1e-9, no tested locus is near the kernel's
drop threshold, the tested counts are the ones the device tests expect, and the two ways of writing
R·U⁻¹ agree at the whitening tests' size."""
import numpy as np
import pytest

import gwas_cases as gc
from test_gpu_gwas import ref_scan

AGREE = 1e-12  # the ordinary cases: three orders under the device bound
AGREE_MINIMUM = 1e-10  # n_train = kc + 3, where s_j/d_j falls to 1e-4: one order under it
RATIO_MIN = 1e-9  # the kernel drops a locus at s_j <= 1e-12 d_j
RATIO_SPAN = 1e-14


def test_inputs_are_what_the_device_tests_need():
    X, y = gc.data("fixture")
    assert X.shape == (333, 1777) and np.array_equal(X * 2, gc.dosage_i8()) and not X.flags.writeable
    assert gc.data("n1100")[0].shape == (1100, 200)  # npad 1152: 18 column blocks, the first size with a 16-panel group
    assert gc.data("p130")[0].shape == (64, 130) and gc.data("tiny")[0].shape == (12, 400)
    X, _ = gc.data("long")
    assert X.shape == (40, 33000) and min(gc.FLAT) < 32768 <= max(gc.FLAT)
    assert not X[:, list(gc.FLAT)].std(axis=0).any()
    assert sorted({gc.CASES[k].kc for k in gc.CASES if k.startswith("fix-kc")}) == [3, 4, 5, 6, 7]
    for name, c in gc.CASES.items():
        idx, Xt, yt, C = gc.inputs(name)
        assert Xt.shape[0] == yt.size == idx.size == (c.n_train or gc.data(c.data)[0].shape[0])
        assert np.all(np.diff(idx) > 0) and (C is None) == (c.kc == 0) and idx.size >= c.kc + 3
        assert C is None or (C.shape == (idx.size, c.kc) and C.flags.f_contiguous)
    assert [gc.CASES[k].n_train for k in gc.MINIMUM] == [10, 10] and all(gc.CASES[k].kc == 7 for k in gc.MINIMUM)
    assert sorted(gc.CASES[k].n_train % 4 for k in gc.CASES if k.startswith("fix-n") and k.endswith("mlm")) == [1, 2, 3]


@pytest.mark.parametrize("name", [k for k, c in gc.CASES.items() if c.literal])
def test_the_two_references_agree(name):
    """z and b of the literal forms (float64) against the long-double Schur route, relative to their
    maxima. Measured: at most 4.3e-15 for the ordinary cases at λ = 0.571 and OLS, 1.1e-14 at λ = 1e-3
    (`fix-kc7-small`), 5.1e-14 at n_train = 12 with kc = 7, and 5.2e-13 at the API minimum n_train = 10
    with kc = 7 (`tiny-n10-kc7-ols`, b)."""
    zl, bl, kl = gc.literal(name)
    z, b, keep, _ = gc.schur(name)
    assert np.array_equal(kl, keep)
    m = gc.compared(name)
    dz, db = gc.rel(zl[m], z[m]), gc.rel(bl[m], b[m])
    print(f"{name}: literal against long double: z {dz:.2e} b {db:.2e}")
    bound = AGREE_MINIMUM if name in gc.MINIMUM else AGREE
    assert dz <= bound and db <= bound
    assert np.all(z[~keep] == 0.0) and np.all(zl[~keep] == 0.0)


def test_the_two_references_agree_on_the_33000_locus_session():
    """The per-marker loop over 33 000 loci is too slow for every run, and OLS statistics of a locus do
    not depend on the other loci: the literal forms on the 464 columns around index 32 768 (the flat loci
    32 760 and 32 775 among them) against the same columns of the vectorised route. The mixed model at
    this size rests on the agreement of the two routes at every other shape. Measured: 5.4e-15."""
    _, X, y, C = gc.inputs("long-ols")
    cols = np.arange(32768 - 232, 33000)
    zl, bl, kl = ref_scan(X[:, cols], y, C)
    z, b, keep, _ = gc.schur("long-ols")
    assert np.array_equal(kl, keep[cols]) and keep[32767] and keep[32768] and not keep[[32760, 32775]].any()
    dz, db = gc.rel(zl, z[cols]), gc.rel(bl, b[cols])
    print(f"long-ols, 464 columns: literal against long double: z {dz:.2e} b {db:.2e}")
    assert dz <= AGREE and db <= AGREE
    for name in ("long-ols", "long-mlm"):
        z, b, keep, _ = gc.schur(name)
        assert not keep[list(gc.FLAT)].any() and not z[list(gc.FLAT)].any() and not b[list(gc.FLAT)].any()
        assert np.isfinite(z).all() and np.abs(z[keep]).min() > 0


@pytest.mark.parametrize("name", list(gc.CASES))
def test_drop_margin_and_tested_count(name):
    """The smallest s_j/d_j over the compared loci is above 1e-9: three orders above the 1e-12 at which
    the kernel drops a locus, so rounding decides no locus' fate. A locus placed in the covariates' span
    sits below 1e-14. Measured: the smallest ratio is 5.6e-4 (`tiny-n10-kc7-ols`), 5.8e-3 at n_train = 12,
    at least 0.55 elsewhere; the span locus of `fix-span2` is at 8.5e-33."""
    _, _, keep, ratio = gc.schur(name)
    m = gc.compared(name)
    print(f"{name}: tested {int(m.sum())}, smallest s/d {ratio[m].min():.2e}")
    assert ratio[m].min() > RATIO_MIN
    assert int(m.sum()) == gc.CASES[name].tested
    span = keep & ~m
    assert int(span.sum()) == len(gc.SPAN.get(name, ()))
    if span.any():
        print(f"{name}: span locus s/d {ratio[span].max():.2e}")
        assert ratio[span].max() < RATIO_SPAN


def test_whitening_reference_forms_agree():
    """R·inv(U) (what the device is compared with, bound 1e-10) against the triangular solve of Uᵀ at
    n = 1100, 129 rows. Measured: 1.3e-15 of the largest entry."""
    R, U = gc.whitening()
    ref = gc.whitening_ref()
    assert R.shape == (129, 1100) and U.shape == (1100, 1100) and not np.tril(U, -1).any()
    err = gc.rel(np.linalg.solve(U.T, R.T).T, ref)
    print(f"whitening reference: inverse against solve {err:.2e}")
    assert err <= 1e-12
