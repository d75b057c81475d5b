"""What tests/test_gpu_ordinal_edges.py rests on, on the CPU (inputs and references: tests/ordinal_cases.py):
the restated Φ, Φ⁻¹ and TN of tests/ordinal_ref.py measured against mpmath, which sets the bounds the library is
held to; the library's own routines (the host compilation of csrc/gibbs_common.h, through
gbm_debug_ordinal_math with dev_out = NULL) within 4 times those figures of the same reference; the exact values
at p = 0, 1/2, 1, on intervals without mass and where pa + u (pb − pa) rounds to 0 or to 1; and the margin, gap,
identification and finiteness conditions of every edge fit's literal loop."""
import math

import numpy as np
import pytest

import gbm
from gbm import _lib

import ordinal_cases as oc
import ordinal_ref as ref

MARGIN = 1e-6  # tests/test_bayes_abc.py's: device rounding (~1e-12) cannot flip an indicator beyond it


def _ref_inv(values):
    return np.array([ref.ppnd16(float(p)) for p in values])


def _ref_tn(rows):
    return np.array([ref.truncnorm(*map(float, r)) for r in rows])


def test_mpmath_reference_solves_its_equations():
    """The reference itself: Φ of every Φ⁻¹ reference value gives p back to 1e-40 relative (the tail that holds
    the digits), and every exact TN draw lies in its interval; a sample of both against scipy to 1e-13."""
    from scipy.special import ndtri
    for p, z in zip(oc.inv_grid(), oc.inv_exact()):
        p = oc._mpf(float(p))
        back, want = (oc._upper(z), 1 - p) if p > 0.5 else (oc._lower(z), p)
        assert abs(back - want) <= want * oc._mpf(10) ** -40
    for row, x in zip(oc.tn_grid(), oc.tn_exact()):
        assert row[1] <= float(x) <= row[2]
    for i in range(0, len(oc.inv_grid()), 37):
        e = float(oc.inv_exact()[i])
        assert abs(float(ndtri(oc.inv_grid()[i])) - e) <= 1e-13 * max(abs(e), 1e-3)


def test_restatement_against_mpmath():
    """tests/ordinal_ref.py's phi, ppnd16 and truncnorm against the 50-digit reference. Measured:
      c_Φ   = 1.55: the worst relative error of Φ on 2000 points of [−37, 8.2] over (1 + x²)·2⁻⁵³;
      c_inv = 7.27e-16: the worst relative error of Φ⁻¹ on test_as241_agrees_with_scipy's grid (scipy: 7.5e-16);
      c_TN  = 1.14e-15: the worst |x − x*| / max(1, |x* − m|) over the admitted points of 12 intervals x 44 u
              (at (0; −1, 2), u → 1).
    The library is held to 4 times these, so they are capped where rounding analysis puts them: Φ's argument
    −x/√2 carries two roundings, which exp(−x²/2) turns into 2 x²·2⁻⁵³, plus erfc's own ulp: c_Φ <= 4; Φ⁻¹
    1e-15 (tests/test_bayes_ordinal.py's bound against scipy); TN on (0; −1, 2) at x = 2: p carries about 3·2⁻⁵³
    from pa and w, over the density 0.054 and |x| = 2 that is 28·2⁻⁵³ = 3.1e-15: c_TN <= 4e-15."""
    c_phi, c_inv, c_tn = oc.restatement_figures()
    print("c_phi %.4g c_inv %.4g c_tn %.4g" % (c_phi, c_inv, c_tn))
    assert c_phi <= 4.0 and c_inv <= 1e-15 and c_tn <= 4e-15
    excluded = [tuple(r) for r in oc.tn_grid() if not oc.admitted(*r)]
    assert {r[:3] for r in excluded} == {(37.0, -math.inf, 0.0)}  # exclusion 2 alone meets the grid
    assert not oc.admitted(0.0, -0.001, 30.0, 1 - 2.0 ** -53) and oc.admitted(0.0, -0.001, 30.0, 0.999)
    assert oc.admitted(0.0, 36.0, math.inf, 2.0 ** -54) and not oc.admitted(-38.0, 0.0, math.inf, 0.5)


def test_library_host_against_mpmath():
    """The host compilation of gibbs_phi, gibbs_ppnd16 and gibbs_truncnorm, pointwise within 4 x (c_Φ, c_inv,
    c_TN) of the mpmath reference on the same grids (4: the host differs from the restatement by the compiler's
    contraction at most, the device by its own erfc, log and sqrt, an ulp or two each; the cancellation in
    pa + u w is common to all), and every TN draw finite and in [a, b]. Measured: 1.55, 7.27e-16, 1.14e-15, the
    restatement's own figures (value for value the same numbers)."""
    host = [oc.library_math(what, grid) for what, grid in enumerate((oc.phi_grid(), oc.inv_grid(), oc.tn_grid()))]
    oc.check_math("host", *host)


@pytest.mark.parametrize("which", ["restatement", "library"])
def test_exact_values_and_the_window(which):
    """Φ⁻¹(0) = −∞, Φ⁻¹(1/2) = 0, Φ⁻¹(1) = +∞; (0; 40, 41) → 40, (0; −41, −40) → −40, (50; −∞, 0) → 0 at every u;
    and every draw finite and in [a, b] in the window TN(m; −∞, 0; u), m = 37.6, 38, 38.4 (Φ(−m) is subnormal and
    u Φ(−m) rounds to 0 at u = 2⁻⁵⁴), its mirror image, and around the mean where pa + u (pb − pa) rounds to 1.
    Before the guards the library returned NaN there (Φ⁻¹(0) = ∞/∞: NaN at m = 37.6, 38, 38.4 and their mirror
    images at u = 2⁻⁵⁴, and at (0.5 | 1 | 3; 0, +∞) at u = 1 − 2⁻⁵³; Φ⁻¹(0) and Φ⁻¹(1) themselves NaN), and the
    restatement −∞ / +∞."""
    inv, tn = (_ref_inv, _ref_tn) if which == "restatement" else (lambda v: oc.library_math(1, v),
                                                                   lambda r: oc.library_math(2, r))
    oc.check_exact_values(which, inv(oc.INV_POINTS), tn(oc.no_mass_grid()), tn(oc.window_grid()))


def test_edge_inputs_reach_what_they_are_for():
    """k32: 32 classes of ten, so the slots 62 and 63; k31_257: an odd K and a second chunk of one individual;
    sorted1100: every 256-individual chunk holds one or two classes; single257: class 2 is row 256 alone;
    n255 / n256: three classes, the last chunk one short / full; tiny3: K = n = 3; labels: n255's classes under
    other names."""
    def counts(name):
        return np.unique(oc.fit_case(name)[1], return_counts=True)
    for name, (n, p, _) in oc.SHAPES.items():
        X, cls = oc.fit_case(name)
        assert X.shape == (n, p) and cls.shape == (n,) and not X.flags.writeable and X.flags.f_contiguous
        assert n <= 1100 and p <= 130
    v, c = counts("k32")
    assert len(v) == 32 and set(c) == {10}
    v, c = counts("k31_257")
    assert len(v) == 31 and c.min() >= 8
    cls = oc.fit_case("sorted1100")[1]
    assert np.all(np.diff(cls) >= 0) and len(np.unique(cls)) == 5
    assert [len(np.unique(cls[i:i + 256])) for i in range(0, 1100, 256)] == [2, 2, 2, 2, 1]
    assert len(np.unique(cls[256:512])) < 5
    cls = oc.fit_case("single257")[1]
    assert list(counts("single257")[1]) == [128, 128, 1] and cls[256] == 2.0 and len(np.unique(cls[:256])) == 2
    assert list(counts("n255")[1]) == [85, 85, 85] and len(counts("n256")[0]) == 3
    assert list(oc.fit_case("tiny3")[1]) == [0.0, 1.0, 2.0] and list(oc.fit_case("tiny2")[1]) == [0.0, 1.0, 1.0]
    assert np.array_equal(counts("labels")[0], oc.LABELS)
    assert np.array_equal(np.searchsorted(oc.LABELS, oc.fit_case("labels")[1]), oc.fit_case("n255")[1])
    assert np.array_equal(oc.fit_case("labels")[0], oc.fit_case("n255")[0])


@pytest.mark.parametrize("name,model", oc.fit_cases())
def test_edge_fit_reference_conditions(name, model):
    """On every edge fit's literal loop no indicator draw is within 1e-6 of its threshold, every threshold is
    drawn from an interval of positive length (none with K = 2), t_1 never moves, the thresholds stay ordered,
    every output is finite and the probabilities' rows sum to 1. Measured: smallest margin 2.2e-4 (BayesB,
    `k31_257`), smallest gap 4.2e-4 (BayesB, `sorted1100`); each loop takes at most 0.1 s."""
    r = oc.fit_reference(name, model)
    K = len(r["classes"])
    print(name, model, "K", K, "margin", r["margin"], "gap", r["gap"])
    assert model == "BayesA" or r["margin"] > MARGIN
    assert r["gap"] > 0.0 and (r["gap"] == math.inf) == (K == 2)
    assert r["t_end"][1] == r["t_start"][1]
    assert all(a < b for a, b in zip(r["t_end"], r["t_end"][1:]))
    assert abs(r["thresholds"][0] - r["t_start"][1]) <= 1e-15 * max(1.0, abs(r["t_start"][1]))
    for k in oc.FIT_NAMES:
        assert np.all(np.isfinite(r[k])), k
    assert r["probs"].shape == (oc.SHAPES[name][0], K) and np.abs(r["probs"].sum(axis=1) - 1.0).max() < 1e-12
    assert r["var"][0] == 1.0
    if name == "labels":
        same = oc.fit_reference("n255", model)
        assert np.array_equal(r["classes"], oc.LABELS)
        assert all(np.array_equal(r[k], same[k]) for k in oc.FIT_NAMES if k != "classes")


def test_debug_ordinal_math_arguments():
    """gbm_debug_ordinal_math refuses NULL in or host_out, m < 1, m > 2^20 and an unknown `what`; with
    dev_out = NULL it touches no device."""
    lib = gbm.load_library()
    E = _lib.GBM_E_ARG
    assert "gbm_debug_ordinal_math" in _lib.EXPORTS
    x, out = np.array([0.25, 0.5, 0.75, 0.9]), np.zeros(4)
    assert lib.gbm_debug_ordinal_math(0, None, 4, 0, _lib.ptr(out), None) == E
    assert "gbm_debug_ordinal_math" in _lib.last_error()
    assert lib.gbm_debug_ordinal_math(0, _lib.ptr(x), 4, 0, None, None) == E
    assert lib.gbm_debug_ordinal_math(0, _lib.ptr(x), 0, 0, _lib.ptr(out), None) == E
    assert lib.gbm_debug_ordinal_math(0, _lib.ptr(x), -1, 0, _lib.ptr(out), None) == E
    assert lib.gbm_debug_ordinal_math(0, _lib.ptr(x), (1 << 20) + 1, 0, _lib.ptr(out), None) == E
    for what in (-1, 3):
        assert lib.gbm_debug_ordinal_math(what, _lib.ptr(x), 4, 0, _lib.ptr(out), None) == E
    assert not out.any()
    big = np.full(1 << 20, 0.5)
    assert np.array_equal(oc.library_math(1, big), np.zeros(1 << 20))  # the largest m
    assert abs(oc.library_math(2, x)[0] - ref.truncnorm(*x)) < 1e-15  # one TN item of four values
    assert lib.gbm_debug_ordinal_math(0, _lib.ptr(x), 4, 0, _lib.ptr(out), None) == 0
    assert np.abs(out - [ref.phi(float(v)) for v in x]).max() < 1e-15
