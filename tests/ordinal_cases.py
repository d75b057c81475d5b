"""Inputs and cached references of the ordinal sampler's second pass (tests/test_ordinal_cases.py on the CPU,
tests/test_gpu_ordinal_edges.py on the device).

Math: grids for Φ, Φ⁻¹ and TN(m; a, b; u) of csrc/gibbs_common.h with an mpmath reference at 50 digits. Φ is
erfc(−x/√2)/2; an interval's masses are taken from the upper tail (erfc of the positive argument) when it lies
above its mean, so nothing is ever formed as 1 − (a number near 1); the exact draw x* solves
Φ(x* − m) = pa + u′(pb − pa) by Newton (u′ = 1 − u for an interval the routine reflects). The routine's error is
|x − x*| / max(1, |x* − m|). Two sets of points are left out of that error bound and out of nothing else (the
interval and finiteness checks take every point); both are inherent to an inverse CDF from one 53-bit uniform:
  1. an interval that straddles its mean with b − m > 8, at u > 0.999: p = pa + u (pb − pa) is then within 1e-3 of
     pb, which is 1 to fp64, so 1 − p has few or no digits left ((0; −0.001, 30) errs by 2e-2 at u = 1 − 2⁻⁵³;
     the intervals of this kind are P_ONE below, held to finiteness and the interval at every u);
  2. a working interval (after the reflection) whose upper end β has |β| >= 37: p = u Φ(β) is then subnormal for
     the smallest u, with as many bits fewer ((37; −∞, 0) errs by 5e-12 at u = 2⁻⁵⁴).

Fits: the edge cases of ordinal_latent_kernel and ordinal_threshold_kernel (K = 32 and an odd K, chunks without
a class, a class of one, n = 255 / 256 / 257, n = 3, class labels that are not 0 … K − 1), each with the literal
loop of tests/ordinal_ref.py as its reference. Every array is built once and is read-only. Not a test module."""
import functools
import math

import mpmath
import numpy as np

import ordinal_ref as ref
from bayes_abc_ref import path_case

INF = math.inf
SEED = 99  # of every fit
MODELS = ("BayesA", "BayesB", "BayesC")
EPS = 2.0 ** -53  # the unit roundoff
BOUND = 4.0  # the library (host and device) against mpmath: this many times the restatement's own figure
_mp = mpmath.mp.clone()
_mp.dps = 50

# ---- the grids -----------------------------------------------------------------------------------
US = tuple(np.linspace(0.001, 0.999, 41)) + (2.0 ** -54, 2.0 ** -20, 1.0 - 2.0 ** -53)
# tests/test_bayes_ordinal.py's intervals with mass (one of them, (0; 9, 9.5), of mass 1e-19), then far and
# half-open ones
TN_INTERVALS = ((0.0, -1.0, 2.0), (0.3, 1.0, 2.5), (0.3, -2.5, -1.0), (1.0, -INF, 0.0), (-1.0, 0.5, INF), (0.0, 9.0, 9.5),
                (0.0, 30.0, 30.001), (12.0, -INF, 0.0), (-20.0, 0.5, INF), (5.0, -INF, 5.0), (37.0, -INF, 0.0),
                (0.0, 36.0, INF))
NO_MASS = (((0.0, 40.0, 41.0), 40.0), ((0.0, -41.0, -40.0), -40.0), ((50.0, -INF, 0.0), 0.0))
# Φ(β) is subnormal, so u Φ(β) underflows to 0 for the smallest u, and the mirror image
WINDOW = tuple((m, -INF, 0.0) for m in (37.6, 38.0, 38.4)) + tuple((-m, 0.0, INF) for m in (37.6, 38.0, 38.4))
# The other end, p → 1, around the mean: clamped at a finite b, and half-open classes, where pa + u (1 − pa)
# rounds to 1 at the largest u (any individual of the top class above its threshold can meet it). Finiteness and
# the interval only: at u >= 0.999 these are exclusion 1's points, and their errors below it (1e-14: 1 − p = 5e-4
# carries p's rounding) would only widen the figure the other intervals are held to.
P_ONE = ((0.0, -0.001, 30.0), (0.5, 0.0, INF), (1.0, 0.0, INF), (3.0, 0.0, INF))


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def phi_grid():
    return _ro(np.linspace(-37.0, 8.2, 2000))


@functools.lru_cache(maxsize=None)
def inv_grid():
    """The grid of tests/test_bayes_ordinal.py::test_as241_agrees_with_scipy."""
    return _ro(np.concatenate([10.0 ** -np.arange(1.0, 301.0), np.linspace(0.001, 0.999, 1999),
                               1.0 - 10.0 ** -np.arange(1.0, 17.0), [0.075, 0.925, 0.0749999, 0.9250001]]))


def _rows(intervals):
    return _ro([(m, a, b, u) for m, a, b in intervals for u in US])


@functools.lru_cache(maxsize=None)
def tn_grid():
    return _rows(TN_INTERVALS)


@functools.lru_cache(maxsize=None)
def window_grid():
    return _rows(WINDOW + P_ONE)


def admitted(m, a, b, u):
    """Does the error bound apply to this point? (The module's two exclusions.)"""
    al, be = a - m, b - m
    if al < 0.0 < be and be > 8.0 and u > 0.999:
        return False
    if al >= 0.0:
        al, be = -be, -al
    return abs(be) < 37.0


# ---- the mpmath reference --------------------------------------------------------------------------
def _mpf(x):
    return _mp.mpf(x)  # exact: every fp64 value, ±inf included


def _upper(x):
    """1 − Φ(x) at 50 digits with full relative precision for x >= 0."""
    return _mp.erfc(x / _mp.sqrt(2)) / 2


def _lower(x):
    return _mp.erfc(-x / _mp.sqrt(2)) / 2


def _solve(p, upper, start):
    """z with Φ(z) = p (upper: 1 − Φ(z) = p) by Newton on the logarithm, from a fp64 start."""
    z, logp = _mpf(start), _mp.log(p)
    tail = _upper if upper else _lower
    for _ in range(100):
        t = tail(z)
        dens = _mp.exp(-z * z / 2) / _mp.sqrt(2 * _mp.pi)
        step = (_mp.log(t) - logp) * t / dens
        z = z + step if upper else z - step
        if abs(step) <= _mp.mpf(10) ** -42 * max(1, abs(z)):
            return z
    raise ArithmeticError(f"no convergence for p = {p}")


@functools.lru_cache(maxsize=None)
def phi_exact():
    return tuple(_lower(_mpf(float(x))) for x in phi_grid())


@functools.lru_cache(maxsize=None)
def inv_exact():
    out = []
    for p in inv_grid():
        p = float(p)
        if p > 0.5:
            out.append(_solve(1 - _mpf(p), True, -ref.ppnd16(1.0 - p)))
        else:
            out.append(_solve(_mpf(p), False, ref.ppnd16(p)))
    return tuple(out)


def tn_exact_one(m, a, b, u):
    """The exact draw x* of TN(m; a, b; u) for the fp64 values m, a, b, u."""
    M, al, be = _mpf(m), _mpf(a) - _mpf(m), _mpf(b) - _mpf(m)
    up = _mpf(u) if al < 0 else 1 - _mpf(u)
    if al >= 0:  # above the mean: upper-tail masses, 1 − Φ(z) = qa − u′ (qa − qb)
        qa, qb = _upper(al), _upper(be)
        q = qa - up * (qa - qb)
        start = -ref.ppnd16(float(q)) if q > _mp.mpf(10) ** -300 else float(al)
        z = _solve(q, True, start)
    else:
        pa, pb = _lower(al), _lower(be)
        p = pa + up * (pb - pa)
        if p > 0.5:  # 1 − p without forming it from p
            q = _upper(be) + (1 - up) * (pb - pa)
            start = -ref.ppnd16(float(q)) if q > _mp.mpf(10) ** -300 else float(min(be, 38.0))
            z = _solve(q, True, start)
        else:
            start = ref.ppnd16(float(p)) if p > _mp.mpf(10) ** -300 else float(be)
            z = _solve(p, False, start)
    return M + z


@functools.lru_cache(maxsize=None)
def tn_exact():
    return tuple(tn_exact_one(*map(float, row)) for row in tn_grid())


# ---- the figures: errors against mpmath, normalised ----------------------------------------------------
def phi_figures(values):
    """Per point: the relative error of Φ over (1 + x²)·2⁻⁵³ (the condition number of exp(−x²/2) times the unit
    roundoff)."""
    out = np.empty(len(values))
    for i, (x, v, e) in enumerate(zip(phi_grid(), values, phi_exact())):
        out[i] = float(abs(_mpf(float(v)) - e) / e) / ((1.0 + x * x) * EPS)
    return out


def inv_figures(values):
    """Per point: the relative error of Φ⁻¹ (absolute where the exact value is 0)."""
    out = np.empty(len(values))
    for i, (v, e) in enumerate(zip(values, inv_exact())):
        out[i] = float(abs(_mpf(float(v)) - e) / (abs(e) if e != 0 else 1))
    return out


def tn_figures(values):
    """Per point: |x − x*| / max(1, |x* − m|), NaN where the error bound does not apply (``admitted``)."""
    out = np.full(len(values), np.nan)
    for i, (row, v, e) in enumerate(zip(tn_grid(), values, tn_exact())):
        if admitted(*row):
            out[i] = float(abs(_mpf(float(v)) - e) / max(1, abs(e - _mpf(float(row[0])))))
    return out


@functools.lru_cache(maxsize=None)
def restatement_figures():
    """(c_Φ, c_inv, c_TN) of tests/ordinal_ref.py's phi, ppnd16 and truncnorm: the worst figure of each grid."""
    c_phi = phi_figures([ref.phi(float(x)) for x in phi_grid()]).max()
    c_inv = inv_figures([ref.ppnd16(float(p)) for p in inv_grid()]).max()
    c_tn = np.nanmax(tn_figures([ref.truncnorm(*map(float, row)) for row in tn_grid()]))
    return float(c_phi), float(c_inv), float(c_tn)


def library_math(what, values, device=False):
    """gbm_debug_ordinal_math on ``values`` (what 2: rows of (m, a, b, u)): the host half, or with ``device``
    (host, device)."""
    import gbm
    from gbm import _lib
    a = np.ascontiguousarray(values, dtype=np.float64)
    m = a.size // (4 if what == 2 else 1)
    host, dev = np.full(m, np.nan), np.full(m, np.nan) if device else None
    _lib.check(gbm.load_library().gbm_debug_ordinal_math(what, _lib.ptr(a), m, 0, _lib.ptr(host), _lib.ptr(dev)),
               "gbm_debug_ordinal_math")
    return (host, dev) if device else host


def check_math(label, phi_values, inv_values, tn_values):
    """The assertions shared by the host and the device: every point within BOUND times the restatement's figure
    of the mpmath reference, normalised as that figure is; every TN draw finite and in its interval. Returns the
    three worst figures (printed first)."""
    c_phi, c_inv, c_tn = restatement_figures()
    f_phi, f_inv, f_tn = phi_figures(phi_values), inv_figures(inv_values), tn_figures(tn_values)
    worst = (float(f_phi.max()), float(f_inv.max()), float(np.nanmax(f_tn)))
    print(label, "c_phi %.3g c_inv %.3g c_tn %.3g" % worst, "restatement: %.3g %.3g %.3g" % (c_phi, c_inv, c_tn))
    grid = tn_grid()
    assert np.all(np.isfinite(tn_values)), label
    assert np.all((grid[:, 1] <= tn_values) & (tn_values <= grid[:, 2])), label
    assert f_phi.max() <= BOUND * c_phi, (label, "phi", float(phi_grid()[f_phi.argmax()]), worst[0])
    assert f_inv.max() <= BOUND * c_inv, (label, "inv", float(inv_grid()[f_inv.argmax()]), worst[1])
    assert worst[2] <= BOUND * c_tn, (label, "tn", tuple(grid[np.nanargmax(f_tn)]), worst[2])
    return worst


INV_POINTS = (0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def no_mass_grid():
    return _rows([iv for iv, _ in NO_MASS])


def check_exact_values(label, inv_values, no_mass_values, window_values):
    """Φ⁻¹ on INV_POINTS is −∞, 0, +∞; the draws on no_mass_grid() are the end nearer the mean at every u; the
    draws on window_grid() (the window and the p → 1 intervals) are all finite and in [a, b]."""
    v = np.asarray(inv_values)
    assert v[0] == -INF and v[1] == 0.0 and v[2] == INF, (label, v)
    assert np.array_equal(no_mass_values, np.repeat([end for _, end in NO_MASS], len(US))), label
    w, got = window_grid(), np.asarray(window_values)
    bad = ~(np.isfinite(got) & (w[:, 1] <= got) & (got <= w[:, 2]))
    assert not bad.any(), (label, [(tuple(r), g) for r, g in zip(w[bad], got[bad])][:6])


def rel(a, b):
    """tests/test_bayes_ordinal.py's: the largest difference relative to the largest reference value; absolute
    where the reference is all zero."""
    scale = np.abs(np.asarray(b)).max()
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (scale if scale > 0.0 else 1.0)


# ---- the edge fits -----------------------------------------------------------------------------------
# name -> (n, p, iters); the schedule of every fit is (iters, 2, 1)
SHAPES = {"k32": (320, 64, 5), "k31_257": (257, 130, 5), "sorted1100": (1100, 129, 5), "single257": (257, 130, 6),
          "n255": (255, 130, 5), "n256": (256, 130, 5), "tiny3": (3, 1, 6), "tiny2": (3, 1, 6), "labels": (255, 130, 5)}
B_ONLY = ("n255", "n256", "labels")
LABELS = (-2.5, 0.0, 1e6)  # in place of 0, 1, 2
FIT_NAMES = ("b_hat", "y_pred", "var", "pip", "classes", "thresholds", "probs")


def models_of(name):
    return ("BayesB",) if name in B_ONLY else MODELS


def fit_cases():
    return [(name, model) for name in SHAPES for model in models_of(name)]


def _equal_classes(y, K):
    """Cut at the k/K quantiles of y."""
    return np.searchsorted(np.quantile(y, np.arange(1, K) / K), y).astype(np.float64)


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """(X, classes) of a named fit, read-only."""
    n, p, _ = SHAPES[name]
    if name in ("tiny3", "tiny2"):
        X = np.array([[0.0], [0.5], [1.0]])
        cls = np.array([0.0, 1.0, 2.0] if name == "tiny3" else [0.0, 1.0, 1.0])
    else:
        X, y = path_case(n, p)
        if name == "k32":
            cls = _equal_classes(y, 32)
        elif name == "k31_257":
            cls = _equal_classes(y, 31)
        elif name == "sorted1100":  # tests/ordinal_ref.py's K = 5 cut, the rows stably sorted by class
            cls = ref.ordinal_case(n, p, 5)[1]
            order = np.argsort(cls, kind="stable")
            X, cls = X[order], cls[order]
        elif name == "single257":  # rows sorted by y: 128, 128 and 1 of them
            X = X[np.argsort(y, kind="stable")]
            cls = np.repeat([0.0, 1.0, 2.0], [128, 128, 1])
        elif name in ("n255", "n256"):
            cls = _equal_classes(y, 3)
        elif name == "labels":
            cls = np.array(LABELS)[fit_case("n255")[1].astype(int)]
        else:
            raise KeyError(name)
    X = np.asfortranarray(X, dtype=np.float64)
    X.setflags(write=False)
    cls.setflags(write=False)
    return X, cls


@functools.lru_cache(maxsize=None)
def fit_reference(name, model):
    X, cls = fit_case(name)
    r = ref.ordinal_gibbs(model, X, cls, n_iter=SHAPES[name][2], n_burnin=2, thin=1, seed=SEED)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def device_fit(name, model, **kw):
    import gbm
    X, cls = fit_case(name)
    return gbm.bayes_ordinal_arrays(model, X, cls, n_iter=SHAPES[name][2], n_burnin=2, thin=1, seed=SEED, **kw)
