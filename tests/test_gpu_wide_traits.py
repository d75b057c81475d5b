"""More than three traits per call, up to the ABI's limit of 63 (include/gbm.h: 1 <= nrhs <= 63; the bordered
Cholesky has room for 1 + 63 right-hand sides). Everything that blocks traits in fours runs past its first,
partial block here: the marker-effects kernels (fp64 rows and int8 rows), the back substitution, whose every
4-trait pass has its own flag hand-off between workgroups, and the predict kernel.

Phenotypes are oracle.synth_phenotypes(X, seed, ntraits = t): every trait has its own QTL and noise, so a
swapped or repeated column inside a block of four fails, and every trait column is checked on its own. The
generator draws trait after trait, so the t-trait phenotypes are the first t columns of the 63-trait ones and one
oracle fit per shape serves every nrhs.

Also here: the nrhs argument checks, and pooled fit contexts reused across shapes (a small fit in buffers a
larger one left behind gives the bits of a fresh context)."""
import ctypes

import numpy as np
import pytest

import oracle

import abi_direct as abi
from abi_direct import Mat, rel
from gbm import _lib

pytestmark = pytest.mark.gpu

TOL_CONTRACT = 1e-6
TOL_TIGHT = 1e-9
TMAX = 63
LAM = 0.8
# (200, 600): two 64-row blocks. (1030, 700): ragged, npad = 1152 = 18 back-substitution blocks (9 workgroups), so
# every 4-trait pass crosses workgroups
SHAPES = {"small": (200, 600, 301), "ragged": (1030, 700, 302)}


class Case:
    def __init__(self, n, p, seed):
        self.n, self.p, self.seed = n, p, seed
        self.X = oracle.synth_genotypes(seed, n, p)
        self.Y = oracle.synth_phenotypes(self.X, seed + 1, ntraits=TMAX)
        assert self.Y.var(axis=0, ddof=1).min() > 1e-6
        assert np.abs(np.corrcoef(self.Y.T) - np.eye(TMAX)).max() < 0.9  # no two traits alike
        self.ref = oracle.gblup_fit(self.X, self.Y, LAM)

    def phenotypes(self, t):
        Y = oracle.synth_phenotypes(self.X, self.seed + 1, ntraits=t)
        assert np.array_equal(Y, self.Y[:, :t])
        return Y


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(*SHAPES[name])
        return made[name]

    return get


def check_fit(fit, X, ref, t):
    """q, mu, and per trait column: GEBVs, b_hat and the predict identity b0 + X b == y_pred."""
    b, y, mu, q = fit[:4]
    assert q == ref["q"]
    assert b.shape[1] == y.shape[1] == t
    assert rel(mu, ref["mu"][:t]) < TOL_TIGHT
    pred = oracle.predict_linear(X, b)
    for k in range(t):
        assert rel(y[:, k], ref["y_pred"][:, k]) < TOL_TIGHT, k
        assert rel(b[:, k], ref["b_hat"][:, k]) < TOL_CONTRACT, k
        assert rel(pred[:, k], y[:, k]) < TOL_TIGHT, k


@pytest.mark.parametrize("t", [4, 5, 8, 63])
@pytest.mark.parametrize("chol", ["dataflow", "panels"])
@pytest.mark.parametrize("grm", ["fp64", "exact"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gblup_fit_wide_matches_oracle(gbm_env, cases, shape, grm, chol, t):
    """grm fp64: the fp64-row marker-effects kernel; exact: the int8-row one (stream_effects_shard).
    panels: GBM_CHOL_FLOW_MAX = 0, the launch-per-panel factorisation instead of the dataflow one."""
    if chol == "panels":
        gbm_env.setenv("GBM_CHOL_FLOW_MAX", "0")
    c = cases(shape)
    fit = abi.gblup_fit_ex(Mat(c.X), Mat(c.phenotypes(t)), LAM, grm)
    assert fit[4] == abi.MODES[grm]
    check_fit(fit, c.X, c.ref, t)


@pytest.mark.parametrize("t", [5, 63])
@pytest.mark.parametrize("grm", ["fp64", "exact"])
def test_gblup_fit_wide_two_shards(cases, grm, t):
    """devices = [0, 0]: the second shard takes a copy of all nrhs x npad of A from the first."""
    c = cases("ragged")
    fit = abi.gblup_fit_ex(Mat(c.X), Mat(c.phenotypes(t)), LAM, grm, devices=[0, 0])
    check_fit(fit, c.X, c.ref, t)


@pytest.fixture(scope="module")
def subset(cases):
    """700 of the ragged shape's 1030 rows and the oracle's 63-trait fit of them."""
    c = cases("ragged")
    train = np.sort(np.random.default_rng(9).choice(c.n, size=700, replace=False))
    return train, c.X[train], c.Y[train], oracle.gblup_fit(c.X[train], c.Y[train], LAM)


@pytest.mark.parametrize("t", [7, 63])
def test_session_fit_wide_on_row_subset(cases, subset, t):
    train, Xs, Ys, ref = subset
    with abi.Session(Mat(cases("ragged").X)) as s:
        fit = s.fit(train, Mat(Ys[:, :t]), LAM)
    check_fit(fit, Xs, ref, t)


@pytest.mark.parametrize("t,bpad", [(1, 0), (4, 0), (5, 3), (9, 0)])
def test_predict_wide(cases, t, bpad):
    """gbm_predict and gbm_session_predict, whose kernel takes the traits four at a time; once with ldb > p + 1."""
    c = cases("small")
    B = np.random.default_rng(40 + t).standard_normal((c.p + 1, t))
    ref = oracle.predict_linear(c.X, B)
    out = abi.predict(Mat(c.X), Mat(B, bpad))
    val = np.sort(np.random.default_rng(41).choice(c.n, size=77, replace=False))
    with abi.Session(Mat(c.X)) as s:
        outs = s.predict(val, Mat(B, bpad))
    for k in range(t):
        assert rel(out[:, k], ref[:, k]) < TOL_TIGHT, k
        assert rel(outs[:, k], ref[val, k]) < TOL_TIGHT, k


def test_reml_fit_wide_equals_single_trait_calls(cases):
    """gbm_gblup_fit_reml_ex solves trait by trait, so five traits in one call are five one-trait calls."""
    c = cases("small")
    t = 5
    Y = c.phenotypes(t)
    b, y, mu, q, lam, s2e, s2u = abi.reml_fit_ex(Mat(c.X), Mat(Y), "fp64")
    for k in range(t):
        b1, y1, mu1, q1, lam1, s2e1, s2u1 = abi.reml_fit_ex(Mat(c.X), Mat(Y[:, k]), "fp64")
        assert q1 == q and lam1[0] == lam[k] and s2e1[0] == s2e[k] and s2u1[0] == s2u[k]
        assert np.array_equal(b1[:, 0], b[:, k]) and np.array_equal(y1[:, 0], y[:, k]) and mu1[0] == mu[k]
        ref = oracle.gblup_fit(c.X, Y[:, k], float(lam[k]))
        assert rel(y[:, k], ref["y_pred"][:, 0]) < TOL_TIGHT and rel(b[:, k], ref["b_hat"][:, 0]) < TOL_CONTRACT


def _refused(rc):
    assert rc == _lib.GBM_E_ARG
    assert _lib.last_error() != ""


@pytest.mark.parametrize("bad", [0, 64])
def test_nrhs_outside_the_limit_is_refused(cases, bad):
    """Argument checks that return before any launch: the host fit, the session fit and, at device level, the
    solve and its prepare phase. Each leaves a message, and a valid fit afterwards still succeeds."""
    import torch

    c = cases("small")
    n, t = c.n, 3
    Y64 = Mat(np.hstack([c.Y, c.Y[:, :1]]))  # 64 readable columns, whatever nrhs says

    def valid_fit():
        check_fit(abi.gblup_fit_ex(Mat(c.X), Mat(c.Y[:, :t]), LAM, "fp64"), c.X, c.ref, t)

    _refused(abi.gblup_fit_ex(Mat(c.X), Y64, LAM, "fp64", nrhs=bad, raw=True))
    valid_fit()
    with abi.Session(Mat(c.X)) as s:
        idx = np.arange(n)
        _refused(s.fit(idx, Y64, LAM, nrhs=bad, raw=True))
        check_fit(s.fit(idx, Mat(c.Y[:, :t]), LAM), c.X, c.ref, t)

    lib = _lib.load()
    npad, gdim = lib.gbm_dev_npad(n), lib.gbm_dev_gdim(n)
    dev = dict(dtype=torch.float64, device="cuda")
    G = torch.eye(gdim, **dev)
    Yd, A, gebv, mu = torch.zeros((64, npad), **dev), torch.zeros((64, npad), **dev), torch.zeros((64, npad), **dev), torch.zeros(64, **dev)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    wsb = lib.gbm_dev_solve_workspace(n, 63)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    p_ = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _refused(lib.gbm_dev_gblup_solve(p_(G), gdim, n, 1.0, None, LAM, p_(Yd), npad, bad, p_(A), p_(gebv), npad, p_(mu),
                                     p_(info), p_(ws), wsb, stream))
    valid_fit()
    _refused(lib.gbm_dev_chol_prepare(p_(G), gdim, n, 1.0, None, LAM, p_(Yd), npad, bad, p_(info), p_(ws), wsb, stream))
    valid_fit()
    torch.cuda.synchronize()
    assert torch.equal(G, torch.eye(gdim, **dev)) and int(info.item()) == 0  # nothing was launched


def test_63_trait_fit_is_bit_identical_over_repeats(cases):
    """16 passes of the back substitution, each handing a between workgroups through its own flag value: a stale
    flag or a visibility race between passes would show as run-to-run differences."""
    c = cases("ragged")
    X, Y = Mat(c.X), Mat(c.Y)
    first = abi.gblup_fit_ex(X, Y, LAM, "fp64")
    check_fit(first, c.X, c.ref, TMAX)
    for _ in range(4):
        again = abi.gblup_fit_ex(X, Y, LAM, "fp64")
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], first[:3]))


@pytest.mark.parametrize("grm", ["fp64", "exact"])
def test_pooled_context_reuse_gives_fresh_context_bits(grm):
    """Pooled fit contexts only grow. On one thread (one context, reused by every call): a large fit, a small one
    in its buffers, a wide one (other n, npad and nrhs), the small and the large one again; then every shape
    once in a fresh pool. Stale padding of Y, A, G beyond npad or B would make a reused context differ."""
    lib = _lib.load()
    shapes = [(1030, 1400, 7), (129, 64, 1), (333, 1777, 63)]
    data = []
    for k, (n, p, t) in enumerate(shapes):
        X = oracle.synth_genotypes(500 + k, n, p)
        data.append((Mat(X), Mat(oracle.synth_phenotypes(X, 600 + k, ntraits=t))))

    def fit(k):
        return abi.gblup_fit_ex(data[k][0], data[k][1], LAM, grm)

    assert lib.gbm_release_device_cache() == 0
    sequence = [(k, fit(k)) for k in (0, 1, 2, 1, 0)]
    fresh = {}
    for k in range(len(shapes)):
        assert lib.gbm_release_device_cache() == 0
        fresh[k] = fit(k)
    for k, got in sequence:
        assert got[3:] == fresh[k][3:]
        for a, b in zip(got[:3], fresh[k][:3]):
            assert np.array_equal(a, b), shapes[k]
