"""The column standardisation (csrc/stats.hip) at the sizes where its launcher changes kernel, against an
extended-precision reference, called at device level on torch tensors: gbm_dev_standardize (in place and out of
place), gbm_dev_standardize_gather (center_only 0 and 1) and gbm_dev_standardize_i8.

launch_standardize picks a register-cached kernel for n <= 1024 / 2048 / 4096 / 8192 (4 / 8 / 16 / 32 values per
thread, the last pass masked with i < n) and a generic one above; n sits on and next to every threshold.
Inputs, 37 loci in one matrix: monomorphic columns at the dyadic constants 0, 0.25, 0.5 and 1 (their sums and
means are exact in any order, so the keep decision does not depend on rounding), a near-constant column
0.97 + 1e-9 N(0, 1), uniform reals in [0, 1] (pooled allele frequencies) and dosage halves; for the int8 kernel
diploid halves and tetraploid quarters. Everything the kernels must not read holds a poison (NaN, or the byte 77),
and Z is pre-filled with NaN.

Reference: two-pass mean, ddof = 1 sd and Z in np.longdouble. keep, q, the zero padding and the zero rows of
dropped loci are exact requirements. For the errors of mean, sd and Z the yardstick is the fp64 numpy oracle
(oracle.colstats / oracle.standardize) on the same inputs: error = max |value − reference| / max |reference| per
quantity, and the kernel's may be at most 8 x the oracle's plus 4 ulp (4 eps of the scaled quantity). The kernel's
fixed-order tree sum and numpy's pairwise sum are both O(log n) eps but not the same tree, hence the factor. The
same rule is applied once more without the near-constant column, whose Z error (the rounding of its mean over
its sd, ~1e-7) would otherwise hide every other column's."""
import ctypes

import numpy as np
import pytest

import oracle

import abi_direct as abi
from abi_direct import Mat, rel
from gbm import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
NS = [1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193]
P = 37
NEAR = 4  # the near-constant column of the fp64 inputs
FACTOR, SLACK = 8.0, 4.0 * EPS


def fp64_input(n, seed):
    rng = np.random.default_rng(seed)
    X = np.empty((n, P), order="F")
    X[:, 0], X[:, 1], X[:, 2], X[:, 3] = 0.0, 0.25, 0.5, 1.0
    X[:, NEAR] = 0.97 + 1e-9 * rng.standard_normal(n)
    X[:, 5:21] = rng.random((n, 16))
    f = rng.uniform(0.02, 0.5, size=16)
    X[:, 21:] = rng.binomial(2, f, size=(n, 16)) / 2.0
    return X


def dosage_input(n, ploidy, seed):
    rng = np.random.default_rng(seed)
    mono = [0, 1, 2] if ploidy == 2 else [0, 1, 2, 4]
    D = np.empty((n, P), dtype=np.int8, order="F")
    for j, d in enumerate(mono):
        D[:, j] = d
    f = rng.uniform(0.02, 0.5, size=P - len(mono))
    D[:, len(mono):] = rng.binomial(ploidy, f, size=(n, P - len(mono)))
    return D


def reference(X, center_only):
    """Two-pass statistics and Z (n x p, zero columns for dropped loci) in extended precision."""
    n = X.shape[0]
    Xl = X.astype(LD)
    m = Xl.sum(axis=0) / LD(n)
    C = Xl - m
    s = np.sqrt((C * C).sum(axis=0) / LD(n - 1))
    # the test's own precondition: the keep mask is decided by the data, not by rounding
    assert np.all((s == 0) | (s >= 1e-10))
    if center_only:
        return m, np.ones(X.shape[1], dtype=LD), np.ones(X.shape[1], dtype=bool), C
    keep = s > 0
    Z = np.zeros_like(C)
    Z[:, keep] = C[:, keep] / s[keep]
    return m, s, keep, Z


def oracle_values(X, center_only):
    m, s, keep = oracle.colstats(X)
    if center_only:
        return m, np.ones_like(s), np.ones_like(keep), X - m
    Z = np.zeros_like(X)
    Z[:, keep] = oracle.standardize(X, m, s, keep)
    return m, s, keep, Z


def scaled_err(a, ref):
    return float(np.abs(np.asarray(a).astype(LD) - ref).max() / np.abs(ref).max())


def check_against_reference(label, got, X, center_only, near=None):
    """got = (mean, sd, keep, q, Z (n x p)) from the device."""
    gm, gs, gk, gq, gZ = got
    rm, rs, rk, rZ = reference(X, center_only)
    om, os_, ok, oZ = oracle_values(X, center_only)
    assert np.array_equal(ok, rk)  # the oracle agrees on the mask, or it could not serve as a yardstick
    assert np.array_equal(gk, rk.astype(np.int32)) and gq == int(rk.sum())
    assert np.all(gZ[:, ~rk] == 0.0)
    if center_only:
        assert np.all(gs == 1.0)
    groups = {"all": np.ones(X.shape[1], dtype=bool)}
    if near is not None:
        groups["regular"] = np.arange(X.shape[1]) != near
    for gname, cols in groups.items():
        for qname, g, o, r in (("mean", gm, om, rm), ("sd", gs, os_, rs), ("Z", gZ, oZ, rZ)):
            g, o, r = (v[..., cols] for v in (g, o, r))
            ek, eo = scaled_err(g, r), scaled_err(o, r)
            print(f"{label} {gname:7s} {qname:4s} kernel {ek:.3e} oracle {eo:.3e} ratio {ek / max(eo, EPS / 64):.2f}")
            assert ek <= FACTOR * eo + SLACK, (label, gname, qname, ek, eo)


class Device:
    """The calling pattern of gbm.sharded.HipShardStages: device pointers of torch tensors, the current stream."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _lib.load()

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def outputs(self, p, ldz, Z=None):
        t = self.torch
        if Z is None:
            Z = t.full((p, ldz), float("nan"), dtype=t.float64, device="cuda")
        return (Z, t.full((p,), float("nan"), dtype=t.float64, device="cuda"),
                t.full((p,), float("nan"), dtype=t.float64, device="cuda"),
                t.full((p,), -1, dtype=t.int32, device="cuda"), t.zeros(1, dtype=t.int64, device="cuda"))

    def collect(self, out, n):
        Z, mean, sd, keep, q = out
        self.torch.cuda.synchronize()
        Zh = Z.cpu().numpy()
        assert np.all(Zh[:, n:] == 0.0)  # the padding columns [n, ldz), NaN before the call
        return mean.cpu().numpy(), sd.cpu().numpy(), keep.cpu().numpy(), int(q.item()), np.ascontiguousarray(Zh[:, :n].T)

    def rows(self, X, ldx):
        """X (n x p) as poisoned locus rows: p x ldx, NaN in the columns [n, ldx)."""
        Xt = np.full((X.shape[1], ldx), np.nan)
        Xt[:, :X.shape[0]] = X.T
        return self.put(Xt)


@pytest.fixture(scope="module")
def dev():
    return Device()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("place", ["in_place", "out_of_place"])
def test_standardize_at_dispatch_edges(dev, place, n):
    lib = dev.lib
    X = fp64_input(n, n)
    ldz = lib.gbm_dev_npad(n)
    if place == "in_place":
        Xt = dev.rows(X, ldz)
        out = dev.outputs(P, ldz, Z=Xt)
        ldx = ldz
    else:
        ldx = n + 7  # rows only 8-byte aligned
        Xt = dev.rows(X, ldx)
        out = dev.outputs(P, ldz)
    _lib.check(lib.gbm_dev_standardize(dev.p(Xt), ldx, P, n, dev.p(out[0]), ldz, dev.p(out[1]), dev.p(out[2]),
                                       dev.p(out[3]), dev.p(out[4]), dev.stream()), "gbm_dev_standardize")
    check_against_reference(f"n={n} {place}", dev.collect(out, n), X, 0, near=NEAR)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("center_only", [0, 1])
def test_standardize_gather_at_dispatch_edges(dev, center_only, n):
    """n training entries gathered from a session-like Xt of n + 211 entries; the entries left out hold NaN."""
    lib = dev.lib
    ntot = n + 211
    rng = np.random.default_rng(7 * n + 1)
    idx = np.sort(rng.permutation(ntot)[:n]).astype(np.int32)  # a shuffled pick, strictly increasing
    assert np.all(np.diff(idx) > 0)
    X = fp64_input(n, n + 1)
    full = np.full((ntot, P), np.nan)
    full[idx] = X
    ldx, ldz = lib.gbm_dev_npad(ntot), lib.gbm_dev_npad(n)
    Xt = dev.rows(full, ldx)
    out = dev.outputs(P, ldz)
    idx_d = dev.put(idx)
    _lib.check(lib.gbm_dev_standardize_gather(dev.p(Xt), ldx, P, dev.p(idx_d), n, dev.p(out[0]), ldz,
                                              dev.p(out[1]), dev.p(out[2]), dev.p(out[3]), dev.p(out[4]), center_only,
                                              dev.stream()), "gbm_dev_standardize_gather")
    check_against_reference(f"n={n} gather center_only={center_only}", dev.collect(out, n), X, center_only, near=NEAR)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("ploidy", [2, 4])
def test_standardize_i8_at_dispatch_edges(dev, ploidy, n):
    """Straight from the dosage bytes: the reference's statistics, and the header's promise of the same bits as
    gbm_dev_expand_dosage_i8 followed by gbm_dev_standardize."""
    lib = dev.lib
    D = Mat(dosage_input(n, ploidy, n + 2), 3)  # ldd = n + 3, the byte 77 in the padding rows
    Dd = dev.put(D.parent.T)                    # column-major n x p with ldd = row-major p x ldd
    ldz = lib.gbm_dev_npad(n)
    out = dev.outputs(P, ldz)
    _lib.check(lib.gbm_dev_standardize_i8(dev.p(Dd), D.ld, P, n, ploidy, dev.p(out[0]), ldz, dev.p(out[1]),
                                          dev.p(out[2]), dev.p(out[3]), dev.p(out[4]), dev.stream()),
               "gbm_dev_standardize_i8")
    got = dev.collect(out, n)
    X = D.parent[:n].astype(np.float64) / ploidy
    check_against_reference(f"n={n} int8 ploidy={ploidy}", got, X, 0)
    Xt = dev.torch.full((P, ldz), float("nan"), dtype=dev.torch.float64, device="cuda")
    _lib.check(lib.gbm_dev_expand_dosage_i8(dev.p(Dd), D.ld, n, P, ploidy, dev.p(Xt), ldz, dev.stream()), "expand")
    two = dev.outputs(P, ldz)
    _lib.check(lib.gbm_dev_standardize(dev.p(Xt), ldz, P, n, dev.p(two[0]), ldz, dev.p(two[1]), dev.p(two[2]),
                                       dev.p(two[3]), dev.p(two[4]), dev.stream()), "gbm_dev_standardize")
    dev.torch.cuda.synchronize()
    assert np.array_equal(Xt.cpu().numpy()[:, :n].T, X) and dev.torch.count_nonzero(Xt[:, n:]).item() == 0
    for a, b in zip(got, dev.collect(two, n)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["fp64", "auto"])
def test_real_valued_genotypes_host_fit_and_grm(mode):
    """Pooled allele frequencies (any real in [0, 1]) through the host entries at the suite's ragged shape: the fit
    in fp64 and auto modes (auto must fall back to the fp64 GRM) and gbm.grm, against the oracle."""
    import gbm

    n, p, t = 333, 1777, 3
    X = np.asfortranarray(np.random.default_rng(1777).random((n, p)))
    Y = oracle.synth_phenotypes(X, 12, ntraits=t)
    ref = oracle.gblup_fit(X, Y, 1.0)
    b, y, mu, q, used = abi.gblup_fit_ex(Mat(X), Mat(Y), 1.0, mode)
    assert used == _lib.GBM_GRM_FP64 and q == ref["q"] == p
    assert rel(y, ref["y_pred"]) < 1e-9 and rel(mu, ref["mu"]) < 1e-9 and rel(b, ref["b_hat"]) < 1e-6
    assert rel(oracle.predict_linear(X, b), y) < 1e-9
    G, qg = gbm.grm(X)
    assert qg == p and rel(G, ref["G"]) < 1e-12 and np.array_equal(G, G.T)
