"""What a finished gbm_dev_gblup_solve leaves behind, read by its three readers behind
every producer: whiten_rows_kernel (the upper U_mk blocks and Linv), gblup_terms_kernel (the diagonal of
Ld, for log det V) and gbm_session_gwas (the lower-copy rows and the off-diagonal entries of the Schur
block). The producers are the dataflow launch, the launch-per-panel path in single panels, pairs and
4/8/16-panel groups, the chain of panel and row-update launches in place of chol_group_kernel, and the
dataflow tail on the trailing sub-matrix. n = 1100 (npad 1152, 18 blocks, gdim 1216) is the smallest
size at which a 16-panel group forms. Each schedule is compared with the references only (the summation
orders differ between schedules); the inputs and references are those of tests/gwas_cases.py."""
import ctypes
import functools
import os

import numpy as np
import pytest

import gbm
import oracle
from gbm import _lib

import gwas_cases as gc

pytestmark = pytest.mark.gpu

N, NB = 1100, 18
TOL = 1e-9  # tests/test_gpu_gwas.py's: z, b and the REML objective
TOL_WHITEN = 1e-10  # tests/test_gpu_gwas.py's whitening bound

_PANELS = {"GBM_CHOL_FLOW_MAX": "0"}  # the launch-per-panel path
_PAIRS = {**_PANELS, "GBM_UPD64_LIM": "128"}


def _group(g, **more):
    knobs = {**_PAIRS, **{f"GBM_CHOL_G{k}_LIM": "0" if k == g else "-1" for k in (4, 8, 16)}}
    return {**knobs, **more}


# id -> (knobs, the panels per step gbm_dev_chol_group_size must report from kb = 0 on)
SCHEDULES = {
    "flow": ({}, None),  # one dataflow launch: the group sizes are not consulted
    "panel1": (_PANELS, [1] * 18),
    "pairs": (_PAIRS, [2] * 8 + [1, 1]),
    "g4": (_group(4), [4] * 4 + [1, 1]),
    "g8": (_group(8), [8, 8, 1, 1]),
    "g16": (_group(16), [16, 1, 1]),
    "g4-chain": (_group(4, GBM_CHOL_GROUP_KERNEL="0"), [4] * 4 + [1, 1]),
    "g4-tail": (_group(4, GBM_CHOL_TAIL_FLOW="704"), [4, 4, 10]),  # gdim − 64·8 = 704: the dataflow tail from kb = 8
}
KNOBS = sorted({k for knobs, _ in SCHEDULES.values() for k in knobs})


def walk(n):
    lib = gbm.load_library()
    nb, kb, out = lib.gbm_dev_npad(n) // 64, 0, []
    while kb < nb:
        g = int(lib.gbm_dev_chol_group_size(n, kb))
        assert 1 <= g <= nb - kb, (kb, g)
        out.append(g)
        kb += g
    return out


@pytest.fixture(params=list(SCHEDULES))
def schedule(request, gbm_env):
    """Sets the schedule's knobs and asserts the schedule itself: a knob that stops forcing its path fails here."""
    name = request.param
    knobs, groups = SCHEDULES[name]
    lib = gbm.load_library()
    assert lib.gbm_dev_npad(N) == 64 * NB and lib.gbm_dev_gdim(N) == 64 * NB + 64
    for k in KNOBS:
        if k not in knobs:
            assert k not in os.environ, f"{k} is set from outside: the schedule '{name}' would not be the one tested"
    for k, v in knobs.items():
        gbm_env.setenv(k, v)
    got = walk(N)
    print(f"{name}: panels per step {got}")
    if name == "flow":
        assert lib.gbm_dev_npad(N) <= 12288 and not knobs  # the default: dataflow up to npad 12 288
        return name
    assert os.environ["GBM_CHOL_FLOW_MAX"] == "0"
    assert got == groups, (name, got)
    forced = {"pairs": 2, "g4": 4, "g8": 8, "g16": 16, "g4-chain": 4, "g4-tail": 4}.get(name)
    if forced:
        assert forced in got and max(got[:-1]) == forced
    if name == "panel1":
        assert set(got) == {1}
    if name == "g4-tail":
        assert sum(got[:-1]) == 8 and got[-1] == NB - 8  # the last group runs to nb
    else:
        assert max(got) <= 16 and got[-1] == 1
    return name


@pytest.fixture(scope="module")
def session():
    with gbm.GenotypeSession(gc.data("n1100")[0]) as s:
        yield s


@pytest.fixture(scope="module")
def stages():
    """The n = 1100 shard up to its GRM (schedule-independent); each test factors a copy of G."""
    import torch

    from gbm.sharded import HipShardStages
    X, y = gc.data("n1100")
    st = HipShardStages(N, X.shape[1], nrhs=1, lambda_=0.6, device=0)
    st.upload_genotypes(X.copy())
    st.load_phenotypes(y.copy())
    st.standardize()
    st.grm_syrk()
    st.grm_reduce()
    torch.cuda.synchronize()
    return st, st.G.clone()


def test_every_schedule_is_listed():
    assert list(SCHEDULES) == ["flow", "panel1", "pairs", "g4", "g8", "g16", "g4-chain", "g4-tail"]


def test_whitening_reads_the_upper_blocks_and_linv(schedule, stages):
    """gbm_dev_whiten_rows after the solve, 129 rows (two full strips and one row) over 18 column blocks,
    against R[:, :n] @ inv(U); the padding columns stay exactly 0; row 128 alone reproduces its bits."""
    import torch
    st, G0 = stages
    st.G.copy_(G0)
    st.solve()
    torch.cuda.synchronize()
    assert int(st.info.item()) == 0
    Rn, _ = gc.whitening()
    rows = Rn.shape[0]
    assert rows == 129
    Rh = np.zeros((rows, st.npad))
    Rh[:, :N] = Rn
    lib = gbm.load_library()
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())

    def whiten(host):
        R = torch.from_numpy(host.copy()).to(st.dev)
        _lib.check(lib.gbm_dev_whiten_rows(p_(st.G), st.gdim, N, p_(st.ws_solve), p_(R), st.npad, host.shape[0],
                                           st._stream()), "gbm_dev_whiten_rows")
        torch.cuda.synchronize()
        return R.cpu().numpy()

    got = whiten(Rh)
    err = gc.rel(got[:, :N], gc.whitening_ref())
    print(f"{schedule}: whitening rel err {err:.3e}")
    assert err < TOL_WHITEN
    assert np.all(got[:, N:] == 0.0)
    assert np.array_equal(whiten(Rh[128:129]), got[128:129])


THETA = np.array([(0.5, 0.5), (0.2, 0.9), (1e-3, 0.7), (0.9, 1e-2), (1.0, 1.0)])  # test_reml_objective_matches_loglikreml's


@functools.lru_cache(maxsize=None)
def reml_reference():
    X, y = gc.data("n1100")
    G, _ = oracle.grm(X)
    return np.array([oracle.loglikreml(t, y, np.ones((N, 1)), G) for t in THETA])


def test_reml_terms_read_the_diagonal_of_ld(schedule, session):
    _, y = gc.data("n1100")
    got = session.reml_objective(np.arange(N), y, THETA[:, 0], THETA[:, 1])
    err = gc.rel(got, reml_reference())
    print(f"{schedule}: REML objective rel err {err:.3e}")
    assert err < TOL


def test_gwas_reads_the_lower_rows_and_the_schur_block(schedule, session):
    _, y = gc.data("n1100")
    all_rows = np.arange(N)
    before = session.gblup(all_rows, y, 0.7)
    for name in gc.READER_CASES:  # kc = 7 (a 9 x 9 Schur read), then kc = 0 on the same session
        c = gc.CASES[name]
        idx, _, yt, C = gc.inputs(name)
        r = session.gwas(idx, yt, covariates=C, model="mlm", sigma2=c.s2)
        z, b, keep = gc.literal(name)
        ez, eb = gc.rel(r["z"], z), gc.rel(r["b"], b)
        print(f"{schedule}: {name} z rel err {ez:.3e} b rel err {eb:.3e}")
        assert ez < TOL and eb < TOL
        assert r["tested"] == c.tested == int(keep.sum()) and (r["sigma2_e"], r["sigma2_u"]) == c.s2
    after = session.gblup(all_rows, y, 0.7)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[2], after[2]) and before[3] == after[3]
