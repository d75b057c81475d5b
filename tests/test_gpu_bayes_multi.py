"""Several BayesA / BayesB / BayesC chains over one genotype matrix in one pass (libgbm ``gbm_bayes_fit_multi``;
``gbm.bayes_multi_arrays``, ``gbm.bayes_multi``, the grouping of ``gbm.cvmultithread``). The contract is exact:
chain c has the bits of ``gbm_bayes_fit`` on the same model, phenotypes, priors, schedule and seed, whatever its
slot (wave c mod 4 of workgroup row c div 4), its neighbours, the number of chains and the genotype storage.
Shapes (csrc/bayes_abc.hip bayes_chain_kernel): (300, 150) has two chunk workgroups with a ragged last chunk and
blocks of 64, 64 and 22 markers; (200, 64) one block (no next-block partials); (3, 1) the smallest the ABI
accepts; (77, 130) with 32 chains fills eight workgroup rows. T = 1, 2, 5, 9 leave slots of the last row empty.
The library places four chains in a workgroup row only when the chains' workgroups outnumber the CUs (at these
shapes never), so the tests of the placement force it with GBM_BAYES_MULTI_WG=4 (and =1: one chain per row).
Inputs and helpers: tests/bayes_multi_cases.py, tests/gibbs_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import gbm
from gbm import _lib

import bayes_multi_cases as mc
import gibbs_cases as gc

pytestmark = pytest.mark.gpu

THINNED = (13, 4, 3)
BIT_CASES = [("dosage", 300, 150, T, gc.DEFAULT) for T in (1, 2, 4, 5, 9)] + [
    ("dosage", 300, 150, 5, THINNED), ("dosage", 200, 64, 4, gc.DEFAULT), ("tiny", 3, 1, 3, gc.DEFAULT),
    ("dosage", 77, 130, 32, gc.DEFAULT)]


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture
def four_per_row(gbm_env):
    gbm_env.setenv("GBM_BAYES_MULTI_WG", "4")


def multi_stats():
    calls, chains = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert gbm.load_library().gbm_debug_bayes_multi_stats(ctypes.byref(calls), ctypes.byref(chains)) == 0
    return calls.value, chains.value


# ---- 1. bit identity with the single fit -----------------------------------------------------------------
@pytest.mark.parametrize("per_row", ["4", "1"])
@pytest.mark.parametrize("kind,n,p,T,schedule", BIT_CASES, ids=_id)
def test_gpu_chain_has_the_bits_of_the_single_fit(gbm_env, kind, n, p, T, schedule, per_row):
    """b_hat, y_pred, var and pip of every chain equal gbm.bayes_arrays of the chain's model, column and seed,
    with byte storage (the default for these k/2 genotypes) and with GBM_BRR_I8=0; the two storages are equal
    to each other as well (as they are for the single fit: tests/test_gpu_gibbs_edges.py). With four chains per
    workgroup row and with one."""
    gbm_env.setenv("GBM_BAYES_MULTI_WG", per_row)
    by_storage = {}
    for storage in ("bytes", "fp64"):
        if storage == "fp64":
            gbm_env.setenv("GBM_BRR_I8", "0")
        outs = mc.multi(kind, n, p, T, schedule)
        assert [a.shape for a in outs] == [(p + 1, T), (n, T), (3, T), (p, T)]
        for c in range(T):
            mc.assert_same_bits(mc.chain(outs, c), mc.single(kind, n, p, c, schedule, storage), (storage, "chain", c))
        by_storage[storage] = outs
    mc.assert_same_bits(by_storage["bytes"], by_storage["fp64"], "bytes vs fp64")
    if T > 1:  # the chains differ (inputs and seeds), so a chain compared with the wrong single fit would show
        assert not np.array_equal(by_storage["bytes"][0][:, 0], by_storage["bytes"][0][:, 1])


def test_gpu_chain_bits_on_non_dyadic_genotypes(four_per_row):
    """X·0.3 + 0.05 fits no byte scale: fp64 storage, (300, 200) with blocks of 64, 64, 64 and 8."""
    T = 5
    outs = mc.multi("scaled", 300, 200, T, gc.DEFAULT)
    for c in range(T):
        mc.assert_same_bits(mc.chain(outs, c), mc.single("scaled", 300, 200, c, gc.DEFAULT, "fp64"), ("chain", c))


def test_gpu_the_mapping_the_library_chooses_has_the_same_bits():
    """No knob set: (300, 150) with five chains (one chain per row here: 10 workgroups on the device's CUs)."""
    outs = mc.multi("dosage", 300, 150, 5, gc.DEFAULT)
    for c in range(5):
        mc.assert_same_bits(mc.chain(outs, c), mc.single("dosage", 300, 150, c, gc.DEFAULT, "bytes"), ("chain", c))


# ---- 2. the literal loop, independent of the single fit ------------------------------------------------------
@pytest.mark.parametrize("name", ["tetra", "tiny63", "degenerate", "wide48"])
def test_gpu_chains_follow_the_literal_loop(four_per_row, name):
    """Chains (BayesA, BayesB, BayesC, BayesC) on one y and one seed against the one-marker-at-a-time loops of
    gibbs_cases to the suite's 1e-9 (tests/test_bayes_abc.py; the references' indicator margins exceed 1e-6,
    tests/test_gibbs_cases.py); the two BayesC chains are the same chain in two slots."""
    X, y = gc.case(name)
    n_iter, n_burnin, thin = gc.schedule_of(name)
    models = ("BayesA", "BayesB", "BayesC", "BayesC")
    outs = gbm.bayes_multi_arrays(models, X, np.column_stack([y] * 4), n_iter=n_iter, n_burnin=n_burnin, thin=thin,
                                  seeds=gc.SEED)
    for c, m in enumerate(models):
        ref = gc.reference(m, name)
        assert m == "BayesA" or ref["margin"] > 1e-6
        errs = {k: gc.rel(a, ref[k]) for k, a in zip(gc.OUTPUTS, mc.chain(outs, c))}
        print(name, c, m, {k: float(f"{v:.3g}") for k, v in errs.items()})
        for k, v in errs.items():
            assert v < 1e-9, (c, m, k, v)
    mc.assert_same_bits(mc.chain(outs, 2), mc.chain(outs, 3), "slots 2 and 3")


# ---- 3. slot independence ------------------------------------------------------------------------------------
def test_gpu_a_chain_does_not_depend_on_its_slot(four_per_row):
    """One (model, y, seed) in slots 0, 3, 4 and 7 of an 8-chain fit (first and last wave of two workgroup rows)
    among other chains: the four are identical, and identical to that chain alone."""
    X, Y = mc.inputs("dosage", 300, 150)
    T, same = 8, (0, 3, 4, 7)
    models = [mc.model_of(c) for c in range(T)]
    seeds = [mc.seed_of(c) for c in range(T)]
    Yc = np.array(Y[:, :T])
    for c in same:
        models[c], seeds[c], Yc[:, c] = "BayesB", 5, Y[:, 20]
    kw = dict(n_iter=9, n_burnin=2, thin=1)
    outs = gbm.bayes_multi_arrays(models, X, Yc, seeds=seeds, **kw)
    alone = gbm.bayes_multi_arrays(["BayesB"], X, Y[:, 20:21], seeds=5, **kw)
    for c in same:
        mc.assert_same_bits(mc.chain(outs, c), mc.chain(alone, 0), ("slot", c))
    assert not np.array_equal(outs[0][:, 0], outs[0][:, 1])


# ---- 4. the pooled context -----------------------------------------------------------------------------------
def test_gpu_pooled_context_across_fits(four_per_row):
    """Multi T = 5, a single fit, multi T = 2 on a smaller shape, multi T = 5 again on one pooled context: the
    first and the last have the same bits and the last allocates nothing (its buffers and its captured
    iteration are those of the first)."""
    lib = gbm.load_library()
    first = mc.multi("dosage", 300, 150, 5, gc.DEFAULT)
    X, Y = mc.inputs("dosage", 300, 150)
    gbm.bayes_arrays("BayesC", X, Y[:, 0], n_iter=9, n_burnin=2, thin=1, seed=3)
    small = mc.multi("dosage", 200, 64, 2, gc.DEFAULT)
    for c in range(2):
        mc.assert_same_bits(mc.chain(small, c), mc.single("dosage", 200, 64, c, gc.DEFAULT, "bytes"), ("small", c))
    a0 = lib.gbm_device_allocations()
    last = mc.multi("dosage", 300, 150, 5, gc.DEFAULT)
    assert lib.gbm_device_allocations() == a0
    mc.assert_same_bits(first, last, "first vs last")


def test_gpu_brr_untouched_by_a_multi_fit(four_per_row):
    path, fb = ctypes.c_int(-1), ctypes.c_int64(0)
    lib = gbm.load_library()

    def brr_stats():
        lib.gbm_debug_brr_stats(ctypes.byref(path), ctypes.byref(fb))
        return path.value, fb.value

    X, Y = mc.inputs("dosage", 300, 150)
    kw = dict(n_iter=6, n_burnin=2, thin=1, seed=5)
    before = gbm.brr_arrays(X, Y[:, 0], **kw)
    stats = brr_stats()
    mc.multi("dosage", 300, 150, 5, gc.DEFAULT)
    assert brr_stats() == stats
    after = gbm.brr_arrays(X, Y[:, 0], **kw)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# ---- 5. the model layer --------------------------------------------------------------------------------------
def test_gpu_bayes_multi_returns_the_model_functions_fits():
    g, ph = mc.panel(missing=())
    kw = dict(genomes=g, phenomes=ph, idx_entries=list(range(3, 58)), idx_loci_alleles=list(range(2, 90)), n_iter=12,
              n_burnin=4)
    c0 = multi_stats()
    fits = gbm.bayes_multi(("BayesA", "BayesB", "BayesC"), idx_traits=[1, 2], **kw)
    assert multi_stats() == (c0[0] + 1, c0[1] + 6)
    assert len(fits) == 6
    k = 0
    for fn in (gbm.bayesa, gbm.bayesb, gbm.bayesc):
        for t in (1, 2):
            want = fn(idx_trait=t, **kw)
            assert fits[k].model == fn.__name__ and fits[k].trait == ph.traits[t - 1]
            assert mc.same_fit(fits[k], want), (fn.__name__, t)
            k += 1


def test_gpu_bayes_multi_refuses_traits_with_different_missing_entries():
    g, ph = mc.panel(missing=((7, 1),))
    with pytest.raises(gbm.ArgumentError, match="different entries"):
        gbm.bayes_multi(("BayesA", "BayesC"), genomes=g, phenomes=ph, idx_traits=[1, 2], n_iter=6, n_burnin=2)
    fits = gbm.bayes_multi(("BayesA", "BayesC"), genomes=g, phenomes=ph, idx_traits=[2], n_iter=6, n_burnin=2)
    assert [f.n for f in fits] == [59, 59]


# ---- 6. farming ----------------------------------------------------------------------------------------------
def _direct(cv0, model, g, ph, loci=None):
    """The CV of one job on the one-model path: the model call and validate (gbm.cvmultithread's `other` jobs)."""
    fit = model(genomes=g, phenomes=ph, idx_entries=[g.entries.index(e) + 1 for e in cv0.fit.entries],
                idx_loci_alleles=loci or list(range(1, len(g.loci_alleles) + 1)),
                idx_trait=ph.traits.index(cv0.fit.trait) + 1, verbose=False)
    return gbm.validate(fit, g, ph, idx_validation=[g.entries.index(e) + 1 for e in cv0.validation_entries],
                        replication=cv0.replication, fold=cv0.fold)


def test_gpu_cvbulk_groups_the_three_models_of_a_fold():
    """cvbulk over (bayesa, bayesb, bayesc) on 60 entries x 90 loci, two traits, one missing phenotype: one multi
    fit of three chains per (trait, fold), and every CV equal, field for field and bit for bit, to the model
    call and validate done directly."""
    g, ph = mc.panel()
    models = tuple(functools.partial(f, n_iter=12, n_burnin=4) for f in (gbm.bayesa, gbm.bayesb, gbm.bayesc))
    placeholders, _, mv = gbm.cvbulk_setup(genomes=g, phenomes=ph, models=models, n_replications=1, n_folds=2)
    c0 = multi_stats()
    cvs, notes = gbm.cvbulk(genomes=g, phenomes=ph, models=models, n_replications=1, n_folds=2)
    assert notes == [] and len(cvs) == 12
    assert multi_stats() == (c0[0] + 4, c0[1] + 12)
    for cv, cv0, model in zip(cvs, placeholders, mv):
        assert cv.fit.model == model.func.__name__
        assert mc.same_cv(cv, _direct(cv0, model, g, ph)), (cv.fit.trait, cv.fold, cv.fit.model)


def test_gpu_cvmultithread_leaves_unshared_jobs_to_the_one_model_path():
    """Of one fold's jobs, bayesa and bayesb with one schedule share a fit; bayesc with another n_iter, and a
    bayesb job on a loci subset, share with nobody and go down the one-model path. All equal the direct CVs."""
    g, ph = mc.panel()
    short = dict(n_iter=12, n_burnin=4)
    models = (functools.partial(gbm.bayesa, **short), functools.partial(gbm.bayesb, **short),
              functools.partial(gbm.bayesc, n_iter=10, n_burnin=4), functools.partial(gbm.bayesb, **short))
    cvs, _, mv = gbm.cvbulk_setup(genomes=g, phenomes=ph, models=models, n_replications=1, n_folds=2)
    cvs, mv = cvs[:4], mv[:4]  # trait t1, fold 1
    cvs[3].fit.b_hat_labels = ["intercept"] + list(g.loci_alleles[10:80])
    placeholders = list(cvs)
    c0 = multi_stats()
    gbm.cvmultithread(cvs, genomes=g, phenomes=ph, models_vector=mv)
    assert multi_stats() == (c0[0] + 1, c0[1] + 2)
    for k, (cv, cv0, model) in enumerate(zip(cvs, placeholders, mv)):
        loci = list(range(11, 81)) if k == 3 else None
        assert mc.same_cv(cv, _direct(cv0, model, g, ph, loci)), k
    assert len(cvs[3].fit.b_hat) == 71
