"""Whole diagonal GRM tiles computed as their 36 upper 16x16 MFMA blocks only (GBM_GRM_DIAG, csrc/grm.hip
diag_tile): every element's sum over the loci keeps its stages, its 4-deep MFMA steps and the range-ordered
slab reduce, so G must be the SAME BITS as with the quadrant form (GBM_GRM_DIAG=0) in every defined (upper)
element — slab and direct epilogues, persistent and hardware-dispatched units, ragged shapes (masked
diagonal tiles keep the quadrant form, the edge kernel runs beside the tiles) and G += accumulation.
The planner's cost of a diagonal unit differs between the two forms and may move the loci split (which
changes the last bits, as another CU count does): the bit comparisons pin it, by GBM_GRM_SPLIT or by one
GBM_GRM_DIAG_COST for both forms.
The GRM is the product of reference src/gwas.jl:124 (GenomicBreedingCore.grmsimple)."""
import numpy as np
import pytest

import gbm
import oracle

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def pin_split(gbm_env, split):
    if split:
        gbm_env.setenv("GBM_GRM_SPLIT", split)
    else:  # the planner's split, from the same unit costs for both forms
        gbm_env.setenv("GBM_GRM_DIAG_COST", "0.93")


@pytest.mark.parametrize("n,p,split,persist", [
    (1030, 1234, "4,2,1,1", 1),  # ragged column of 6 (edge kernel beside the tiles), 8 whole diagonal tiles, partial last stage
    (2048, 3000, None, 1),       # whole tiles, no edge, the planner's split
    (1100, 2049, "3,1", 1),      # last diagonal tile masked: quadrant form there, upper blocks on the others, one launch
    (256, 40, None, 1),          # 3 stages: one range, straight into G; the K tail zero-filled
    (700, 5000, "1,1,1,1,1,1,1,1", 1),  # many small ranges
    (1030, 1234, "4,2,1,1", 0),  # hardware-dispatched workgroups
])
def test_grm_diag_blocks_same_bits(gbm_env, n, p, split, persist):
    X = oracle.synth_genotypes(n * 3 + p, n, p)
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    gbm_env.setenv("GBM_GRM_PERSIST", str(persist))
    pin_split(gbm_env, split)
    slices = gbm.load_library().gbm_dev_grm_slices
    gbm_env.setenv("GBM_GRM_DIAG", "0")
    s0 = slices(n, p)
    G0, q0 = gbm.grm(X)
    gbm_env.setenv("GBM_GRM_DIAG", "1")
    s1 = slices(n, p)
    G1, q1 = gbm.grm(X)
    G2, _ = gbm.grm(X)  # the workspace (slabs, queue counters) reused by a second call
    Gr, qr = oracle.grm(X)
    assert s0 == s1
    assert s1 == 1 if p == 40 else s1 > 1  # (one range: the direct epilogue; else the slabs)
    assert q0 == q1 == qr
    assert np.array_equal(G0, G1) and np.array_equal(G1, G2)
    assert rel(G1, Gr) < 1e-12


def test_streamed_accumulating_fit_diag_same_bits(gbm_env):
    """Loci-streamed fit: every chunk's GRM is added into G (accum) by the slab reduce."""
    n, p, chunk = 700, 5000, 1500
    X = oracle.synth_genotypes(77, n, p)
    Y = oracle.synth_phenotypes(X, 78, ntraits=2)
    gbm_env.setenv("GBM_HOST_CHUNK", str(chunk))
    gbm_env.setenv("GBM_STREAM_CHUNK", str(chunk))
    pin_split(gbm_env, None)
    gbm_env.setenv("GBM_GRM_DIAG", "0")
    r = gbm.gblup_arrays(X, Y)
    gbm_env.setenv("GBM_GRM_DIAG", "1")
    s = gbm.gblup_arrays(X, Y)
    for a, b in zip(s, r):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_gblup_diag_matches_oracle(gbm_env):
    gbm_env.setenv("GBM_GRM_DIAG", "1")
    n, p = 1030, 3000
    X = oracle.synth_genotypes(21, n, p)
    Y = oracle.synth_phenotypes(X, 22, ntraits=2)
    b_hat, y_pred, mu, q = gbm.gblup_arrays(X, Y, lambda_=1.0)
    ref = oracle.gblup_fit(X, Y, 1.0)
    assert q == ref["q"] and rel(y_pred, ref["y_pred"]) < 1e-9 and rel(b_hat, ref["b_hat"]) < 1e-6
