"""The standardisation of the loci behind the GRM's first range beside that range's tiles
(gbm_dev_standardize_grm_syrk, csrc/grm.hip launch_standardize_grm_syrk; GBM_GRM_STD_OVERLAP): the first range's
rows are standardised ahead of the persistent tile launch A (range 0), the others on the helper stream beside it,
followed there by the edge kernel and launch B (ranges 1 .. S − 1). The kernels, the units and each unit's
summation order are those of the serial sequence, so Z, mean, sd, keep, q and G after the reduce must be the SAME
BITS with the overlap on and off, on every shape that takes the overlapped path and every one that falls back.
The standardisation is reference src/gwas.jl:112-115,127-130, the GRM product src/gwas.jl:124."""
import numpy as np
import pytest

import gbm
import oracle
from gbm.sharded import HipShardStages, LocalComm, assemble_b_hat, sharded_gblup_step

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def monomorphic_rows(p):
    """loci on both sides of every split used here (the first range ends at about p/2 or 2p/3)"""
    return sorted({1, p // 2 - 1, p // 2, p // 2 + 1, p - 2} & set(range(p)))


def make_stages(n, p, seed=4242, nrhs=1):
    st = HipShardStages(n, p, nrhs=nrhs, lambda_=1.0, device=0)
    st.generate(seed, 0)
    for j in monomorphic_rows(p):
        st.X[j, :n] = 0.5
    return st


def grm_step(st):
    """standardize + GRM on torch's current stream with every output poisoned first; the outputs cloned on
    that stream right behind the calls (Z before the reduce: ordered by the call's own join)"""
    import torch
    st.Z.fill_(float("nan"))
    st.mean.fill_(float("nan"))
    st.sd.fill_(float("nan"))
    st.keep.fill_(-1)
    st.G.zero_()
    st.standardize()
    st.grm_syrk()
    out = {"Z": st.Z.clone()}
    st.grm_reduce()
    out.update(mean=st.mean.clone(), sd=st.sd.clone(), keep=st.keep.clone(), q=st.q.clone(),
               G=torch.triu(st.G[:st.n, :st.n]))
    return out


def same_bits(a, b):
    import torch
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in ("Z", "mean", "sd", "keep", "q", "G"))


def on_and_off(gbm_env, st):
    import torch
    gbm_env.setenv("GBM_GRM_STD_OVERLAP", "0")
    off = grm_step(st)
    gbm_env.setenv("GBM_GRM_STD_OVERLAP", "1")
    on = grm_step(st)
    torch.cuda.synchronize()
    return on, off


def check_filter(st, res):
    """keep = 0 exactly at the monomorphic loci, q counts the others, every kept Z row is finite"""
    import torch
    mono = monomorphic_rows(st.p)
    keep = res["keep"].cpu().numpy()
    assert not keep[mono].any() and int(keep.sum()) == st.p - len(mono) == int(res["q"].item())
    assert bool(torch.isfinite(res["Z"]).all()) and not bool(res["Z"][mono].any())


@pytest.mark.parametrize("n,p,split,slices", [
    (1032, 3000, "3,2,1", 3),  # ragged last column of 8: the edge kernel on the helper stream; p no multiple of 16
    (1024, 2048, "2,1", 2),    # whole tiles, no edge
    (5120, 512, "1,1", 2),     # the largest overlapped n (the 20-values-per-thread standardisation)
    (5121, 512, "1,1", 2),     # one more individual: serial
    (1024, 256, None, 1),      # a single range (h = p): serial
])
def test_overlap_same_bits(gbm_env, n, p, split, slices):
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    if split:
        gbm_env.setenv("GBM_GRM_SPLIT", split)
    assert gbm.load_library().gbm_dev_grm_slices(n, p) == slices
    st = make_stages(n, p)
    on, off = on_and_off(gbm_env, st)
    assert same_bits(on, off)
    check_filter(st, on)


@pytest.mark.parametrize("knob,value", [("GBM_GRM_CARRY", "1"), ("GBM_GRM_FUSED", "1"), ("GBM_GRM_PERSIST", "0")])
def test_fallback_modes_same_bits(gbm_env, knob, value):
    n, p = 1032, 3000
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    gbm_env.setenv("GBM_GRM_SPLIT", "3,2,1")
    gbm_env.setenv(knob, value)
    st = make_stages(n, p)  # (the workspace is sized for the mode)
    on, off = on_and_off(gbm_env, st)
    assert same_bits(on, off)
    check_filter(st, on)


def test_three_steps_same_bits(gbm_env):
    """counters, q and the slabs are reused by every step on one HipShardStages"""
    import torch
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    gbm_env.setenv("GBM_GRM_SPLIT", "3,2,1")
    st = make_stages(1032, 3000)
    steps = [grm_step(st) for _ in range(3)]
    torch.cuda.synchronize()
    assert same_bits(steps[0], steps[1]) and same_bits(steps[1], steps[2])
    check_filter(st, steps[2])


def test_non_default_stream_and_join(gbm_env):
    """on a side stream of torch's; the Z cloned on that stream right behind the call (no sync) is the finished Z"""
    import torch
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    gbm_env.setenv("GBM_GRM_SPLIT", "3,2,1")
    st = make_stages(1032, 3000)
    gbm_env.setenv("GBM_GRM_STD_OVERLAP", "0")
    off = grm_step(st)
    torch.cuda.synchronize()
    gbm_env.setenv("GBM_GRM_STD_OVERLAP", "1")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on = grm_step(st)
    side.synchronize()
    assert same_bits(on, off)


def test_stage_buffers_read_between_the_calls(gbm_env):
    """reading Z or q after standardize() runs the standardisation at once; grm_syrk() is then the GRM alone"""
    import torch
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    gbm_env.setenv("GBM_GRM_SPLIT", "3,2,1")
    st = make_stages(1032, 3000)
    ref = grm_step(st)
    st.Z.fill_(float("nan"))
    st.G.zero_()
    st.standardize()
    assert int(st.q.item()) == int(ref["q"].item())
    assert torch.equal(bits(st.Z), bits(ref["Z"]))
    st.grm_syrk()
    st.grm_syrk()  # (again, without a standardize(): q stays)
    st.grm_reduce()
    assert int(st.q.item()) == int(ref["q"].item())
    assert torch.equal(bits(torch.triu(st.G[:st.n, :st.n])), bits(ref["G"]))


def test_full_fit_matches_oracle(gbm_env):
    import torch
    n, p, t = 1032, 3000, 2
    gbm_env.setenv("GBM_GRM_CARRY", "0")
    gbm_env.setenv("GBM_GRM_SPLIT", "3,2,1")
    X = oracle.synth_genotypes(31, n, p)
    Y = oracle.synth_phenotypes(X, 32, ntraits=t)
    st = HipShardStages(n, p, nrhs=t, lambda_=1.0, device=0)
    st.upload_genotypes(X)
    st.load_phenotypes(Y)
    out = sharded_gblup_step(st, LocalComm())
    torch.cuda.synchronize()
    ref = oracle.gblup_fit(X, Y, 1.0)
    assert int(st.q.item()) == ref["q"]
    b_hat = assemble_b_hat(out["mu"], out["msum"], [out["B"]], p)
    assert rel(out["y_pred"], ref["y_pred"]) < 1e-9 and rel(out["mu"], ref["mu"]) < 1e-9
    assert rel(b_hat, ref["b_hat"]) < 1e-6

