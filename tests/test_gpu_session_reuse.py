"""A session's device buffers only grow (csrc/session.h): a training set smaller than an earlier one runs in the
buffers the larger one left, at its own pitches. Whatever a session has held before, every entry must answer bit for
bit as a fresh session given only that call's training set does. The sequence is tools/session_digest.py's: all
300 entries (npad 384), 257 (the same pitch), 120 (npad 128, smaller) and all 300 again, with 1, 3, 1 and 3 traits;
the GWAS scan runs in chunks of 64 loci; once on host genotypes with the fp64 GRM, once on a synthetic session with
grm_mode exact."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("session_digest", os.path.join(ROOT, "tools", "session_digest.py"))
sd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sd)


@pytest.mark.parametrize("kind", sd.KINDS)
def test_reused_session_answers_as_a_fresh_one(kind, gbm_env):
    gbm_env.setenv("GBM_GWAS_CHUNK", str(sd.GWAS_CHUNK))
    with sd.open_session(kind) as reused:
        for step, (idx, ntraits) in enumerate(sd.STEPS):
            got = sd.run_step(reused, idx, ntraits)
            with sd.open_session(kind) as fresh:
                want = sd.run_step(fresh, idx, ntraits)
                assert reused.grm_used() == fresh.grm_used() == ("exact" if kind == "synthetic-exact" else "fp64")
            assert list(got) == list(want)
            for entry in want:
                assert len(got[entry]) == len(want[entry])
                for k, (a, b) in enumerate(zip(got[entry], want[entry])):
                    assert np.array_equal(a, b), f"{kind} step {step + 1} (n_train {idx.size}): {entry} output {k}"
