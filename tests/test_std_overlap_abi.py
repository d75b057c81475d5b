"""gbm_dev_standardize_grm_syrk (include/gbm.h; the standardisation and GRM stage 1 in one call) is declared,
bound, exported, and checks its arguments before any device use."""
import re
import subprocess

import gbm
from gbm import _lib


def test_library_exports_standardize_grm_syrk():
    assert "gbm_dev_standardize_grm_syrk" in _lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "gbm_dev_standardize_grm_syrk" in set(re.findall(r" T (gbm_[a-z0-9_]+)", out))
    lib = gbm.load_library()
    assert hasattr(lib, "gbm_dev_standardize_grm_syrk") and lib.gbm_version() == 212


def test_bad_arguments_are_refused():
    lib = gbm.load_library()
    rc = lib.gbm_dev_standardize_grm_syrk(None, 0, 0, 0, None, 0, None, None, None, None, None, 0, None, 0, None)
    assert rc == _lib.GBM_E_ARG and "bad arguments" in _lib.last_error()
