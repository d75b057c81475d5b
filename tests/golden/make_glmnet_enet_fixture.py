"""Extract R-glmnet known answers for the lasso and the elastic net (alpha = 1 and alpha = 0.5) from the
statsmodels test suite of the installed statsmodels (statsmodels/regression/tests/results: lasso_data.csv +
glmnet_r_results.py, written by R's glmnet; BSD-licensed test data) into tests/golden/enet/glmnet_enet_r.npz
(a directory of its own: tests/test_oracle.py takes every tests/golden/*.npz but the two R files it names for a
GBLUP fixture).
The source and the layout are those of make_glmnet_fixture.py: each case is [n, p, alpha, λ, coefficients
padded to 5]; the data are the first n rows and p columns, y and X centred and scaled (ddof=1) as the
statsmodels harness does. Used by tests/test_lasso.py and tests/test_gpu_lasso.py."""
import importlib.util
import os

import numpy as np

SRC = "/opt/conda/lib/python3.9/site-packages/statsmodels/regression/tests/results"  # as make_glmnet_fixture.py
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "enet", "glmnet_enet_r.npz")

data = np.loadtxt(os.path.join(SRC, "lasso_data.csv"), delimiter=",")
spec = importlib.util.spec_from_file_location("glmnet_r_results", os.path.join(SRC, "glmnet_r_results.py"))
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
cases = []
for name in sorted(x for x in dir(mod) if x.startswith("rslt_")):
    v = getattr(mod, name)
    if float(v[2]) not in (0.5, 1.0):
        continue  # the ridge cases are glmnet_ridge_r.npz
    cases.append(np.concatenate([v[:4], np.pad(v[4:], (0, 5 - (v.size - 4)))]))
np.savez(OUT, data=data, cases=np.array(cases))
print(OUT, len(cases), "cases")
