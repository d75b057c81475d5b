"""The literal single-site loop of the BayesA / BayesB / BayesC Gibbs samplers (Gaussian response)
that ``gbm_bayes_fit`` runs on the device — the test reference of tests/test_bayes_abc.py. It is
the text of include/gbm.h (gbm_bayes_fit) restated one marker at a time on the oracle's
counter-based random numbers (oracle.brr_u01 / brr_normal / brr_chisq), so the device chain and this
loop follow the same sample path. Not a test module."""
import functools
import math

import numpy as np

import oracle

MODELS = {"BayesA": 1, "BayesB": 2, "BayesC": 3}
SHAPE0 = 1.1


def _gamma(seed, a, shape, rate):
    return oracle.brr_chisq(seed, a, 2.0 * shape) / (2.0 * rate)


def bayes_gibbs(model, X, y, n_iter, n_burnin, thin=5, r2=0.5, df0=5.0, prob_in=0.5, counts=10.0, seed=42):
    """Returns b_hat (p+1), y_pred, var = [varE, mean_j varB_j, π] (posterior means), pip, and
    ``margin``: the smallest |logOdds − logit(u)| over every indicator draw (inf for BayesA)."""
    assert model in MODELS
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    cols = [np.ascontiguousarray(X[:, j]) for j in range(p)]
    x2 = (X * X).sum(axis=0)
    msx = x2.sum() / n - (X.mean(axis=0) ** 2).sum()
    vy = y.var(ddof=1)
    S0e = vy * (1 - r2) * (df0 + 2)
    varE = S0e / (df0 + 2)
    S0 = vy * r2 / msx * (df0 + 2)
    if model != "BayesA":
        S0 = S0 / prob_in
    S = S0
    rate0 = (SHAPE0 - 1) / S0
    varB = np.full(p, S0 / (df0 + 2))
    pi, c_in, c_out = prob_in, counts * prob_in, counts * (1 - prob_in)
    mu = y.mean()
    e = y - mu
    b = np.zeros(p)
    d = np.ones(p)
    bbar, dbar = np.zeros(p), np.zeros(p)
    mubar = varEbar = varBbar = pibar = 0.0
    nsum = 0
    margin = math.inf
    for it in range(n_iter):
        A = 8 * it
        # 1. intercept
        s = (e + mu).sum()
        mu_new = s / n + np.sqrt(varE / n) * oracle.brr_normal(seed, A, 0xFFFFFFFF)
        e = (e + mu) - mu_new
        mu = mu_new
        # 2. markers in order
        log_pi = math.log(pi / (1 - pi))
        for j in range(p):
            xj = cols[j]
            eff = d[j] * b[j]
            r = float(xj @ e) + x2[j] * eff
            xi = oracle.brr_normal(seed, A, j)
            if model == "BayesA":
                d_new = 1.0
            else:
                u = oracle.brr_u01(seed, A + 3, j)
                log_odds = log_pi + (2 * b[j] * r - b[j] * b[j] * x2[j]) / (2 * varE)
                lu = math.log(u / (1 - u))
                margin = min(margin, abs(log_odds - lu))
                d_new = 1.0 if log_odds > lu else 0.0
            if d_new == 0.0:
                b_new = math.sqrt(varB[j]) * xi
            else:
                C = x2[j] / varE + 1.0 / varB[j]
                b_new = (r / varE) / C + math.sqrt(1.0 / C) * xi
            e += (eff - d_new * b_new) * xj
            b[j] = b_new
            d[j] = d_new
        # 3. variances
        if model in ("BayesA", "BayesB"):
            PM = (1 << 63) | (it << 40)
            for j in range(p):
                varB[j] = (S + b[j] * b[j]) / oracle.brr_chisq(seed, PM | j, df0 + 1)
            S = _gamma(seed, A + 4, p * df0 / 2 + SHAPE0, (1.0 / varB).sum() / 2 + rate0)
        else:
            vb = ((b * b).sum() + S) / oracle.brr_chisq(seed, A + 1, df0 + p)
            varB[:] = vb
            S = _gamma(seed, A + 4, df0 / 2 + SHAPE0, 1.0 / (2 * vb) + rate0)
        if model != "BayesA":
            m = d.sum()
            g1 = _gamma(seed, A + 5, m + c_in, 1.0)
            g2 = _gamma(seed, A + 6, p - m + c_out, 1.0)
            pi = g1 / (g1 + g2)
        varE = ((e * e).sum() + S0e) / oracle.brr_chisq(seed, A + 2, df0 + n)
        # 4. running means
        i = it + 1
        if i % thin == 0 and i > n_burnin:
            nsum += 1
            k = float(nsum)
            w0, w1 = (k - 1) / k, 1 / k
            bbar = bbar * w0 + (d * b) * w1
            dbar = dbar * w0 + d * w1
            mubar = mubar * w0 + mu * w1
            varEbar = varEbar * w0 + varE * w1
            varBbar = varBbar * w0 + varB.mean() * w1
            pibar = pibar * w0 + pi * w1
    return {"b_hat": np.concatenate([[mubar], bbar]), "y_pred": mubar + X @ bbar,
            "var": np.array([varEbar, varBbar, pibar]), "pip": dbar, "margin": margin}


@functools.lru_cache(maxsize=None)
def path_case(n, p, seed_x=None, scale=False):
    """The synthetic data of the same-sample-path tests (tests/test_brr.py's recipe)."""
    X = oracle.synth_genotypes(61 + p if seed_x is None else seed_x, n, p)
    if scale:
        X = X * 0.3 + 0.05
    y = oracle.synth_phenotypes(X, 62)[:, 0]
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def path_ref(model, n, p, iters, seed=99, seed_x=None, scale=False):
    X, y = path_case(n, p, seed_x, scale)
    return bayes_gibbs(model, X, y, n_iter=iters, n_burnin=2, thin=1, seed=seed)


@functools.lru_cache(maxsize=None)
def sparse_case():
    """Eight QTL of effect ±1 among 1000 markers, h² = 0.5."""
    n, p = 300, 1000
    X = oracle.synth_genotypes(7001, n, p)
    qtl = np.arange(40, 1000, 120)
    beta = np.zeros(p)
    beta[qtl] = np.where(np.arange(len(qtl)) % 2 == 0, 1.0, -1.0)
    g = X @ beta
    y = g + np.random.default_rng(5).standard_normal(n) * g.std(ddof=1)
    return X, y, g, qtl


SPARSE_FIT = dict(n_iter=600, n_burnin=200, thin=5, seed=3)


def check_sparse(model, b_hat, y_pred, pip):
    """The sparse-signal assertions (thresholds fixed on the reference loop; see test 2)."""
    X, y, g, qtl = sparse_case()
    rest = np.setdiff1d(np.arange(X.shape[1]), qtl)
    cor = np.corrcoef(y_pred, g)[0, 1]
    ab = np.abs(b_hat[1:])
    figures = {"pip_qtl": pip[qtl].mean(), "pip_rest": pip[rest].mean(), "cor": cor,
               "absb_qtl": ab[qtl].mean(), "absb_rest": ab[rest].mean()}
    print(model, figures)
    if model == "BayesA":
        assert figures["absb_qtl"] >= 10 * figures["absb_rest"], figures
        assert cor >= 0.75, figures
    else:
        assert figures["pip_qtl"] >= 0.75, figures
        assert figures["pip_rest"] <= 0.3, figures
        assert cor >= 0.8, figures
    return figures
