"""The literal single-site loop of the BayesA / BayesB / BayesC Gibbs samplers with an ordinal
(threshold-model) response that ``gbm_bayes_fit_ordinal`` runs on the device — the test reference of
tests/test_bayes_ordinal.py. It is the text of include/gbm.h (gbm_bayes_fit_ordinal) restated one
marker and one individual at a time on the oracle's counter-based random numbers (oracle.brr_u01 /
brr_normal / brr_chisq), with its own AS241 PPND16 and ``math.erfc``, so the device chain and this
loop follow the same sample path. Not a test module."""
import functools
import math

import numpy as np

import oracle
from bayes_abc_ref import MODELS, SHAPE0, _gamma, path_case, sparse_case

U64_MAX = (1 << 64) - 1
THRESHOLD_COUNTER = 0xFFFFFFFF00000000
QUANTILES = {2: (0.5,), 3: (0.3, 0.8), 5: (0.1, 0.35, 0.6, 0.9)}


def ppnd16(p):
    """Φ⁻¹(p): Wichura's AS241, routine PPND16, operation by operation as csrc/gibbs_common.h."""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        num = (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r
                   + 45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r
                + 133.14166789178437745) * r + 3.387132872796366608)
        den = (((((((r * 5226.495278852854561 + 28729.085735721942674) * r + 39307.89580009271061) * r
                   + 21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r
                + 42.313330701600911252) * r + 1.0)
        return q * num / den
    tail = p if q < 0.0 else 1.0 - p
    if tail <= 0.0:
        return -math.inf if q < 0.0 else math.inf
    r = math.sqrt(-math.log(tail))
    if r <= 5.0:
        r -= 1.6
        num = (((((((r * 7.7454501427834140764e-4 + 0.0227238449892691845833) * r + 0.24178072517745061177) * r
                   + 1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r
                + 4.6303378461565452959) * r + 1.42343711074968357734)
        den = (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r
                   + 0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r
                + 2.05319162663775882187) * r + 1.0)
    else:
        r -= 5.0
        num = (((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r
                   + 0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r
                + 5.4637849111641143699) * r + 6.6579046435011037772)
        den = (((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r
                   + 7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r
                + 0.59983220655588793769) * r + 1.0)
    val = num / den
    return -val if q < 0.0 else val


def phi(x):
    return 0.5 * math.erfc(-x * 0.7071067811865476)


def truncnorm(m, a, b, u):
    """TN(m; a, b; u) of include/gbm.h."""
    al, be = a - m, b - m
    refl = al >= 0.0
    if refl:
        al, be = -be, -al
    pa = phi(al)
    w = phi(be) - pa
    x = math.inf
    if w > 0.0:
        x = min(max(ppnd16(pa + u * w), al), be)
    if not math.isfinite(x):  # no mass, or pa + u w rounded to 0 or 1: the finite end nearer the mean
        x = be if abs(be) <= abs(al) else al
    return m - x if refl else m + x


def classes_of(y):
    """(class values, z, the start thresholds t_0 … t_K)."""
    values = np.unique(y)
    z = np.searchsorted(values, y)
    K, n = len(values), len(y)
    t = [-math.inf] + [ppnd16(float((z < k).sum()) / n) for k in range(1, K)] + [math.inf]
    return values, z, t


def ordinal_gibbs(model, X, y, n_iter, n_burnin, thin=5, r2=0.5, df0=5.0, prob_in=0.5, counts=10.0, seed=42):
    """Returns b_hat (p+1), y_pred (the liability), var = [1, mean_j varB_j, π] (posterior means), pip,
    classes, thresholds (posterior means of t_1 … t_{K−1}), probs (n x K), ``margin`` (the smallest
    |logOdds − logit(u)| of any indicator draw; inf for BayesA), ``gap`` (the smallest hi − lo of any
    threshold draw; inf for K = 2), t_start and t_end (the thresholds before and after the chain) and
    phi_pm (n x 2: the running means of Φ(t_1 − ŷ) and Φ(−(t_1 − ŷ)))."""
    assert model in MODELS
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    values, z, t = classes_of(y)
    K = len(values)
    assert 2 <= K <= 32
    t_start = list(t)
    members = [np.flatnonzero(z == k) for k in range(K)]
    ystar = np.array([truncnorm(0.0, t[z[i]], t[z[i] + 1], oracle.brr_u01(seed, U64_MAX, i)) for i in range(n)])
    cols = [np.ascontiguousarray(X[:, j]) for j in range(p)]
    x2 = (X * X).sum(axis=0)
    msx = x2.sum() / n - (X.mean(axis=0) ** 2).sum()
    vy = ystar.var(ddof=1)
    varE = 1.0
    S0 = vy * r2 / msx * (df0 + 2)
    if model != "BayesA":
        S0 = S0 / prob_in
    S = S0
    rate0 = (SHAPE0 - 1) / S0
    varB = np.full(p, S0 / (df0 + 2))
    pi, c_in, c_out = prob_in, counts * prob_in, counts * (1 - prob_in)
    mu = ystar.mean()
    e = ystar - mu
    b = np.zeros(p)
    d = np.ones(p)
    bbar, dbar = np.zeros(p), np.zeros(p)
    tbar = np.zeros(K + 1)
    pbar = np.zeros((n, K))
    phi_pm = np.zeros((n, 2))
    mubar = varBbar = pibar = 0.0
    nsum = 0
    margin = gap = math.inf
    for it in range(n_iter):
        A = 8 * it
        i1 = it + 1
        gated = i1 % thin == 0 and i1 > n_burnin
        k = float(nsum + 1)
        w0, w1 = (k - 1) / k, 1 / k
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
        # (a) the liabilities
        yhat = ystar - e
        for i in range(n):
            ystar[i] = truncnorm(yhat[i], t[z[i]], t[z[i] + 1], oracle.brr_u01(seed, A + 7, i))
        e = ystar - yhat
        # (b) the thresholds t_2 … t_{K−1}
        for m in range(2, K):
            lo = max(ystar[members[m - 1]].max(), t[m - 1])
            hi = min(ystar[members[m]].min(), t[m + 1])
            gap = min(gap, hi - lo)
            t[m] = lo + (hi - lo) * oracle.brr_u01(seed, A + 7, THRESHOLD_COUNTER + m)
        # (c) their running means and the class probabilities'
        if gated:
            for m in range(1, K):
                tbar[m] = tbar[m] * w0 + t[m] * w1
            for i in range(n):
                prev = 0.0
                for c in range(K):
                    nxt = phi(t[c + 1] - yhat[i]) if c + 1 < K else 1.0
                    pbar[i, c] = pbar[i, c] * w0 + (nxt - prev) * w1
                    prev = nxt
                phi_pm[i, 0] = phi_pm[i, 0] * w0 + phi(t[1] - yhat[i]) * w1
                phi_pm[i, 1] = phi_pm[i, 1] * w0 + phi(-(t[1] - yhat[i])) * w1
        # 3. variances (varE stays 1)
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
        # 4. running means
        if gated:
            nsum += 1
            bbar = bbar * w0 + (d * b) * w1
            dbar = dbar * w0 + d * w1
            mubar = mubar * w0 + mu * w1
            varBbar = varBbar * w0 + varB.mean() * w1
            pibar = pibar * w0 + pi * w1
    return {"b_hat": np.concatenate([[mubar], bbar]), "y_pred": mubar + X @ bbar,
            "var": np.array([1.0, varBbar, pibar]), "pip": dbar, "classes": values,
            "thresholds": tbar[1:K].copy(), "probs": pbar, "margin": margin, "gap": gap,
            "t_start": t_start, "t_end": list(t), "phi_pm": phi_pm}


@functools.lru_cache(maxsize=None)
def ordinal_case(n, p, K, scale=False):
    """tests/bayes_abc_ref.py's same-path data with y cut into K classes at fixed quantiles."""
    X, y = path_case(n, p, None, scale)
    cls = np.searchsorted(np.quantile(y, QUANTILES[K]), y).astype(np.float64)
    cls.setflags(write=False)
    return X, cls


@functools.lru_cache(maxsize=None)
def ordinal_path_ref(model, n, p, iters, K, scale=False, n_burnin=2, thin=1, seed=99):
    X, cls = ordinal_case(n, p, K, scale)
    return ordinal_gibbs(model, X, cls, n_iter=iters, n_burnin=n_burnin, thin=thin, seed=seed)


# ---- recovery: the sparse case's liability cut into four classes --------------------------------
SPARSE_CUTS = (-0.8, 0.1, 1.0)  # in standard deviations of the liability around its mean


@functools.lru_cache(maxsize=None)
def sparse_ordinal_case(permuted=False):
    """sparse_case()'s eight QTL; its phenotype g + noise is the liability, cut at SPARSE_CUTS. ``permuted``:
    the same classes dealt to the individuals at random (no signal: what the bounds are set against)."""
    X, y, g, qtl = sparse_case()
    lz = (y - y.mean()) / y.std(ddof=1)
    cls = np.searchsorted(np.array(SPARSE_CUTS), lz).astype(np.float64)
    if permuted:
        cls = np.random.default_rng(11).permutation(cls)
    return X, cls, g, qtl


def sparse_figures(y_pred, pip, thresholds):
    """cor(ŷ, g), the mean PIP at the QTL and elsewhere, and the largest error of the thresholds on the
    liability's own scale: (t̄_k − mean ŷ)/sqrt(var ŷ + 1) against SPARSE_CUTS (the fitted liability has
    variance var ŷ + 1)."""
    X, cls, g, qtl = sparse_ordinal_case()
    rest = np.setdiff1d(np.arange(X.shape[1]), qtl)
    sd = math.sqrt(y_pred.var(ddof=1) + 1.0)
    thr = (np.asarray(thresholds) - y_pred.mean()) / sd
    return {"cor": float(np.corrcoef(y_pred, g)[0, 1]), "pip_qtl": float(pip[qtl].mean()),
            "pip_rest": float(pip[rest].mean()), "thr_err": float(np.abs(thr - np.array(SPARSE_CUTS)).max())}
