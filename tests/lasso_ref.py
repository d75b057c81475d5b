"""The elastic-net path of include/gbm.h (gbm_session_enet_path) as a literal numpy loop: one marker at a
time, the dots taken directly from the centred columns, the same admission order, per-pass stopping rule
and early stop as the device schedule. The checker of tests/test_lasso.py, tests/test_gpu_lasso.py and, through
tests/lasso_cases.py, tests/test_gpu_lasso_edges.py (test infrastructure, not the product)."""
import numpy as np


def enet_path(X, y, lambdas, alpha=1.0, tol=1e-7, max_passes=1_000_000, dev_max=np.inf, fdev=0.0, tie=0.0):
    """Returns dict(b_path (p+1, nl_done), lambdas, dev_ratio, passes, nnz, nl_done, active (the list at the
    end, in order of admission), nactive (its length after each λ), margin (the smallest
    | |g_j| − thr | / thr over the inactive j of every screen after the first λ), margin0 (the same over the
    screens of the first λ, against the threshold they used), stop_margin (the smallest
    | dmax − tol σ_y² | / (tol σ_y²) over every pass of every λ: how far the stopping rule's closest decision
    lies from its threshold), admits (one (k, list length before, markers admitted) per non-empty admission), hit
    (max_passes reached), first_hit (the first λ, from 0, that reached it; −1 if none)).

    ``tie``: the screens of the first λ admit |g_j| > thr (1 + tie). A path that starts at λ_max itself has
    |g_j| = thr for the marker that defines λ_max, up to the rounding of two different sums: either side is
    the stated schedule. tie = ±1e-9 takes one side on purpose; 0 is the plain rule."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    lambdas = np.atleast_1d(np.asarray(lambdas, dtype=np.float64))
    n, p = X.shape
    mean = X.mean(axis=0)
    Xc = np.asfortranarray(X - mean)
    x2 = (Xc * Xc).sum(axis=0)
    ym = y.mean()
    ys = np.sqrt(((y - ym) ** 2).sum() / n)
    yss = ((y - ym) ** 2).sum()
    e = y - ym
    b = np.zeros(p)
    active = np.zeros(p, dtype=bool)
    act = []
    nl = lambdas.size
    mnl = min(5, nl)
    out_b, dev, passes_out, nnz, nact = [], [], [], [], []
    margin, margin0, stop_margin, hit_any, dev_prev = np.inf, np.inf, np.inf, False, 0.0
    admits, first_hit = [], -1
    for k, lam in enumerate(lambdas):
        thr = n * lam * alpha
        l2 = n * lam * (1.0 - alpha) / ys
        passes, hit = 0, False
        while True:
            while act:
                if passes >= max_passes:
                    hit = True
                    break
                dmax = 0.0
                for j in act:
                    xj = Xc[:, j]
                    g = xj @ e + x2[j] * b[j]
                    bn = np.sign(g) * max(abs(g) - thr, 0.0) / (x2[j] + l2)
                    d = b[j] - bn
                    if d != 0.0:
                        e += d * xj
                        b[j] = bn
                    dmax = max(dmax, x2[j] * d * d / n)
                passes += 1
                stop_margin = min(stop_margin, abs(dmax - tol * ys * ys) / (tol * ys * ys))
                if dmax < tol * ys * ys:
                    break
            if hit:
                break
            g = Xc.T @ e
            cand = ~active & (x2 > 0.0)
            thr_s = thr * (1.0 + tie) if k == 0 else thr
            if k > 0 and cand.any():
                margin = min(margin, np.abs(np.abs(g[cand]) - thr).min() / thr)
            elif cand.any():
                margin0 = min(margin0, np.abs(np.abs(g[cand]) - thr_s).min() / thr_s)
            new = np.flatnonzero(cand & (np.abs(g) > thr_s))
            if new.size == 0:
                break
            admits.append((k, len(act), int(new.size)))
            active[new] = True
            act.extend(int(j) for j in new)
        hit_any |= hit
        if hit and first_hit < 0:
            first_hit = k
        out_b.append(np.concatenate([[ym - mean @ b], b]))
        d = 1.0 - (e @ e) / yss
        dev.append(d)
        passes_out.append(passes)
        nnz.append(int(np.count_nonzero(b)))
        nact.append(len(act))
        if k + 1 >= mnl and (d > dev_max or (fdev > 0.0 and d - dev_prev < fdev * d)):
            break
        dev_prev = d
    done = len(dev)
    return {"b_path": np.array(out_b).T, "lambdas": lambdas[:done].copy(), "dev_ratio": np.array(dev),
            "passes": np.array(passes_out), "nnz": np.array(nnz), "nl_done": done, "active": list(act),
            "nactive": np.array(nact), "margin": margin, "margin0": margin0, "stop_margin": stop_margin,
            "admits": admits, "hit": hit_any, "first_hit": first_hit}


def kkt_residual(X, y, lam, alpha, b):
    """The KKT residual of slopes b (p,) at λ, divided by nλ: |x_jᵀe − nλ(1−α)b_j/σ_y − thr·sign b_j| on the
    support and max(|x_jᵀe| − thr, 0) off it (columns with x2 = 0 excluded), e = y − ȳ − X_c b."""
    n = X.shape[0]
    Xc = X - X.mean(axis=0)
    ym = y.mean()
    ys = np.sqrt(((y - ym) ** 2).sum() / n)
    e = (y - ym) - Xc @ b
    g = Xc.T @ e
    thr = n * lam * alpha
    on = b != 0.0
    r = np.where(on, np.abs(g - n * lam * (1.0 - alpha) * b / ys - thr * np.sign(b)), np.maximum(np.abs(g) - thr, 0.0))
    r[(Xc * Xc).sum(axis=0) == 0.0] = 0.0
    return r.max() / (n * lam)


def lambda_path(X, y, alpha, nl, ratio):
    """nl λ from glmnet's λ_max = max_j |x_cjᵀ(y − ȳ)|/(n max(α, 1e-3)) down to ratio·λ_max (log-spaced)."""
    Xc = X - X.mean(axis=0)
    lmax = np.abs(Xc.T @ (y - y.mean())).max() / X.shape[0] / max(alpha, 1e-3)
    return lmax * ratio ** (np.arange(nl) / (nl - 1))


def enet_path_cv(X, y, folds, alpha=1.0, nlambda=100, lambda_min_ratio=0.01, tol=1e-7):
    """gbm.enet_path_cv with this loop: the full path with glmnet's early stop, every fold at the λ kept with
    the stop off."""
    lam = lambda_path(X, y, alpha, nlambda, lambda_min_ratio)
    full = enet_path(X, y, lam, alpha=alpha, tol=tol, dev_max=0.999, fdev=1e-5)
    lam = full["lambdas"]
    nf = int(folds.max())
    loss = np.zeros((lam.size, nf))
    for f in range(1, nf + 1):
        tr, ho = folds != f, folds == f
        r = enet_path(X[tr], y[tr], lam, alpha=alpha, tol=tol)
        pred = r["b_path"][0][None, :] + X[ho] @ r["b_path"][1:]
        loss[:, f - 1] = ((pred - y[ho, None]) ** 2).mean(axis=0)
    return {"lambda": lam, "a0": full["b_path"][0], "betas": full["b_path"][1:], "meanloss": loss.mean(axis=1)}


def planted(seed, n, p, k):
    """A planted design: k common-allele columns (the support S, effects ±[2, 3]) among p − k rare-allele
    columns, y = 0.5 + X_S b_S without noise, so that a lasso at 0.1 λ_max admits S and nothing else.
    Returns (X, y, S)."""
    rng = np.random.default_rng(seed)
    S = np.sort(rng.choice(p, k, replace=False))
    X = rng.binomial(2, 0.01, (n, p)) / 2.0
    X[0, :] = 0.5  # every column varies
    X[:, S] = rng.binomial(2, 0.5, (n, k)) / 2.0
    b = np.zeros(p)
    b[S] = rng.choice([-1.0, 1.0], k) * rng.uniform(2.0, 3.0, k)
    return X, 0.5 + X @ b, S
