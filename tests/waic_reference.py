"""The reference of the WAIC tests (tests/test_waic_host.py, tests/test_gpu_waic.py; tests/README.waic.md).

The pointwise terms l_si come from the host twins the project pins against V8 -- amwg_log, amwg_exp (libamwg.so) and amwg_ld_host (libamwg_selftest.so) -- with the
reference's operations in the reference's order, one IEEE rounding each (numpy's elementwise fp64: no fused operation).  lppd_i and p_i are computed from those
doubles in extended precision (numpy longdouble: 64 significand bits here, so its own error, about 2^-64 S relative, is 2^-11 of the bounds below)."""
import math

import numpy as np

import amwg_ctypes

U = 2.0 ** -53
LD_NORM, LD_BERN, LD_LFACTORIAL = 0, 3, 19      # ids of amwg_ld_host (include/amwg_selftest.h)


def _map(fn, a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([fn(float(v)) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def v8_log(a):
    return _map(amwg_ctypes.lib().amwg_log, a)


def v8_exp(a):
    return _map(amwg_ctypes.lib().amwg_exp, a)


def ld_host(ld_id, x, a=0.0, b=0.0, c=0.0):
    return amwg_ctypes.selftest_lib().amwg_ld_host(ld_id, float(x), float(a), float(b), float(c))


# ---- the terms, [S][n], draw s = row * cpd + chain

def loglik_normal(x, mu, sigma):
    """ld.norm(x_i, mu_s, sigma_s) = -0.5 log(2 pi) - log(sd) - (t t) / (2 sd sd), left to right"""
    x, mu, sigma = (np.asarray(v, dtype=np.float64) for v in (x, mu, sigma))
    with np.errstate(all="ignore"):
        c = (-0.5 * v8_log(2 * math.pi)) - v8_log(sigma)
        den = (2 * sigma) * sigma
        t = x[None, :] - mu[:, None]
        return c[:, None] - (t * t) / den[:, None]


def loglik_hier(y, g, theta, sigma):
    """ld.norm(y_i, theta_s[g_i], sigma_s); theta [S][G]"""
    y, theta, sigma = (np.asarray(v, dtype=np.float64) for v in (y, theta, sigma))
    with np.errstate(all="ignore"):
        c = (-0.5 * v8_log(2 * math.pi)) - v8_log(sigma)
        den = (2 * sigma) * sigma
        t = y[None, :] - theta[:, np.asarray(g, dtype=np.int64)]
        return c[:, None] - (t * t) / den[:, None]


def loglik_bern(x, theta):
    """ld.bern(x_i, theta_s) = log(x p + (1 - x)(1 - p)): log(p) at x = 1, log(1 - p) at x = 0, -inf for any other x"""
    x, theta = np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    with np.errstate(all="ignore"):
        l1, l0 = v8_log(theta), v8_log(1 - theta)
    out = np.full((theta.size, x.size), -np.inf)
    out[:, x == 1] = l1[:, None]
    out[:, x == 0] = l0[:, None]
    return out


def loglik_pois(X, y, beta, cp):
    """ld.pois(y_i, exp(eta)) = log(lambda) y - lambda - lfactorial(y); eta = X[i][0] b[0] + ... + X[i][6] b[6] in that order, + b[7] from i >= cp on.
    X [n][7], beta [S][8], cp [S]"""
    X, y, beta, cp = (np.asarray(v, dtype=np.float64) for v in (X, y, beta, cp))
    n = y.size
    X = X.reshape(n, 7)
    with np.errstate(all="ignore"):
        eta = X[None, :, 0] * beta[:, None, 0]
        for k in range(1, 7):
            eta = eta + X[None, :, k] * beta[:, None, k]
        late = np.arange(n)[None, :] >= cp[:, None]
        eta = np.where(late, eta + beta[:, None, 7], eta)
        lam = v8_exp(eta)
        lg = v8_log(lam)
        lf = np.array([math.inf if v < 0 else ld_host(LD_LFACTORIAL, v) for v in y])
        return lg * y[None, :] - lam - lf[None, :]


def draws_of_dataset(draws, D, d):
    """draws [rows][PR][C] -> dataset d's [S][PR] in draw order s = row * cpd + chain"""
    rows, PR, C = draws.shape
    cpd = C // D
    return np.ascontiguousarray(draws[:, :, d * cpd:(d + 1) * cpd].transpose(0, 2, 1).reshape(rows * cpd, PR))


def loglik_of(spec, sd):
    """the terms of one dataset's spec (model, data) under its draws sd [S][PR]"""
    data, model = spec["data"], spec["model"]
    if model == "normal":
        return loglik_normal(data["x"], sd[:, 0], sd[:, 1])
    if model == "beta_bern":
        return loglik_bern(data["x"], sd[:, 0])
    if model == "hier_normal":
        G = int(spec["G"])
        return loglik_hier(data["x"], data["g"], sd[:, :G], sd[:, G + 1])
    return loglik_pois(data["x"], data["y"], sd[:, :8], sd[:, 8])


# ---- lppd_i, p_i and the bounds

def pointwise(ll):
    """ll [S][n] -> (lppd [n], p [n], mean [n], maxabs [n]) in extended precision; NaN where a term of the column is not finite"""
    ll = np.asarray(ll, dtype=np.float64)
    S, n = ll.shape
    ok = np.isfinite(ll).all(axis=0)
    q = np.where(ok[None, :], ll, 0.0).astype(np.longdouble)
    m = q.max(axis=0)
    lppd = m + np.log(np.exp(q - m[None, :]).sum(axis=0)) - np.log(np.longdouble(S))
    mean = q.sum(axis=0) / np.longdouble(S)
    dev = q - mean[None, :]
    p = (dev * dev).sum(axis=0) / np.longdouble(S - 1)
    nan = np.where(ok, 0.0, np.nan)
    return lppd.astype(np.float64) + nan, p.astype(np.float64) + nan, mean.astype(np.float64), np.abs(ll).max(axis=0)


def bounds(S, lppd, p, mean, maxabs):
    """the error bounds of include/amwg.h: u = 2^-53, E = 8 (S + 16) u"""
    E = 8.0 * (S + 16) * U
    with np.errstate(all="ignore"):
        return E + 4 * U * np.abs(lppd), E * np.sqrt(p * (p + mean * mean)) + (E * maxabs) ** 2


def one_pass_p(ll):
    """the scheme the cancellation case must defeat: (sum l^2 - (sum l)^2 / S) / (S - 1) in fp64"""
    ll = np.asarray(ll, dtype=np.float64)
    S = ll.shape[0]
    s1 = s2 = np.zeros(ll.shape[1])
    for s in range(S):
        s1 = s1 + ll[s]
        s2 = s2 + ll[s] * ll[s]
    return (s2 - s1 * s1 / S) / (S - 1)


def worst_ratio(got_pw, ll):
    """got_pw [n][2] against the exact values of ll [S][n] -> (largest |lppd error| / bound, largest |p error| / bound); the NaN pattern must be the reference's"""
    S = ll.shape[0]
    lppd, p, mean, maxabs = pointwise(ll)
    bl, bp = bounds(S, lppd, p, mean, maxabs)
    got_pw = np.asarray(got_pw)
    nan = np.isnan(lppd)
    assert (np.isnan(got_pw[:, 0]) == nan).all() and (np.isnan(got_pw[:, 1]) == nan).all(), "the NaN pattern differs from the reference's"
    if nan.all():
        return 0.0, 0.0
    k = ~nan
    with np.errstate(all="ignore"):
        rl = np.abs(got_pw[k, 0] - lppd[k]) / bl[k]
        rp = np.where(got_pw[k, 1] == p[k], 0.0, np.abs(got_pw[k, 1] - p[k]) / bp[k])
    return float(rl.max()), float(rp.max())


def self_check():
    """the reference against closed forms and against amwg_ld_host; raises AssertionError"""
    S, a, b = 64, -1.25, -3.5
    same = np.full((S, 3), a)
    lppd, p, _, _ = pointwise(same)
    assert (lppd == a).all() and (p == 0.0).all()
    two = np.where((np.arange(S) % 2 == 0)[:, None], a, b) * np.ones((S, 2))
    lppd, p, _, _ = pointwise(two)
    assert np.allclose(lppd, math.log((math.exp(a) + math.exp(b)) / 2), rtol=0, atol=4 * U * 4) and np.allclose(p, S / (S - 1) * (a - b) ** 2 / 4, rtol=4 * U, atol=0)
    lppd, p, _, _ = pointwise(np.array([[0.0, -np.inf], [1.0, 2.0]]))
    assert np.isnan(lppd[1]) and np.isnan(p[1]) and not np.isnan(lppd[0])
    rng = np.random.default_rng(5)
    x, mu, sg = rng.normal(size=7), rng.normal(size=5), rng.uniform(0.5, 2, size=5)
    ll = loglik_normal(x, mu, sg)
    for s in range(5):
        for i in range(7):
            assert ll[s, i].tobytes() == np.float64(ld_host(LD_NORM, x[i], mu[s], sg[s])).tobytes()
    xb, th = np.array([1.0, 0.0, 1.0, 0.5]), rng.uniform(0.1, 0.9, size=4)
    lb = loglik_bern(xb, th)
    for s in range(4):
        for i in range(4):
            assert lb[s, i].tobytes() == np.float64(ld_host(LD_BERN, xb[i], th[s])).tobytes()
    # the Poisson term against ld.pois of the host twin at lambda = exp(eta)
    X, y = rng.normal(size=(6, 7)) * 0.3, np.array([0.0, 1, 2, 5, 3, 1])
    beta, cp = rng.normal(size=(3, 8)) * 0.2, np.array([0.0, 3.0, 2.5])
    lp = loglik_pois(X, y, beta, cp)
    for s in range(3):
        for i in range(6):
            eta = X[i, 0] * beta[s, 0]
            for k in range(1, 7):
                eta = eta + X[i, k] * beta[s, k]
            if i >= cp[s]:
                eta = eta + beta[s, 7]
            assert lp[s, i].tobytes() == np.float64(ld_host(4, y[i], amwg_ctypes.lib().amwg_exp(float(eta)))).tobytes()
