"""The reference of the PSIS-LOO predictive calibration tests (tests/README.loo_predictive.md): the weight rule of amwg_last_sample_dataset_loo_predictive
(include/amwg.h) in numpy longdouble over one column of fp64 terms, starting from the fp64 excesses that loo_reference pins, and the weighted means over the exact
rows of predictive_reference in mpmath."""
import math

import mpmath as mp
import numpy as np

import loo_reference as lr
import predictive_reference as pr
import waic_reference as wr

T = np.longdouble


def keys(col):
    b = np.ascontiguousarray(col, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ np.uint64(1 << 63))


def smoothed(a, M):
    """(khat, lw~ [M] by rank r = 1 ... M, B + sum_r exp(lw~_r)) of the sorted terms a, or None on the raw route: the fit and the smoothing of loo_reference.point,
    which keeps lw~ to itself"""
    if M < 5:
        return None
    ec, x, _ = lr.excesses(a, M)
    mm, xs, xM = lr.thetas(M), x[(M + 2) // 4 - 1], x[M - 1]
    if not xs > 0 or not xM > 0:
        return None
    with np.errstate(all="ignore"):
        x, xs, xM, ec = x.astype(T), T(xs), T(xM), T(ec)
        theta = 1 / xM + (1 - np.sqrt(T(mm) / (np.arange(1, mm + 1).astype(T) - T(0.5)))) / (3 * xs)
        k = np.log1p(-theta[:, None] * x[None, :]).sum(axis=1) / T(M)
        L = T(M) * (np.log(-theta / k) - k - 1)
        th = (theta / np.exp(L[:, None] - L[None, :]).sum(axis=0)).sum()
        kp = np.log1p(-th * x).sum() / T(M)
        sigma, khat = -kp / th, (T(M) * kp + 5) / (T(M) + 10)
        if not np.isfinite(khat):
            return None
        lp = np.log1p(-((np.arange(1, M + 1).astype(T) - T(0.5)) / T(M)))
        lwt = np.minimum(np.log((-sigma * lp if khat == 0 else sigma * np.expm1(-khat * lp) / khat) + ec), T(0))
        return khat, lwt, np.exp(a.astype(T)[0] - a.astype(T)[M:]).sum() + np.exp(lwt).sum()


def weights(col):
    """one observation's finite terms col [S] -> (w [S] longdouble in draw order, khat, LOO's denominator): a class average over sorted positions"""
    col = np.ascontiguousarray(col, dtype=np.float64)
    M, key = lr.tail_len(len(col)), keys(col)
    order = np.argsort(key, kind="stable")
    a, ks = col[order], key[order]
    w = np.exp(T(a[0]) - col.astype(T))
    fit = smoothed(a, M)
    if fit is None:
        return w, np.inf, w.sum()
    sm = np.exp(fit[1][::-1])      # by sorted position t < M: rank M - t
    for k in np.unique(ks[:M]):
        pos = np.flatnonzero(ks == k)
        below = pos[pos < M]
        w[order[pos]] = (sm[below].sum() + (len(pos) - len(below)) * np.exp(T(a[0]) - T(a[pos[0]]))) / len(pos)
    return w, float(fit[0]), fit[2]


def brute_weights(col):
    """the rule once more, draw by draw in plain loops: the weight of draw s from the sorted positions that hold its key"""
    col = [float(v) for v in col]
    S, M = len(col), lr.tail_len(len(col))
    a = lr.key_sort(col)
    fit = smoothed(a, M)
    out = []
    for s in range(S):
        same = [t for t in range(S) if a[t] == col[s] and math.copysign(1, a[t]) == math.copysign(1, col[s])]
        below = [t for t in same if t < M]
        if fit is None or not below:
            out.append(np.exp(T(a[0]) - T(col[s])))
            continue
        total = T(0)
        for t in below:
            total = total + np.exp(fit[1][M - t - 1])
        out.append((total + (len(same) - len(below)) * np.exp(T(a[0]) - T(col[s]))) / len(same))
    return np.array(out, dtype=T)


def to_mp(v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - T(hi)))


def pointwise(spec, sd, ll):
    """-> (values [n][5] = pit_hi, pit_lo, pred_mean, pred_sd, khat; bounds [n][4], the last on pred_sd^2) from the dataset's draws sd [S][PR] and its fp64 terms
    ll [S][n]; NaN rows where a term or a functional is not finite.  Bounds: predictive_reference's forms with the weighted mean of the distribution function's
    bound, plus 4 ln(2 M) E_k (loo_reference.bounds)"""
    S, M, model = len(sd), lr.tail_len(len(sd)), spec["model"]
    E = 8.0 * (S + 16) * wr.U
    vals, tols = np.full((spec["n_obs"], 5), np.nan), np.full((spec["n_obs"], 4), np.nan)
    for j, col in enumerate(pr.rows_of(spec, sd)):
        if not np.isfinite(ll[:, j]).all() or any(mp.isnan(v) or mp.isinf(v) for t in col for v in t):
            continue
        w, khat, _ = weights(ll[:, j])
        w = [to_mp(v) for v in w]
        W = mp.fsum(w)
        hi, lo, mean = (mp.fsum(wi * t[k] for wi, t in zip(w, col)) / W for k in range(3))
        var = mp.fsum(wi * (t[3] + (t[2] - mean) ** 2) for wi, t in zip(w, col)) / W
        cdf = [0.0, 0.0] if model == "beta_bern" else [pr.ERFC_REL, pr.ERFC_REL]
        if model == "pois_glm":
            cdf = [float(mp.fsum(wi * pr.POIS_REL * min(t[k], 1 - t[k]) for wi, t in zip(w, col)) / W) + wr.U for k in range(2)]
        extra = 4 * math.log(max(2 * M, 2)) * float(lr.bounds(S, 0.0, np.float64(khat))[1])
        vals[j] = [float(hi), float(lo), float(mean), float(mp.sqrt(var)), khat]
        tols[j] = [E + cdf[0] + extra, E + cdf[1] + extra, E * float(max(abs(t[2]) for t in col)) + extra,
                   4 * E * float(max(t[3] for t in col) + max(t[2] ** 2 for t in col)) + extra]
    return vals, tols
