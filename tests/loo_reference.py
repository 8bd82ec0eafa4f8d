"""The reference of the PSIS-LOO tests (tests/test_loo_host.py, tests/test_gpu_loo.py; tests/README.loo.md).

The rule of include/amwg.h (amwg_last_sample_dataset_loo) stated twice over one column of terms l_s (the doubles of waic_reference.loglik_of, or the device's own
from waic_check(loglik=True)): once in numpy fp64, once in numpy longdouble (64 significand bits here).  Both start from the SAME fp64 excesses x_r -- the rule pins
them to the bit: exp through amwg_exp of the host library -- so that the cancellation near the cutoff is in neither error.  The cases of the GPU test are built
here, so that the host test measures the fp64 restatement over the very same columns."""
import math

import numpy as np

import amwg_ctypes
import waic_reference as wr
from waic_reference import loglik_of      # noqa: F401  (the terms of a dataset's spec under its draws: the tests take them from here)

U = wr.U
SEED = 20261021


def tail_len(S):
    """M = min(S // 5, m3), m3 the smallest integer with m3^2 >= 9 S"""
    S = int(S)
    m3 = math.isqrt(9 * S)
    if m3 * m3 < 9 * S:
        m3 += 1
    return min(S // 5, m3)


def thetas(M):
    return 30 + math.isqrt(M)


def key_sort(col):
    """ascending by the key order of doubles: -0.0 before +0.0 (np.sort leaves that pair in any order)"""
    col = np.ascontiguousarray(col, dtype=np.float64)
    b = col.view(np.uint64)
    key = np.where(b >> np.uint64(63) != 0, ~b, b ^ np.uint64(1 << 63))
    return col[np.argsort(key, kind="stable")]


def excesses(a, M):
    """the pinned part: (ec, x [M] ascending, lw [M]) from the sorted terms; fp64, exp = amwg_exp"""
    a0 = a[0]
    ec = wr.v8_exp(a0 - a[M])
    lw = a0 - a[M - 1::-1][:M]      # r = 1 ... M: a_0 - a_{M - r}
    x = wr.v8_exp(lw) - ec
    return float(ec), x, lw


def point(col, T):
    """one observation's (elpd_loo_i, khat_i) from its S finite terms, the sums in type T (np.float64 or np.longdouble)"""
    S = len(col)
    M = tail_len(S)
    a = key_sort(col)
    aT = a.astype(T)
    a0 = aT[0]
    with np.errstate(all="ignore"):
        def raw():
            return a0 + np.log(T(S)) - np.log(np.exp(a0 - aT).sum()), np.inf
        if M < 5:
            return raw()
        ec, x, _ = excesses(a, M)
        mm = thetas(M)
        xs, xM = x[(M + 2) // 4 - 1], x[M - 1]
        if not xs > 0 or not xM > 0:
            return raw()
        x, xs, xM, ec = x.astype(T), T(xs), T(xM), T(ec)
        j = np.arange(1, mm + 1).astype(T)
        theta = 1 / xM + (1 - np.sqrt(T(mm) / (j - T(0.5)))) / (3 * xs)
        k = np.log1p(-theta[:, None] * x[None, :]).sum(axis=1) / T(M)
        L = T(M) * (np.log(-theta / k) - k - 1)
        w = 1 / np.exp(L[:, None] - L[None, :]).sum(axis=0)
        th = (theta * w).sum()
        kp = np.log1p(-th * x).sum() / T(M)
        sigma = -kp / th
        khat = (T(M) * kp + 5) / (T(M) + 10)
        if not np.isfinite(khat):
            return raw()
        r = np.arange(1, M + 1).astype(T)
        lp = np.log1p(-((r - T(0.5)) / T(M)))
        q = -sigma * lp if khat == 0 else sigma * np.expm1(-khat * lp) / khat
        lwt = np.minimum(np.log(q + ec), T(0))
        lw = a0 - aT[M - 1::-1][:M]
        B = np.exp(a0 - aT[M:]).sum()
        return a0 + np.log(T(S - M) + np.exp(lwt - lw).sum()) - np.log(B + np.exp(lwt).sum()), khat


def pointwise(ll, T=np.longdouble):
    """ll [S][n] -> (elpd_loo [n], khat [n]) as fp64; NaN where a term of the column is not finite"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.shape[1]
    elpd, khat = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        if np.isfinite(ll[:, i]).all():
            e, k = point(ll[:, i], T)
            elpd[i], khat[i] = float(e), float(k)
    return elpd, khat


def tails(ll):
    """ll [S][n] -> [n][M + 1], the sorted smallest terms of each column"""
    M = tail_len(ll.shape[0])
    return np.stack([key_sort(ll[:, i])[:M + 1] for i in range(ll.shape[1])])


def bounds(S, elpd, khat):
    """the bounds of include/amwg.h: E_k = M (M + mm) u (1 + |khat|), E (1 + |elpd|) + 4 ln(2 M) E_k with E = 8 (S + 16) u; khat = +inf (no fit): no E_k"""
    M = tail_len(S)
    E = 8.0 * (S + 16) * U
    fit = np.isfinite(khat)
    Ek = np.where(fit, M * (M + thetas(M)) * U * (1 + np.abs(np.where(fit, khat, 0.0))), 0.0)
    return E * (1 + np.abs(elpd)) + 4 * math.log(max(2 * M, 2)) * Ek, Ek


def ratios(elpd, khat, ref_elpd, ref_khat, S):
    """(largest |elpd error| / bound, largest |khat error| / bound); the NaN pattern and the +inf pattern of khat must be the reference's"""
    elpd, khat = np.asarray(elpd, dtype=np.float64), np.asarray(khat, dtype=np.float64)
    nan = np.isnan(ref_elpd)
    assert (np.isnan(elpd) == nan).all() and (np.isnan(khat) == nan).all(), "the NaN pattern differs from the reference's"
    k = ~nan
    if not k.any():
        return 0.0, 0.0
    inf = np.isinf(ref_khat[k])
    assert ((khat[k] == np.inf) == inf).all(), "khat = +inf (no fit) where the reference fits, or the reverse"
    be, bk = bounds(S, ref_elpd[k], ref_khat[k])
    re = np.abs(elpd[k] - ref_elpd[k]) / be
    rk = np.where(inf, 0.0, np.abs(np.where(inf, 0.0, khat[k]) - np.where(inf, 0.0, ref_khat[k])) / np.where(inf, 1.0, bk))
    return float(re.max()), float(rk.max())


# ---- the cases of tests/test_gpu_loo.py: (name, draws [rows][PR][C], specs)

N_OBS = [1, 2, 63, 64, 65, 257]
SHAPES = [(2, 1), (1, 3), (8, 3), (25, 1), (75, 3), (226, 1), (5, 65), (17, 64), (64, 64)]      # S = 2, 3 (M = 0), 24 (M = 4), 25 (M = 5), 225, 226, 325, 1088, 4096


def spec_of(model, n, rng, G=5):
    if model == "normal":
        return {"model": model, "n_obs": n, "data": {"x": rng.normal(1.0, 1.5, size=n)}}
    if model == "beta_bern":
        return {"model": model, "n_obs": n, "data": {"x": (rng.uniform(size=n) < 0.4).astype(np.float64)}}
    if model == "hier_normal":
        return {"model": model, "n_obs": n, "G": G, "data": {"x": rng.normal(0.0, 2.0, size=n), "g": rng.integers(0, G, size=n).astype(np.int32)}}
    X = rng.normal(0.0, 0.4, size=(n, 7))
    return {"model": model, "n_obs": n, "K": 7, "data": {"x": X.reshape(-1), "y": rng.poisson(2.0, size=n).astype(np.float64)}}


def draws_for(model, rows, C, rng, n_obs=10, G=5):
    """posterior-like draws [rows][PR][C] of a family"""
    if model == "normal":
        return np.stack([rng.normal(1.0, 0.3, size=(rows, C)), rng.uniform(0.8, 2.5, size=(rows, C))], axis=1)
    if model == "beta_bern":
        return rng.uniform(0.05, 0.95, size=(rows, 1, C))
    if model == "hier_normal":
        return np.concatenate([rng.normal(0.0, 1.0, size=(rows, G, C)), rng.normal(size=(rows, 1, C)), rng.uniform(1.0, 3.0, size=(rows, 1, C))], axis=1)
    return np.concatenate([rng.normal(0.0, 0.3, size=(rows, 8, C)), rng.uniform(-1.0, n_obs + 1.0, size=(rows, 1, C))], axis=1)


def shape_case(k):
    """Normal, three ragged datasets, the sizes rotating through N_OBS"""
    rows, cpd = SHAPES[k]
    rng = np.random.default_rng(SEED + k)
    sizes = [N_OBS[k % 6], N_OBS[(k + 2) % 6], N_OBS[(k + 4) % 6]]
    specs = [spec_of("normal", n, rng) for n in sizes]
    return draws_for("normal", rows, 3 * cpd, rng), specs


FAMILY_SHAPES = [(25, 1), (5, 65), (17, 64)]


def family_case(model, rows, cpd):
    rng = np.random.default_rng(SEED + 100 + rows)
    D = 1 if model == "hier_normal" else 3
    sizes = {25: [65, 2, 63], 5: [1, 64, 130], 17: [63, 2, 70]}[rows][:D]
    specs = [spec_of(model, n, rng) for n in sizes]
    if model == "beta_bern":
        specs[0]["data"]["x"][0] = 0.5      # an invalid observation: -inf in every draw
    return draws_for(model, rows, D * cpd, rng, n_obs=max(sizes)), specs


def normal_case(x, mu, sigma, rows):
    """one Normal dataset under the draws (mu_s, sigma_s), s in draw order"""
    S = len(mu)
    cpd = S // rows
    assert cpd * rows == S
    draws = np.stack([np.asarray(mu, dtype=np.float64).reshape(rows, cpd), np.asarray(sigma, dtype=np.float64).reshape(rows, cpd)], axis=1)
    return draws, [{"model": "normal", "n_obs": len(x), "data": {"x": np.asarray(x, dtype=np.float64)}}]


PATTERNS = ["identical", "ties_of_ten", "a_tie_wider_than_the_tail", "dominating_first", "dominating_last", "dominating_inside", "one_far_draw", "tiny_sigma", "outlier",
            "near_tied", "both_signs", "a_tail_beyond_64_KB"]


def pattern_case(name):
    rng = np.random.default_rng([SEED, PATTERNS.index(name)])
    x = rng.normal(1.0, 1.5, size=65)
    if name == "identical":
        return normal_case(x, np.full(1088, 0.3), np.full(1088, 1.7), 17)
    if name == "ties_of_ten":      # each distinct term ten times, S = 100: M = 20, the cutoff a_20 opens the third group
        return normal_case(x, np.repeat(rng.normal(1.0, 0.3, size=10), 10)[rng.permutation(100)], np.full(100, 1.3), 4)
    if name == "a_tie_wider_than_the_tail":      # S = 400: M = 60, a tail of 64 slots; 50 distinct draws and one repeated 350 times, which holds rank 60 for most observations
        mu = np.concatenate([rng.normal(1.0, 2.0, size=50), np.full(350, 1.0)])[rng.permutation(400)]
        return normal_case(x, mu, np.full(400, 1.5), 8)
    if name.startswith("dominating"):      # one draw carries the predictive density (WAIC's case): every other term is far below it
        S, rows = 1105, 17
        at = {"dominating_first": 0, "dominating_last": S - 1, "dominating_inside": 617}[name]
        mu = np.full(S, 1e3) + rng.normal(size=S)
        mu[at] = 0.0
        return normal_case(x, mu, np.ones(S), rows)
    if name == "one_far_draw":      # one draw carries the importance weight: its term is far below every other
        mu = rng.normal(1.0, 0.3, size=1088)
        mu[700] = 1e3
        return normal_case(x, mu, np.ones(1088), 17)
    if name == "tiny_sigma":      # |l| about 1e12
        return normal_case(x, rng.normal(size=1105), np.full(1105, 1e-6), 17)
    if name == "outlier":      # a planted outlier: khat > 0.7
        x[7] = 9.0
        return normal_case(x, rng.normal(1.0, 0.3, size=4096), rng.uniform(0.8, 2.5, size=4096), 64)
    if name == "near_tied":      # mu spread 1e-3
        return normal_case(x, 1.0 + 1e-3 * rng.normal(size=1088), np.full(1088, 1.2), 17)
    if name == "both_signs":      # sigma = 0.05: terms up to +2.08 at the mode, far below zero elsewhere
        return normal_case(np.concatenate([1.0 + 0.05 * rng.normal(size=40), x[:25]]), 1.0 + 0.02 * rng.normal(size=1088), np.full(1088, 0.05), 17)
    if name == "a_tail_beyond_64_KB":      # S = 1 871 870: M = 4 105, 8 192 slots: the fit's workgroup asks for more than 64 KB of LDS.  Two observations.
        S = 1870 * 1001
        return normal_case(x[:2], rng.normal(1.0, 0.3, size=S), rng.uniform(0.8, 2.5, size=S), 1870)
    raise KeyError(name)


def all_cases():
    for k in range(len(SHAPES)):
        yield ("shape %d" % k,) + shape_case(k)
    for model in ("beta_bern", "pois_glm", "hier_normal"):
        for rows, cpd in FAMILY_SHAPES:
            yield ("%s %dx%d" % (model, rows, cpd),) + family_case(model, rows, cpd)
    for name in PATTERNS:
        yield (name,) + pattern_case(name)


def self_check():
    """the reference against closed forms; raises AssertionError"""
    assert [tail_len(S) for S in (24, 25, 29, 30, 224, 225, 226, 1088, 4096, 256000)] == [4, 5, 5, 6, 44, 45, 45, 99, 192, 1518]
    rng = np.random.default_rng(11)
    # M < 5: the harmonic-mean form, elpd = log S - log sum exp(-l)
    col = rng.normal(-2.0, 1.0, size=24)
    e, k = point(col, np.longdouble)
    assert k == np.inf and abs(float(e) - (math.log(24) - math.log(np.exp(-col).sum()))) < 1e-13
    # identical draws: no fit, elpd = l
    for T in (np.float64, np.longdouble):
        e, k = point(np.full(1088, -1.25), T)
        assert k == np.inf and float(e) == -1.25
    # -0.0 sorts before +0.0
    assert key_sort(np.array([0.0, -0.0, 1.0, -1.0])).tobytes() == np.array([-1.0, -0.0, 0.0, 1.0]).tobytes()
    # excesses at the quantiles of a generalised Pareto (k, sigma), M = 192 of S = 4096: khat orders with k
    S, M = 4096, 192
    got = []
    for kk in (-0.2, 0.3, 0.9):
        p = (np.arange(1, M + 1) - 0.5) / M
        xq = 0.05 * np.expm1(-kk * np.log1p(-p)) / kk      # ascending excesses over the cutoff ratio ec = 1 (a_M = a_0 - ... fixed below)
        ratio = 1.0 + xq      # importance ratios relative to the cutoff: exp(a_M - a_{M-r})
        a_tail = -np.log(ratio[::-1])      # a_0 ... a_{M-1} relative to a_M = 0
        col = np.concatenate([a_tail, [0.0], rng.uniform(0.0, 3.0, size=S - M - 1)])
        e, k = point(col, np.longdouble)
        assert np.isfinite(k)
        got.append(float(k))
    assert got[0] < got[1] < got[2], got
