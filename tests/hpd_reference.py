"""Host reference of the highest-density interval (amwg_last_sample_dataset_hpd; include/amwg.h states the rule), used by test_hpd_host.py and test_gpu_hpd.py.

hpd(x, p)        the rule by a full key-ordered sort of the N draws.
hpd_tails(x, p)  the device's route restated: the two order statistics t_lo = x_(k-1) and t_hi = x_(g), the tails compacted around them (every key beyond the
                 threshold plus as many copies of the threshold as reach k), each tail sorted, the first smallest of the k widths.
Both return (lower, upper, g, k, i*), the bounds as numpy float64; (nan, nan, g, k, -1) where the rule says NaN.  THE RULE, per slice of N draws and probability p:
the draws are ordered by the key order of the doubles (the order of the doubles, with -0 before +0), x_(0) <= ... <= x_(N-1); g = floor(p * (double)N), one fp64
multiply then floor, clamped to [1, N - 1]; k = N - g; w_i = x_(i+g) - x_(i) in fp64 for i = 0 .. k - 1; i* the smallest i whose w_i is minimal, widths compared
as doubles; the result (x_(i*), x_(i*+g)).  A p that is NaN or outside the open interval (0, 1) gives (NaN, NaN); a NaN or +-inf among the draws gives (NaN, NaN)
for every p."""
import math

import numpy as np

KINDS = ("continuous", "binary", "quarter_grid", "log_normal")
SIGN = np.uint64(1 << 63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(x):
    """the monotone u64 key of each double: order of the keys = order of the doubles, -0 before +0"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, b ^ ALL, b ^ SIGN)


def values(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k ^ SIGN, k ^ ALL).view(np.float64)


def rank_g(p, N):
    """g of the rule, or None for a p that gives NaN"""
    if not (p > 0.0 and p < 1.0):
        return None
    g = int(math.floor(float(p) * float(N)))      # one fp64 multiply, then floor
    return min(max(g, 1), N - 1)


def _first_narrowest(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        w = hi - lo
    i = int(np.argmin(w))      # numpy: the first of equal minima
    return lo[i], hi[i], i


def hpd(x, p):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    N = x.size
    assert N >= 2
    g = rank_g(p, N)
    if g is None:
        return np.float64("nan"), np.float64("nan"), None, None, -1
    k = N - g
    if not np.all(np.isfinite(x)):
        return np.float64("nan"), np.float64("nan"), g, k, -1
    s = values(np.sort(keys(x)))
    lo, hi, i = _first_narrowest(s[:k], s[g:])
    return lo, hi, g, k, i


def hpd_tails(x, p):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    N = x.size
    assert N >= 2
    g = rank_g(p, N)
    if g is None:
        return np.float64("nan"), np.float64("nan"), None, None, -1
    k = N - g
    if not np.all(np.isfinite(x)):
        return np.float64("nan"), np.float64("nan"), g, k, -1
    ks = keys(x)
    t_lo = np.partition(ks, k - 1)[k - 1]      # the select: two order statistics, nothing sorted
    t_hi = np.partition(ks, g)[g]
    below, above = ks[ks < t_lo], ks[ks > t_hi]
    assert below.size < k and above.size < k
    lo = np.sort(np.concatenate([below, np.full(k - below.size, t_lo, dtype=np.uint64)]))
    hi = np.sort(np.concatenate([above, np.full(k - above.size, t_hi, dtype=np.uint64)]))
    a, b, i = _first_narrowest(values(lo), values(hi))
    return a, b, g, k, i


def pair_bytes(r):
    return np.array([r[0], r[1]], dtype=np.float64).tobytes()


def draws_of(kind, n, rng):
    """n draws of one of the four kinds the rule was checked on"""
    if kind == "continuous":
        return rng.standard_normal(n) * 3.0 + 1.0
    if kind == "binary":
        return (rng.random(n) < rng.random()).astype(np.float64)
    if kind == "quarter_grid":      # multiples of 1/4 around zero, zeros of both signs
        v = rng.integers(-6, 7, n).astype(np.float64) / 4.0
        return np.where((v == 0.0) & (rng.random(n) < 0.5), -0.0, v)
    if kind == "log_normal":
        return np.exp(rng.standard_normal(n) * 1.5)
    raise ValueError(kind)


def of_array(draws, D, probs):
    """the rule over draws [rows][PR][C], D datasets of C / D columns each -> array [D][PR][len(probs)][2]"""
    draws = np.asarray(draws, dtype=np.float64)
    rows, PR, C = draws.shape
    cpd = C // D
    out = np.empty((D, PR, len(probs), 2))
    for d in range(D):
        for v in range(PR):
            x = draws[:, v, d * cpd:(d + 1) * cpd]
            for q, p in enumerate(probs):
                r = hpd(x, p)
                out[d, v, q, 0], out[d, v, q, 1] = r[0], r[1]
    return out


def same_bytes(a, b):
    """equal as bytes, every NaN counting as one value (the payload of a NaN is not part of the contract)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes())
