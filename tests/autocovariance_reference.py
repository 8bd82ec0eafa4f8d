"""References for the on-device autocovariance (csrc/amwg_autocov.hip), shared by tests/test_autocovariance_host.py and tests/test_gpu_autocovariance.py.  Not a
test file.  Standard library + numpy + tests/summary_reference.py only.

    kernel_order(x, L)    the ARITHMETIC of include/amwg.h restated in numpy float64 (bit for bit what the device must give) for one (dataset, value): x [rows][cpd]
                          -> acov [L + 1], mean, between -- the per-chain lag sums about the pilot in row order, the finish, the 256-strided sums and the halving tree
    exact(x, L)           the definition in Fractions, rounded once: acov_l = (1 / cpd) sum_c (1 / n) sum_(t >= l) (x_t - xbar_c)(x_(t-l) - xbar_c); mean; between
    kappa(x)              1 + max over the chains of max|x - x_0| / sd, sd^2 = the exact acov_0: what the pilot centring leaves of the conditioning
    acov_bound(...)       the cap against exact (tests/README.autocorrelation.md)
    Array / array(...)    draws [rows][4][3 cpd] of a pattern and its references, computed once"""
import functools
import math
from fractions import Fraction

import numpy as np

import summary_reference as sr

U = sr.U
NAN = float("nan")
THREADS = 256            # autocov_dataset_kernel's workgroup (fold_moments_kernel's)
PR, D = 4, 3
VALUES = (2, 0, 3)       # a non-trivial order, with value 1 left out
# |got - exact| <= F Lc u kappa^2 acov_0.  F = 1: the restated order alone stays under a quarter of it (test_autocovariance_host.py re-measures that)
CAP_FACTOR = 1.0
HOST_SHAPES = [(3, 1), (5, 3), (9, 64), (17, 2), (64, 70)]


def host_lags(rows):
    return sorted({l for l in (1, 2, 8, min(16, rows - 1)) if l < rows})


# ---- the kernels' order in numpy float64

def chain_sums(x, L):
    """per chain, in row order: a = x_0, y = x - a, Y += y_t, S_l += y_t y_(t-l) for l = 0 .. min(t, L).  x [rows][cpd] -> a, y, Y, S [L + 1][cpd]"""
    rows, cpd = x.shape
    a = x[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        y = x - a[None, :]
        Y, S = np.zeros(cpd), np.zeros((L + 1, cpd))
        for t in range(rows):
            Y = Y + y[t]
            top = min(t, L)      # (all the lags of a row at once: each S_l is still one running sum in ascending t)
            S[:top + 1] = S[:top + 1] + y[t][None, :] * y[t - top:t + 1][::-1]
    return a, y, Y, S


def chain_finish(x, L):
    """-> gamma [L + 1][cpd], m [cpd]: the per-chain finish of include/amwg.h"""
    rows, cpd = x.shape
    a, y, Y, S = chain_sums(x, L)
    n = np.float64(rows)
    gamma = np.empty((L + 1, cpd))
    with np.errstate(invalid="ignore", over="ignore"):
        yb = Y / n
        H, T = np.zeros(cpd), np.zeros(cpd)
        for l in range(L + 1):
            gamma[l] = ((S[l] - yb * ((Y - H) + (Y - T))) + np.float64(rows - l) * (yb * yb)) / n
            if l < L:
                H = H + y[l]
                T = T + y[rows - 1 - l]
        return gamma, a + yb


def kernel_order(x, L, threads=THREADS):
    """one (dataset, value): x [rows][cpd] -> acov [L + 1], mean, between, as the device must return them, every byte"""
    x = np.asarray(x, dtype=np.float64)
    rows, cpd = x.shape
    gamma, m = chain_finish(x, L)
    same = lambda t: t
    with np.errstate(invalid="ignore", over="ignore"):
        acov = np.array([sr.tree_sum(sr.strided_sums(gamma[l], same, threads), threads) / np.float64(cpd) for l in range(L + 1)])
        gm = sr.tree_sum(sr.strided_sums(m, same, threads), threads) / np.float64(cpd)
        dm = m - gm
        tot = sr.tree_sum(sr.strided_sums(dm * dm, same, threads), threads)
        between = tot / np.float64(cpd - 1) if cpd > 1 else np.float64(0.0)
    if not math.isfinite(acov[0]):      # a NaN or an infinity among the draws (or sums that overflowed)
        return acov, np.float64(NAN), np.float64(NAN)
    return acov, np.float64(gm), np.float64(between)


def kernel_order_all(draws, n_datasets, values, L):
    """draws [rows][PR][C] -> acov [D][K][L + 1], mean [D][K], between [D][K] as amwg_autocovariance_check must return them"""
    K, cpd = len(values), draws.shape[2] // n_datasets
    acov, mean, between = np.empty((n_datasets, K, L + 1)), np.empty((n_datasets, K)), np.empty((n_datasets, K))
    for d in range(n_datasets):
        for k, p in enumerate(values):
            acov[d, k], mean[d, k], between[d, k] = kernel_order(np.ascontiguousarray(draws[:, p, d * cpd:(d + 1) * cpd]), L)
    return acov, mean, between


# ---- exact

def exact(x, L):
    """-> acov [L + 1], mean, between (floats, each rounded once from the exact rational); NaN throughout when a value is not finite"""
    x = np.asarray(x, dtype=np.float64)
    rows, cpd = x.shape
    if not np.all(np.isfinite(x)):
        return np.full(L + 1, NAN), NAN, NAN
    fr = [Fraction(float(v)) for v in x.reshape(-1)]
    den = max(f.denominator for f in fr)      # (denominators of doubles are powers of two: the largest is a common one)
    ints = np.array([f.numerator * (den // f.denominator) for f in fr], dtype=object).reshape(rows, cpd)      # Python integers: exact
    s = ints.sum(axis=0)
    dev = rows * ints - s[None, :]            # rows den (x_t - xbar_c)
    scale = cpd * rows * (rows * den) ** 2
    acov = [float(Fraction(int((dev[l:] * dev[:rows - l]).sum()), scale)) for l in range(L + 1)]
    means = [Fraction(int(v), rows * den) for v in s]
    gm = sum(means) / cpd
    between = sum((m - gm) ** 2 for m in means) / (cpd - 1) if cpd > 1 else Fraction(0)
    return np.array(acov), float(gm), float(between)


def kappa(x, acov0):
    """1 + max|x - x_0| / sd over the chains of the (dataset, value), sd^2 = acov_0 (exact); inf where sd = 0"""
    x = np.asarray(x, dtype=np.float64)
    big = float(np.max(np.abs(x - x[0][None, :])))
    return 1.0 + big / math.sqrt(acov0) if acov0 > 0 else math.inf


# ---- the cap

def cap_length(rows, cpd):
    return rows + cpd / 256.0 + 8.0


def acov_bound(k, acov0, rows, cpd):
    """|got - exact| <= F Lc u kappa^2 acov_0 for every lag (tests/README.autocorrelation.md); acov_0 = 0 (every chain constant): exactly 0 -- the deviations about
    the pilot are exact zeros whatever the constant"""
    if acov0 == 0:
        return 0.0
    return CAP_FACTOR * cap_length(rows, cpd) * U * k * k * acov0


def quarter(x):
    x = np.asarray(x)
    return bool(np.all(4.0 * x == np.floor(4.0 * x)))


# ---- arrays

class Array:
    """draws [rows][PR][D cpd]: values 0, 2, 3 independent segments of `pattern`, value 1 (not selected) noise; exact references per (dataset, value) computed once"""
    def __init__(self, pattern, rows, cpd, n_datasets=D, values=VALUES, pr=PR):
        rng = np.random.default_rng([sr.SEED, rows, cpd, sr.PATTERNS.index(pattern), 77])
        self.pattern, self.rows, self.cpd, self.values, self.D = pattern, rows, cpd, tuple(values), n_datasets
        self.draws = np.empty((rows, pr, n_datasets * cpd))
        for d in range(n_datasets):
            sl = slice(d * cpd, (d + 1) * cpd)
            for p in range(pr):
                self.draws[:, p, sl] = rng.standard_normal((rows, cpd)) if p == 1 else segment_of(pattern, rng, rows, cpd, 3 * p + d)
        self.draws.setflags(write=False)

    def segment(self, d, p):
        return np.ascontiguousarray(self.draws[:, p, d * self.cpd:(d + 1) * self.cpd])

    @functools.cached_property
    def _exact_all_lags(self):
        """the exact references up to the longest lag any test asks of this array (an autocovariance at lag l does not depend on L): computed once"""
        top = min(self.rows - 1, 33)
        out = {}
        for d in range(self.D):
            for k, p in enumerate(self.values):
                x = self.segment(d, p)
                acov, mean, between = exact(x, top)
                out[(d, k)] = (acov, mean, between, kappa(x, acov[0]) if math.isfinite(acov[0]) else NAN)
        return out

    def exact(self, L):
        """{(dataset, position in values): (acov [L + 1], mean, between, kappa)}"""
        return {key: (acov[:L + 1], mean, between, kap) for key, (acov, mean, between, kap) in self._exact_all_lags.items()}

    @functools.lru_cache(maxsize=None)
    def want(self, L):
        return kernel_order_all(self.draws, self.D, self.values, L)


def segment_of(name, rng, rows, cpd, k):
    """summary_reference.pattern (its one_nan / one_inf put their value into row 1)"""
    return sr.pattern(name, rng, rows, cpd, k)


@functools.lru_cache(maxsize=None)
def array(pattern, rows, cpd):
    return Array(pattern, rows, cpd)


def held_to_exact(got, arr, L, label, worst):
    """got = (acov [D][K][L + 1], mean, between) against arr.exact(L): every lag inside acov_bound, the mean inside summary_reference.mean_cap; a (dataset, value)
    with a value that is not finite must be NaN throughout.  Records the largest ratio in worst = [ratio, label]."""
    acov, mean, between = got
    for (d, k), (ea, em, eb, kap) in arr.exact(L).items():
        if math.isnan(ea[0]):
            assert np.all(np.isnan(acov[d, k])) and math.isnan(mean[d, k]) and math.isnan(between[d, k]), "%s d %d value %d: a draw that is not finite must give NaN" % (label, d, k)
            continue
        bound = acov_bound(kap, ea[0], arr.rows, arr.cpd)
        for l in range(L + 1):
            ok, ratio = sr.within(float(acov[d, k, l]), float(ea[l]), bound)
            if ratio > worst[0]:
                worst[0], worst[1] = ratio, "%s d %d value %d lag %d" % (label, d, k, l)
            assert ok, "%s d %d value %d lag %d: got %r, exact %r, cap %r (ratio %.3g)" % (label, d, k, l, float(acov[d, k, l]), float(ea[l]), bound, ratio)
        # the mean: a + Y / n per chain (rows running adds of |y| <= 2 max|x|), then cpd / 256 strided adds and the tree: 2 Lc u max|x|
        x = arr.segment(d, arr.values[k])
        ok, _ = sr.within(float(mean[d, k]), em, 2.0 * cap_length(arr.rows, arr.cpd) * U * float(np.max(np.abs(x))))
        assert ok, "%s d %d value %d: mean %r, exact %r" % (label, d, k, float(mean[d, k]), em)
