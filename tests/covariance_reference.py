"""References for the on-device covariance (csrc/amwg_covariance.hip), shared by tests/test_covariance_host.py and tests/test_gpu_covariance.py.  Not a test file.
Standard library + numpy + tests/summary_reference.py only.

    exact_cov(x, y)         one pair of segments x, y [rows][cpd] in exact rational arithmetic: sum (x - mean x)(y - mean y) / (n - 1), rounded at the very end
    exact_column(x)         what the cap needs of one column: exact sd, kappa = 1 + max|x| / sd, mean |x|, whether it is a constant multiple of 1/4
    kernel_order_cov(x, y)  the ORDER of the co-moment kernels + covariance_finish_kernel restated in numpy float64 (bit for bit what the device must give);
                            x is the value with the SMALLER index among the recorded values; y=None: the diagonal, fold_moments_kernel's ss / (n - 1)
    cov_bound(...)          the cap against exact_cov (tests/README.covariance.md)
    Array / array(...)      draws [rows][4][3 cpd] of a pattern with a partner, and its references, computed once"""
import functools
import math
from fractions import Fraction

import numpy as np

import summary_reference as sr

U = sr.U
NAN = float("nan")
THREADS = 256            # covariance_finish_kernel's workgroup (fold_moments_kernel's)
PR, D = 4, 3
VALUES = (2, 0, 3)       # a non-trivial order, with value 1 left out
# |got - exact| <= F L u (kappa_i + kappa_j) sd_i sd_j.  F = 1: the restated order alone stays under a quarter of it (test_covariance_host.py re-measures that)
CAP_FACTOR = 1.0
SHAPES = [(1, 2), (2, 1), (4, 2), (5, 3), (9, 64), (8, 255), (8, 256), (8, 257), (6, 513), (64, 70)]
PARTNERS = ["independent", "mixed", "anti"]
SPECIAL = ["all_equal", "one_nan", "one_inf"]


# ---- exact

def _ints(v):
    """finite doubles -> (Python ints, denominator)"""
    fr = [Fraction(float(a)) for a in v]
    den = max(f.denominator for f in fr)
    return [f.numerator * (den // f.denominator) for f in fr], den


def exact_cov(x, y):
    """-> float: the exact covariance (n - 1 denominator) of the values of x and y, rounded once; NaN when either holds a value that is not finite (what IEEE
    arithmetic gives in any order: the deviations hold inf - inf or a NaN)"""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    n = x.size
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        return NAN
    xi, dx = _ints(x)
    yi, dy = _ints(y)
    sx, sy, sxy = sum(xi), sum(yi), sum(a * b for a, b in zip(xi, yi))
    return float(Fraction(n * sxy - sx * sy, n * (n - 1) * dx * dy))


def exact_column(x):
    """-> dict sd (exact, rounded once; NaN when not finite), kappa = 1 + max|x| / sd (inf where sd = 0), mean_abs, quarter (a constant multiple of 1/4)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(x)):
        return {"sd": NAN, "kappa": NAN, "mean_abs": NAN, "quarter": False, "var": NAN}
    var = exact_cov(x, x)
    sd = math.sqrt(var)
    return {"sd": sd, "var": var, "kappa": 1.0 + float(np.max(np.abs(x))) / sd if sd > 0 else math.inf, "mean_abs": float(np.mean(np.abs(x))),
            "quarter": bool(np.all(x == x[0]) and (4.0 * x[0]) == math.floor(4.0 * x[0]))}


# ---- the kernels' order in numpy float64

def chain_comoments(x, y):
    """per chain, in row order: the means, the whole-chain M2 of x (welford_add) and C_xy += dx (y - m_y), m_y already advanced.  x, y [rows][cpd] -> mx, my, M2x, Cxy"""
    rows, cpd = x.shape
    mx, my, m2, cxy = (np.zeros(cpd) for _ in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            k = np.float64(r + 1)
            dx = x[r] - mx
            mx = mx + dx / k
            m2 = m2 + dx * (x[r] - mx)
            dy = y[r] - my
            my = my + dy / k
            cxy = cxy + dx * (y[r] - my)
    return mx, my, m2, cxy


def kernel_order_cov(x, y=None, threads=THREADS):
    """covariance_finish_kernel over one dataset: x (the smaller index) and y [rows][cpd]; y=None: the diagonal entry of x"""
    x = np.asarray(x, dtype=np.float64)
    diag = y is None
    y = x if diag else np.asarray(y, dtype=np.float64)
    rows, cpd = x.shape
    mx, my, m2, cxy = chain_comoments(x, y)
    same = lambda t: t
    with np.errstate(invalid="ignore", over="ignore"):
        gi = sr.tree_sum(sr.strided_sums(mx, same, threads), threads) / np.float64(cpd)
        gj = sr.tree_sum(sr.strided_sums(my, same, threads), threads) / np.float64(cpd)
        within = sr.tree_sum(sr.strided_sums(m2 if diag else cxy, same, threads), threads)
        between = sr.tree_sum(sr.strided_sums((mx - gi) * (my - gj), same, threads), threads)
        ss = within + np.float64(rows) * between
        n = np.float64(rows) * np.float64(cpd)
        return np.float64(ss / (n - 1))


def kernel_order_matrix(draws, n_datasets, values):
    """draws [rows][PR][C] -> [D][K][K] as amwg_covariance_check must return it, every byte"""
    K = len(values)
    cpd = draws.shape[2] // n_datasets
    out = np.empty((n_datasets, K, K))
    for d in range(n_datasets):
        seg = lambda p: np.ascontiguousarray(draws[:, p, d * cpd:(d + 1) * cpd])
        for i in range(K):
            out[d, i, i] = kernel_order_cov(seg(values[i]))
            for j in range(i + 1, K):
                lo, hi = min(values[i], values[j]), max(values[i], values[j])
                out[d, i, j] = out[d, j, i] = kernel_order_cov(seg(lo), seg(hi))
    return out


# ---- the cap

def cap_length(rows, cpd):
    return rows + cpd / 256.0 + 8.0


def cov_bound(ci, cj, rows, cpd):
    """the absolute bound on |got - exact| for a pair whose columns have exact_column() ci, cj, over rows x cpd values each.
    Both sd > 0: F L u (kappa_i + kappa_j) sd_i sd_j, from a rounding error of u |x| in each deviation over sums of length L.  One sd = 0 (a constant column): the
    deviations of that column are the error of its mean and nothing else, 2 mean_cap sd_other; both 0: the product of the two means' errors, and exactly 0 when both
    constants are multiples of 1/4 (every sum of them is exact)."""
    n = rows * cpd
    if ci["sd"] > 0 and cj["sd"] > 0:
        return CAP_FACTOR * cap_length(rows, cpd) * U * (ci["kappa"] + cj["kappa"]) * ci["sd"] * cj["sd"]
    if ci["sd"] == 0 and cj["sd"] == 0:
        return 0.0 if ci["quarter"] and cj["quarter"] else 4.0 * sr.mean_cap(n, ci["mean_abs"]) * sr.mean_cap(n, cj["mean_abs"])
    const, other = (ci, cj) if ci["sd"] == 0 else (cj, ci)
    return 2.0 * sr.mean_cap(n, const["mean_abs"]) * other["sd"]


def held(got, want, bound):
    """-> (ok, ratio); a NaN is held to a NaN"""
    return sr.within(float(got), float(want), bound)


# ---- arrays

def partner(kind, x, rng, fresh):
    """the partner column of x [rows][cpd]: `fresh` (another segment of x's pattern) when independent; 0.6 x + 0.8 s z (correlation ~ 0.6); -x + 1e-3 s z (~ -1)"""
    s = float(np.std(x)) or 1.0
    z = rng.standard_normal(x.shape)
    if kind == "independent":
        return fresh
    if kind == "mixed":
        return 0.6 * x + 0.8 * s * z
    if kind == "anti":
        return -x + 1e-3 * s * z
    raise ValueError(kind)


def segment_of(name, rng, rows, cpd, k):
    """summary_reference.pattern; its one_nan / one_inf put their value into row 1, which a single row does not have: there it goes into row 0"""
    if name in sr.NON_FINITE and rows < 2:
        x = 3.0 + rng.standard_normal((rows, cpd))
        x[0, cpd // 2] = NAN if name == "one_nan" else math.inf
        return x
    return sr.pattern(name, rng, rows, cpd, k)


class Array:
    """draws [rows][PR][D cpd]: value 0 a segment of `pattern`, value 3 its `kind` partner, value 2 an independent segment of the pattern, value 1 (not selected)
    noise; the references over VALUES per dataset and over all chains as one dataset, computed once and read-only"""
    def __init__(self, pattern, kind, rows, cpd, n_datasets=D, values=VALUES, pr=PR):
        names = sr.PATTERNS
        rng = np.random.default_rng([sr.SEED, rows, cpd, names.index(pattern), (PARTNERS + [None]).index(kind)])
        self.pattern, self.kind, self.rows, self.cpd, self.values, self.D = pattern, kind, rows, cpd, tuple(values), n_datasets
        self.draws = np.empty((rows, pr, n_datasets * cpd))
        for d in range(n_datasets):
            sl = slice(d * cpd, (d + 1) * cpd)
            x = segment_of(pattern, rng, rows, cpd, d)
            fresh = segment_of(pattern, rng, rows, cpd, 3 + d)
            self.draws[:, 0, sl] = x
            self.draws[:, 1, sl] = rng.standard_normal((rows, cpd))
            self.draws[:, 2, sl] = segment_of(pattern, rng, rows, cpd, 6 + d)
            self.draws[:, 3, sl] = fresh if kind is None else partner(kind, x, rng, fresh)
            for p in range(4, pr):      # (wider arrays: independent segments of the pattern)
                self.draws[:, p, sl] = segment_of(pattern, rng, rows, cpd, 2 * p + d)
        self.draws.setflags(write=False)

    @functools.cached_property
    def want(self):
        """[D][K][K]: the kernels' order"""
        m = kernel_order_matrix(self.draws, self.D, self.values)
        m.setflags(write=False)
        return m

    def columns(self, n_datasets):
        cpd = self.draws.shape[2] // n_datasets
        return [[np.ascontiguousarray(self.draws[:, p, d * cpd:(d + 1) * cpd]) for p in self.values] for d in range(n_datasets)]

    @functools.lru_cache(maxsize=None)
    def exact(self, n_datasets):
        """per dataset: (the exact matrix [K][K], the exact_column() of every selected value)"""
        out = []
        K = len(self.values)
        for cols in self.columns(n_datasets):
            info = [exact_column(c) for c in cols]
            m = np.empty((K, K))
            for i in range(K):
                m[i, i] = info[i]["var"]
                for j in range(i + 1, K):
                    m[i, j] = m[j, i] = exact_cov(cols[i], cols[j])
            out.append((m, info))
        return out


@functools.lru_cache(maxsize=None)
def array(pattern, kind, rows, cpd):
    return Array(pattern, kind, rows, cpd)


def CASES():
    return [(p, k) for p in sr.FINITE for k in PARTNERS] + [(p, None) for p in SPECIAL]


def held_to_exact(got, arr, n_datasets, label, worst):
    """got [n_datasets][K][K] against arr.exact(n_datasets); asserts every entry inside cov_bound and records the largest ratio in worst[0] (a list [ratio, label])"""
    cpd = arr.draws.shape[2] // n_datasets
    K = len(arr.values)
    for d, (m, info) in enumerate(arr.exact(n_datasets)):
        for i in range(K):
            for j in range(K):
                if math.isnan(info[i]["sd"]) or math.isnan(info[j]["sd"]):
                    assert math.isnan(got[d, i, j]), "%s d %d (%d, %d): a value that is not finite among the draws must give NaN, got %r" % (label, d, i, j, got[d, i, j])
                    continue
                bound = cov_bound(info[i], info[j], arr.rows, cpd)
                ok, ratio = held(got[d, i, j], m[i, j], bound)
                if ratio > worst[0]:
                    worst[0], worst[1] = ratio, "%s d %d (%d, %d)" % (label, d, i, j)
                assert ok, "%s d %d (%d, %d): got %r, exact %r, cap %r (ratio %.3g)" % (label, d, i, j, float(got[d, i, j]), m[i, j], bound, ratio)
