"""References for the on-device summaries (split-R-hat, ESS, mean, sd; csrc/amwg_diag.hip), shared by tests/test_summary_reference_host.py,
tests/test_gpu_summary_arrays.py and tests/test_gpu_pooled_moments.py.  Not a test file.  Standard library + numpy only.

    exact(x)          one segment x[rows][cpd] in exact rational arithmetic, by the definitions of include/amwg.h
    kernel_order(x)   the ORDER of welford_add + dataset_diagnostics_kernel restated in numpy float64 (bit for bit what the device must give)
    kernel_order_moments(v)   the order of dataset_moments_kernel
    patterns(rng, rows, cpd)  named value patterns; SHAPES; case(name, rows, cpd): one array [rows][PR][D cpd] with its references, computed once
    cap(...)          the error bound the summaries are held to against exact() (tests/README.summaries.md)

Definitions (include/amwg.h, amwg_last_sample_diagnostics): half = rows // 2, an odd last row is ignored; every chain gives two half-chains of `half` draws, with
mean m_hc and (half - 1) variance v_hc; W = mean of the 2 cpd variances; B/n = sum (m_hc - mean m)^2 / (2 cpd - 1); var_plus = (half - 1) / half W + B/n;
chain mean = (m_0c + m_1c) / 2; Var(chain mean) with cpd - 1; rhat = sqrt(var_plus / W), ess = cpd var_plus / Var(chain mean).  W = 0 -> rhat NaN;
Var(chain mean) = 0 -> ess NaN; a used draw that is not finite -> both NaN."""
import functools
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SEED = 20261019
PR, D = 3, 3
DIAG_THREADS = 256       # dataset_diagnostics_kernel's workgroup
MOMENT_THREADS = 1024    # dataset_moments_kernel's
NAN = float("nan")


# ---- exact

def _integers(values):
    """finite doubles -> (Python ints, denominator): values[i] == ints[i] / denominator exactly (every double is a Fraction with a power-of-two denominator)"""
    fr = [Fraction(float(v)) for v in values]
    den = max(f.denominator for f in fr)
    return [f.numerator * (den // f.denominator) for f in fr], den


def _mean_var(ints, den):
    """exact mean and (n - 1) variance of ints / den, as Fractions (variance 0 for n = 1)"""
    n = len(ints)
    s = sum(ints)
    q = sum(i * i for i in ints)
    mean = Fraction(s, n * den)
    var = Fraction(q * n - s * s, n * (n - 1) * den * den) if n > 1 else Fraction(0)
    return mean, var


def exact(x):
    """x[rows][cpd] -> dict: rhat, ess, mean, sd (floats, each the exact value rounded at the very end), kappa_r = 1 + max|x| / sqrt(W) and
    kappa_e = 1 + max|x| / sqrt(Var(chain mean)) (max over the rows the diagnostics use; inf where the variance is 0), mean_abs = mean |x| over all rows."""
    x = np.asarray(x, dtype=np.float64)
    rows, cpd = x.shape
    half = rows // 2
    out = {"rows": rows, "cpd": cpd, "half": half}
    flat = x.reshape(-1)
    out["mean_abs"] = float(np.mean(np.abs(flat)))
    if np.all(np.isfinite(flat)):
        ints, den = _integers(flat)
        mean, var = _mean_var(ints, den)
        out["mean"], out["sd"] = float(mean), math.sqrt(float(var))
    else:      # what IEEE arithmetic gives in any order: a NaN, or +inf and -inf together, is NaN; an infinity alone is itself; the deviations hold inf - inf
        with np.errstate(invalid="ignore"):
            out["mean"], out["sd"] = float(np.sum(flat) / flat.size), NAN
    used = x[:2 * half]
    if not np.all(np.isfinite(used)):
        out.update(rhat=NAN, ess=NAN, kappa_r=NAN, kappa_e=NAN)
        return out
    ints, den = _integers(used.reshape(-1))
    m, v = [], []      # [2][cpd]
    for h in range(2):
        mv = [_mean_var([ints[(h * half + r) * cpd + c] for r in range(half)], den) for c in range(cpd)]
        m.append([a for a, _ in mv])
        v.append([b for _, b in mv])
    n_half = 2 * cpd
    W = sum(v[0] + v[1]) / n_half
    gm = sum(m[0] + m[1]) / n_half
    B_over_n = sum((a - gm) ** 2 for a in m[0] + m[1]) / (n_half - 1)
    var_plus = Fraction(half - 1, half) * W + B_over_n
    cm = [(a + b) / 2 for a, b in zip(m[0], m[1])]
    gmc = sum(cm) / cpd
    vcm = sum((a - gmc) ** 2 for a in cm) / (cpd - 1)
    big = float(np.max(np.abs(used)))
    out["rhat"] = math.sqrt(float(var_plus / W)) if W > 0 else NAN
    out["ess"] = float(cpd * var_plus / vcm) if vcm > 0 else NAN
    out["kappa_r"] = 1.0 + big / math.sqrt(float(W)) if W > 0 else math.inf
    out["kappa_e"] = 1.0 + big / math.sqrt(float(vcm)) if vcm > 0 else math.inf
    return out


# ---- the kernels' order in numpy float64

def tree_sum(partial, threads=MOMENT_THREADS):
    """block_sum: the halving tree over the workgroup's partial sums"""
    red = np.array(partial, dtype=np.float64)
    o = threads // 2
    while o:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    return red[0]


def strided_sums(v, term, threads=MOMENT_THREADS):
    """[threads]: thread t's running sum of term(v[i]) over i = t, t + threads, ...; the padding of the last round is masked, not added"""
    rounds = -(-v.size // threads)
    x = np.zeros(rounds * threads)
    x[:v.size] = v
    have = (np.arange(rounds * threads) < v.size).reshape(rounds, threads)
    acc = np.zeros(threads)
    for r, row in enumerate(x.reshape(rounds, threads)):
        acc = np.where(have[r], acc + term(row), acc)
    return acc


def kernel_order_moments(v, threads=MOMENT_THREADS):
    """dataset_moments_kernel over the values v (a segment's rows laid end to end) -> mean, sd"""
    n = v.size
    with np.errstate(invalid="ignore", over="ignore"):
        m = tree_sum(strided_sums(v, lambda x: x, threads), threads) / np.float64(n)

        def square_about_the_mean(x):
            dlt = x - m
            return dlt * dlt
        tot = tree_sum(strided_sums(v, square_about_the_mean, threads), threads)
        return m, (np.sqrt(tot / np.float64(n - 1)) if n > 1 else np.float64(0.0))


def kernel_order_halves(x):
    """chain_halves_kernel (and the fold: the same recurrence in the same row order) on x[rows][cpd] -> m0, v0, m1, v1, arrays [cpd]: welford_add row by row,
    vectorised over the chains; the half M2 as a variance M2 / (half - 1), 0 when half <= 1"""
    rows, cpd = x.shape
    half = rows // 2
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(2):
            m, m2 = np.zeros(cpd), np.zeros(cpd)
            for r in range(half):
                xr = x[h * half + r]
                dlt = xr - m
                m = m + dlt / np.float64(r + 1)
                m2 = m2 + dlt * (xr - m)
            out += [m, m2 / np.float64(half - 1) if half > 1 else np.zeros(cpd)]
    return out


def kernel_order(x, threads=DIAG_THREADS):
    """dataset_diagnostics_kernel on the halves of x[rows][cpd] -> rhat, ess: `threads` strided partial sums (thread t over the chains t, t + threads, ...), the
    halving tree, the five reductions in the kernel's sequence (W, grand mean, grand chain mean; then B/n and Var(chain mean) about those), W > 0 ? sqrt : NaN."""
    x = np.asarray(x, dtype=np.float64)
    rows, cpd = x.shape
    m0, v0, m1, v1 = kernel_order_halves(x)
    n, m = np.float64(rows // 2), np.float64(2.0 * cpd)
    same = lambda t: t
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cm = 0.5 * (m0 + m1)
        W = tree_sum(strided_sums(v0 + v1, same, threads), threads) / m
        gm = tree_sum(strided_sums(m0 + m1, same, threads), threads) / m
        gmc = tree_sum(strided_sums(cm, same, threads), threads) / np.float64(cpd)
        a, b, w = m0 - gm, m1 - gm, cm - gmc
        B_over_n = tree_sum(strided_sums(a * a + b * b, same, threads), threads) / (m - 1)
        vcm = tree_sum(strided_sums(w * w, same, threads), threads) / (np.float64(cpd) - 1)
        var_plus = (n - 1) / n * W + B_over_n
        rhat = np.sqrt(var_plus / W) if W > 0 else np.float64(NAN)
        ess = np.float64(cpd) * var_plus / vcm if vcm > 0 else np.float64(NAN)
    return np.float64(rhat), np.float64(ess)


# ---- the caps (tests/README.summaries.md)

CAP_FACTOR = 4.0


def cap_length(half, cpd):
    return half + cpd / 256.0 + 8.0


def cap(want, kappa, half, cpd):
    """|got - want| <= 4 L kappa u |want|, L = half + cpd / 256 + 8"""
    return CAP_FACTOR * cap_length(half, cpd) * kappa * U * abs(want)


# The restated order alone used 0.2549 of (ceil(n / 1024) + 11) u mean|x| at `trend` 9 x 64 (d 0, p 1) -- more than a quarter --, so the factor is four times
# that, 1.02 (tests/README.summaries.md); every other quantity stayed under a quarter of its cap as derived.
MEAN_CAP_SCALE = 1.02


def mean_cap(n, mean_abs):
    return MEAN_CAP_SCALE * (-(-n // 1024) + 11) * U * mean_abs


def sd_cap(n, mean_abs, sd):
    """absolute; a constant column (sd = 0) may show the mean's own error, no more"""
    if sd == 0:
        return 2.0 * mean_cap(n, mean_abs)
    return sd * ((-(-n // 1024) + 16) * U + (mean_cap(n, mean_abs) / sd) ** 2)


def within(got, want, bound):
    """-> (ok, |got - want| / bound); a NaN is held to a NaN, an infinity to itself"""
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got), 0.0
    if math.isinf(want) or math.isinf(got):
        return got == want, 0.0
    err = abs(got - want)
    if err == 0:
        return True, 0.0
    return err <= bound, (err / bound if bound > 0 else math.inf)


# ---- patterns, shapes, cases

FINITE = ["healthy", "offset1e6", "offset1e9_sd1e-3", "two_camps", "trend", "one_stuck", "integers", "tiny_between"]
W_ZERO = ["all_equal", "constant_chains_that_differ"]
NON_FINITE = ["one_nan", "one_inf"]
PATTERNS = FINITE + W_ZERO + NON_FINITE
# (rows, cpd): the minima the calls accept; an odd last row; one wavefront; around the workgroup of 256; a third strided round; long halves
SHAPES = [(4, 2), (5, 3), (9, 64), (8, 255), (8, 256), (8, 257), (6, 513), (64, 70)]


def pattern(name, rng, rows, cpd, k=0):
    """one segment [rows][cpd] of the named pattern; k moves the constant patterns, so that no two segments of an array are equal"""
    z = rng.standard_normal((rows, cpd))
    c = np.arange(cpd, dtype=np.float64)[None, :]
    if name == "healthy":
        return 3.0 + z
    if name == "offset1e6":
        return 1e6 + z
    if name == "offset1e9_sd1e-3":
        return 1e9 + 1e-3 * z
    if name == "two_camps":           # rhat ~ 5 ... 8
        return z + 10.0 * (c % 2)
    if name == "trend":               # every chain drifts: split-R-hat sees it, an unsplit one would not
        return z + np.linspace(0.0, 5.0, rows)[:, None]
    if name == "one_stuck":
        x = 3.0 + z
        x[:, 0] = 3.5 + k
        return x
    if name == "integers":            # ties
        return rng.integers(-3, 4, (rows, cpd)).astype(np.float64)
    if name == "tiny_between":
        return 5.0 + 1e-6 * z + 1e-12 * c
    if name == "all_equal":           # W = 0 and B = 0; (a multiple of 1/4: every sum of it is exact, so the kernels see Var(chain mean) = 0 too)
        return np.full((rows, cpd), 1.25 + 0.5 * k)
    if name == "constant_chains_that_differ":      # W = 0 and B > 0
        return np.broadcast_to(1.0 + 0.5 * k + 0.25 * (c % 7), (rows, cpd)).copy()
    if name in ("one_nan", "one_inf"):             # one element of one chain, in a row the diagnostics use
        x = 3.0 + z
        x[1, cpd // 2] = NAN if name == "one_nan" else math.inf
        return x
    raise ValueError(name)


def patterns(rng, rows, cpd, k=0):
    """name -> segment [rows][cpd], every pattern"""
    return {name: pattern(name, rng, rows, cpd, k) for name in PATTERNS}


def segment(draws, d, p, n_datasets=D):
    cpd = draws.shape[2] // n_datasets
    return np.ascontiguousarray(draws[:, p, d * cpd:(d + 1) * cpd])


class Case:
    """An array draws[rows][PR][D cpd] of one pattern and its references: per segment (d, p) exact() and the kernels' order, per value p exact() over all the chains"""
    def __init__(self, name, rows, cpd):
        rng = np.random.default_rng([SEED, rows, cpd, PATTERNS.index(name)])
        self.name, self.rows, self.cpd = name, rows, cpd
        self.draws = np.empty((rows, PR, D * cpd))
        for p in range(PR):
            for d in range(D):
                self.draws[:, p, d * cpd:(d + 1) * cpd] = pattern(name, rng, rows, cpd, 3 * p + d)
        self.exact = [[exact(segment(self.draws, d, p)) for p in range(PR)] for d in range(D)]
        self.pooled = [exact(self.draws[:, p, :]) for p in range(PR)]
        self.rhat, self.ess, self.mean, self.sd = (np.empty((D, PR)) for _ in range(4))
        for d in range(D):
            for p in range(PR):
                x = segment(self.draws, d, p)
                self.rhat[d, p], self.ess[d, p] = kernel_order(x)
                self.mean[d, p], self.sd[d, p] = kernel_order_moments(x.reshape(-1))
        for a in (self.draws, self.rhat, self.ess, self.mean, self.sd):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name, rows, cpd):
    return Case(name, rows, cpd)


def held_to_exact(got, half, cpd, n, label, worst):
    """got: triples (quantity in mean | sd | rhat | ess, the figure, the exact() dict of its segment of n values, `half` used rows x cpd chains).
    Asserts every figure inside its cap; records the largest |error| / cap per quantity in `worst` (dict quantity -> (ratio, label))."""
    for key, g, e in got:
        if key == "rhat":
            bound = cap(e["rhat"], e["kappa_r"], half, cpd)
        elif key == "ess":
            bound = cap(e["ess"], e["kappa_e"], half, cpd)
        elif key == "mean":
            bound = mean_cap(n, e["mean_abs"])
        else:
            bound = sd_cap(n, e["mean_abs"], e["sd"])
        ok, ratio = within(float(g), e[key], bound)
        if ratio > worst.get(key, (0.0, ""))[0]:
            worst[key] = (ratio, label)
        assert ok, "%s %s: got %r, exact %r, cap %r (ratio %.3g)" % (label, key, float(g), e[key], bound, ratio)
