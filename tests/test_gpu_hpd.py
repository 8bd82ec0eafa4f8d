"""Highest-density intervals per dataset on the device (csrc/amwg_hpd.hip), on the GPU.  tests/README.hpd.md says what each test pins.

Every case is compared AS BYTES with the rule by a full sort on the host (hpd_reference.hpd): order statistics are exact, there is no tolerance.
(1) the kernels on synthetic arrays, through the test library (amwg_hpd_check): shapes, the sizes at which the route changes (the LDS sort's capacity, the pads
    of the network, the batches under a scratch budget), ties at the thresholds, isolation of a (dataset, value) from its neighbours.
(2) samplers: the Normal family, ragged datasets, a translated closure with a derived quantity, the refusals.
(3) the JavaScript front end (tests/js/test_gpu_hpd.js)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import hpd_reference as hr
import model_spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
ROWS = [2, 3, 17, 64]
CPDS = [1, 2, 3, 64, 255, 256, 257, 513]
PROBS = [0.5, 0.9, 0.95, 1e-9, 1 - 1e-12]      # the last two: g clamped to 1 (k = N - 1, the longest tails) and to N - 1 (k = 1: the range)
PATTERNS = hr.KINDS + ("three_valued",)


def pattern_draws(pattern, n, rng):
    if pattern == "three_valued":
        return rng.choice(np.array([-1.0, 0.0, 2.0]), size=n, p=[0.2, 0.6, 0.2])
    return hr.draws_of(pattern, n, rng)


def array_of(rows, PR, cpd, D, rng, first_pattern=0):
    """draws [rows][PR][D * cpd]: the pattern rotates over the (dataset, value) slices"""
    draws = np.empty((rows, PR, D * cpd))
    for d in range(D):
        for v in range(PR):
            draws[:, v, d * cpd:(d + 1) * cpd] = pattern_draws(PATTERNS[(first_pattern + d * PR + v) % len(PATTERNS)], rows * cpd, rng).reshape(rows, cpd)
    return draws


def of_slices(slices, rows):
    """draws [rows][1][D * cpd] holding the 1-d arrays `slices` (all of one length, a multiple of rows) as the D datasets of one value"""
    n = len(slices[0])
    cpd = n // rows
    assert cpd * rows == n and all(len(s) == n for s in slices)
    draws = np.empty((rows, 1, len(slices) * cpd))
    for d, s in enumerate(slices):
        draws[:, 0, d * cpd:(d + 1) * cpd] = np.asarray(s, dtype=np.float64).reshape(rows, cpd)
    return draws


def held(draws, D, probs):
    got = amwg_ctypes.hpd_check(draws, D, probs)
    want = hr.of_array(draws, D, probs)
    assert got.shape == want.shape and hr.same_bytes(got, want), (draws.shape, D, list(probs), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
    return got


def p_for(N, k):
    """a p whose g = floor(p N) is N - k: the middle of the interval of such p"""
    p = (N - k + 0.5) / N
    assert hr.rank_g(p, N) == N - k
    return p


# ---- (1) the kernels on synthetic arrays

@pytest.mark.parametrize("cpd", CPDS)
@pytest.mark.parametrize("rows", ROWS)
def test_shapes(rows, cpd):
    case = ROWS.index(rows) * len(CPDS) + CPDS.index(cpd)
    held(array_of(rows, 4, cpd, 3, np.random.default_rng([SEED, rows, cpd]), first_pattern=case), 3, PROBS)


_limits = {}


def lds_keys():
    if not _limits:
        _limits["keys"] = amwg_ctypes.hpd_limits(0)[0]
    return _limits["keys"]


BIG_ROWS, BIG_CPD = 40, 1000      # N = 40 000 per slice


def test_the_lds_sort_capacity_and_the_first_global_sizes():
    """k just below, at and just above every size m = capacity x 2^j that a slice of 40 000 reaches: at m the padded tail grows from m to 2 m keys -- at the capacity
    itself the sort leaves the LDS for the first global size (one global step), at 2 x capacity the network gains a second global step"""
    cap, N = lds_keys(), BIG_ROWS * BIG_CPD
    assert cap >= 128 and cap & (cap - 1) == 0, cap
    sizes, m = [], cap
    while m + 1 <= N - 1:
        sizes += [m - 1, m, m + 1]
        m *= 2
    assert sizes, (cap, N)
    print("LDS sort capacity %d keys; k = %s at N = %d" % (cap, sizes, N))
    rng = np.random.default_rng([SEED, 1])
    draws = array_of(BIG_ROWS, 2, BIG_CPD, 2, rng)      # continuous, binary / quarter grid, log-normal
    held(draws, 2, [p_for(N, k) for k in sizes])


@pytest.mark.parametrize("m", [2, 4, 64, 128, 1024, 2048, 4096])
def test_the_pads_of_the_network_inside_the_lds(m):
    """k = m - 1, m, m + 1 for powers of two m below the capacity: the pad grows at m + 1; the sort's workgroup is 64 threads up to a pad of 128, a thread per pair of
    keys up to 2048, 1024 threads beyond"""
    rows, cpd = 16, 512      # N = 8192
    N = rows * cpd
    held(array_of(rows, 2, cpd, 2, np.random.default_rng([SEED, 2, m]), first_pattern=m), 2, [p_for(N, k) for k in (m - 1, m, m + 1) if 1 <= k <= N - 1])


@pytest.mark.parametrize("budget,batches", [(4 * 1024, "4 + 2 | 2 + 2 + 2"), (1024, "1 x 6 | alone"), (100, "alone: a pair's tails exceed the budget")])
def test_batches_under_a_scratch_budget(budget, batches):
    """6 (dataset, value) pairs, k = 63, 64, 65: a pair's two tails take 1024 bytes up to k = 64 and 2048 from k = 65, so a budget of 4096 bytes serves 4 pairs a
    batch, then 2; with 1024 bytes one pair a batch, then a pair that exceeds the budget and runs alone; the results are those of one batch"""
    rows, cpd, D, PR = 8, 32, 3, 2
    N = rows * cpd
    draws = array_of(rows, PR, cpd, D, np.random.default_rng([SEED, 3]), first_pattern=1)
    probs = [p_for(N, k) for k in (63, 64, 65)]
    whole = held(draws, D, probs)
    assert amwg_ctypes.hpd_limits(budget, lds=False)[1] == 256 << 20
    try:
        assert hr.same_bytes(held(draws, D, probs), whole)
    finally:
        assert amwg_ctypes.hpd_limits(0, lds=False)[1] == budget


TIE_N, TIE_ROWS = 600, 6


def tie_slices(rng):
    n = TIE_N
    shuffled = lambda a: rng.permutation(np.asarray(a, dtype=np.float64))
    return {
        "binary_30": shuffled([1.0] * 180 + [0.0] * 420),            # p = 0.5: t_lo = t_hi = 0, which occurs 420 > k = 300 times
        "binary_97": shuffled([1.0] * 582 + [0.0] * 18),             # p = 0.95: k = 30, 18 zeros below t_lo = 1, nothing above t_hi = 1
        "three_valued": shuffled([-1.0] * 120 + [0.0] * 360 + [2.0] * 120),      # p = 0.5: both thresholds are 0; p = 0.9: t_lo = -1 (120 > k = 60), t_hi = 2
        "three_skewed": shuffled([-1.0] * 10 + [0.0] * 20 + [2.0] * 570),       # the threshold value 2 occurs more often than k at every p
        "constant": np.full(n, 2.5),
        "zeros": shuffled([0.0] * 250 + [-0.0] * 250 + [1.0] * 50 + [-1.0] * 50),      # -0 before +0 in the returned bytes
        "subnormal": rng.integers(-1000, 1001, n).astype(np.float64) * 5e-324,
        "negative": -np.exp(rng.standard_normal(n)),
        "straddling": rng.standard_normal(n),
        "huge": shuffled(np.concatenate([-1e308 - 1e305 * np.arange(300), 1e308 + 1e305 * np.arange(300)])),      # every width overflows to +inf: i* = 0
    }


def test_ties_at_the_thresholds_and_extreme_values():
    s = tie_slices(np.random.default_rng([SEED, 4]))
    probs = [0.5, 0.9, 0.95, 0.05]
    names = list(s)
    got = held(of_slices([s[k] for k in names], TIE_ROWS), len(names), probs)
    at = lambda name, p: got[names.index(name), 0, probs.index(p)]
    assert at("binary_30", 0.5).tolist() == [0.0, 0.0] and at("binary_97", 0.95).tolist() == [1.0, 1.0] and at("three_valued", 0.5).tolist() == [0.0, 0.0]
    assert at("constant", 0.9).tolist() == [2.5, 2.5]
    lo, hi = at("zeros", 0.5)      # g = 300 of 50, 250, 250, 50: the first window of width 0 is (-0 at rank 50, +0 at rank 350)
    assert lo == 0.0 and hi == 0.0 and math.copysign(1.0, lo) == -1.0 and math.copysign(1.0, hi) == 1.0
    for p in (0.5, 0.9):
        r = hr.hpd(s["huge"], p)
        assert r[4] == 0 and float(r[1]) - float(r[0]) == math.inf and at("huge", p).tolist() == [r[0], r[1]]


ISO = dict(rows=17, PR=4, cpd=33, D=3)
ISO_PROBS = [0.5, 0.95, 0.29]


def iso_base():
    if "iso" not in _limits:
        draws = array_of(ISO["rows"], ISO["PR"], ISO["cpd"], ISO["D"], np.random.default_rng([SEED, 5]))
        _limits["iso"] = (draws, held(draws, ISO["D"], ISO_PROBS))
    return _limits["iso"]


def test_neighbours_do_not_reach_an_output():
    draws, base = iso_base()
    cpd = ISO["cpd"]
    for (d, v), fill in (((1, 2), math.nan), ((0, 0), 1e300), ((2, 3), math.nan)):
        x = np.full_like(draws, fill)
        x[:, v, d * cpd:(d + 1) * cpd] = draws[:, v, d * cpd:(d + 1) * cpd]
        got = amwg_ctypes.hpd_check(x, ISO["D"], ISO_PROBS)
        assert hr.same_bytes(got[d, v], base[d, v]), (d, v, fill)
        others = np.ones(base.shape[:2], dtype=bool)
        others[d, v] = False
        assert np.all(np.isnan(got[others])) if math.isnan(fill) else np.all(got[others] == fill)


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_one_non_finite_draw_reaches_its_own_slice_only(bad):
    draws, base = iso_base()
    cpd = ISO["cpd"]
    for (d, v, row, c) in ((1, 2, 0, 0), (2, 3, 16, 32), (0, 0, 8, 5)):
        x = draws.copy()
        x[row, v, d * cpd + c] = bad
        got = amwg_ctypes.hpd_check(x, ISO["D"], ISO_PROBS)
        assert np.all(np.isnan(got[d, v]))
        keep = np.ones(base.shape[:2], dtype=bool)
        keep[d, v] = False
        assert hr.same_bytes(got[keep], base[keep]), (bad, d, v)


def test_permutations_inside_and_of_datasets():
    draws, base = iso_base()
    rng = np.random.default_rng([SEED, 6])
    rows, cpd, D = ISO["rows"], ISO["cpd"], ISO["D"]
    x = draws[rng.permutation(rows)]
    for d in range(D):
        x[:, :, d * cpd:(d + 1) * cpd] = x[:, :, d * cpd + rng.permutation(cpd)]
    assert hr.same_bytes(amwg_ctypes.hpd_check(x, D, ISO_PROBS), base)      # an order statistic does not know where a draw stood
    order = [2, 0, 1]
    y = np.concatenate([draws[:, :, d * cpd:(d + 1) * cpd] for d in order], axis=2)
    assert hr.same_bytes(amwg_ctypes.hpd_check(y, D, ISO_PROBS), base[order])


def test_the_widest_interval_is_the_range_of_the_select():
    draws, base = iso_base()
    N = ISO["rows"] * ISO["cpd"]
    got = amwg_ctypes.hpd_check(draws, ISO["D"], [p_for(N, 1), 1 - 1e-12])      # g = N - 1 twice
    want = amwg_ctypes.dataset_quantiles_check(draws, ISO["D"], [0.0, 1.0])
    assert got[:, :, 0].tobytes() == want.tobytes() == got[:, :, 1].tobytes()
    bad = amwg_ctypes.hpd_check(draws, ISO["D"], [0.0, 0.5, 1.0, math.nan, -0.1, 1.5])
    assert np.all(np.isnan(bad[:, :, [0, 2, 3, 4, 5]])) and hr.same_bytes(bad[:, :, 1], base[:, :, 0])      # a bad p is NaN for that p alone


# ---- (2) samplers

def normal_spec(n_obs=50, seed=500):
    data = model_spec.make_data("normal", n_obs, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


BURN, CHAINS = 120, 128
SAMPLER_PROBS = [0.5, 0.95]


def test_a_normal_sampler():
    s = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_hpd(SAMPLER_PROBS)
    assert "amwg_last_sample_dataset_hpd" in str(ei.value) and "no sample() call yet" in str(ei.value)
    s.burn(BURN)
    draws = s.sample(40)
    got, pooled = s.dataset_hpd(SAMPLER_PROBS), s.hpd(SAMPLER_PROBS)
    mean, sd = s.moments()
    want = hr.of_array(draws, 1, SAMPLER_PROBS)
    assert got.shape == (1, s.PR, 2, 2) and hr.same_bytes(got, want) and hr.same_bytes(pooled, want[0])
    N = draws.shape[0] * CHAINS
    g = hr.rank_g(0.95, N)
    x = np.sort(draws[:, 0, :].ravel())      # mu
    a = (N - g) // 2
    lo, hi = got[0, 0, 1]
    assert lo <= mean[0] <= hi and hi - lo <= x[a + g] - x[a]      # the 95 % interval holds the mean and is no wider than the central window of g + 1 draws
    s.summarize(40, 1, 0)
    for call in (lambda: s.dataset_hpd(SAMPLER_PROBS), lambda: s.hpd(SAMPLER_PROBS)):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_last_sample_dataset_hpd" in str(ei.value) and "amwg_sample_summarize" in str(ei.value), str(ei.value)
    s.close()


def test_a_ragged_dataset_sampler_answers_per_dataset():
    sizes = (20, 50, 35, 64)
    specs = [normal_spec(n_obs, 500 + 7 * d) for d, n_obs in enumerate(sizes)]
    a = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True)
    a.burn(BURN)
    draws = a.sample(40)
    got = a.dataset_hpd(SAMPLER_PROBS)
    assert got.shape == (4, a.PR, 2, 2) and hr.same_bytes(got, hr.of_array(draws, 4, SAMPLER_PROBS))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        a.hpd(SAMPLER_PROBS)
    assert "pooled summaries are refused" in str(ei.value) and "amwg_last_sample_dataset_hpd" in str(ei.value) and "dataset_hpd" in str(ei.value)
    a.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_a_translated_closure_with_a_derived_quantity():
    import golden_io
    import user_host
    name = "norm_post_derived"
    rec = golden_io.load("user_" + name)["chains"][0]
    src, arrays, meta = user_host.translated(name)
    params, init, opts = [], [], []
    for p in rec["params_completed"]:
        params.append({"type": p["type"], "len": int(np.prod(p["dim"])), "top": p["dim"][0], "multidim": 0 if p["dim"] == [1] else 1, "lower": p["lower"], "upper": p["upper"]})
        init += p["init"]
    for o in rec["comp_opts"]:
        opts.append({"prop_log_scale": o.get("prop_log_scale", 0.0), "max_adaptation": o.get("max_adaptation", 0.33), "initial_adaptation": o.get("initial_adaptation", 1.0),
                     "target_accept_rate": o.get("target_accept_rate", 0.44), "batch_size": o.get("batch_size", 50), "is_adapting": o.get("is_adapting", True)})
    spec = {"user": user_host.user_spec_part(src, arrays, meta), "params": params, "P": len(init), "init": init, "comp_opts": opts}
    a = amwg_ctypes.Sampler(spec, chains=96, seed=7, lanes_per_chain=1)
    assert a.PR > a.P
    a.burn(BURN)
    draws = a.sample(30, 3)
    got = a.dataset_hpd(SAMPLER_PROBS)
    a.close()
    assert got.shape == (1, a.PR, 2, 2) and hr.same_bytes(got, hr.of_array(draws, 1, SAMPLER_PROBS))


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_hpd_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_hpd.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu hpd ok" in p.stdout, p.stdout + "\n" + p.stderr
