"""Posterior histograms over caller-given edges (dataset_histogram_kernel of csrc/amwg_histogram.hip), on the GPU.  tests/README.histogram.md says what each test pins.

(1) the kernel on synthetic arrays, through the test library (amwg_histogram_check): counts == np.searchsorted(edges, x, side="right") - 1, EXACTLY, over shapes,
    numbers of bins, windows and value patterns; every cell sums to its input; neighbours do not reach a cell; the kernel adds.
(2) a sampler that summarises with an armed histogram against its twin that stores: the same counts, both numpy's on the twin's draws; arming perturbs nothing;
    the twin's quantiles lie inside interval_brackets of the summarised counts.  Dataset samplers, a translated closure with a derived quantity, the refusals.
(3) the JavaScript front end (tests/js/test_gpu_histogram.js).

Counts are integers: there is no tolerance anywhere in this file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import model_spec
from histogram_reference import counts_of, counts_of_array

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261019
PR = 3
BINS = [1, 2, 63, 64, 65, 1000, 4096]
WINDOWS = [0, 1, 3]


def grid_array(rng, rows, PR, C):
    """N(0, 1) with every recorded value at its own location and scale and every chain with its own offset: a wrong stride, value or dataset shows"""
    x = rng.standard_normal((rows, PR, C))
    for p in range(PR):
        x[:, p, :] = (p - 1) * 1.5 + (0.5 + 0.5 * p) * x[:, p, :] + 0.25 * rng.standard_normal(C)[None, :]
    return x


def edges_for(bins, lo=-4.0, hi=4.0):
    """[PR][bins + 1]: uniform over [lo, hi], shifted per recorded value"""
    return np.array([np.linspace(lo + 0.37 * p, hi + 0.37 * p, bins + 1) for p in range(PR)])


def check(draws, D, edges, windows=WINDOWS, what=""):
    want = counts_of_array(draws, D, edges)
    rows, _, C = draws.shape
    assert np.all(want.sum(axis=2) == rows * (C // D))      # every cell sums to its input
    for w in windows:
        got = amwg_ctypes.histogram_check(draws, D, edges, w)
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got, want), (what, "window_rows", w, np.argwhere(got != want)[:5].tolist())
    return want


# ---- (1) the kernel on synthetic arrays

@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("cpd", [2, 64, 255, 256, 257])
@pytest.mark.parametrize("rows", [1, 4, 5, 9])
def test_counts_equal_numpy_over_shapes_bins_and_windows(rows, cpd, D):
    rng = np.random.default_rng([SEED, rows, cpd, D])
    draws = grid_array(rng, rows, PR, cpd * D)
    for bins in BINS:
        check(draws, D, edges_for(bins), what="rows=%d cpd=%d D=%d bins=%d" % (rows, cpd, D, bins))


@pytest.mark.parametrize("rows,cpd,D", [(40, 320, 1), (40, 320, 3), (70, 33, 2), (9, 4096, 1), (130, 8, 1), (33, 1000, 2)])
def test_counts_equal_numpy_where_a_cell_is_cut_into_slices(rows, cpd, D):
    """shapes of more than 2 048 values per cell: the launcher cuts a cell into row slices and column slices (several workgroups add to one cell), with ragged last
    slices; 33 and 8 columns: a wavefront's lanes cover several rows at a time"""
    rng = np.random.default_rng([SEED, rows, cpd, D, 1])
    draws = grid_array(rng, rows, PR, cpd * D)
    for bins in (1, 65, 4096):
        check(draws, D, edges_for(bins), windows=[0, 7], what="rows=%d cpd=%d D=%d bins=%d" % (rows, cpd, D, bins))


SHAPE = (9, PR, 3 * 257)      # rows, PR, C: three datasets of 257 chains -- the middle value and the middle dataset at nonzero, odd offsets


def test_a_constant_column_lands_in_one_bin():
    rng = np.random.default_rng([SEED, 2])
    draws = grid_array(rng, *SHAPE)
    draws[:, 1, :] = 0.625
    for bins in (1, 64, 4096):
        want = check(draws, 3, edges_for(bins), what="constant bins=%d" % bins)
        assert np.all(np.count_nonzero(want[:, 1, :], axis=1) == 1)      # all 64 lanes of every wave instruction name the same counter


def test_values_on_edges_and_one_ulp_either_side():
    rng = np.random.default_rng([SEED, 3])
    for edges in (np.linspace(-1.0, 1.0, 65), np.arange(0.0, 6.45, 0.1)[:65], np.logspace(-8, 8, 65)):
        e = np.broadcast_to(edges, (PR, 65))
        on = rng.choice(edges, size=SHAPE)                                  # exactly on an edge: the bin that STARTS there (the last edge: over)
        below, above = np.nextafter(on, -np.inf), np.nextafter(on, np.inf)
        for name, draws in (("on", on), ("below", below), ("above", above)):
            want = check(draws, 3, e, what="edges %s" % name)
            if name != "above":
                assert want[:, :, 64 + (1 if name == "on" else 0)].sum() > 0      # `on` reaches over through the last edge, `below` reaches under through the first
        mixed = np.where(rng.random(SHAPE) < 0.5, below, on)
        check(mixed, 3, e, what="edges mixed")


def test_signed_zeros_with_an_edge_at_zero_and_subnormals():
    rng = np.random.default_rng([SEED, 4])
    tiny = np.float64(5e-324)
    edges = np.array([-1.0, -tiny, 0.0, tiny, 2 * tiny, 2.2250738585072014e-308, 1.0])
    values = np.array([-0.0, 0.0, -tiny, tiny, 2 * tiny, 3 * tiny, 1e-310, -1e-310, 2.2250738585072014e-308, 2.225073858507201e-308, 0.5, -0.5])
    draws = rng.choice(values, size=SHAPE)
    want = check(draws, 3, edges, what="zeros and subnormals")
    zeros = np.zeros(SHAPE)
    zeros[::2] = -0.0
    want = check(zeros, 3, edges, what="signed zeros")
    assert np.all(want[:, :, 2] == 9 * 257)      # -0 == +0: both in the bin that starts at 0


def test_infinities_and_nans_in_single_elements():
    rng = np.random.default_rng([SEED, 5])
    draws = grid_array(rng, *SHAPE)
    draws[2, 0, 5] = np.nan
    draws[6, 1, 257 + 70] = np.inf
    draws[8, 2, 2 * 257 + 256] = -np.inf
    draws[0, 1, 300] = -np.nan
    for bins in (1, 65, 1000):
        want = check(draws, 3, edges_for(bins), what="inf nan bins=%d" % bins)
        assert want[0, 0, bins + 2] == 1 and want[1, 1, bins + 2] == 1 and want[:, :, bins + 2].sum() == 2      # the NaNs stay in their cells
        assert want[1, 1, bins + 1] >= 1 and want[2, 2, bins] >= 1                                               # +inf is over, -inf is under
    allnan = np.full(SHAPE, np.nan)
    want = check(allnan, 3, edges_for(4), what="all nan")
    assert np.all(want[:, :, 6] == 9 * 257)


def test_everything_under_and_everything_over():
    rng = np.random.default_rng([SEED, 6])
    draws = grid_array(rng, *SHAPE)
    for bins in (1, 64, 4096):
        want = check(draws, 3, edges_for(bins, 50.0, 60.0), what="under")
        assert np.all(want[:, :, bins] == 9 * 257)
        want = check(draws, 3, edges_for(bins, -60.0, -50.0), what="over")
        assert np.all(want[:, :, bins + 1] == 9 * 257)


def test_log_spaced_edges_and_a_width_that_is_not_representable():
    rng = np.random.default_rng([SEED, 7])
    draws = np.exp(3.0 * rng.standard_normal(SHAPE))
    for bins in (2, 63, 1000):
        check(draws, 3, np.logspace(-4, 4, bins + 1), what="log-spaced bins=%d" % bins)
    lin = 10.0 * rng.random(SHAPE)
    lin[::2] = np.round(lin[::2], 1)      # many values on (or an ulp from) multiples of 0.1
    for bins in (10, 100, 1000):
        check(lin, 3, 0.1 * np.arange(bins + 1), what="width 0.1 bins=%d" % bins)
        check(lin, 3, np.arange(bins + 1) / 10.0, what="width 1/10 bins=%d" % bins)


def test_grids_that_are_nearly_uniform_and_grids_at_the_ends_of_the_range():
    """the corrected uniform guess must give the comparison rule's answer whatever the arithmetic does: edges jittered by up to 0.45 of a bin (the guess is a bin
    off for many values), a grid far from zero whose width is below the spacing of the doubles' products, and edges whose span overflows"""
    rng = np.random.default_rng([SEED, 10])
    for bins in (2, 64, 1000, 4096):
        grid = np.linspace(-3.0, 3.0, bins + 1)
        w = grid[1] - grid[0]
        jit = grid.copy()
        jit[1:-1] += w * rng.uniform(-0.45, 0.45, bins - 1)
        draws = 1.2 * rng.standard_normal(SHAPE)
        draws[::3] = rng.choice(jit, size=draws[::3].shape)      # a third of the values on the jittered edges themselves
        check(draws, 3, jit, what="jittered bins=%d" % bins)
    far = 1e15 + np.arange(65.0)
    draws = 1e15 + 64.0 * rng.random(SHAPE) + rng.choice([-2.0, 0.0, 0.0, 0.0, 3.0], size=SHAPE)
    check(draws, 3, far, what="grid at 1e15")
    check(np.nextafter(rng.choice(far, size=SHAPE), rng.choice([-np.inf, np.inf], size=SHAPE)), 3, far, what="an ulp from the grid at 1e15")
    huge = rng.choice([-1.7e308, -1e308, -1.0, 0.0, 1.0, 1e308, 1.7e308, np.inf, -np.inf], size=SHAPE)
    check(huge, 3, np.array([-1.7e308, 0.0, 1.7e308]), what="span overflows")
    check(huge, 3, np.array([-1.7e308, 1.7e308]), what="span overflows, one bin")
    check(huge, 3, (np.arange(65.0) - 32.0) * 3.125e306, what="uniform at the ends of the range")


def test_neighbours_do_not_reach_a_cell():
    rng = np.random.default_rng([SEED, 8])
    draws = grid_array(rng, *SHAPE)
    edges = edges_for(65)
    base = amwg_ctypes.histogram_check(draws, 3, edges, 0)
    for d, p in ((1, 1), (0, 2), (2, 0)):
        other = 100.0 * rng.standard_normal(SHAPE)
        other[:, p, d * 257:(d + 1) * 257] = draws[:, p, d * 257:(d + 1) * 257]
        for w in WINDOWS:
            got = amwg_ctypes.histogram_check(other, 3, edges, w)
            assert np.array_equal(got[d, p], base[d, p]), (d, p, w)
            assert not np.array_equal(got, base)


def test_the_kernel_adds_to_the_counts():
    rng = np.random.default_rng([SEED, 9])
    draws = grid_array(rng, 40, PR, 320)
    edges = edges_for(1000)
    whole = check(draws, 1, edges, windows=[0], what="whole")
    first = amwg_ctypes.histogram_check(draws[:17], 1, edges, 0)
    both = amwg_ctypes.histogram_check(draws[17:], 1, edges, 3, counts=first)
    assert np.array_equal(both, whole)
    start = np.full(whole.shape, 2 ** 40, dtype=np.uint64)      # (beyond 32 bits: the counts in memory are 64 bits wide)
    assert np.array_equal(amwg_ctypes.histogram_check(draws, 1, edges, 0, counts=start), whole + np.uint64(2 ** 40))


# ---- (2) samplers

def normal_spec(n_obs=50, seed=500):
    data = model_spec.make_data("normal", n_obs, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


BURN, CHAINS = 120, 128
PROBS = (0.025, 0.5, 0.975)
TWIN_BINS = 40


def edges_from(draws, D, bins):
    """[PR][bins + 1] from the draws' own minimum and maximum widened by one bin: every value, hence every rank, falls into a real bin"""
    out = []
    for p in range(draws.shape[1]):
        lo, hi = float(draws[:, p].min()), float(draws[:, p].max())
        w = (hi - lo) / (bins - 2) if hi > lo else 1.0
        out.append(lo - w + w * np.arange(bins + 1))
    return np.array(out)


def brackets_hold(counts, edges, quantiles, what):
    """counts [D][PR][bins + 3], quantiles [D][PR][len(PROBS)]: under == over == nan == 0, every quantile inside its bracket, no bracket wider than two bins"""
    bins = edges.shape[1] - 1
    assert np.all(counts[:, :, bins:] == 0), what
    for d in range(counts.shape[0]):
        for p in range(counts.shape[1]):
            br = amwg_ctypes.interval_brackets(counts[d, p], edges[p], PROBS)
            width = edges[p][1] - edges[p][0]
            for k in range(len(PROBS)):
                lo, hi, q = br[k, 0], br[k, 1], quantiles[d, p, k]
                assert np.isfinite(lo) and np.isfinite(hi) and lo <= q <= hi, (what, d, p, PROBS[k], lo, q, hi)
                assert hi - lo <= 2.0 * width * (1 + 1e-9), (what, d, p, PROBS[k], lo, hi, width)


_stored = {}


def stored_twin(n, thin):
    """the storing twin, shared by the window sizes that compare against it"""
    if (n, thin) not in _stored:
        a = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
        a.burn(BURN)
        a.sample_async(n, thin)
        a.sync()
        draws = a.fetch_draws()
        edges = edges_from(draws, 1, TWIN_BINS)
        _stored[(n, thin)] = {"draws": draws, "edges": edges, "hist": a.dataset_histogram(edges), "conv": a.convergence(), "state": a.state(),
                              "quantiles": a.quantiles(PROBS), "info": a.histogram_info()}
        a.close()
    return _stored[(n, thin)]


@pytest.mark.parametrize("window_rows", [1, 7, 0])
@pytest.mark.parametrize("n,thin", [(40, 3), (43, 3)])
def test_summarising_sampler_counts_what_its_storing_twin_counts(n, thin, window_rows):
    A = stored_twin(n, thin)
    assert A["info"] == {"bins": 0, "bytes": 0}
    want = counts_of_array(A["draws"], 1, A["edges"])
    assert np.array_equal(A["hist"], want)
    plain = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)      # the same call without a histogram: what arming must not change
    plain.burn(BURN)
    plain.summarize(n, thin, window_rows)
    si_plain, launches_plain = plain.summary_info(), plain.launch_info()["n_launches"]
    plain.close()
    b = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    b.burn(BURN)
    b.set_histogram(A["edges"])
    assert b.histogram_info() == {"bins": TWIN_BINS, "bytes": b.PR * (TWIN_BINS + 1) * 8 + b.PR * (TWIN_BINS + 3) * 8}
    b.summarize(n, thin, window_rows)
    got = b.dataset_histogram()
    assert got.shape == (1, b.PR, TWIN_BINS + 3) and np.array_equal(got, want), (n, thin, window_rows)
    conv = b.convergence()
    assert conv[0].tobytes() == A["conv"][0].tobytes() and conv[1].tobytes() == A["conv"][1].tobytes()
    assert b.state().tobytes() == A["state"].tobytes()
    assert b.summary_info() == si_plain and b.launch_info()["n_launches"] == launches_plain
    brackets_hold(got, A["edges"], A["quantiles"][None], "n=%d thin=%d window=%d" % (n, thin, window_rows))
    # a second summarising call starts its counts afresh; edges afterwards, or another number of bins, are refused
    b.summarize(n, thin, window_rows)
    assert int(b.dataset_histogram().sum()) == b.PR * CHAINS * (-(-n // thin))
    for call in (lambda: b.dataset_histogram(A["edges"]), lambda: amwg_ctypes._check(amwg_ctypes.lib().amwg_last_sample_dataset_histogram(b.h, None, TWIN_BINS + 1, got.ctypes.data_as(amwg_ctypes.C.POINTER(amwg_ctypes.C.c_uint64))))):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_set_histogram" in str(ei.value), str(ei.value)
    b.set_histogram(None)
    assert b.histogram_info() == {"bins": 0, "bytes": 0}
    b.close()


@pytest.mark.parametrize("sizes", [(50, 50, 50, 50), (20, 50, 35, 64)])
def test_a_dataset_sampler_counts_per_dataset(sizes):
    specs = [normal_spec(n_obs, 500 + 7 * d) for d, n_obs in enumerate(sizes)]
    ragged = len(set(sizes)) > 1
    a = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=ragged)
    a.burn(BURN)
    a.sample_async(40, 3)
    a.sync()
    draws = a.fetch_draws()
    # One set of edges per recorded value serves all four datasets, whose posteriors overlap only in part.  A bracket is two bins wide at most when the two order
    # statistics it interpolates lie in one bin or in neighbours, i.e. when a bin is wider than the gap between them: a dataset holds 448 values, and at rank 11
    # (q = 0.025) neighbouring order statistics of a bell-shaped sample are about sd / (448 * 0.058) = 0.04 sd apart.  16 bins over the pooled range (some ten
    # posterior sd) are 0.6 sd wide, fifteen such gaps; 64 bins (0.15 sd) are not enough -- a gap of three of those was met.
    NB = 16
    edges = edges_from(draws, 4, NB)
    want = counts_of_array(draws, 4, edges)
    stored = a.dataset_histogram(edges)
    assert stored.shape == (4, a.PR, NB + 3) and np.array_equal(stored, want)
    for d in range(4):
        assert np.array_equal(stored[d], counts_of_array(draws[:, :, d * 32:(d + 1) * 32], 1, edges)[0])
    fine = edges_from(draws, 4, 500)      # (the counts themselves, under bins far narrower than the brackets' argument allows)
    assert np.array_equal(a.dataset_histogram(fine), counts_of_array(draws, 4, fine))
    quantiles = a.dataset_quantiles(PROBS)
    a.close()
    brackets_hold(stored, edges, quantiles, "datasets " + str(sizes))
    b = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=ragged)
    b.burn(BURN)
    b.set_histogram(edges)
    b.summarize(40, 3, 4)
    assert np.array_equal(b.dataset_histogram(), want)
    b.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_a_translated_closure_counts_its_derived_quantity():
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
    finite = np.where(np.isfinite(draws), draws, 0.0)
    edges = edges_from(finite, 1, 32)
    want = counts_of_array(draws, 1, edges)
    got = a.dataset_histogram(edges)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0, a.P:], want[0, a.P:]) and int(got[0, a.P].sum()) == 10 * 96      # the derived quantity's own cell
    a.close()
    b = amwg_ctypes.Sampler(spec, chains=96, seed=7, lanes_per_chain=1)
    b.burn(BURN)
    b.set_histogram(edges)
    b.summarize(30, 3, 4)
    assert np.array_equal(b.dataset_histogram(), want)
    b.close()


def test_after_summarize_without_an_armed_histogram():
    s = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    edges = np.linspace(-50.0, 250.0, 33)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_histogram(edges)
    assert "amwg_last_sample_dataset_histogram" in str(ei.value) and "no sample() call yet" in str(ei.value)
    s.burn(BURN)
    s.summarize(40, 3, 4)
    for call in (lambda: s.dataset_histogram(), lambda: s.dataset_histogram(edges)):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_set_histogram" in str(ei.value) and "amwg_last_sample_dataset_histogram" in str(ei.value), str(ei.value)
    s.set_histogram(edges)      # armed AFTER the call: there is still nothing counted for it
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_histogram()
    assert "amwg_set_histogram" in str(ei.value)
    draws = s.sample(8)
    got = s.dataset_histogram(edges)
    assert got.shape == (1, s.PR, 35) and np.array_equal(got, counts_of_array(draws, 1, edges))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:      # after a stored call, edges are needed
        s.dataset_histogram()
    assert "null edges" in str(ei.value)
    for bad, why in ((np.array([0.0, 1.0, 1.0]), "not strictly ascending"), (np.array([0.0, np.nan, 2.0]), "not finite"), (np.array([1.0]), "0 bins")):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            s.dataset_histogram(bad)
        assert why in str(ei.value), str(ei.value)
    s.close()


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_histogram_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_histogram.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu histogram ok" in p.stdout, p.stdout + "\n" + p.stderr
