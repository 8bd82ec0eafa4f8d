"""Per-dataset quantiles (amwg_last_sample_dataset_quantiles; the radix select at the end of csrc/amwg_summaries.hip), on the GPU.

The oracle everywhere is numpy on the host: x = np.sort(segment), h = (n - 1) q, lo = floor h, hi = min(lo + 1, n - 1), x[lo] + (h - lo) (x[hi] - x[lo]) --
the rule of the pooled call, every operation rounded once.  Results are compared as VALUES (np.array_equal; NaN equal to NaN, which the refused probabilities
and inf - inf produce on both sides): a segment may hold both -0.0 and +0.0, whose order is the key's, and that is the only licence the comparison gives.

(a) the kernel on synthetic arrays draws[rows][3][3 cpd] through the test library (amwg_dataset_quantiles_check): three datasets, so the middle one sits at a
    nonzero offset; every (value, dataset) is checked; shapes from one element to many times the workgroup, value patterns that stress one pass of the select
    each, probability lists that are unsorted, repeat, hit exact ranks, are refused, or cross the kernel's 24 probabilities per launch.
(b) a dataset sampler end to end against the oracle on its own returned draws and against the pooled call (gather + hipCUB sort) of the ordinary twin sampler
    on each dataset -- two independent implementations.
(c) the JavaScript front end (tests/js/test_gpu_dataset_quantiles.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import model_spec
import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261018
PR, D = 3, 3
WORKGROUP = 512      # kSelThreads of csrc/amwg_summaries.hip
P3 = [0.025, 0.5, 0.975]


def oracle(draws, n_datasets, probs):
    """-> [D][PR][len(probs)] by sorting every segment on the host.  A NaN may come only from a refused probability or from an infinite x[lo] or x[hi]
    (inf - inf, 0 * inf): asserted here, so that NaN == NaN in same_values never covers for anything else."""
    rows, pr, chains = draws.shape
    cpd = chains // n_datasets
    n = rows * cpd
    out = np.empty((n_datasets, pr, len(probs)))
    with np.errstate(invalid="ignore"):
        for d in range(n_datasets):
            for p in range(pr):
                x = np.sort(draws[:, p, d * cpd:(d + 1) * cpd].reshape(-1))
                for k, q in enumerate(probs):
                    q = np.float64(q)
                    if not (q >= 0.0 and q <= 1.0):
                        out[d, p, k] = np.nan
                        continue
                    h = np.float64(n - 1) * q
                    lo = int(np.floor(h))
                    hi = min(lo + 1, n - 1)
                    out[d, p, k] = x[lo] + (h - np.float64(lo)) * (x[hi] - x[lo])
                    assert not np.isnan(out[d, p, k]) or np.isinf(x[lo]) or np.isinf(x[hi])
    return out


def same_values(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- (a) synthetic arrays

SHAPES = [(1, 1), (37, 1), (1, 65), (5, 3), (16, 64), (64, 1031), (27, 19)]      # (rows, cpd); 27 x 19 = 513 = the workgroup + 1
assert 27 * 19 == WORKGROUP + 1


def from_bits(u):
    return np.asarray(u, dtype=np.uint64).view(np.float64)


def values(kind, rng, n):
    """the n doubles of one segment, of one pattern"""
    if kind == "narrow_normal":      # N(3, 1e-4): sign, exponent and the leading mantissa digits constant -- every lane of a wavefront names the same bin
        return 3.0 + 1e-4 * rng.standard_normal(n)
    if kind == "all_equal":
        return np.full(n, 1.25)
    if kind == "two_values":         # n // 2 times 1.5, the rest 2.5, scattered: the probability (n // 2 - 0.5) / (n - 1) puts lo on the last 1.5 and hi on the first 2.5
        return rng.permutation(np.where(np.arange(n) < n // 2, 1.5, 2.5))
    if kind == "lowest_byte":        # equal until the eighth pass
        return from_bits(np.float64(1.5).view(np.uint64) + rng.integers(0, 256, n).astype(np.uint64))
    if kind == "mixed_signs":
        v = 1e3 * rng.standard_normal(n)
        v[rng.random(n) < 0.1] = -1e300
        v[rng.random(n) < 0.1] = -3e150
        return v
    if kind == "infinities":
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.15] = np.inf
        v[rng.random(n) < 0.15] = -np.inf
        return v
    if kind == "denormals":
        v = from_bits(rng.integers(0, 1 << 20, n).astype(np.uint64))
        return np.where(rng.random(n) < 0.5, -v, v)
    if kind == "signed_zeros":
        return np.where(rng.random(n) < 0.5, -0.0, 0.0)
    if kind == "small_integers":     # heavy ties
        return rng.integers(-3, 4, n).astype(np.float64)
    raise ValueError(kind)


KINDS = ["narrow_normal", "all_equal", "two_values", "lowest_byte", "mixed_signs", "infinities", "denormals", "signed_zeros", "small_integers"]


def probability_lists(rng, n):
    lists = [[0.5], [0.0, 1.0], [0.975, 0.025, 0.5, 0.5], [-0.1, 1.5, float("nan")], list(rng.random(70))]
    if n > 1:
        exact = [k / (n - 1) for k in sorted({0, 1, n // 3, n // 2, n - 2, n - 1}) if 0 <= k <= n - 1 and float(n - 1) * (k / (n - 1)) == k]
        assert len(exact) >= 2      # (0 and n - 1 always are)
        lists.append(exact)
        lists.append([(m - 0.5) / (n - 1) for m in sorted({1, n // 2, n - 1}) if m >= 1])      # lo = m - 1 and hi = m: neighbours, of different value where the data has a step there
    return lists


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cpd", SHAPES)
def test_kernel_on_synthetic_arrays(rows, cpd, kind):
    rng = np.random.default_rng([SEED, rows, cpd, KINDS.index(kind)])
    n = rows * cpd
    draws = np.empty((rows, PR, D * cpd))
    for p in range(PR):
        for d in range(D):
            draws[:, p, d * cpd:(d + 1) * cpd] = values(kind, rng, n).reshape(rows, cpd)
    for probs in probability_lists(rng, n):
        got = amwg_ctypes.dataset_quantiles_check(draws, D, probs)
        want = oracle(draws, D, probs)
        assert got.shape == (D, PR, len(probs))
        assert same_values(got, want), (rows, cpd, kind, probs[:4], got[:, :, :4], want[:, :, :4])
    if kind == "infinities" and n > 1:
        # the type-7 rule turns every quantile next to an infinity into NaN, on both sides; here the infinities are +-1e300 instead (1e300 - -1e300 does not overflow) -- the same ranks, at
        # the ends of the key range of finite doubles, and every answer a number
        finite = np.where(np.isinf(draws), np.sign(draws) * 1e300, draws)
        probs = [0.0, 0.05, 0.14, 0.5, 0.86, 0.95, 1.0]
        got, want = amwg_ctypes.dataset_quantiles_check(finite, D, probs), oracle(finite, D, probs)
        assert not np.any(np.isnan(want)) and np.array_equal(got, want)
    if kind == "two_values" and n > 1:
        step = amwg_ctypes.dataset_quantiles_check(draws, D, [(n // 2 - 0.5) / (n - 1)])
        assert np.all(step > 1.5) and np.all(step < 2.5)      # strictly between: lo and hi straddle the step


def test_components_and_datasets_are_kept_apart():
    """Every (value, dataset) of one array holds another pattern and another location: a wrong offset or stride shows as another segment's answer."""
    rng = np.random.default_rng([SEED, 99])
    rows, cpd = 9, 70
    draws = np.empty((rows, PR, D * cpd))
    for p in range(PR):
        for d in range(D):
            kind = KINDS[(3 * p + d) % len(KINDS)]
            draws[:, p, d * cpd:(d + 1) * cpd] = (10.0 * (3 * p + d) + values(kind, rng, rows * cpd)).reshape(rows, cpd)
    probs = [0.1, 0.5, 0.9]
    assert same_values(amwg_ctypes.dataset_quantiles_check(draws, D, probs), oracle(draws, D, probs))
    assert same_values(amwg_ctypes.dataset_quantiles_check(draws, 1, probs), oracle(draws, 1, probs))      # one dataset: the whole width


# ---- (b) end to end

def dataset_specs(model, n_obs, n_datasets):
    out = []
    for d in range(n_datasets):
        kw = {"exp": oracle_lib.lib().orc_exp} if model == "pois_glm" else {}
        data = model_spec.make_data(model, n_obs, 500 + 7 * d, **kw)
        data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
        out.append(model_spec.build_spec(model, data))
    return out


def against_oracle_and_twins(model, n_obs, cpd, lanes, block):
    specs = dataset_specs(model, n_obs, 3)
    ds = amwg_ctypes.Sampler(specs, chains=3 * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:      # nothing sampled yet
        ds.dataset_quantiles(P3)
    assert "amwg error -1" in str(ei.value) and "amwg_last_sample_dataset_quantiles" in str(ei.value) and "no sample() call yet" in str(ei.value)
    ds.burn(120)
    draws = ds.sample(160, 3)
    got = ds.dataset_quantiles(P3)
    assert got.shape == (3, ds.PR, 3)
    assert same_values(got, oracle(draws, 3, P3))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:      # the pooled call stays refused, and its message names the way out
        ds.quantiles(P3)
    assert "amwg_last_sample_dataset_quantiles" in str(ei.value)
    for d in range(3):
        twin = amwg_ctypes.Sampler(specs[d], chains=cpd, seed=SEED, chain_offset=d * cpd, lanes_per_chain=lanes, block_threads=block)
        twin.burn(120)
        twin.sample(160, 3)
        assert np.array_equal(got[d], twin.quantiles(P3)), d
        twin.close()
    return ds, got


def test_normal_datasets_equal_the_oracle_and_the_pooled_call_of_each_twin():
    ds, first = against_oracle_and_twins("normal", 300, 64, 1, 64)
    # a second sample() of another length, then a second call: the new sample's quantiles, nothing left over from the first
    draws = ds.sample(50, 2)
    second = ds.dataset_quantiles(P3)
    assert same_values(second, oracle(draws, 3, P3)) and not np.array_equal(first, second)
    ds.close()


def test_poisson_glm_datasets_more_than_two_recorded_values():
    ds, got = against_oracle_and_twins("pois_glm", 300, 16, 16, 256)
    assert ds.PR > 2
    ds.close()


def test_an_ordinary_sampler_gives_the_pooled_result():
    spec = dataset_specs("normal", 300, 1)[0]
    s = amwg_ctypes.Sampler(spec, chains=64, seed=SEED, lanes_per_chain=1, block_threads=64)
    s.burn(120)
    s.sample(40, 3)
    probs = [0.025, 0.25, 0.5, 0.75, 0.975, 0.0, 1.0]
    got = s.dataset_quantiles(probs)
    assert got.shape == (1, s.PR, len(probs)) and np.array_equal(got[0], s.quantiles(probs))
    s.close()


# ---- (c) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_dataset_quantiles_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_dataset_quantiles.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu dataset quantiles ok" in p.stdout, p.stdout + "\n" + p.stderr
