"""-m gpu: split-R-hat, ESS, mean and sd of stored draws (csrc/amwg_diag.hip: chain_halves_kernel / the fold, dataset_diagnostics_kernel, dataset_moments_kernel, the
pooled call's host reduction) on synthetic arrays, through the launchers the sampler's calls use (amwg_summaries_check in the test library).

Every array is draws[rows][3][3 cpd]: three values and three datasets, so the middle dataset and the middle value sit at nonzero offsets, and every (dataset, value)
holds other numbers.  The references are tests/summary_reference.py: the kernels' ORDER restated in numpy float64 (bit for bit) and exact rational arithmetic (inside
the caps of tests/README.summaries.md, which come from the reference alone: tests/test_summary_reference_host.py).  Patterns: R-hat near 1 and far from it, a
stuck chain, integers, W = 0, a NaN, an infinity; shapes: the minima, an odd last row, 255 / 256 / 257 and 513 chains per dataset around the 256-thread workgroup.

(a) bit for bit against the restated order, stored and folded halves; (b) against exact; (c) neighbours, permutations, scaling by powers of two;
(d) a real sampler started far from convergence, through convergence(), group_convergence, dataset_convergence() and summarize()."""
import math

import numpy as np
import pytest

import amwg_ctypes
import model_spec
import summary_reference as R

pytestmark = pytest.mark.gpu
PR, D = R.PR, R.D
DS_KEYS = ("mean", "sd", "rhat_ds", "ess_ds")
ALL_KEYS = DS_KEYS + ("rhat_pooled", "ess_pooled")


def ids(shape):
    return "%dx%d" % shape


def same_bytes(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def same_values(a, b):
    """bit for bit, a NaN equal to a NaN whatever its payload (numpy's and the device's quiet NaN need not share one)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))


# ---- (a) + (b)

@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("name", R.PATTERNS)
def test_kernels_follow_the_restated_order_and_stay_inside_the_cap(name, shape):
    rows, cpd = shape
    c = R.case(name, rows, cpd)
    got = amwg_ctypes.summaries_check(c.draws, D)
    print("%s %dx%d rhat_ds %r\n  restated %r\n  ess_ds %r\n  restated %r" % (name, rows, cpd, got["rhat_ds"].tolist(), c.rhat.tolist(), got["ess_ds"].tolist(), c.ess.tolist()))
    assert same_values(got["rhat_ds"], c.rhat), (got["rhat_ds"], c.rhat)
    assert same_values(got["ess_ds"], c.ess), (got["ess_ds"], c.ess)
    assert same_values(got["mean"], c.mean), (got["mean"], c.mean)
    assert same_values(got["sd"], c.sd), (got["sd"], c.sd)
    # the summarised path: the fold in windows of 1, 3 and all the rows gives the stored path's bytes -- the device's own NaNs included
    for window_rows in (1, 3, rows):
        folded = amwg_ctypes.summaries_check(c.draws, D, window_rows)
        for k in ALL_KEYS:
            assert same_bytes(folded[k], got[k]), (k, window_rows, folded[k], got[k])
    # against exact: per segment, and the pooled call's long double host order (not restated) over all the chains
    worst, half = {}, rows // 2
    for d in range(D):
        for p in range(PR):
            e = c.exact[d][p]
            R.held_to_exact([("rhat", got["rhat_ds"][d, p], e), ("ess", got["ess_ds"][d, p], e), ("mean", got["mean"][d, p], e), ("sd", got["sd"][d, p], e)],
                            half, cpd, rows * cpd, "%s %dx%d (d %d, p %d)" % (name, rows, cpd, d, p), worst)
    for p in range(PR):
        e = c.pooled[p]
        R.held_to_exact([("rhat", got["rhat_pooled"][p], e), ("ess", got["ess_pooled"][p], e)], half, D * cpd, rows * D * cpd, "%s %dx%d (pooled, p %d)" % (name, rows, cpd, p), worst)
    print("largest |device - exact| / cap:", worst)
    # one dataset of all the chains: the dataset kernel and the pooled call answer the same question in two orders
    one = amwg_ctypes.summaries_check(c.draws, 1)
    for p in range(PR):
        e = c.pooled[p]
        R.held_to_exact([("rhat", one["rhat_ds"][0, p], e), ("ess", one["ess_ds"][0, p], e), ("mean", one["mean"][0, p], e), ("sd", one["sd"][0, p], e)],
                        half, D * cpd, rows * D * cpd, "%s %dx%d (D = 1, p %d)" % (name, rows, cpd, p), worst)
        want = R.kernel_order(np.ascontiguousarray(c.draws[:, p, :]))      # (up to 1 539 chains in one workgroup: seven strided rounds)
        assert same_values(one["rhat_ds"][0, p], want[0]) and same_values(one["ess_ds"][0, p], want[1]), (p, one["rhat_ds"][0, p], one["ess_ds"][0, p], want)
    assert same_bytes(one["rhat_pooled"], got["rhat_pooled"]) and same_bytes(one["ess_pooled"], got["ess_pooled"])
    if name in R.W_ZERO + R.NON_FINITE:      # the library's rule for degenerate columns (include/amwg.h)
        assert np.all(np.isnan(got["rhat_ds"])) and np.all(np.isnan(got["rhat_pooled"]))
        if name != "constant_chains_that_differ":
            assert np.all(np.isnan(got["ess_ds"]))
    if name == "two_camps":
        assert np.all(got["rhat_ds"] > 2.5) and np.all(got["rhat_pooled"] > 2.5)


# ---- (c)

SMALL = [(5, 3), (8, 257), (64, 70)]


@pytest.mark.parametrize("shape", SMALL, ids=ids)
@pytest.mark.parametrize("filler", [float("nan"), 1e300])
def test_neighbours_do_not_reach_a_segment(shape, filler):
    """Everything but one (dataset, value) overwritten: that segment's mean, sd, rhat and ess keep their bytes; everything but one value overwritten: that value's
    pooled rhat and ess keep theirs.  A wrong stride or offset reads the filler."""
    rows, cpd = shape
    c = R.case("two_camps", rows, cpd)
    base = amwg_ctypes.summaries_check(c.draws, D)
    for d, p in ((1, 1), (0, 2), (2, 0)):
        alone = np.full_like(c.draws, filler)
        alone[:, p, d * cpd:(d + 1) * cpd] = c.draws[:, p, d * cpd:(d + 1) * cpd]
        got = amwg_ctypes.summaries_check(alone, D)
        for k in DS_KEYS:
            assert same_bytes(got[k][d, p], base[k][d, p]), (k, d, p, got[k][d, p], base[k][d, p])
        alone = np.full_like(c.draws, filler)
        alone[:, p, :] = c.draws[:, p, :]
        got = amwg_ctypes.summaries_check(alone, D)
        for k in ("rhat_pooled", "ess_pooled"):
            assert same_bytes(got[k][p], base[k][p]), (k, p, got[k], base[k])


@pytest.mark.parametrize("shape", SMALL, ids=ids)
def test_permuting_datasets_or_values_permutes_the_outputs(shape):
    rows, cpd = shape
    c = R.case("trend", rows, cpd)
    base = amwg_ctypes.summaries_check(c.draws, D)
    for perm in ((1, 2, 0), (2, 1, 0)):
        by_value = amwg_ctypes.summaries_check(c.draws[:, perm, :], D)
        for k in DS_KEYS:
            assert same_bytes(by_value[k], base[k][:, perm]), (k, perm)
        for k in ("rhat_pooled", "ess_pooled"):
            assert same_bytes(by_value[k], base[k][list(perm)]), (k, perm)
        blocks = np.concatenate([c.draws[:, :, d * cpd:(d + 1) * cpd] for d in perm], axis=2)
        by_dataset = amwg_ctypes.summaries_check(blocks, D)
        for k in DS_KEYS:      # (the pooled call sums the chains in another order then: held to exact above, not to bytes)
            assert same_bytes(by_dataset[k], base[k][list(perm), :]), (k, perm)


@pytest.mark.parametrize("shape", SMALL, ids=ids)
@pytest.mark.parametrize("k", [-200, 300])
def test_scaling_by_a_power_of_two_is_exact(shape, k):
    """x 2^k with nothing overflowing, underflowing or subnormal: every operation of the kernels commutes with it, so R-hat and ESS keep their bytes, mean and sd scale"""
    rows, cpd = shape
    for name in ("healthy", "offset1e9_sd1e-3", "two_camps", "integers", "tiny_between", "one_stuck"):
        c = R.case(name, rows, cpd)
        base = amwg_ctypes.summaries_check(c.draws, D)
        got = amwg_ctypes.summaries_check(np.ldexp(c.draws, k), D)
        for key in ("rhat_ds", "ess_ds", "rhat_pooled", "ess_pooled"):
            assert same_bytes(got[key], base[key]), (name, key, got[key], base[key])
        for key in ("mean", "sd"):
            assert same_bytes(got[key], np.ldexp(base[key], k)), (name, key)


# ---- (d) a real sampler that has not converged: the paths no array can be fed into

CHAINS, KEPT = 192, 9


def normal_spec(seed):
    data = model_spec.make_data("normal", 400, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


def far_apart(chains, first=0):
    """mu = +50 / -50 in alternating chains (by global chain id), sigma = 2"""
    c = np.arange(first, first + chains)
    return np.stack([np.where(c % 2 == 0, 50.0, -50.0), np.full(chains, 2.0)])


def held(rhat, ess, draws, n_datasets, label):
    """rhat, ess [n_datasets][PR] against exact on the draws the call itself returned"""
    rows, pr, chains = draws.shape
    cpd, worst = chains // n_datasets, {}
    for d in range(n_datasets):
        for p in range(pr):
            e = R.exact(R.segment(draws, d, p, n_datasets))
            print("%s (d %d, p %d): rhat %r exact %r, ess %r exact %r" % (label, d, p, rhat[d][p], e["rhat"], ess[d][p], e["ess"]))
            R.held_to_exact([("rhat", rhat[d][p], e), ("ess", ess[d][p], e)], rows // 2, cpd, rows * cpd, "%s (d %d, p %d)" % (label, d, p), worst)
        assert rhat[d][0] > 2 and math.isfinite(ess[d][0]), (label, d, rhat[d], ess[d])      # it must not quietly become a healthy case
    print(label, "largest |device - exact| / cap:", worst)


def test_an_unconverged_sampler_pooled_group_and_summarised():
    spec = normal_spec(5)
    s = amwg_ctypes.Sampler(spec, chains=CHAINS, seed=31, lanes_per_chain=1)
    s.set_state(far_apart(CHAINS))
    draws = s.sample(KEPT, 1)
    assert draws.shape == (KEPT, 2, CHAINS)      # an odd number of kept draws: the last is ignored
    rhat, ess = s.convergence()
    held([rhat], [ess], draws, 1, "convergence()")
    # the same question through the kernels on the returned array
    chk = amwg_ctypes.summaries_check(draws, 1)
    assert same_bytes(chk["rhat_pooled"], rhat) and same_bytes(chk["ess_pooled"], ess)
    rd, ed = s.dataset_convergence()
    assert same_bytes(chk["rhat_ds"], rd) and same_bytes(chk["ess_ds"], ed)
    held(rd, ed, draws, 1, "dataset_convergence() of an ordinary sampler")
    m, sd = s.moments()
    assert same_bytes(chk["mean"][0], m) and same_bytes(chk["sd"][0], sd)
    # three unequal shards of the same job
    shards, blocks, first = [], [], 0
    for n in (72, 64, 56):
        q = amwg_ctypes.Sampler(spec, chains=n, seed=31, chain_offset=first, lanes_per_chain=1)
        q.set_state(far_apart(n, first))
        blocks.append(q.sample(KEPT, 1))
        shards.append(q)
        first += n
    pooled = np.concatenate(blocks, axis=2)
    assert pooled.tobytes() == draws.tobytes()
    rg, eg = amwg_ctypes.group_convergence(shards)
    held([rg], [eg], pooled, 1, "group_convergence")
    for q in shards:
        q.close()
    # the summarising twin: its storing twin's bytes
    t = amwg_ctypes.Sampler(spec, chains=CHAINS, seed=31, lanes_per_chain=1)
    t.set_state(far_apart(CHAINS))
    assert t.summarize(KEPT, 1, 4) == KEPT
    rt, et = t.convergence()
    assert same_bytes(rt, rhat) and same_bytes(et, ess), (rt, rhat, et, ess)
    t.close()
    s.close()


def test_an_unconverged_dataset_sampler_stored_and_summarised():
    specs = [normal_spec(500 + 7 * d) for d in range(3)]
    s = amwg_ctypes.Sampler(specs, chains=CHAINS, seed=31, lanes_per_chain=1)
    s.set_state(far_apart(CHAINS))
    draws = s.sample(KEPT, 1)
    rhat, ess = s.dataset_convergence()
    assert rhat.shape == (3, 2)
    held(rhat, ess, draws, 3, "dataset_convergence()")
    chk = amwg_ctypes.summaries_check(draws, 3)
    assert same_bytes(chk["rhat_ds"], rhat) and same_bytes(chk["ess_ds"], ess)
    s.close()
    t = amwg_ctypes.Sampler(specs, chains=CHAINS, seed=31, lanes_per_chain=1)
    t.set_state(far_apart(CHAINS))
    t.summarize(KEPT, 1, 2)
    rt, et = t.dataset_convergence()
    assert same_bytes(rt, rhat) and same_bytes(et, ess), (rt, rhat, et, ess)
    t.close()
