"""Autocovariance along the chains on the device (csrc/amwg_autocov.hip), on the GPU.  tests/README.autocorrelation.md says what each test pins.

(1) the kernels on synthetic arrays, through the test library (amwg_autocovariance_check): bit for bit the restated order (autocovariance_reference.kernel_order),
    inside the cap of exact rational arithmetic, the same bytes however the rows are cut into windows; neighbours, permutations, scaling, the pilot centring.
(2) a sampler that summarises with an armed autocovariance against its twin that stores; dataset samplers; a translated closure with a derived quantity; one
    chain; refusals; tau against thinning and the between-chain ESS.
(3) the JavaScript front end (tests/js/test_gpu_autocorrelation.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import autocovariance_reference as ar
import model_spec
import summary_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
ROWS_LAGS = [(2, 1), (3, 2), (5, 4), (9, 8), (17, 16), (40, 7), (64, 33)]      # L = rows - 1; lag tiles of 8 with a last tile of 1; L no multiple of the tile
CPDS = [1, 2, 3, 64, 255, 256, 257, 513]


def same_bytes(a, b):
    """equal as bytes; a NaN is held to a NaN (its sign and payload are not pinned)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a.view(np.uint64)[keep], b.view(np.uint64)[keep])


def same3(got, want):
    return all(same_bytes(g, w) for g, w in zip(got, want))


# ---- (1) the kernels on synthetic arrays

_worst = [0.0, ""]      # the largest |device - exact| / cap over this file's cases (printed; tests/README.autocorrelation.md records it)


@pytest.mark.parametrize("cpd", CPDS)
@pytest.mark.parametrize("rows,L", ROWS_LAGS)
def test_bytes_cap_and_windows(rows, L, cpd):
    """the pattern rotates over summary_reference's finite ones with the case, so that each is met at several shapes"""
    pattern = sr.FINITE[(ROWS_LAGS.index((rows, L)) + CPDS.index(cpd)) % len(sr.FINITE)]
    a = ar.array(pattern, rows, cpd)
    label = "%s %dx%d L %d" % (pattern, rows, cpd, L)
    got = amwg_ctypes.autocovariance_check(a.draws, ar.D, ar.VALUES, L)
    assert got[0].shape == (ar.D, 3, L + 1) and got[1].shape == got[2].shape == (ar.D, 3)
    want = a.want(L)
    for name, g, w in zip(("acov", "mean", "between"), got, want):
        assert same_bytes(g, w), (label, name, np.argwhere(g != w)[:5].tolist())      # 1. bit for bit the restated order
    worst = [0.0, ""]
    ar.held_to_exact(got, a, L, label, worst)                                       # 2. inside the cap against exact
    for w in sorted({1, 3, max(L - 1, 1), L, L + 1, rows}):                         # 3. windows give the stored path's bytes
        assert same3(amwg_ctypes.autocovariance_check(a.draws, ar.D, ar.VALUES, L, w), got), (label, "window_rows", w)
    if worst[0] > _worst[0]:
        _worst[:] = worst
    print("device vs exact, %s: largest |error| / cap = %.4f (%s); largest so far %.4f (%s)" % (label, worst[0], worst[1], _worst[0], _worst[1]))


@pytest.mark.parametrize("pattern", ["all_equal", "constant_chains_that_differ", "one_nan", "one_inf"])
def test_constant_and_non_finite_columns(pattern):
    a = ar.array(pattern, 9, 64)
    for w in (0, 2):
        acov, mean, between = amwg_ctypes.autocovariance_check(a.draws, ar.D, ar.VALUES, 4, w)
        if pattern in sr.NON_FINITE:
            assert np.all(np.isnan(acov)) and np.all(np.isnan(mean)) and np.all(np.isnan(between))
        else:
            assert np.all(acov == 0.0)      # a constant chain has exact zero deviations about its pilot
            ar.held_to_exact((acov, mean, between), a, 4, pattern, [0.0, ""])
        assert same3((acov, mean, between), a.want(4))


def test_neighbours_do_not_reach_an_output():
    cpd, L = 257, 5
    a = ar.array("healthy", 8, cpd)
    base = amwg_ctypes.autocovariance_check(a.draws, ar.D, ar.VALUES, L)
    for d in range(ar.D):
        for fill in (np.nan, 1e300):
            other = np.full(a.draws.shape, fill)
            for p in ar.VALUES:
                other[:, p, d * cpd:(d + 1) * cpd] = a.draws[:, p, d * cpd:(d + 1) * cpd]
            for w in (0, 3):
                got = amwg_ctypes.autocovariance_check(other, ar.D, ar.VALUES, L, w)
                assert all(same_bytes(g[d], b[d]) for g, b in zip(got, base)), (d, fill, w)
    for fill in (np.nan, 1e300, 0.0):      # the value that was not selected
        other = a.draws.copy()
        other[:, 1, :] = fill
        assert same3(amwg_ctypes.autocovariance_check(other, ar.D, ar.VALUES, L), base), fill
    # a NaN or an infinity among ONE selected value's draws in one dataset: that (dataset, value) is NaN, every other output keeps its bytes
    for bad, w in ((np.nan, 0), (np.inf, 3), (-np.inf, 1)):
        other = a.draws.copy()
        other[5, 0, cpd + 9] = bad      # value 0 = position 1 of VALUES, dataset 1
        got = amwg_ctypes.autocovariance_check(other, ar.D, ar.VALUES, L, w)
        for g, b in zip(got, base):
            hit = np.zeros(b.shape, dtype=bool)
            hit[1, 1] = True
            assert np.all(np.isnan(g[hit])) and same_bytes(g[~hit], b[~hit]), (bad, w)


def test_permutations_of_values_and_datasets():
    a = ar.array("offset1e6", 9, 64)
    L = 8
    base = amwg_ctypes.autocovariance_check(a.draws, ar.D, (0, 2, 3), L)
    for perm in ((2, 0, 3), (3, 2, 0), (0, 3, 2), (3, 0, 2), (2, 3, 0)):
        got = amwg_ctypes.autocovariance_check(a.draws, ar.D, perm, L, 4)
        idx = [(0, 2, 3).index(p) for p in perm]
        assert same3(got, [b[:, idx] for b in base]), perm
    order = [2, 0, 1]
    moved = np.concatenate([a.draws[:, :, d * 64:(d + 1) * 64] for d in order], axis=2)
    assert same3(amwg_ctypes.autocovariance_check(moved, ar.D, (0, 2, 3), L), [b[order] for b in base])


@pytest.mark.parametrize("k", [-200, 300])
def test_scaling_a_value_scales_its_outputs_exactly(k):
    a = ar.array("healthy", 9, 64)
    L = 4
    base = amwg_ctypes.autocovariance_check(a.draws, ar.D, ar.VALUES, L)
    for pos, p in enumerate(ar.VALUES):
        scaled = a.draws.copy()
        scaled[:, p, :] = np.ldexp(scaled[:, p, :], k)
        acov, mean, between = amwg_ctypes.autocovariance_check(scaled, ar.D, ar.VALUES, L, 4)
        want_acov, want_mean = base[0].copy(), base[1].copy()
        want_acov[:, pos] = np.ldexp(want_acov[:, pos], 2 * k)
        want_mean[:, pos] = np.ldexp(want_mean[:, pos], k)
        assert np.all(np.isfinite(want_acov)) and np.all(want_acov[:, pos, 0] > 0)
        assert same_bytes(acov, want_acov) and same_bytes(mean, want_mean), (k, p)


def test_an_exactly_representable_offset_leaves_acov_unchanged():
    """the pilot centring: multiples of 2^-20 (below 2^10) plus 2^20 are exact, so every deviation about the pilot keeps its bits"""
    rng = np.random.default_rng([SEED, 5])
    x = np.round(rng.standard_normal((17, ar.PR, 3 * 70)) * 2.0 ** 18) * 2.0 ** -20
    base = amwg_ctypes.autocovariance_check(x, ar.D, ar.VALUES, 9)
    moved = amwg_ctypes.autocovariance_check(x + 2.0 ** 20, ar.D, ar.VALUES, 9, 5)
    assert same_bytes(moved[0], base[0])      # (mean and between round at the size of the offset: m_c = a + ybar)
    assert np.all(np.abs(moved[1] - base[1] - 2.0 ** 20) <= 2.0 ** 20 * 2.0 ** -52)


# ---- (2) samplers

def normal_spec(n_obs=50, seed=500):
    data = model_spec.make_data("normal", n_obs, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


BURN, CHAINS, LAG = 120, 128, 5
_stored = {}


def stored_twin(n, thin):
    if (n, thin) not in _stored:
        a = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
        a.burn(BURN)
        a.sample_async(n, thin)
        a.sync()
        _stored[(n, thin)] = {"acf": a.dataset_autocovariance(max_lag=LAG), "draws": a.fetch_draws(), "conv": a.convergence(), "state": a.state(),
                              "info": a.autocovariance_info()}
        a.sample_async(n, thin)      # a second batch, which continues the first: what a second summarising call of the twin must give
        a.sync()
        _stored[(n, thin)].update(acf2=a.dataset_autocovariance(max_lag=LAG), draws2=a.fetch_draws())
        a.close()
    return _stored[(n, thin)]


@pytest.mark.parametrize("window_rows", [1, 7, 0])
@pytest.mark.parametrize("n,thin", [(40, 3), (43, 3)])
def test_summarising_sampler_gives_its_storing_twins_bytes(n, thin, window_rows):
    A = stored_twin(n, thin)
    assert A["info"] == {"n_values": 0, "max_lag": 0, "bytes": 0}
    plain = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)      # the same call unarmed: what arming must not change
    plain.burn(BURN)
    plain.summarize(n, thin, window_rows)
    plain_conv, plain_state, plain_mom = plain.convergence(), plain.state(), plain.moments()
    si_plain, launches_plain = plain.summary_info(), plain.launch_info()["n_launches"]
    plain.close()
    b = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    b.burn(BURN)
    K = b.PR
    b.set_autocovariance(range(K), LAG)
    assert b.autocovariance_info() == {"n_values": K, "max_lag": LAG, "bytes": (3 * LAG + 2) * K * CHAINS * 8 + K * 4}
    b.summarize(n, thin, window_rows)
    got = b.dataset_autocovariance()
    assert got[0].shape == (1, K, LAG + 1) and same3(got, A["acf"]), (n, thin, window_rows)
    assert same3(got, ar.kernel_order_all(A["draws"], 1, range(K), LAG))
    mean, sd = b.moments()
    for k in range(K):
        assert abs(got[1][0, k] - mean[k]) <= sr.mean_cap(A["draws"].shape[0] * CHAINS, float(np.mean(np.abs(A["draws"][:, k, :])))), (k, got[1][0, k], mean[k])
    assert same_bytes(mean, plain_mom[0]) and same_bytes(sd, plain_mom[1])
    conv = b.convergence()
    for i in range(2):
        assert conv[i].tobytes() == plain_conv[i].tobytes() == A["conv"][i].tobytes()
    assert b.state().tobytes() == plain_state.tobytes() == A["state"].tobytes()
    assert b.summary_info() == si_plain and b.launch_info()["n_launches"] == launches_plain
    b.summarize(n, thin, window_rows)      # a second call starts afresh: the twin's second batch alone, every byte
    again = b.dataset_autocovariance()
    assert same3(again, A["acf2"]) and same3(again, ar.kernel_order_all(A["draws2"], 1, range(K), LAG)) and not same_bytes(again[0], got[0])
    cd = lambda a: a.ctypes.data_as(amwg_ctypes.C.POINTER(amwg_ctypes.C.c_double))
    raw = lambda k, lag: amwg_ctypes._check(amwg_ctypes.lib().amwg_last_sample_dataset_autocovariance(b.h, None, k, lag, cd(got[0].copy()), cd(got[1].copy()), cd(got[2].copy())))
    for call in (lambda: b.dataset_autocovariance(range(K), LAG), lambda: b.dataset_autocovariance([0]), lambda: b.dataset_autocovariance(max_lag=LAG - 1),
                 lambda: raw(K - 1, LAG), lambda: raw(K, LAG + 1)):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_set_autocovariance" in str(ei.value), str(ei.value)
    # max_lag >= the kept draws: refused before any launch, the chains' state as it was
    state = b.state()
    kept = -(-n // thin)
    b.set_autocovariance([0], kept)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        b.summarize(n, thin, window_rows)
    assert "amwg error -1" in str(ei.value) and "amwg_sample_summarize" in str(ei.value) and "max_lag" in str(ei.value), str(ei.value)
    assert b.state().tobytes() == state.tobytes()
    b.set_autocovariance(None)
    assert b.autocovariance_info() == {"n_values": 0, "max_lag": 0, "bytes": 0}
    b.close()


def test_a_ragged_dataset_sampler_answers_per_dataset():
    sizes = (20, 50, 35, 64)
    specs = [normal_spec(n_obs, 500 + 7 * d) for d, n_obs in enumerate(sizes)]
    a = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True)
    a.burn(BURN)
    a.sample_async(40, 3)
    a.sync()
    draws = a.fetch_draws()
    values = list(range(a.PR))[::-1]
    stored = a.dataset_autocovariance(values, LAG)
    a.close()
    assert stored[0].shape == (4, len(values), LAG + 1) and same3(stored, ar.kernel_order_all(draws, 4, values, LAG))
    b = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True)
    b.burn(BURN)
    b.set_autocovariance(values, LAG)
    b.summarize(40, 3, 4)
    assert same3(b.dataset_autocovariance(), stored)
    b.close()


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
    got = a.dataset_autocovariance(max_lag=LAG)
    a.close()
    assert got[0].shape == (1, a.PR, LAG + 1) and same3(got, ar.kernel_order_all(draws, 1, range(a.PR), LAG))
    b = amwg_ctypes.Sampler(spec, chains=96, seed=7, lanes_per_chain=1)
    b.burn(BURN)
    b.set_autocovariance(range(b.PR), LAG)
    b.summarize(30, 3, 4)
    assert same3(b.dataset_autocovariance(), got)
    b.close()


def test_one_chain_gets_an_effective_sample_size():
    s = amwg_ctypes.Sampler(normal_spec(), chains=1, seed=SEED)
    s.burn(400)
    draws = s.sample(600)
    acov, mean, between = s.dataset_autocovariance(max_lag=60)
    assert same3((acov, mean, between), ar.kernel_order_all(draws, 1, range(s.PR), 60)) and np.all(between == 0.0)
    for k in range(s.PR):
        r = amwg_ctypes.autocorrelation_ess(acov[0, k], between[0, k], 600, 1)
        assert r["rho"][0] == 1.0 and 0.9 <= r["tau"] and 600 / 60.0 < r["ess"] <= 600 / 0.9, r      # a one-at-a-time sampler: tau of a few draws
    with pytest.raises(amwg_ctypes.AmwgError):
        s.convergence()      # the between-chain estimator still needs two chains
    s.close()


def test_without_an_armed_autocovariance_and_without_a_sample():
    s = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_autocovariance([0, 1], 3)
    assert "amwg_last_sample_dataset_autocovariance" in str(ei.value) and "no sample() call yet" in str(ei.value)
    s.burn(BURN)
    s.summarize(40, 3, 4)
    for call in (lambda: s.dataset_autocovariance(), lambda: s.dataset_autocovariance([0, 1], 3)):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_set_autocovariance" in str(ei.value) and "amwg_last_sample_dataset_autocovariance" in str(ei.value), str(ei.value)
    s.set_autocovariance([1, 0], 3)      # armed AFTER the call: there is still nothing folded for it
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_autocovariance()
    assert "amwg_set_autocovariance" in str(ei.value)
    for bad, lag, why in (([0, 0], 3, "listed twice"), ([0, s.PR], 3, "outside the recorded values"), (list(range(s.PR + 1)), 3, "values"), ([0], 0, "max_lag"),
                          ([0], 1025, "max_lag")):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            s.set_autocovariance(bad, lag)
        assert "amwg_set_autocovariance" in str(ei.value) and why in str(ei.value), str(ei.value)
    draws = s.sample(8)
    got = s.dataset_autocovariance([1, 0], 7)
    assert same3(got, ar.kernel_order_all(draws, 1, (1, 0), 7))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_autocovariance([1, 0], 8)      # max_lag >= kept draws
    assert "max_lag" in str(ei.value)
    s.close()


def test_tau_falls_with_thinning_and_the_ess_agrees_with_the_between_chain_one():
    tau, ess, ess_between = {}, {}, {}
    for thin in (1, 5):
        s = amwg_ctypes.Sampler(normal_spec(), chains=256, seed=SEED)
        s.burn(1000)
        s.set_autocovariance(range(s.PR), 50)
        s.summarize(2000 * thin, thin)
        acov, mean, between = s.dataset_autocovariance()
        res = [amwg_ctypes.autocorrelation_ess(acov[0, k], between[0, k], 2000, 256) for k in range(s.PR)]
        tau[thin], ess[thin] = [r["tau"] for r in res], [r["ess"] for r in res]
        ess_between[thin] = s.convergence()[1]
        assert all(r["truncated"] for r in res), res
        s.close()
    print("tau thin 1 %s, thin 5 %s; ess %s / %s against between-chain %s / %s" % (tau[1], tau[5], ess[1], ess[5], ess_between[1], ess_between[5]))
    for k in range(len(tau[1])):
        assert tau[1][k] > tau[5][k] >= 0.9, (k, tau)
        for thin in (1, 5):
            assert 0.5 <= ess[thin][k] / ess_between[thin][k] <= 2.0, (k, thin, ess, ess_between)


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_autocorrelation_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_autocorrelation.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu autocorrelation ok" in p.stdout, p.stdout + "\n" + p.stderr
