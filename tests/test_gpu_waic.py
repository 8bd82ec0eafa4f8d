"""WAIC per dataset on the device (csrc/amwg_waic.hip), on the GPU.  tests/README.waic.md says what each test pins.

(1) the kernels on synthetic draws and data, through the test library (amwg_waic_check): the terms l_si AS BYTES against the host twins for all four families;
    lppd_i and p_i within the bounds of include/amwg.h (u = 2^-53, E = 8 (S + 16) u) against extended precision; the totals AS BYTES against waic_totals of the
    returned pointwise bytes; the draw patterns that break a careless accumulation; isolation, non-finite draws, repeatability, batches under a scratch budget.
(2) samplers: Normal, ragged Normal, Poisson and Bernoulli dataset samplers, the hierarchical family; the refusals by their messages.
(3) the JavaScript front end (tests/js/test_gpu_waic.js).
Every comparison prints its largest error / bound ratio before it asserts."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import model_spec
import waic_reference as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021
N_OBS = [1, 2, 63, 64, 65, 257, 1025]
SHAPES = [(rows, cpd) for rows in (1, 2, 17) for cpd in (1, 2, 3, 64, 65) if rows * cpd >= 2]


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


worst = {"lppd": 0.0, "p": 0.0}


def same_values(a, b):
    """the same NaN pattern, and the same bytes wherever there is a number"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


def held(draws, specs, loglik=True, **kw):
    """the device's answer for draws [rows][PR][C] over the datasets `specs`, compared with the reference: terms as bytes, pairs within the bounds, totals as bytes"""
    D = len(specs)
    got = amwg_ctypes.waic_check(draws, specs, pointwise=True, loglik=loglik, **kw)
    for d, spec in enumerate(specs):
        n = spec["n_obs"]
        ll = wr.loglik_of(spec, wr.draws_of_dataset(draws, D, d))
        if loglik:
            dev = got["loglik"][d][:, :n]
            assert dev.tobytes() == ll.tobytes(), (spec["model"], d, draws.shape, np.argwhere(dev.view(np.uint64) != ll.view(np.uint64))[:5])
            assert np.isnan(got["loglik"][d][:, n:]).all()
        pw = got["pointwise"][d]
        rl, rp = wr.worst_ratio(pw[:n], ll)
        print("%s rows %d C %d dataset %d n %d: lppd error / bound %.3g, p error / bound %.3g" % (spec["model"], draws.shape[0], draws.shape[2], d, n, rl, rp))
        worst["lppd"], worst["p"] = max(worst["lppd"], rl), max(worst["p"], rp)
        assert rl <= 1.0 and rp <= 1.0, (spec["model"], d, draws.shape, rl, rp)
        assert np.isnan(pw[n:]).all()
        summary, high = amwg_ctypes.waic_totals(pw, n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d], (summary, got["summary"][d], high, got["high"][d])
    return got


# ---- (1) the kernels on synthetic draws and data

@pytest.mark.parametrize("k,shape", list(enumerate(SHAPES)))
def test_shapes_normal_ragged(k, shape):
    rows, cpd = shape
    rng = np.random.default_rng(SEED + k)
    sizes = [N_OBS[k % 7], N_OBS[(k + 2) % 7], N_OBS[(k + 4) % 7]]
    specs = [spec_of("normal", n, rng) for n in sizes]
    held(draws_for("normal", rows, 3 * cpd, rng), specs)


@pytest.mark.parametrize("model", ["beta_bern", "pois_glm", "hier_normal"])
@pytest.mark.parametrize("rows,cpd", [(1, 2), (2, 3), (17, 65)])
def test_shapes_of_the_other_families(model, rows, cpd):
    rng = np.random.default_rng(SEED + 100 + rows)
    D = 1 if model == "hier_normal" else 3
    sizes = {1: [65, 2, 63], 2: [1, 64, 257], 17: [63, 2, 130]}[rows][:D]
    specs = [spec_of(model, n, rng) for n in sizes]
    if model == "beta_bern":
        specs[0]["data"]["x"][0] = 0.5      # an invalid observation: -inf in every draw, NaN for its pair and its dataset's totals
    got = held(draws_for(model, rows, D * cpd, rng, n_obs=max(sizes)), specs)
    if model == "beta_bern":
        assert np.isnan(got["pointwise"][0][0]).all() and np.isnan(got["summary"][0]).all() and not np.isnan(got["summary"][1:]).any()


def test_a_poisson_change_point_inside_the_data_and_negative_counts():
    rng = np.random.default_rng(SEED + 7)
    spec = spec_of("pois_glm", 70, rng)
    spec["data"]["y"][5] = -1.0      # lfactorial = +inf: the term is -inf in every draw
    draws = draws_for("pois_glm", 3, 8, rng, n_obs=70)
    draws[:, 8, :] = rng.integers(0, 70, size=(3, 8))
    draws[0, 8, 0], draws[1, 8, 1] = np.nan, 1e12      # a change point that never arrives
    got = held(draws, [spec])
    assert np.isnan(got["pointwise"][0][5]).all() and not np.isnan(got["pointwise"][0][:5]).any()


def normal_case(x, mu, sigma, rows):
    """one Normal dataset under the draws (mu_s, sigma_s), s in draw order"""
    S = len(mu)
    cpd = S // rows
    assert cpd * rows == S
    draws = np.stack([np.asarray(mu, dtype=np.float64).reshape(rows, cpd), np.asarray(sigma, dtype=np.float64).reshape(rows, cpd)], axis=1)
    return draws, [{"model": "normal", "n_obs": len(x), "data": {"x": np.asarray(x, dtype=np.float64)}}]


@pytest.mark.parametrize("S,rows", [(2, 1), (65, 1), (17 * 64, 17), (4096, 8)])
def test_identical_draws(S, rows):
    rng = np.random.default_rng(SEED + 20)
    draws, specs = normal_case(rng.normal(size=65), np.full(S, 0.3), np.full(S, 1.7), rows)
    got = held(draws, specs)
    ll = wr.loglik_normal(specs[0]["data"]["x"], [0.3], [1.7])[0]
    assert (got["pointwise"][0][:, 1] == 0.0).all() and np.abs(got["pointwise"][0][:, 0] - ll).max() <= 8 * (S + 16) * wr.U + 4 * wr.U * np.abs(ll).max()


@pytest.mark.parametrize("S,rows,at", [(65, 1, 0), (1105, 17, 1104), (4096, 8, 1234)])
def test_one_dominating_draw(S, rows, at):
    rng = np.random.default_rng(SEED + 21)
    mu, sigma = np.full(S, 1e3) + rng.normal(size=S), np.ones(S)
    mu[at] = 0.0
    draws, specs = normal_case(rng.normal(size=64), mu, sigma, rows)
    got = held(draws, specs)
    assert (got["pointwise"][0][:, 0] < -np.log(S) + 0.0).all() and (got["pointwise"][0][:, 0] > -np.log(S) - 20).all()      # lppd_i = l_(at, i) - log S: the rest underflow


@pytest.mark.parametrize("S,rows", [(65, 1), (1105, 17)])
def test_a_tiny_sigma(S, rows):
    rng = np.random.default_rng(SEED + 22)
    draws, specs = normal_case(rng.normal(size=65), rng.normal(size=S), np.full(S, 1e-6), rows)
    ll = wr.loglik_normal(specs[0]["data"]["x"], draws[:, 0].ravel(), draws[:, 1].ravel())
    assert np.abs(ll).max() > 1e11
    held(draws, specs)


@pytest.mark.parametrize("S,rows", [(65, 1), (1105, 17), (4096, 8)])
def test_cancellation(S, rows):
    rng = np.random.default_rng(SEED + 23)
    x = 1000.0 + rng.normal(size=65)
    draws, specs = normal_case(x, 1e-3 * rng.normal(size=S), np.full(S, 10.0), rows)
    ll = wr.loglik_normal(x, draws[:, 0].ravel(), draws[:, 1].ravel())
    lppd, p, mean, maxabs = wr.pointwise(ll)
    assert (mean * mean / p >= 1e8).all()
    _, bp = wr.bounds(S, lppd, p, mean, maxabs)
    assert (np.abs(wr.one_pass_p(ll) - p) > bp).any(), "the case went soft: a one-pass sum of squares passes it"
    held(draws, specs)


def iso_case(model, rng):
    sizes = [65, 130, 20]
    specs = [spec_of(model, n, rng) for n in sizes]
    return draws_for(model, 6, 3 * 40, rng, n_obs=130), specs


@pytest.mark.parametrize("model", ["normal", "beta_bern", "pois_glm"])
@pytest.mark.parametrize("fill", [np.nan, 1e300])
def test_neighbours_do_not_reach_a_dataset(model, fill):
    rng = np.random.default_rng(SEED + 30)
    draws, specs = iso_case(model, rng)
    base = amwg_ctypes.waic_check(draws, specs)
    other = draws.copy()
    other[:, :, :40] = fill
    other[:, :, 80:] = fill
    others = [dict(s, data={k: (np.full_like(v, fill) if v.dtype == np.float64 else v) for k, v in s["data"].items()}) for s in specs]
    others[1] = specs[1]
    got = amwg_ctypes.waic_check(other, others)
    assert got["pointwise"][1].tobytes() == base["pointwise"][1].tobytes() and got["summary"][1].tobytes() == base["summary"][1].tobytes() and got["high"][1] == base["high"][1]
    assert not np.isnan(base["summary"]).any()
    # ... nor does the number of datasets beside it: dataset 1 alone, at the same (rows, C / D)
    alone = amwg_ctypes.waic_check(np.ascontiguousarray(draws[:, :, 40:80]), [specs[1]])
    assert alone["pointwise"][0][:130].tobytes() == base["pointwise"][1][:130].tobytes() and alone["summary"][0].tobytes() == base["summary"][1].tobytes()


def test_one_non_finite_draw_reaches_its_own_dataset_only():
    rng = np.random.default_rng(SEED + 31)
    draws, specs = iso_case("normal", rng)
    base = amwg_ctypes.waic_check(draws, specs)
    bad = draws.copy()
    bad[3, 1, 40 + 17] = 0.0      # sigma = 0 in one draw of dataset 1
    got = held(bad, specs)
    assert np.isnan(got["pointwise"][1]).all() and np.isnan(got["summary"][1]).all()
    for d in (0, 2):
        assert got["pointwise"][d].tobytes() == base["pointwise"][d].tobytes() and got["summary"][d].tobytes() == base["summary"][d].tobytes()
    draws, specs = iso_case("beta_bern", rng)
    base = amwg_ctypes.waic_check(draws, specs)
    bad = draws.copy()
    bad[2, 0, 40 + 5] = 0.0       # theta = 0: log(theta) = -inf for the observations with x_i = 1
    got = held(bad, specs)
    ones = specs[1]["data"]["x"] == 1
    assert ones.any() and not ones.all()
    assert np.isnan(got["pointwise"][1][:130][ones]).all() and not np.isnan(got["pointwise"][1][:130][~ones]).any()      # (x_i = 0: log(1 - 0) = 0 in that draw, within the bounds: held)
    assert np.isnan(got["summary"][1]).all()
    for d in (0, 2):
        assert got["pointwise"][d].tobytes() == base["pointwise"][d].tobytes() and got["summary"][d].tobytes() == base["summary"][d].tobytes()


def test_two_calls_and_any_scratch_budget_return_the_same_bytes():
    rng = np.random.default_rng(SEED + 32)
    specs = [spec_of("normal", n, rng) for n in (257, 65, 1025, 2)]
    draws = draws_for("normal", 17, 4 * 65, rng)      # S = 1105: four runs of draws per dataset, 32 bytes a partial
    base = held(draws, specs, loglik=False)
    again = amwg_ctypes.waic_check(draws, specs)
    sizes = [4 * n * 32 for n in (257, 65, 1025, 2)]
    for budget in (1, sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2] - 1, sum(sizes)):      # every dataset alone; (0, 1) (2) (3); (0, 1) (2, 3); all four at once
        got = amwg_ctypes.waic_check(draws, specs, scratch_bytes=budget)
        for k in ("pointwise", "summary", "high"):
            assert got[k].tobytes() == base[k].tobytes() == again[k].tobytes(), (budget, k)


def test_refused_before_a_device_call():
    x = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}
    for draws, specs, words in ((np.zeros((1, 2, 1)), [x], "fewer than 2 draws"), (np.zeros((2, 1, 2)), [x], "reads 2 components"), (np.zeros((2, 2, 3)), [x, x], "bad shape"),
                                (np.zeros((2, 2, 2)), [x, dict(x, model="beta_bern")], "is of model")):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            amwg_ctypes.waic_check(draws, specs, device=99)      # (no such device: the refusal comes first)
        assert "amwg_waic_check" in str(ei.value) and words in str(ei.value), str(ei.value)


# ---- (2) samplers

def family_spec(model, n_obs, seed, G=8):
    data = model_spec.make_data(model, n_obs, seed, G=G)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype != np.int32 else v) for k, v in data.items()}
    return model_spec.build_spec(model, data, G=G if model == "hier_normal" else None)


BURN = 200


def against_reference(s, specs, draws, got):
    D = len(specs)
    assert got["summary"].shape == (D, 4) and got["pointwise"].shape == (D, max(q["n_obs"] for q in specs), 2)
    for d, spec in enumerate(specs):
        n = spec["n_obs"]
        ll = wr.loglik_of(spec, wr.draws_of_dataset(draws, D, d))
        rl, rp = wr.worst_ratio(got["pointwise"][d][:n], ll)
        print("%s sampler, dataset %d (n = %d): lppd error / bound %.3g, p error / bound %.3g; elpd %.4f se %.4f p_waic %.4f" % ((spec["model"], d, n, rl, rp) + tuple(got["summary"][d][:3])))
        assert rl <= 1.0 and rp <= 1.0
        summary, high = amwg_ctypes.waic_totals(got["pointwise"][d], n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d]
        assert np.isnan(got["pointwise"][d][n:]).all()


def test_a_normal_sampler():
    spec = family_spec("normal", 50, 500)
    s = amwg_ctypes.Sampler(spec, chains=128, seed=SEED)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_waic()
    assert "amwg_last_sample_dataset_waic" in str(ei.value) and "no sample() call yet" in str(ei.value)
    s.burn(BURN)
    draws = s.sample(40)
    got = s.dataset_waic(pointwise=True)
    against_reference(s, [spec], draws, got)
    one, plain = s.waic(pointwise=True), s.dataset_waic()
    assert [one["elpd_waic"], one["se"], one["p_waic"], one["lppd"]] == got["summary"][0].tolist() and one["high"] == got["high"][0]
    assert one["pointwise"].tobytes() == got["pointwise"][0].tobytes() and plain["summary"].tobytes() == got["summary"].tobytes() and "pointwise" not in plain
    print("Normal model, n = 50, 128 chains x 40 draws: p_waic = %.4f (two parameters)" % one["p_waic"])
    s.summarize(40, 1, 0)
    for call in (s.dataset_waic, s.waic):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_last_sample_dataset_waic" in str(ei.value) and "amwg_sample_summarize" in str(ei.value), str(ei.value)
    s.close()


def test_a_ragged_normal_dataset_sampler():
    specs = [family_spec("normal", n, 500 + 7 * d) for d, n in enumerate((20, 50, 35, 64))]
    a = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True)
    a.burn(BURN)
    draws = a.sample(40)
    against_reference(a, specs, draws, a.dataset_waic(pointwise=True))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        a.waic()
    assert "pooled summaries are refused" in str(ei.value) and "amwg_last_sample_dataset_waic" in str(ei.value) and "dataset_waic" in str(ei.value)
    a.close()


@pytest.mark.parametrize("model,n_obs", [("pois_glm", 40), ("beta_bern", 70)])
def test_a_dataset_sampler_of(model, n_obs):
    specs = [family_spec(model, n_obs, 600 + 11 * d) for d in range(2)]
    a = amwg_ctypes.Sampler(specs, chains=2 * 32, seed=SEED)
    a.burn(BURN)
    draws = a.sample(30)
    against_reference(a, specs, draws, a.dataset_waic(pointwise=True))
    a.close()


def test_the_hierarchical_family():
    spec = family_spec("hier_normal", 96, 700, G=8)
    s = amwg_ctypes.Sampler(spec, chains=64, seed=SEED)
    s.burn(BURN)
    draws = s.sample(30)
    against_reference(s, [spec], draws, s.dataset_waic(pointwise=True))
    s.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_a_translated_closure_is_refused():
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
    a.burn(50)
    a.sample(10)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        a.dataset_waic()
    a.close()
    assert "amwg_last_sample_dataset_waic" in str(ei.value) and "the pointwise terms of a closure are not known to the library; built-in families only" in str(ei.value)


def test_the_largest_ratios_seen():
    """(runs last in this file: what tests/README.waic.md quotes)"""
    print("largest error / bound over this run: lppd %.3g, p %.3g" % (worst["lppd"], worst["p"]))
    assert worst["lppd"] <= 1.0 and worst["p"] <= 1.0


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_waic_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_waic.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu waic ok" in p.stdout, p.stdout + "\n" + p.stderr
