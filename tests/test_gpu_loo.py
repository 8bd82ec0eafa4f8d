"""PSIS-LOO per dataset on the device (csrc/amwg_loo.hip), on the GPU.  tests/README.loo.md says what each test pins.

(1) the kernels on synthetic draws and data, through the test library (amwg_loo_check): the M + 1 smallest terms of every observation, sorted, AS BYTES against the
    key-order sort of the device's own terms (waic_check(loglik=True), which tests/test_gpu_waic.py pins against the host twins); khat_i and elpd_loo_i within the
    bounds of include/amwg.h against the rule in extended precision (tests/loo_reference.py); lppd_i AS BYTES against WAIC's and within WAIC's bound; the totals and
    `high` AS BYTES against loo_totals of the returned pointwise bytes; the draw patterns; isolation, non-finite draws, repeatability, batches under a scratch budget.
(2) samplers: Normal, ragged Normal, Poisson and Bernoulli dataset samplers, the hierarchical family; the refusals by their messages.
(3) the JavaScript front end (tests/js/test_gpu_loo.js).
Every comparison prints its largest error / bound ratio before it asserts."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import loo_reference as lr
import model_spec
import waic_reference as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = lr.SEED

worst = {"elpd": 0.0, "khat": 0.0, "lppd": 0.0, "seen": 0}


def same_values(a, b):
    """the same NaN pattern, and the same bytes wherever there is a number"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


def compare(label, pw, ll, S):
    """one dataset's triples pw [n][3] against the reference over its terms ll [S][n]"""
    ref_e, ref_k = lr.pointwise(ll)
    re, rk = lr.ratios(pw[:, 0], pw[:, 2], ref_e, ref_k, S)
    lppd, p, mean, maxabs = wr.pointwise(ll)
    bl, _ = wr.bounds(S, lppd, p, mean, maxabs)
    ok = ~np.isnan(ref_e)
    assert (np.isnan(pw[:, 1]) == ~ok).all(), "lppd_i: the NaN pattern differs from the reference's"
    rl = float((np.abs(pw[ok, 1] - lppd[ok]) / bl[ok]).max()) if ok.any() else 0.0
    fit = np.isfinite(ref_k)
    print("%s: elpd_loo error / bound %.3g, khat error / bound %.3g, lppd error / bound %.3g; %d fitted (khat up to %.3g), %d unfitted, %d NaN"
          % (label, re, rk, rl, fit.sum(), ref_k[fit].max() if fit.any() else float("nan"), np.isinf(ref_k).sum(), (~ok).sum()))
    worst["elpd"], worst["khat"], worst["lppd"] = max(worst["elpd"], re), max(worst["khat"], rk), max(worst["lppd"], rl)
    worst["seen"] += 1
    assert re <= 1.0 and rk <= 1.0 and rl <= 1.0, (label, re, rk, rl)
    return ref_e, ref_k


def held(draws, specs, **kw):
    """the device's answer for draws [rows][PR][C] over the datasets `specs`, compared with the reference: tails as bytes, triples within the bounds, totals as bytes"""
    D = len(specs)
    S = draws.shape[0] * draws.shape[2] // D
    M = lr.tail_len(S)
    device_terms = S <= 65535      # (the test library's view of the terms is a grid row per draw; beyond that the host twins', which test_gpu_waic.py pins as the same bytes)
    terms = amwg_ctypes.waic_check(draws, specs, pointwise=True, loglik=device_terms)
    got = amwg_ctypes.loo_check(draws, specs, pointwise=True, tails=True, **kw)
    assert got["tails"].shape == (D, max(q["n_obs"] for q in specs), M + 1)
    for d, spec in enumerate(specs):
        n = spec["n_obs"]
        ll = terms["loglik"][d][:, :n] if device_terms else wr.loglik_of(spec, wr.draws_of_dataset(draws, D, d))
        finite = np.isfinite(ll).all(axis=0)
        tl = got["tails"][d]
        assert tl[:n][finite].tobytes() == lr.tails(ll[:, finite]).tobytes() if finite.any() else True, (spec["model"], d, draws.shape)
        assert np.isnan(tl[:n][~finite]).all() and np.isnan(tl[n:]).all()
        pw = got["pointwise"][d]
        compare("%s rows %d C %d dataset %d n %d" % (spec["model"], draws.shape[0], draws.shape[2], d, n), pw[:n], ll, S)
        assert same_values(pw[:n, 1], terms["pointwise"][d][:n, 0])      # lppd_i is WAIC's
        assert np.isnan(pw[n:]).all()
        summary, high = amwg_ctypes.loo_totals(pw, n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d], (summary, got["summary"][d], high, got["high"][d])
    return got


# ---- (1) the kernels on synthetic draws and data

@pytest.mark.parametrize("k", range(len(lr.SHAPES)))
def test_shapes_normal_ragged(k):
    held(*lr.shape_case(k))


@pytest.mark.parametrize("model", ["beta_bern", "pois_glm", "hier_normal"])
@pytest.mark.parametrize("rows,cpd", lr.FAMILY_SHAPES)
def test_shapes_of_the_other_families(model, rows, cpd):
    got = held(*lr.family_case(model, rows, cpd))
    if model == "beta_bern":      # the invalid observation: NaN for its triple and its dataset's totals only
        assert np.isnan(got["pointwise"][0][0]).all() and np.isnan(got["summary"][0]).all() and not np.isnan(got["summary"][1:]).any()


@pytest.mark.parametrize("name", lr.PATTERNS)
def test_draw_patterns(name):
    draws, specs = lr.pattern_case(name)
    got = held(draws, specs)
    pw = got["pointwise"][0]
    n = specs[0]["n_obs"]
    if name == "identical":      # no excess is positive: no fit, and elpd_loo_i is the term itself
        ll = wr.loglik_normal(specs[0]["data"]["x"], [0.3], [1.7])[0]
        assert (pw[:, 2] == np.inf).all() and pw[:, 0].tobytes() == ll.tobytes() and got["high"][0] == n
    if name == "a_tie_wider_than_the_tail":      # both routes occur: the tie holds the cutoff for most observations (no fit), not for all
        assert np.isinf(pw[:, 2]).sum() > 30 and np.isfinite(pw[:, 2]).sum() > 0
    if name in ("one_far_draw", "tiny_sigma") or name.startswith("dominating"):
        assert (pw[:, 2] == np.inf).any()
    if name == "outlier":
        assert pw[7, 2] > 0.7 and got["high"][0] >= 1 and got["high"][0] == int((pw[:, 2] > 0.7).sum())
        print("the planted outlier: khat %.3f, elpd_loo_i %.3f beside lppd_i %.3f; %d of 65 observations above 0.7" % (pw[7, 2], pw[7, 0], pw[7, 1], got["high"][0]))
    if name == "a_tail_beyond_64_KB":
        assert got["tails"].shape[2] == 4106 and np.isfinite(pw[:, 2]).all()
    if name == "both_signs":
        tl = got["tails"][0]
        assert (tl[:, 0] < 0).any() and (tl > 0).any()


def iso_case(model, rng):
    sizes = [65, 130, 20]
    specs = [lr.spec_of(model, n, rng) for n in sizes]
    return lr.draws_for(model, 6, 3 * 40, rng, n_obs=130), specs      # S = 240: M = 47, a tail of 64 slots


@pytest.mark.parametrize("model", ["normal", "beta_bern", "pois_glm"])
@pytest.mark.parametrize("fill", [np.nan, 1e300])
def test_neighbours_do_not_reach_a_dataset(model, fill):
    rng = np.random.default_rng(SEED + 30)
    draws, specs = iso_case(model, rng)
    base = amwg_ctypes.loo_check(draws, specs)
    other = draws.copy()
    other[:, :, :40] = fill
    other[:, :, 80:] = fill
    others = [dict(s, data={k: (np.full_like(v, fill) if v.dtype == np.float64 else v) for k, v in s["data"].items()}) for s in specs]
    others[1] = specs[1]
    got = amwg_ctypes.loo_check(other, others)
    assert got["pointwise"][1].tobytes() == base["pointwise"][1].tobytes() and got["summary"][1].tobytes() == base["summary"][1].tobytes() and got["high"][1] == base["high"][1]
    assert not np.isnan(base["summary"]).any()
    # ... nor does the number of datasets beside it: dataset 1 alone, at the same (rows, C / D)
    alone = amwg_ctypes.loo_check(np.ascontiguousarray(draws[:, :, 40:80]), [specs[1]])
    assert alone["pointwise"][0][:130].tobytes() == base["pointwise"][1][:130].tobytes() and alone["summary"][0].tobytes() == base["summary"][1].tobytes()


def test_one_non_finite_draw_reaches_its_own_dataset_only():
    rng = np.random.default_rng(SEED + 31)
    draws, specs = iso_case("normal", rng)
    base = amwg_ctypes.loo_check(draws, specs)
    bad = draws.copy()
    bad[3, 1, 40 + 17] = 0.0      # sigma = 0 in one draw of dataset 1
    got = held(bad, specs)
    assert np.isnan(got["pointwise"][1]).all() and np.isnan(got["summary"][1]).all()
    for d in (0, 2):
        assert got["pointwise"][d].tobytes() == base["pointwise"][d].tobytes() and got["summary"][d].tobytes() == base["summary"][d].tobytes()
    draws, specs = iso_case("beta_bern", rng)
    base = amwg_ctypes.loo_check(draws, specs)
    bad = draws.copy()
    bad[2, 0, 40 + 5] = 0.0       # theta = 0: log(theta) = -inf for the observations with x_i = 1
    got = held(bad, specs)
    ones = specs[1]["data"]["x"] == 1
    assert ones.any() and not ones.all()
    assert np.isnan(got["pointwise"][1][:130][ones]).all() and not np.isnan(got["pointwise"][1][:130][~ones]).any()
    assert np.isnan(got["summary"][1]).all()
    for d in (0, 2):
        assert got["pointwise"][d].tobytes() == base["pointwise"][d].tobytes() and got["summary"][d].tobytes() == base["summary"][d].tobytes()


def test_two_calls_and_any_scratch_budget_return_the_same_bytes():
    rng = np.random.default_rng(SEED + 32)
    sizes = (257, 65, 1025, 2)      # (the third alone needs more scratch than the first two together)
    specs = [lr.spec_of("normal", n, rng) for n in sizes]
    draws = lr.draws_for("normal", 17, 4 * 65, rng)      # S = 1105: four runs of draws per dataset; M = 100, a tail of 128 slots
    base = held(draws, specs)
    again = amwg_ctypes.loo_check(draws, specs, tails=True)
    per = [n * (128 * 8 + 512 + 48) + 4 * n * 8 for n in sizes]      # csrc/amwg_loo.h: the tail, the counters, the state and a double per run of draws
    assert per[2] > per[0] + per[1] and per[3] < per[0] + per[1]
    for budget in (1, per[0] + per[1], per[0] + per[1] + per[2] - 1, sum(per)):      # every dataset alone; (0, 1) (2) (3); (0, 1) (2, 3); all four at once
        got = amwg_ctypes.loo_check(draws, specs, tails=True, scratch_bytes=budget)
        for k in ("pointwise", "summary", "high", "tails"):
            assert got[k].tobytes() == base[k].tobytes() == again[k].tobytes(), (budget, k)
    passes, ms = amwg_ctypes.loo_stats()
    assert 1 <= passes <= 10 and ms is None
    print("S = 1105, M = 100: the select took %d passes over the terms" % passes)


def test_refused_before_a_device_call():
    x = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}
    for draws, specs, words in ((np.zeros((1, 2, 1)), [x], "fewer than 2 draws"), (np.zeros((2, 1, 2)), [x], "reads 2 components"), (np.zeros((2, 2, 3)), [x, x], "bad shape"),
                                (np.zeros((2, 2, 2)), [x, dict(x, model="beta_bern")], "is of model")):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            amwg_ctypes.loo_check(draws, specs, device=99)      # (no such device: the refusal comes first)
        assert "amwg_loo_check" in str(ei.value) and words in str(ei.value), str(ei.value)


# ---- (2) samplers

def family_spec(model, n_obs, seed, G=8):
    data = model_spec.make_data(model, n_obs, seed, G=G)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype != np.int32 else v) for k, v in data.items()}
    return model_spec.build_spec(model, data, G=G if model == "hier_normal" else None)


BURN = 200


def against_reference(s, specs, draws, got):
    D = len(specs)
    S = draws.shape[0] * draws.shape[2] // D
    waic = s.dataset_waic(pointwise=True)
    assert got["summary"].shape == (D, 4) and got["pointwise"].shape == (D, max(q["n_obs"] for q in specs), 3)
    for d, spec in enumerate(specs):
        n = spec["n_obs"]
        ll = wr.loglik_of(spec, wr.draws_of_dataset(draws, D, d))
        compare("%s sampler, dataset %d (n = %d)" % (spec["model"], d, n), got["pointwise"][d][:n], ll, S)
        assert same_values(got["pointwise"][d][:n, 1], waic["pointwise"][d][:n, 0])
        summary, high = amwg_ctypes.loo_totals(got["pointwise"][d], n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d]
        assert np.isnan(got["pointwise"][d][n:]).all()
        print("    elpd_loo %.4f se %.4f p_loo %.4f beside elpd_waic %.4f p_waic %.4f; khat > 0.7 at %d observations"
              % (got["summary"][d][0], got["summary"][d][1], got["summary"][d][2], waic["summary"][d][0], waic["summary"][d][2], got["high"][d]))


def test_a_normal_sampler():
    spec = family_spec("normal", 50, 500)
    s = amwg_ctypes.Sampler(spec, chains=128, seed=SEED)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_loo()
    assert "amwg_last_sample_dataset_loo" in str(ei.value) and "no sample() call yet" in str(ei.value)
    s.burn(BURN)
    draws = s.sample(40)
    got = s.dataset_loo(pointwise=True)
    against_reference(s, [spec], draws, got)
    one, plain, waic = s.loo(pointwise=True), s.dataset_loo(), s.waic()
    assert [one["elpd_loo"], one["se"], one["p_loo"], one["lppd"]] == got["summary"][0].tolist() and one["high"] == got["high"][0]
    assert one["pointwise"].tobytes() == got["pointwise"][0].tobytes() and plain["summary"].tobytes() == got["summary"].tobytes() and "pointwise" not in plain
    print("Normal model, n = 50, 128 chains x 40 draws: elpd_waic = %.4f, elpd_loo = %.4f; p_waic = %.4f, p_loo = %.4f (two parameters)"
          % (waic["elpd_waic"], one["elpd_loo"], waic["p_waic"], one["p_loo"]))
    assert abs(waic["elpd_waic"] - one["elpd_loo"]) < 0.5 and one["lppd"] == waic["lppd"]
    s.summarize(40, 1, 0)
    for call in (s.dataset_loo, s.loo):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_last_sample_dataset_loo" in str(ei.value) and "amwg_sample_summarize" in str(ei.value), str(ei.value)
    s.close()


def test_a_ragged_normal_dataset_sampler():
    specs = [family_spec("normal", n, 500 + 7 * d) for d, n in enumerate((20, 50, 35, 64))]
    a = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True)
    a.burn(BURN)
    draws = a.sample(40)
    against_reference(a, specs, draws, a.dataset_loo(pointwise=True))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        a.loo()
    assert "pooled summaries are refused" in str(ei.value) and "amwg_last_sample_dataset_loo" in str(ei.value) and "dataset_loo" in str(ei.value)
    a.close()


@pytest.mark.parametrize("model,n_obs", [("pois_glm", 40), ("beta_bern", 70)])
def test_a_dataset_sampler_of(model, n_obs):
    specs = [family_spec(model, n_obs, 600 + 11 * d) for d in range(2)]
    a = amwg_ctypes.Sampler(specs, chains=2 * 32, seed=SEED)
    a.burn(BURN)
    draws = a.sample(30)
    against_reference(a, specs, draws, a.dataset_loo(pointwise=True))
    a.close()


def test_the_hierarchical_family():
    spec = family_spec("hier_normal", 96, 700, G=8)
    s = amwg_ctypes.Sampler(spec, chains=64, seed=SEED)
    s.burn(BURN)
    draws = s.sample(30)
    against_reference(s, [spec], draws, s.dataset_loo(pointwise=True))
    s.close()


def test_a_group_local_sampler_and_a_single_draw_are_refused():
    spec = family_spec("hier_normal", 96, 700, G=8)
    s = amwg_ctypes.Sampler(spec, chains=3, seed=SEED, group_local=1)
    s.burn(20)
    s.sample(5)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_loo()
    s.close()
    assert "amwg_last_sample_dataset_loo" in str(ei.value) and "group_local" in str(ei.value) and "index order" in str(ei.value), str(ei.value)
    s = amwg_ctypes.Sampler(family_spec("normal", 20, 500), chains=1, seed=SEED)
    s.burn(20)
    s.sample(1)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_loo()
    assert "amwg_last_sample_dataset_loo" in str(ei.value) and "fewer than 2 draws per dataset" in str(ei.value), str(ei.value)
    s.sample(2)
    assert np.isfinite(s.dataset_loo()["summary"]).all()
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
        a.dataset_loo()
    a.close()
    assert "amwg_last_sample_dataset_loo" in str(ei.value) and "the pointwise terms of a closure are not known to the library; built-in families only" in str(ei.value)


def test_the_largest_ratios_seen():
    """(runs last among the comparisons of this file: what tests/README.loo.md quotes; run alone, it makes one comparison of its own)"""
    if not worst["seen"]:
        held(*lr.shape_case(3))
    assert worst["seen"] > 0
    print("largest error / bound over this run: elpd_loo %.3g, khat %.3g, lppd %.3g" % (worst["elpd"], worst["khat"], worst["lppd"]))
    assert worst["elpd"] <= 1.0 and worst["khat"] <= 1.0 and worst["lppd"] <= 1.0


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_loo_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_loo.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu loo ok" in p.stdout, p.stdout + "\n" + p.stderr
