"""WAIC without stored draws (amwg_set_waic; csrc/amwg_waic_fold.hip, waic_fold_body), on the GPU.  tests/README.waic_fold.md says what each test pins.

(1) the fold through the test library (amwg_waic_fold_check: the launcher of the summarising call over an array cut into windows): lppd_i and p_i within the bounds
    of include/amwg.h against extended precision (waic_reference), S the whole array's draws; totals AS BYTES; NaN beyond n_d; the bytes of the records as the split
    rule predicts; the other families; draw patterns that break a careless carry across windows; determinism and isolation.
(2) samplers: an armed summarize() against the same seeded sampler's stored draws; a closure against its family; the refusals.   (3) tests/js/test_gpu_waic_fold.js.
Every comparison prints its largest error / bound ratio before it asserts."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes as A
import waic_reference as wr
from test_gpu_waic import BURN, SEED, draws_for, family_spec, normal_case, same_values, spec_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OBS = [1, 2, 63, 64, 65, 257]
CASES = [(rows, cpd, w) for rows in (1, 2, 17) for cpd in (1, 3, 65) for w in sorted({1, 2, 5, rows, rows + 3}) if rows * cpd >= 2]
CASES.append((769, 1, 768))      # three splits, and a last window of one draw: two of its runs are empty
worst = {"lppd": 0.0, "p": 0.0}


def fold_splits(Sw, n):
    """the split rule of csrc/amwg_pointwise.h restated"""
    tiles = (n + 63) // 64
    return min(max(1, max(128, Sw // 128) // tiles), max(1, Sw // 256), 65535)


def held(draws, specs, window_rows):
    """the fold's answer for draws [rows][PR][C] in windows of window_rows rows, against the reference over ALL the draws: pairs within the bounds, totals as bytes"""
    D = len(specs)
    got = A.waic_fold_check(draws, specs, window_rows)
    cpd = draws.shape[2] // D
    n_eff = [2 if s["model"] == "beta_bern" else s["n_obs"] for s in specs]
    assert got["state_bytes"] == 32 * sum(fold_splits(window_rows * cpd, n) * n for n in n_eff)
    for d, spec in enumerate(specs):
        n = spec["n_obs"]
        pw = got["pointwise"][d]
        rl, rp = wr.worst_ratio(pw[:n], wr.loglik_of(spec, wr.draws_of_dataset(draws, D, d)))
        print("%s rows %d cpd %d window %d dataset %d n %d: lppd error / bound %.3g, p error / bound %.3g" % (spec["model"], draws.shape[0], cpd, window_rows, d, n, rl, rp))
        worst["lppd"], worst["p"] = max(worst["lppd"], rl), max(worst["p"], rp)
        assert rl <= 1.0 and rp <= 1.0, (spec["model"], d, draws.shape, window_rows, rl, rp)
        assert np.isnan(pw[n:]).all()
        summary, high = A.waic_totals(pw, n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d]
    return got


# ---- (1) the fold through the test library

@pytest.mark.parametrize("k,case", list(enumerate(CASES)))
def test_shapes_normal_ragged(k, case):
    rows, cpd, window_rows = case
    rng = np.random.default_rng(SEED + k)
    specs = [spec_of("normal", N_OBS[(k + j) % 6], rng) for j in (0, 2, 4)]
    held(draws_for("normal", rows, 3 * cpd, rng), specs, window_rows)


@pytest.mark.parametrize("model", ["beta_bern", "pois_glm", "hier_normal"])
@pytest.mark.parametrize("nan_draw", [False, True])
def test_the_other_families_over_four_windows(model, nan_draw):
    rng = np.random.default_rng(SEED + 100)
    D = 1 if model == "hier_normal" else 3
    sizes = [63, 2, 130][:D]
    specs = [spec_of(model, n, rng) for n in sizes]
    if model == "beta_bern":
        specs[0]["data"]["x"][0] = 0.5      # an invalid observation: NaN for its pair and its dataset's totals
    draws = draws_for(model, 17, D * 65, rng, n_obs=max(sizes))
    base = held(draws, specs, 5)
    if model == "beta_bern":
        assert np.isnan(base["pointwise"][0][0]).all() and np.isnan(base["summary"][0]).all() and not np.isnan(base["summary"][1:]).any()
    if nan_draw:      # a NaN in the second window reaches its own (dataset, observation) only: the reference's NaN pattern, every other pair as before
        bad = draws.copy()
        bad[7, 0, 5] = np.nan      # theta of dataset 0 | beta[0] of dataset 0 | the mean of group 0
        got = held(bad, specs, 5)
        hit = np.isnan(got["pointwise"]) & ~np.isnan(base["pointwise"])
        assert hit.any() and not hit[1:].any() and same_values(got["pointwise"][~hit], base["pointwise"][~hit])
        if model == "hier_normal":
            assert (hit[0, :, 0] == (specs[0]["data"]["g"] == 0)).all() and not hit[0, :, 0].all()


@pytest.mark.parametrize("at", [0, 600, 1104])
def test_one_dominating_draw_in_the_first_a_middle_and_the_last_window(at):
    rng = np.random.default_rng(SEED + 21)
    S = 17 * 65
    mu = np.full(S, 1e3) + rng.normal(size=S)
    mu[at] = 0.0
    draws, specs = normal_case(rng.normal(size=64), mu, np.ones(S), 17)
    got = held(draws, specs, 5)
    assert (got["pointwise"][0][:, 0] < -np.log(S)).all() and (got["pointwise"][0][:, 0] > -np.log(S) - 20).all()      # lppd_i = l_(at, i) - log S: the rest underflow


@pytest.mark.parametrize("window_rows", [1, 5, 17])
def test_identical_draws_and_a_large_mean_with_a_tiny_spread(window_rows):
    rng = np.random.default_rng(SEED + 23)
    S = 17 * 65
    draws, specs = normal_case(rng.normal(size=65), np.full(S, 0.3), np.full(S, 1.7), 17)
    assert (held(draws, specs, window_rows)["pointwise"][0][:, 1] == 0.0).all()
    x = 1000.0 + rng.normal(size=65)
    draws, specs = normal_case(x, 1e-3 * rng.normal(size=S), np.full(S, 10.0), 17)
    lppd, p, mean, maxabs = wr.pointwise(wr.loglik_normal(x, draws[:, 0].ravel(), draws[:, 1].ravel()))
    assert (mean * mean / p >= 1e8).all()      # cancellation in a carried (mean, M2) would show
    held(draws, specs, window_rows)


def test_two_calls_agree_and_neighbours_do_not_reach_a_dataset():
    rng = np.random.default_rng(SEED + 30)
    specs = [spec_of("normal", n, rng) for n in (65, 130, 20)]
    draws = draws_for("normal", 17, 3 * 65, rng)
    a, b = A.waic_fold_check(draws, specs, 5), A.waic_fold_check(draws, specs, 5)
    for k in ("pointwise", "summary", "high"):
        assert a[k].tobytes() == b[k].tobytes(), k
    alone = A.waic_fold_check(np.ascontiguousarray(draws[:, :, 65:130]), [specs[1]], 5)
    assert alone["pointwise"][0].tobytes() == a["pointwise"][1].tobytes() and alone["summary"][0].tobytes() == a["summary"][1].tobytes()
    other = A.waic_fold_check(draws, specs, 4)      # (another window: other runs of draws; within the bounds, not the same bytes by promise)
    assert np.abs(other["pointwise"] - a["pointwise"])[~np.isnan(a["pointwise"])].max() < 1e-9


# ---- (2) samplers

def test_an_armed_summarize_against_the_stored_draws_of_the_same_seed():
    specs = [family_spec("normal", n, 500 + 7 * d) for d, n in enumerate((20, 50, 35, 64))]
    stored, folded = (A.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True) for _ in range(2))
    stored.burn(BURN), folded.burn(BURN)
    draws = stored.sample(40)
    assert folded.waic_info() == {"armed": False, "bytes": 0}
    folded.summarize(40, 1, 13)
    with pytest.raises(A.AmwgError) as ei:
        folded.dataset_waic()
    assert "amwg_last_sample_dataset_waic" in str(ei.value) and "amwg_sample_summarize" in str(ei.value) and "amwg_set_waic" in str(ei.value)
    folded.close()
    folded = A.Sampler(specs, chains=4 * 32, seed=SEED, ragged=True)
    folded.burn(BURN)
    folded.set_waic()
    folded.summarize(40, 1, 13)
    assert folded.summary_info()["windows"] == 4 and folded.waic_info() == {"armed": True, "bytes": 32 * (20 + 50 + 35 + 64)}      # 13 x 32 draws a window: one split
    got = folded.dataset_waic(pointwise=True)
    for d, spec in enumerate(specs):
        n = spec["n_obs"]
        rl, rp = wr.worst_ratio(got["pointwise"][d][:n], wr.loglik_of(spec, wr.draws_of_dataset(draws, 4, d)))
        print("ragged Normal sampler, dataset %d (n = %d): lppd error / bound %.3g, p error / bound %.3g" % (d, n, rl, rp))
        assert rl <= 1.0 and rp <= 1.0 and np.isnan(got["pointwise"][d][n:]).all()
        summary, high = A.waic_totals(got["pointwise"][d], n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d]
    assert folded.dataset_waic(pointwise=True)["pointwise"].tobytes() == got["pointwise"].tobytes()
    with pytest.raises(A.AmwgError, match="amwg_sample_summarize"):
        folded.dataset_loo()
    folded.set_waic(False)
    with pytest.raises(A.AmwgError, match="amwg_set_waic"):
        folded.dataset_waic()
    stored.close(), folded.close()
    one = A.Sampler(specs[0], chains=1, seed=SEED, lanes_per_chain=1)
    one.set_waic()
    with pytest.raises(A.AmwgError) as ei:
        one.summarize(1)
    assert "amwg_sample_summarize" in str(ei.value) and "fewer than 2 draws" in str(ei.value)
    one.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_a_closure_folds_the_bytes_of_its_family():
    from test_gpu_pointwise import normal_pair
    m, fam, clo = normal_pair()
    f, c = A.Sampler(fam, chains=64, seed=SEED, lanes_per_chain=1), A.Sampler(clo, chains=64, seed=SEED, lanes_per_chain=1)
    for s in (f, c):
        s.burn(100)
        s.set_waic()
        s.summarize(20, 1, 7)
    fw, cw = f.waic(pointwise=True), c.waic(pointwise=True)
    assert fw["pointwise"].tobytes() == cw["pointwise"].tobytes() and not np.isnan(fw["pointwise"]).any()
    for k in ("elpd_waic", "se", "p_waic", "lppd", "high"):
        assert fw[k] == cw[k], k
    assert f.waic_info() == c.waic_info() == {"armed": True, "bytes": 32 * 50}
    f.close(), c.close()
    m, fam, clo = normal_pair(with_text=False)
    c = A.Sampler(clo, chains=64, seed=SEED, lanes_per_chain=1)
    with pytest.raises(A.AmwgError) as ei:
        c.set_waic()
    assert "amwg_set_waic" in str(ei.value) and "pointwise terms of a closure" in str(ei.value)
    c.close()


def test_the_largest_ratios_seen():
    """(runs after the cases above: what tests/README.waic_fold.md quotes)"""
    print("largest error / bound of the fold over this run: lppd %.3g, p %.3g" % (worst["lppd"], worst["p"]))
    assert worst["lppd"] <= 1.0 and worst["p"] <= 1.0


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_waic_fold_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_waic_fold.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu waic fold ok" in p.stdout, p.stdout + "\n" + p.stderr
