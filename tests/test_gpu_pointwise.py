"""options.pointwise -- WAIC and PSIS-LOO for translated closures -- on the GPU.  tests/README.pointwise.md says what each test pins.

(1) the check library on synthetic draws (amwg_user_waic_check, amwg_user_loo_check): the loglik matrix AS BYTES against Node's term(state, data, i) for every
    accepted fixture of tests/js/pointwise_models.js; lppd_i, p_i, elpd_loo_i and khat_i within the header's bounds against extended precision (waic_reference,
    loo_reference); the totals AS BYTES against waic_totals / loo_totals of the returned pointwise bytes.
(2) twins: the Normal and Poisson-GLM closures give the built-in families' pointwise BYTES on the same draws and data (the same kernel text, splits and staged run);
    the hierarchical twin too while its Draw keeps the staged run at 256; the Bernoulli twin within the bounds (the family computes two observations: other splits).
(3) samplers: a closure sampler and the built-in Normal sampler under one seed; D = 3 datasets against lone samplers and under a small scratch budget; the -Infinity
    observation; repeat calls.
(4) the refusals by their messages.   (5) tests/js/test_gpu_pointwise.js.
Every comparison prints its largest error / bound ratio before it asserts."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes as A
import loo_reference as lr
import model_spec
import pointwise_lib as pl
import waic_reference as wr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021
N_OBS = [1, 2, 63, 64, 65, 257]
SHAPES = [(1, 2), (2, 3), (5, 64), (17, 65)]      # (rows, chains per dataset): a lone pair of draws; below, at and beyond one staged run
STATES = 17 * 65      # a state of its own for every draw of the largest shape: repeated draws make ties, and a tail of two distinct values has no Pareto fit to speak of


def same_values(a, b):
    """the same NaN pattern, and the same bytes wherever there is a number"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


def node_loglik(m, rows, chains):
    """[S][n]: Node's terms of the draws pl.draws_of lays out, in draw order s = row * chains + chain"""
    return np.stack([m["terms"][s % len(m["states"])] for s in range(rows * chains)])


def held(m, rows, cpd, D=1, **kw):
    """the device's answer for the fixture's synthetic draws (D copies of the dataset side by side), against Node's terms and the references"""
    n = m["n_obs"]
    draws = pl.draws_of(m, rows, D * cpd)
    users = [pl.user_spec(m)] * D
    got = A.user_waic_check(draws, users, m["terms_source"], m["P"], n, pointwise=True, loglik=True, **kw)
    loo = A.user_loo_check(draws, users, m["terms_source"], m["P"], n, pointwise=True, tails=True, **kw)
    S = rows * cpd
    for d in range(D):
        ll = np.stack([m["terms"][((s // cpd) * D * cpd + d * cpd + s % cpd) % len(m["states"])] for s in range(S)])
        assert got["loglik"][d].tobytes() == ll.tobytes(), (m["name"], d, rows, cpd, np.argwhere(got["loglik"][d].view(np.uint64) != ll.view(np.uint64))[:5])
        rl, rp = wr.worst_ratio(got["pointwise"][d], ll)
        ref_e, ref_k = lr.pointwise(ll)
        re, rk = lr.ratios(loo["pointwise"][d][:, 0], loo["pointwise"][d][:, 2], ref_e, ref_k, S)
        print("%s n %d rows %d cpd %d dataset %d: lppd error / bound %.3g, p %.3g, elpd_loo %.3g, khat %.3g" % (m["name"], n, rows, cpd, d, rl, rp, re, rk))
        assert rl <= 1.0 and rp <= 1.0 and re <= 1.0 and rk <= 1.0, (m["name"], rows, cpd, rl, rp, re, rk)
        assert same_values(loo["pointwise"][d][:, 1], got["pointwise"][d][:, 0])      # lppd_i is WAIC's
        finite = np.isfinite(ll).all(axis=0)
        if finite.any():
            assert loo["tails"][d][finite].tobytes() == lr.tails(ll[:, finite]).tobytes()
        summary, high = A.waic_totals(got["pointwise"][d], n)
        assert same_values(summary, got["summary"][d]) and high == got["high"][d]
        summary, high = A.loo_totals(loo["pointwise"][d], n)
        assert same_values(summary, loo["summary"][d]) and high == loo["high"][d]
    return got, loo


def fixture(name, n, states=STATES):
    m = dict(pl.fixtures(n, states, (name,))["models"][name])
    m["name"] = name
    return m


# ---- (1) the check library on synthetic draws

@pytest.mark.parametrize("name", pl.NAMES)
def test_every_fixture_in_every_shape(name):
    m = fixture(name, 65)
    for rows, cpd in SHAPES:
        got, loo = held(m, rows, cpd)
        if m["bad_obs"] is not None:      # the -Infinity observation: NaN for itself and its dataset's totals only
            i = m["bad_obs"]
            assert np.isnan(got["pointwise"][0][i]).all() and np.isnan(loo["pointwise"][0][i]).all() and np.isnan(got["summary"][0]).all() and np.isnan(loo["summary"][0]).all()
            assert not np.isnan(np.delete(got["pointwise"][0], i, axis=0)).any() and not np.isnan(np.delete(loo["pointwise"][0], i, axis=0)).any()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 257])
@pytest.mark.parametrize("name", ["normal", "logistic", "wide_state"])
def test_observation_counts_around_the_tile(name, n):
    m = fixture(name, n)
    for rows, cpd in SHAPES:
        held(m, rows, cpd)


def test_datasets_side_by_side_and_a_small_scratch_budget():
    m = fixture("locals", 65)
    a, la = held(m, 5, 64, D=3)
    b, lb = held(m, 5, 64, D=3, scratch_bytes=4096)      # (every dataset then runs in a batch of its own)
    assert a["pointwise"].tobytes() == b["pointwise"].tobytes() and same_values(la["pointwise"], lb["pointwise"])
    assert a["summary"].tobytes() == b["summary"].tobytes() and same_values(la["summary"], lb["summary"])


# ---- (2) twins

def family_specs(m):
    n, d = m["n_obs"], m["data"]
    if m["twin"] == "normal":
        return {"model": "normal", "n_obs": n, "data": {"x": np.array(d, dtype=np.float64)}}
    if m["twin"] == "beta_bern":
        return {"model": "beta_bern", "n_obs": n, "data": {"x": np.array(d, dtype=np.float64)}}
    if m["twin"] == "hier_normal":
        return {"model": "hier_normal", "n_obs": n, "G": 5, "data": {"x": np.array(d["y"], dtype=np.float64), "g": np.array(d["g"], dtype=np.int32)}}
    return {"model": "pois_glm", "n_obs": n, "K": 7, "data": {"x": np.array(d["X"], dtype=np.float64), "y": np.array(d["y"], dtype=np.float64)}}


@pytest.mark.parametrize("name", ["normal", "pois_glm", "hier", "bern"])
def test_the_twin_of_a_family(name):
    m = fixture(name, 257)
    spec = family_specs(m)
    for rows, cpd in ((2, 3), (17, 65)):
        draws = pl.draws_of(m, rows, cpd)
        user = [pl.user_spec(m)]
        cw = A.user_waic_check(draws, user, m["terms_source"], m["P"], m["n_obs"], loglik=True)
        cl = A.user_loo_check(draws, user, m["terms_source"], m["P"], m["n_obs"])
        fw = A.waic_check(draws, [spec], loglik=True)
        fl = A.loo_check(draws, [spec])
        assert cw["loglik"].tobytes() == fw["loglik"].tobytes(), name      # the same doubles
        if name in ("normal", "pois_glm") or (name == "hier" and "double st[" not in m["terms_source"]):
            assert cw["pointwise"].tobytes() == fw["pointwise"].tobytes() and same_values(cl["pointwise"], fl["pointwise"]), name
            assert cw["summary"].tobytes() == fw["summary"].tobytes() and same_values(cl["summary"], fl["summary"])
        else:      # other splits (the Bernoulli family computes two observations): within the bounds of the same terms
            ll = node_loglik(m, rows, cpd)
            for got in (cw, fw):
                rl, rp = wr.worst_ratio(got["pointwise"][0], ll)
                print("%s twin rows %d cpd %d: lppd error / bound %.3g, p %.3g" % (name, rows, cpd, rl, rp))
                assert rl <= 1.0 and rp <= 1.0
            ref_e, ref_k = lr.pointwise(ll)
            for got in (cl, fl):
                re, rk = lr.ratios(got["pointwise"][0][:, 0], got["pointwise"][0][:, 2], ref_e, ref_k, rows * cpd)
                print("%s twin rows %d cpd %d: elpd_loo error / bound %.3g, khat %.3g" % (name, rows, cpd, re, rk))
                assert re <= 1.0 and rk <= 1.0


# ---- (3) samplers

def closure_spec(m, family, with_text=True):
    """the closure as a Sampler spec, with the parameters, starting point and stepper options of its family's spec"""
    user = pl.user_spec(m)
    if with_text:
        user["pointwise"] = m["terms_source"]
    return {"user": user, "params": family["params"], "P": family["P"], "init": family["init"], "comp_opts": family["comp_opts"]}


def normal_pair(n=50, with_text=True):
    m = fixture("normal", n, 4)
    fam = model_spec.build_spec("normal", {"x": np.array(m["data"], dtype=np.float64)})
    return m, fam, closure_spec(m, fam, with_text)


def test_a_closure_sampler_and_the_normal_family_under_one_seed():
    m, fam, clo = normal_pair()
    f = A.Sampler(fam, chains=64, seed=SEED, lanes_per_chain=1)
    c = A.Sampler(clo, chains=64, seed=SEED, lanes_per_chain=1)
    assert c.pointwise_n_obs() == 50 and f.pointwise_n_obs() == 0 and c.dataset_n_obs() == [0]
    f.burn(100), c.burn(100)
    df, dc = f.sample(20), c.sample(20)
    assert df.tobytes() == dc.tobytes()      # the same chains
    fw, cw, fl, cl = f.waic(pointwise=True), c.waic(pointwise=True), f.loo(pointwise=True), c.loo(pointwise=True)
    assert fw["pointwise"].tobytes() == cw["pointwise"].tobytes() and same_values(fl["pointwise"], cl["pointwise"])
    for k in ("elpd_waic", "se", "p_waic", "lppd", "high"):
        assert fw[k] == cw[k], k
    for k in ("elpd_loo", "se", "p_loo", "lppd", "high"):
        assert fl[k] == cl[k], k
    again = c.waic(pointwise=True), c.loo(pointwise=True)      # repeat calls: the same bytes
    assert again[0]["pointwise"].tobytes() == cw["pointwise"].tobytes() and same_values(again[1]["pointwise"], cl["pointwise"])
    c.summarize(20, 1, 0)
    for call in (c.dataset_waic, c.dataset_loo):
        with pytest.raises(A.AmwgError, match="amwg_sample_summarize"):
            call()
    f.close(), c.close()


def test_three_datasets_in_one_closure_sampler():
    base = pl.fixtures(40, 4, ("head_local",))["models"]["head_local"]
    sets = []
    for d in range(3):      # the same closure and text on three datasets: the arrays differ, nothing else
        m = dict(base)
        m["arrays"] = [a + (0.25 * d if a.size == 40 else 0.0) for a in base["arrays"]]
        sets.append(m)
    fam = {"params": [{"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": -np.inf, "upper": np.inf}] * 2, "P": 2, "init": [3.0, 0.0],
           "comp_opts": [dict(model_spec.DEFAULT_OPT) for _ in range(2)]}
    a = A.Sampler([closure_spec(m, fam) for m in sets], chains=3 * 64, seed=SEED, lanes_per_chain=1)
    a.burn(60)
    a.sample(10)
    wa, la = a.dataset_waic(pointwise=True), a.dataset_loo(pointwise=True)
    assert wa["pointwise"].shape == (3, 40, 2) and la["pointwise"].shape == (3, 40, 3)
    for d, m in enumerate(sets):
        lone = A.Sampler(closure_spec(m, fam), chains=64, seed=SEED, chain_offset=64 * d, lanes_per_chain=1)
        lone.burn(60)
        lone.sample(10)
        w, l = lone.waic(pointwise=True), lone.loo(pointwise=True)
        assert w["pointwise"].tobytes() == wa["pointwise"][d].tobytes() and same_values(l["pointwise"], la["pointwise"][d]), d
        lone.close()
    with pytest.raises(A.AmwgError, match="pooled summaries are refused"):
        a.waic()
    a.close()


def test_an_infinite_observation_spoils_its_own_dataset_only():
    """three datasets in one closure sampler; the middle one holds the observation whose term is -Infinity under every draw"""
    t = pl.fixtures(40, 1, ("@inf_datasets",))["inf_datasets"]      # one source over the three datasets (translate_datasets)
    i = t["bad_obs"]
    sets = [dict(t, arrays=[pl.unhex(a) for a in row]) for row in t["arrays"]]
    fam = {"params": [{"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": -np.inf, "upper": np.inf}], "P": 1, "init": [1.0], "comp_opts": [dict(model_spec.DEFAULT_OPT)]}
    s = A.Sampler([closure_spec(m, fam) for m in sets], chains=3 * 64, seed=SEED, lanes_per_chain=1)
    s.set_state(np.full((1, 3 * 64), 1.0) + 0.01 * np.arange(3 * 64)[None, :])      # (the middle dataset's chains cannot move from a log_post of -inf: any finite state serves)
    s.sample(6)
    for got, width in ((s.dataset_waic(pointwise=True), 2), (s.dataset_loo(pointwise=True), 3)):
        pw, summary = got["pointwise"], got["summary"]
        assert pw.shape == (3, 40, width)
        assert np.isnan(pw[1][i]).all() and not np.isnan(np.delete(pw[1], i, axis=0)).any() and np.isnan(summary[1]).all()
        assert not np.isnan(pw[0]).any() and not np.isnan(pw[2]).any() and not np.isnan(summary[0]).any() and not np.isnan(summary[2]).any()
    s.close()


# ---- (4) refusals by message

def test_refusals():
    m, fam, clo = normal_pair(with_text=False)
    c = A.Sampler(clo, chains=64, seed=SEED, lanes_per_chain=1)
    c.burn(20)
    c.sample(4)
    for call, name in ((c.dataset_waic, "amwg_last_sample_dataset_waic"), (c.dataset_loo, "amwg_last_sample_dataset_loo")):
        with pytest.raises(A.AmwgError) as ei:
            call()
        assert name in str(ei.value) and "the pointwise terms of a closure are not known to the library; built-in families only" in str(ei.value)
    c.close()
    with pytest.raises(A.AmwgError, match="needs no flag"):
        A.Sampler(dict(fam, pointwise=m["terms_source"]), chains=64, seed=SEED)
    f = A.Sampler(fam, chains=64, seed=SEED)
    assert A.lib().amwg_set_pointwise(f.h, m["terms_source"].encode()) == -1 and "amwg_set_pointwise" in A.lib().amwg_last_error().decode() and "built-in family" in A.lib().amwg_last_error().decode()
    f.close()
    m, fam, clo = normal_pair()
    one = A.Sampler(clo, chains=1, seed=SEED, lanes_per_chain=1)
    one.burn(10)
    one.sample(1)
    for call in (one.dataset_waic, one.dataset_loo):
        with pytest.raises(A.AmwgError, match="fewer than 2 draws per dataset"):
            call()
    one.close()


# ---- (5) the JavaScript front end

def test_javascript_front_end():
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "test_gpu_pointwise.js")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stderr[-3000:]
