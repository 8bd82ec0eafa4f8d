"""WAIC and PSIS-LOO over groups of observations (amwg_last_sample_dataset_waic_grouped / _loo_grouped; tests/README.grouped.md says what each test pins): the joint
term to the bit, singleton groups as the ungrouped bytes, the estimates within the ungrouped tests' bounds, samplers against the test library, the refusals."""
import functools
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

pytestmark = pytest.mark.gpu
N, ROWS, CPD = 130, 17, 65      # S = 1105: four staged runs and a rest, no multiple of any block of draws
CASES = [("normal", 1), ("normal", 3), ("normal", 33), ("normal", 65), ("pois_glm", 3), ("pois_glm", 65), ("hier_normal", 0)]      # (model, G; 0: the family's own g)


def labels_for(n, G, rng):
    """unsorted, non-dense labels: one group of more than half the observations, singletons, the rest uneven"""
    if G == 1:
        return np.full(n, 7, dtype=np.int32)
    sizes = np.ones(G, dtype=int)
    sizes[0] = n // 2 + 1
    first = 1 + (G - 1) // 2      # groups 1 .. first - 1 stay singletons
    np.add.at(sizes, first + np.arange(n - sizes.sum()) % (G - first), 1)
    names = 3 * rng.choice(np.arange(-50, 1000), size=G, replace=False)
    return rng.permutation(np.repeat(names, sizes)).astype(np.int32)


def group_sum(ll, labels):
    """the rule: ll [S][n] -> [S][G], per group a left-to-right fp64 sum over its members in ascending observation index"""
    out = []
    for name in np.unique(labels):
        members = np.flatnonzero(labels == name)
        acc = ll[:, members[0]].copy()
        for i in members[1:]:
            acc = acc + ll[:, i]
        out.append(acc)
    return np.stack(out, axis=1)


@functools.lru_cache(maxsize=None)
def case(model, G):
    rng = np.random.default_rng([lr.SEED, len(model), G])
    spec = lr.spec_of(model, N, rng)
    labels = spec["data"]["g"].copy() if model == "hier_normal" else labels_for(N, G, rng)
    draws = lr.draws_for(model, ROWS, CPD, rng, n_obs=N)
    ll = A.waic_check(draws, [spec], loglik=True)["loglik"][0]
    return draws, spec, labels, group_sum(ll, labels)


@pytest.mark.parametrize("model,G", CASES)
def test_the_group_sum_to_the_bit_and_the_estimates(model, G):
    draws, spec, labels, LL = case(model, G)
    S, Gd = LL.shape
    w = A.waic_check(draws, [spec], loglik=True, groups=[labels])
    assert w["n_groups"][0] == Gd == (G or 5) and w["loglik"].shape == (1, S, Gd)
    assert w["loglik"][0].tobytes() == LL.tobytes()
    rl, rp = wr.worst_ratio(w["pointwise"][0], LL)
    l = A.loo_check(draws, [spec], groups=[labels])
    re, rk = lr.ratios(l["pointwise"][0][:, 0], l["pointwise"][0][:, 2], *lr.pointwise(LL), S)
    print("%s G %d: error / bound lppd %.3g p %.3g elpd_loo %.3g khat %.3g" % (model, Gd, rl, rp, re, rk))
    assert max(rl, rp, re, rk) <= 1.0
    assert l["pointwise"][0][:, 1].tobytes() == w["pointwise"][0][:, 0].tobytes()      # lppd_g is WAIC's
    for got, totals in ((w, A.waic_totals), (l, A.loo_totals)):
        summary, high = totals(got["pointwise"][0], Gd)
        assert summary.tobytes() == got["summary"][0].tobytes() and high == got["high"][0]


@pytest.mark.parametrize("model", ["normal", "pois_glm"])
def test_singleton_groups_are_the_ungrouped_bytes(model):
    draws, spec, _, _ = case(model, 65)
    for check in (A.waic_check, A.loo_check):
        plain = check(draws, [spec])
        up, down = check(draws, [spec], groups=[np.arange(N)]), check(draws, [spec], groups=[np.arange(N)[::-1]])
        assert up["pointwise"].tobytes() == plain["pointwise"].tobytes() and up["summary"].tobytes() == plain["summary"].tobytes()
        assert down["pointwise"][0][::-1].tobytes() == plain["pointwise"][0].tobytes()


def test_a_tie_wider_than_the_tail_in_two_groups_and_a_group_with_a_non_finite_term():
    draws, specs = lr.pattern_case("a_tie_wider_than_the_tail")
    labels = (np.arange(65) % 5 == 0).astype(np.int32)
    LL = group_sum(A.waic_check(draws, specs, loglik=True)["loglik"][0], labels)
    pw = A.loo_check(draws, specs, groups=[labels])["pointwise"][0]
    re, rk = lr.ratios(pw[:, 0], pw[:, 2], *lr.pointwise(LL), LL.shape[0])
    assert pw.shape == (2, 3) and re <= 1.0 and rk <= 1.0, (re, rk)
    draws, spec, labels, _ = case("normal", 33)
    bad = {"model": "normal", "n_obs": N, "data": {"x": spec["data"]["x"].copy()}}
    bad["data"]["x"][11] = np.inf
    hit = int(np.searchsorted(np.unique(labels), labels[11]))
    for check in (A.waic_check, A.loo_check):
        got, clean = check(draws, [bad], groups=[labels]), check(draws, [spec], groups=[labels])
        nan = np.isnan(got["pointwise"][0]).all(axis=1)
        assert nan[hit] and nan.sum() == 1 and np.isnan(got["summary"][0]).all()
        assert np.delete(got["pointwise"][0], hit, axis=0).tobytes() == np.delete(clean["pointwise"][0], hit, axis=0).tobytes()


def same_as_the_test_library(s, draws, lib_waic, lib_loo, groups):
    for _ in range(2):      # a second identical call: identical bytes
        w, l = s.dataset_waic(pointwise=True, groups=groups), s.dataset_loo(pointwise=True, groups=groups)
        for got, want in ((w, lib_waic), (l, lib_loo)):
            for k in ("summary", "high", "pointwise", "n_groups"):
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


def family_spec(model, n_obs, seed):
    data = model_spec.make_data(model, n_obs, seed)
    return model_spec.build_spec(model, {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype != np.int32 else v) for k, v in data.items()})


def test_a_ragged_normal_dataset_sampler():
    sizes, rng = (20, 50, 35), np.random.default_rng(lr.SEED)
    specs = [family_spec("normal", n, 500 + d) for d, n in enumerate(sizes)]
    groups = [rng.integers(0, 4 + 3 * d, size=n).astype(np.int32) for d, n in enumerate(sizes)]
    s = A.Sampler(specs, chains=3 * 32, seed=lr.SEED, ragged=True)
    s.burn(100)
    draws = s.sample(20)
    same_as_the_test_library(s, draws, A.waic_check(draws, specs, groups=groups), A.loo_check(draws, specs, groups=groups), groups)
    with pytest.raises(A.AmwgError, match="amwg_last_sample_dataset_waic_grouped: NULL labels"):
        A._check(A.lib().amwg_last_sample_dataset_waic_grouped(s.h, None, A._dp(np.empty((3, 4))), None, None, None))
    s.summarize(20, 1, 0)
    with pytest.raises(A.AmwgError, match="amwg_last_sample_dataset_loo_grouped.*amwg_sample_summarize"):
        s.dataset_loo(groups=groups)
    s.close()
    b = A.Sampler(family_spec("beta_bern", 30, 5), chains=32, seed=1)
    b.sample(4)
    with pytest.raises(A.AmwgError, match="amwg_last_sample_dataset_waic_grouped: the Bernoulli family"):
        b.dataset_waic(groups=[np.arange(30) % 3])
    b.close()


def test_a_translated_poisson_regression():
    m = dict(pl.fixtures(40, 4, ("pois_glm",))["models"]["pois_glm"])
    fam = model_spec.build_spec("pois_glm", {"x": np.array(m["data"]["X"], dtype=np.float64).reshape(-1), "y": np.array(m["data"]["y"], dtype=np.float64), "K": 7})
    user = pl.user_spec(m)
    groups = [np.arange(40, dtype=np.int32) % 7]
    for text in (True, False):
        spec = {"user": dict(user, pointwise=m["terms_source"]) if text else user, "params": fam["params"], "P": fam["P"], "init": fam["init"], "comp_opts": fam["comp_opts"]}
        s = A.Sampler(spec, chains=64, seed=lr.SEED)
        s.burn(50)
        draws = s.sample(10)
        if text:      # the hiprtc instantiation against the rule itself: the grouped terms are numpy's sums of the ungrouped device terms
            ll = A.user_waic_check(draws, [user], m["terms_source"], m["P"], 40, loglik=True)["loglik"][0]
            grouped = A.user_waic_check(draws, [user], m["terms_source"], m["P"], 40, loglik=True, groups=groups)["loglik"][0]
            assert grouped.tobytes() == group_sum(ll, groups[0]).tobytes()
            same_as_the_test_library(s, draws, A.user_waic_check(draws, [user], m["terms_source"], m["P"], 40, groups=groups),
                                     A.user_loo_check(draws, [user], m["terms_source"], m["P"], 40, groups=groups), groups)
        else:
            with pytest.raises(A.AmwgError, match="amwg_last_sample_dataset_waic_grouped: the pointwise terms of a closure are not known"):
                A._check(A.lib().amwg_last_sample_dataset_waic_grouped(s.h, groups[0].ctypes.data_as(A.C.POINTER(A.C.c_int32)), A._dp(np.empty(4)), None, None, None))
        s.close()


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_grouped_on_gpu():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([shutil.which("node"), os.path.join(root, "tests", "js", "test_gpu_grouped.js")], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu grouped ok" in p.stdout, p.stdout + "\n" + p.stderr
