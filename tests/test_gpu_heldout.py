"""Held-out predictive density per dataset on the device (csrc/amwg_heldout.hip), on the GPU.  tests/README.heldout.md says what each test pins and by which reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import waic_reference as wr
from test_gpu_waic import draws_for, family_spec, normal_case, same_values, spec_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261126
MODELS = ["normal", "beta_bern", "hier_normal", "pois_glm"]
SHAPES = [(1, 2), (2, 3), (17, 65), (8, 512)]      # fewer draws than lanes per observation; one staged run; several runs; several splits
TRIPLES = [(1, 0, 65), (2, 33, 130), (3, 64, 0)]   # Np = 1, 2, 4, 64; a second tile; a ragged last tile; an empty dataset


def totals(lppd, m):
    """the finish of include/amwg.h restated: running sums from 0.0 in index order"""
    elpd = ss = np.float64(0.0)
    for j in range(m):
        elpd = elpd + lppd[j]
    for j in range(m):
        ss = ss + (lppd[j] - elpd / np.float64(m)) * (lppd[j] - elpd / np.float64(m))
    return np.array([elpd, np.sqrt(np.float64(m) * ss / np.float64(m - 1)) if m > 1 else np.nan])


def scored(draws, specs, held, index=None, got=None):
    """the device's answer (got: a sampler's; else the check library's) against the reference: lppd_j within the bound, the reference's NaN pattern, NaN beyond m_d,
    the totals as bytes -> (answer, worst ratio).  index (Poisson): the reference sees the held-out rows at those positions of a longer series of zero rows"""
    D, S = len(specs), draws.shape[0] * (draws.shape[2] // len(specs))
    got = got or amwg_ctypes.heldout_check(draws, specs, held, index=index)
    worst = 0.0
    for d, h in enumerate(held):
        m, pw = h["n_obs"], got["pointwise"][d]
        assert np.isnan(pw[m:]).all() and same_values(totals(pw, m), got["summary"][d]), (d, m, got["summary"][d])
        if m == 0:
            continue
        at, n = (index[d], int(max(index[d])) + 1) if index else (np.arange(m), m)
        if index:
            X, y = np.zeros((n, 7)), np.zeros(n)
            X[at], y[at] = h["data"]["x"].reshape(m, 7), h["data"]["y"]
            h = dict(h, n_obs=n, data={"x": X.reshape(-1), "y": y})
        lppd, p, mean, maxabs = wr.pointwise(wr.loglik_of(h, wr.draws_of_dataset(draws, D, d))[:, at])
        assert (np.isnan(pw[:m]) == np.isnan(lppd)).all(), (d, np.isnan(pw[:m]), np.isnan(lppd))
        ok = ~np.isnan(lppd)
        worst = max([worst] + list(np.abs(pw[:m][ok] - lppd[ok]) / wr.bounds(S, lppd, p, mean, maxabs)[0][ok]))
    print("%s draws %s held %s: largest lppd error / bound %.3g" % (specs[0]["model"], draws.shape, [h["n_obs"] for h in held], worst))
    assert worst <= 1.0
    return got, worst


@pytest.mark.parametrize("rows,cpd", SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_against_extended_precision(model, rows, cpd):
    rng = np.random.default_rng(SEED + rows)
    cases = [[m] for t in TRIPLES for m in t if m] if model == "hier_normal" else TRIPLES      # (the hierarchical family runs on one dataset)
    for sizes in cases:
        held = [spec_of(model, m, rng) for m in sizes]
        scored(draws_for(model, rows, len(sizes) * cpd, rng, n_obs=max(sizes)), [spec_of(model, 1, rng) for _ in sizes], held)


@pytest.mark.parametrize("model", MODELS)
def test_against_the_projects_own_waic(model):
    rng = np.random.default_rng(SEED + 50)
    n, rows, cpd = 70, 17, 65
    spec = spec_of(model, n, rng)
    draws = draws_for(model, rows, cpd, rng, n_obs=n)
    held, index, perm = spec, None, np.arange(n)
    if model == "pois_glm":      # a change point inside the data; the observations permuted, their positions given alike
        draws[:, 8, :] = rng.integers(1, n - 1, size=(rows, cpd))
        perm = rng.permutation(n)
        held = dict(spec, data={"x": spec["data"]["x"].reshape(n, 7)[perm].reshape(-1), "y": spec["data"]["y"][perm]})
        index = [perm]
    got = amwg_ctypes.heldout_check(draws, [spec], [held], index=index)["pointwise"][0]
    want = amwg_ctypes.waic_check(draws, [spec])["pointwise"][0][perm, 0]
    bound = 2 * (8.0 * (rows * cpd + 16) * wr.U + 4 * wr.U * np.abs(want))
    print("%s: largest |heldout - waic| / bound %.3g" % (model, (np.abs(got - want) / bound).max()))
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("kind", ["dominating", "identical", "deep"])
def test_hard_draws(kind, m):
    rng = np.random.default_rng(SEED + 60)
    S, rows = 4096, 8
    mu, sigma = np.full(S, 0.3), np.full(S, 1.7)
    if kind == "dominating":
        mu, sigma = np.full(S, 1e3) + rng.normal(size=S), np.ones(S)
        mu[1234] = 0.0
    if kind == "deep":      # terms from about -1 down to about -746 under sigma = 1
        mu, sigma = rng.permutation(np.linspace(0.0, np.sqrt(2 * 745.0), S)), np.ones(S)
    draws, specs = normal_case(rng.normal(scale=0.2, size=m), mu, sigma, rows)
    scored(draws, specs, specs)


@pytest.mark.parametrize("model", MODELS)
def test_non_finite_values_stay_where_they_are(model):
    rng = np.random.default_rng(SEED + 70)
    D, cpd = (1, 6) if model == "hier_normal" else (3, 2)
    held = [spec_of(model, m, rng) for m in (65, 3, 33)[:D]]
    draws = draws_for(model, 17, D * cpd, rng, n_obs=65)
    draws[(3, 2, 1) if model == "hier_normal" else (3, 0, cpd)] = np.nan      # theta of group 2 in one draw: that group's observations alone | a draw of dataset 1
    if model in ("beta_bern", "pois_glm"):      # an x that is neither 0 nor 1 | a negative count
        held[0]["data"]["x" if model == "beta_bern" else "y"][2] = 0.5 if model == "beta_bern" else -1.0
    got, _ = scored(draws, [spec_of(model, 1, rng) for _ in held], held)      # (the NaN pattern is the reference's)
    nan = [np.isnan(got["pointwise"][d][:h["n_obs"]]) for d, h in enumerate(held)]
    if model == "hier_normal":
        assert (nan[0] == (held[0]["data"]["g"] == 2)).all() and nan[0].any() and not nan[0].all()
    else:
        assert nan[1].all() and not nan[2].any() and nan[0].sum() == (0 if model == "normal" else 1)
        assert np.isnan(got["summary"][1]).all() and not np.isnan(got["summary"][2]).any() and np.isnan(got["summary"][0][0]) == (model != "normal")


def test_the_same_bytes_whatever_the_budget_and_the_neighbours():
    rng = np.random.default_rng(SEED + 80)
    rows, cpd = 128, 1024      # 512 runs: dataset 0 alone holds more than 1 MiB of partials
    held, own = [spec_of("normal", m, rng) for m in (130, 33, 65)], [spec_of("normal", 1, rng)] * 3
    draws = draws_for("normal", rows, 3 * cpd, rng)
    a = amwg_ctypes.heldout_check(draws, own, held)
    for other in (amwg_ctypes.heldout_check(draws, own, held), amwg_ctypes.heldout_check(draws, own, held, scratch_bytes=1 << 20)):
        assert other["pointwise"].tobytes() == a["pointwise"].tobytes() and other["summary"].tobytes() == a["summary"].tobytes()
    alone = amwg_ctypes.heldout_check(np.ascontiguousarray(draws[:, :, 2 * cpd:]), own[2:], held[2:])
    assert alone["pointwise"][0].tobytes() == a["pointwise"][2][:65].tobytes() and alone["summary"][0].tobytes() == a["summary"][2].tobytes()


@pytest.mark.parametrize("model,sizes,ragged", [("normal", (20, 50, 35, 64), True), ("pois_glm", (40, 40), False)])
def test_through_real_samplers(model, sizes, ragged):
    specs = [family_spec(model, n, 500 + 7 * d) for d, n in enumerate(sizes)]
    held = [family_spec(model, m, 900 + d) for d, m in enumerate((7, 33, 65, 1)[:len(sizes)])]
    index = [np.arange(7) * 5 + 2, np.arange(33) + 9] if model == "pois_glm" else None      # distinct positions per dataset, in and beyond the fitted series
    s = amwg_ctypes.Sampler(specs, chains=len(sizes) * 32, seed=SEED, ragged=ragged)
    s.burn(200)
    draws = s.sample(40)
    for d, at in enumerate(index or []):      # the change point of some draw falls between the held-out positions of either dataset
        cp = draws[:, 8, d * 32:(d + 1) * 32]
        assert ((cp > at.min()) & (cp <= at.max())).any(), (d, cp.min(), cp.max())
    scored(draws, specs, held, index=index, got=s.dataset_heldout(held, index=index, pointwise=True))


def test_what_a_sampler_refuses():
    spec = family_spec("hier_normal", 64, 41)
    held = dict(spec, n_obs=3, data={"x": np.zeros(3), "g": np.zeros(3, dtype=np.int32)})
    s, gl = amwg_ctypes.Sampler(spec, chains=64, seed=SEED), amwg_ctypes.Sampler(spec, chains=64, seed=SEED, group_local=1)
    gl.sample(4)
    steps = [(s, held, "no sample() call yet", s.sample), (gl, held, "group_local", None), (s, dict(held, G=spec["G"] + 1), "G = ", None),
             (s, dict(held, model="normal"), "is of model", s.summarize), (s, held, "amwg_sample_summarize", None)]
    for who, arg, words, then in steps:
        with pytest.raises(amwg_ctypes.AmwgError, match="amwg_last_sample_dataset_heldout") as ei:
            who.dataset_heldout([arg])
        assert words in str(ei.value), str(ei.value)
        if then:
            then(4)


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_javascript_front_end():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_heldout.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
