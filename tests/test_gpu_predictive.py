"""Posterior predictive calibration per dataset on the device (csrc/amwg_predictive.hip), on the GPU.  tests/README.predictive.md says what each test pins."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import predictive_reference as pr
import waic_reference as wr
from test_gpu_waic import draws_for, family_spec, same_values, spec_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261127
MODELS = ["normal", "beta_bern", "hier_normal", "pois_glm"]
# (rows, chains per dataset, the datasets' m): 6 draws -- fewer than the lanes of an observation, a block cut short; 515 draws -- 2 splits of 257 and 258, a last
# staged run of 1 or 2 draws.  m: a short tile (Np = 1, 4, 8), a full tile, two tiles, an empty dataset
SHAPES = [(3, 2, (1, 0, 65)), (103, 5, (3, 64, 5))]


def scored(draws, specs, held=None, index=None, got=None):
    """the device's answer against the reference: every value within its tolerance, the reference's NaN pattern, NaN beyond m_d, the summary as the finish gives it
    from the pointwise values (the finish itself: tests/test_predictive_host.py)"""
    got, worst = got or amwg_ctypes.predictive_check(draws, specs, held, index=index), np.zeros(4)
    for d, h in enumerate(held or specs):
        m, pw = h["n_obs"], got["pointwise"][d]
        assert np.isnan(pw[m:]).all() and same_values(amwg_ctypes.predictive_totals(pw[:m], h["data"]["y" if h["model"] == "pois_glm" else "x"][:m]), got["summary"][d]), (d, m, got["summary"][d])
        want, tol = pr.pointwise(h, wr.draws_of_dataset(draws, len(specs), d), index[d] if index else None)
        assert (np.isnan(pw[:m]) == np.isnan(want)).all(), (d, pw[:m], want)
        ok, err = ~np.isnan(want[:, 0]), np.abs(pw[:m] - want)
        err[:, 3] = np.abs(pw[:m, 3] ** 2 - want[:, 3] ** 2)
        if ok.any():
            worst = np.maximum(worst, (err[ok] / tol[ok]).max(axis=0))
    print("%s draws %s m %s: largest error / bound, pit_hi pit_lo mean sd^2: %s" % (specs[0]["model"], draws.shape, [h["n_obs"] for h in held or specs], worst))
    assert (worst <= 1.0).all()
    return got


@pytest.mark.parametrize("rows,cpd,sizes", SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_in_sample_against_the_rule(model, rows, cpd, sizes):
    rng = np.random.default_rng(SEED + rows)
    for ms in ([[m] for m in sizes if m] if model == "hier_normal" else [sizes]):      # (the hierarchical family runs on one dataset)
        scored(draws_for(model, rows, len(ms) * cpd, rng, n_obs=max(ms)), [spec_of(model, m, rng) for m in ms])


def test_poisson_positions_across_the_change_point():
    rng = np.random.default_rng(SEED + 1)
    held, index, draws = [spec_of("pois_glm", 9, rng)], [rng.permutation(40)[:9]], draws_for("pois_glm", 3, 5, rng)
    draws[:, 8, :] = rng.integers(int(index[0].min()) + 1, int(index[0].max()), size=(3, 5))      # every draw's change point falls between the positions
    with_index = scored(draws, [spec_of("pois_glm", 1, rng)], held, index=index)
    assert not same_values(with_index["pointwise"], amwg_ctypes.predictive_check(draws, held)["pointwise"])


@pytest.mark.parametrize("model", MODELS)
def test_non_finite_values_stay_where_they_are(model):
    rng = np.random.default_rng(SEED + 2)
    D, cpd = (1, 6) if model == "hier_normal" else (3, 2)
    held = [spec_of(model, m, rng) for m in (65, 3, 5)[:D]]
    draws = draws_for(model, 7, D * cpd, rng, n_obs=65)
    draws[(3, 2, 1) if model == "hier_normal" else (3, 0, cpd)] = np.nan      # theta of group 2 in one draw: that group's observations alone | a draw of dataset 1
    if model in ("beta_bern", "pois_glm"):      # an x that is neither 0 nor 1 | a count that is no integer
        held[0]["data"]["x" if model == "beta_bern" else "y"][2] = 0.5
    got = scored(draws, [spec_of(model, 1, rng) for _ in held], held)      # (the NaN pattern is the reference's)
    nan = [np.isnan(got["pointwise"][d][:h["n_obs"], 0]) for d, h in enumerate(held)]
    if model == "hier_normal":
        assert (nan[0] == (held[0]["data"]["g"] == 2)).all() and nan[0].any() and not nan[0].all() and np.isnan(got["summary"][0]).all()
    else:
        assert nan[1].all() and not nan[2].any() and nan[0].sum() == (0 if model == "normal" else 1) and (model == "normal" or nan[0][2])
        assert np.isnan(got["summary"][1]).all() and not np.isnan(got["summary"][2]).any() and np.isnan(got["summary"][0]).all() == (model != "normal")


def test_the_same_bytes_whatever_the_budget_and_the_neighbours():
    rng = np.random.default_rng(SEED + 3)
    cpd, specs = 16, [spec_of("normal", m, rng) for m in (130, 5, 65)]
    draws = draws_for("normal", 64, 3 * cpd, rng)      # 1 024 draws per dataset: 4 splits
    a = amwg_ctypes.predictive_check(draws, specs)
    other = amwg_ctypes.predictive_check(draws, specs, scratch_bytes=1 << 12)      # every dataset a batch of its own
    assert other["pointwise"].tobytes() == a["pointwise"].tobytes() and other["summary"].tobytes() == a["summary"].tobytes()
    alone = amwg_ctypes.predictive_check(np.ascontiguousarray(draws[:, :, 2 * cpd:]), specs[2:])
    assert alone["pointwise"][0].tobytes() == a["pointwise"][2][:65].tobytes() and alone["summary"][0].tobytes() == a["summary"][2].tobytes()


@pytest.mark.parametrize("model,sizes", [("normal", (70, 5)), ("beta_bern", (70, 5)), ("hier_normal", (70,)), ("pois_glm", (40, 40))])
def test_a_samplers_own_data_given_as_held_out_gives_the_in_sample_bytes(model, sizes):
    specs = [family_spec(model, n, 500 + 7 * d) for d, n in enumerate(sizes)]
    s = amwg_ctypes.Sampler(specs if len(specs) > 1 else specs[0], chains=len(sizes) * 32, seed=SEED, ragged=len(set(sizes)) > 1)
    s.burn(100)
    draws = s.sample(20)
    own, given = s.dataset_predictive(), s.dataset_predictive(specs)
    assert own["pointwise"].tobytes() == given["pointwise"].tobytes() and own["summary"].tobytes() == given["summary"].tobytes()
    assert not np.isnan(own["summary"]).any() and own["pointwise"].shape == (len(sizes), max(sizes), 4)
    assert same_values(own["pointwise"], amwg_ctypes.predictive_check(draws, specs)["pointwise"])


def test_what_a_sampler_refuses():
    spec = family_spec("hier_normal", 64, 41)
    held = dict(spec, n_obs=3, data={"x": np.zeros(3), "g": np.zeros(3, dtype=np.int32)})
    s, gl = amwg_ctypes.Sampler(spec, chains=64, seed=SEED), amwg_ctypes.Sampler(spec, chains=64, seed=SEED, group_local=1)
    gl.sample(4)
    steps = [(s, None, "no sample() call yet", s.sample), (gl, None, "group_local", None), (s, dict(held, G=spec["G"] + 1), "G = ", None),
             (s, dict(held, model="normal"), "is of model", s.summarize), (s, held, "amwg_sample_summarize", None)]
    for who, arg, words, then in steps:
        with pytest.raises(amwg_ctypes.AmwgError, match="amwg_last_sample_dataset_predictive") as ei:
            who.dataset_predictive([arg] if arg else None)
        assert words in str(ei.value), str(ei.value)
        then and then(4)


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_javascript_front_end():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_predictive.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
