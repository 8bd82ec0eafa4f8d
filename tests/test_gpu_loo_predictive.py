"""PSIS-LOO predictive calibration per dataset on the device (csrc/amwg_loo_predictive.hip), on the GPU.  tests/README.loo_predictive.md says what each case pins."""
import numpy as np
import pytest

import amwg_ctypes
import loo_predictive_reference as lpr
import loo_reference as lr
import waic_reference as wr
from test_gpu_waic import family_spec, same_values

pytestmark = pytest.mark.gpu
SEED = 20261126


def normal(x, mu, sigma, rows):
    return lr.normal_case(x, mu, np.broadcast_to(sigma, np.shape(mu)), rows)


def tied(rng, smaller):
    """S = 2 000 (M = 135, 256 slots): 1 500 draws share one term, `smaller` distinct draws lie below it -- 0: the tie is the smallest term, a degenerate tail, the raw
    route over the class record; 120: x* stands on distinct terms, the smoothed route with 15 slots of the class below M.  sigma = 3 keeps the terms within a few
    units of each other: the class carries a weight the comparison sees"""
    mu = np.concatenate([4.2 + 0.01 * np.arange(smaller), np.full(1500, 4.0), rng.normal(1.0, 0.3, size=500 - smaller)])[rng.permutation(2000)]
    return normal(np.array([0.2, -0.5]), mu, 3.0, 25)


def case(name):
    rng = np.random.default_rng([SEED, sorted(CASES).index(name)])
    if name.startswith("S = "):      # the routes: M = 4 (raw), M = 5 (the smallest smoothed), M + 1 > 128 (the 256-thread sort)
        rows, cpd = {"S = 20": (4, 5), "S = 25": (5, 5), "S = 1900": (25, 76)}[name]
        return lr.draws_for("normal", rows, cpd, rng), [lr.spec_of("normal", 3, rng)]
    if name == "ragged":      # the tile edges, three datasets together
        return lr.draws_for("normal", 5, 15, rng), [lr.spec_of("normal", n, rng) for n in (1, 63, 65)]
    if name in ("hier_normal", "nan_draw"):
        draws, specs = lr.draws_for("hier_normal", 5, 5, rng), [lr.spec_of("hier_normal", 9, rng)]
        specs[0]["data"]["g"][:3] = [2, 0, 2]
        if name == "nan_draw":
            draws[3, 2, 1] = np.nan      # theta of group 2 in one draw
        return draws, specs
    if name in ("pois_glm", "beta_bern"):
        return lr.draws_for(name, 6, 10, rng, n_obs=6), [lr.spec_of(name, n, rng) for n in (6, 5)]
    x = np.array([0.0, 0.7])
    if name == "repeated":      # 24 draws repeated 3, 2, 4, 1, ... times in the order of observation 0's terms: S = 60, M = 12, the fifth run holds positions 10, 11, 12
        mu = rng.normal(0.0, 1.0, size=24)
        mu = np.repeat(mu[np.argsort(-np.abs(mu))], [3, 2, 4, 1] * 6)[rng.permutation(60)]
        return normal(x, mu, 1.3, 6)
    if name == "mirrored":      # mu = +-delta about x_0 = 0 under one sigma: equal terms, different F; S = 35, M = 7: the fourth pair holds positions 6 and 7
        delta = rng.uniform(0.2, 3.0, size=17)
        return normal(x, np.concatenate([delta, -delta, [0.0]])[rng.permutation(35)], 1.1, 5)
    return tied(rng, {"tie_smallest": 0, "tie_at_the_cutoff": 120}[name])


CASES = {"S = 20": 0, "S = 25": 0, "S = 1900": 0, "ragged": 0, "hier_normal": 0, "pois_glm": 0, "beta_bern": 0, "repeated": 0, "mirrored": 0, "tie_smallest": 0,
         "tie_at_the_cutoff": 0, "nan_draw": 0}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_rule(name):
    draws, specs = case(name)
    D, S = len(specs), draws.shape[0] * draws.shape[2] // len(specs)
    got = amwg_ctypes.loo_predictive_check(draws, specs)
    ll = amwg_ctypes.waic_check(draws, specs, loglik=True)["loglik"]
    loo = amwg_ctypes.loo_check(draws, specs)
    worst = np.zeros(4)
    for d, spec in enumerate(specs):
        n, pw = spec["n_obs"], got["pointwise"][d]
        want, tol = lpr.pointwise(spec, wr.draws_of_dataset(draws, D, d), ll[d][:, :n])
        assert np.isnan(pw[n:]).all() and (np.isnan(pw[:n]) == np.isnan(want)).all(), (d, pw[:n], want)
        assert np.array_equal(pw[:n, 4], loo["pointwise"][d][:n, 2], equal_nan=True) and np.array_equal(np.isinf(pw[:n, 4]), np.isinf(want[:, 4]))      # khat_i: LOO's bytes
        y = spec["data"]["y" if spec["model"] == "pois_glm" else "x"][:n]
        assert same_values(amwg_ctypes.predictive_totals(pw[:n, :4], y), got["summary"][d]) and got["high"][d] == (pw[:n, 4] > 0.7).sum()
        ok, err = ~np.isnan(want[:, 0]), np.abs(pw[:n, :4] - want[:, :4])
        err[:, 3] = np.abs(pw[:n, 3] ** 2 - want[:, 3] ** 2)
        if ok.any():
            worst = np.maximum(worst, (err[ok] / tol[ok]).max(axis=0))
    print("%s (S = %d): largest error / bound, pit_hi pit_lo mean sd^2: %s" % (name, S, worst))
    assert (worst <= 1.0).all()
    if name == "ragged":      # the middle dataset alone, and under a scratch budget that makes every dataset a batch: the same bytes
        alone = amwg_ctypes.loo_predictive_check(np.ascontiguousarray(draws[:, :, 5:10]), specs[1:2])
        tight = amwg_ctypes.loo_predictive_check(draws, specs, scratch_bytes=1 << 12)
        assert alone["pointwise"][0].tobytes() == got["pointwise"][1][:63].tobytes() and tight["pointwise"].tobytes() == got["pointwise"].tobytes()
    if name == "nan_draw":
        nan = np.isnan(got["pointwise"][0][:, 0])
        assert (nan == (specs[0]["data"]["g"] == 2)).all() and np.isnan(got["pointwise"][0][nan]).all() and np.isnan(got["summary"][0]).all()
    if name == "mirrored":      # observation 0: the two draws of a pair weigh the same, so pred_mean is the shared centre whatever the PSIS weights are
        assert abs(got["pointwise"][0][0, 2]) <= 1e-12


def test_a_sampler_gives_the_bytes_of_the_check_call_on_its_draws():
    specs = [family_spec("normal", n, 900 + d) for d, n in enumerate((70, 5, 33))]
    s = amwg_ctypes.Sampler(specs, chains=24, seed=SEED, ragged=True)
    s.burn(100)
    with pytest.raises(amwg_ctypes.AmwgError, match="amwg_last_sample_dataset_loo_predictive.*no sample"):
        s.dataset_predictive(loo=True)
    draws = s.sample(40)
    got, want = s.dataset_predictive(loo=True), amwg_ctypes.loo_predictive_check(draws, specs)
    assert got["pointwise"].shape == (3, 70, 5) and not np.isnan(got["summary"]).any()
    for k in ("pointwise", "summary", "high"):
        assert got[k].tobytes() == want[k].tobytes(), k
