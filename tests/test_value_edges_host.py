"""No GPU: the host twin of tests/test_gpu_value_edges.py (README.edges.md).  It validates the INPUTS of that file without a device:
  * mid_range / wide_range of csrc/amwg_div.h restated in numpy on the high words, against their stated ranges at the edges;
  * every case's `reaches` -- asserted on the data, den = 2 sigma^2 and mu that the case starts from: outside the range where it means to be outside, inside where
    it means to be inside;
  * the oracle side of every case (oracle_lib.OracleChain, chains 0 and C - 1, the schedule of the GPU file): alive cases accept and reject in every adapting
    component, stuck cases accept nothing, and log_post is what the case says (-inf, NaN, finite);
  * the case list is complete, and the comparison's own rules: a NaN equals a NaN of another sign and payload in log_post only, -0.0 is not +0.0 in a state."""
import numpy as np
import pytest

import value_edges_cases as V

ALL = [(f, n) for f in V.EXPECTED for n in V.EXPECTED[f]]


def test_case_list_is_complete():
    for fam, names in V.EXPECTED.items():
        assert [c["name"] for c in V.cases(fam)] == names
        assert all(c["kind"] in ("alive", "alive_any", "stuck", "frozen") for c in V.cases(fam))
    assert set(V.DAGGER) <= set(V.EXPECTED["normal"])
    assert (V.CHAINS, V.BURN, V.N1, V.THIN, V.N2) == (100, 50, 70, 3, 5)      # a partial second wavefront; the first sample call crosses the batch boundary at 50
    for name in V.EXPECTED["normal"]:
        assert V.case("normal", name)["spec"]["n_obs"] == (2049 if name == "a_2049_observations" else 200)
    assert all(c["spec"]["n_obs"] == 300 for f in ("beta_bern", "pois_glm") for c in V.cases(f))
    assert all(c["spec"]["n_obs"] == 640 and c["spec"]["G"] == 8 for c in V.cases("hier_normal"))


def test_range_predicates_restated_on_the_high_words():
    two = lambda k: float(np.ldexp(1.0, k))
    below = lambda v: float(np.nextafter(v, 0.0))
    above = lambda v: float(np.nextafter(v, np.inf))
    assert V.mid_range([two(-200), two(200), 1.0, 1e-40, 1e40]).all()
    assert not V.mid_range([below(two(-200)), two(201), 0.0, -1.0, np.inf, np.nan, 1e70, 1e-70, 5e-324]).any()
    assert V.mid_range(above(two(200))).all() and not V.mid_range(two(200) * (1.0 + 2.0 ** -19)).any()      # the test is on the high word: 2^200 (1 + 2^-20) is the first value outside
    assert not V.mid_range(below(two(201))).any()
    assert V.wide_range([two(-600), two(600), -two(600), 1.0, -1e140, 1e-160]).all()
    assert not V.wide_range([0.0, below(two(-600)), two(601), np.inf, np.nan, 1e250 * 1e50, 1e-200]).any()
    assert V.hi_word(1.0)[0] == 0x3FF00000 and V.hi_word(two(200))[0] == 0x4C700000 and V.hi_word(two(-200))[0] == 0x33700000


def test_the_comparison_rules():
    nan_cpu, nan_gpu = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64), np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    assert V.same("log_post1", nan_cpu, nan_gpu) and not V.same("log_post1", nan_cpu, [-np.inf]) and not V.same("log_post1", [1.0], [np.nextafter(1.0, 2.0)])
    assert not V.same("state", nan_cpu, nan_gpu)      # a NaN in a draw or state is compared as bytes
    assert not V.same("state", [-0.0], [0.0]) and V.same("state", [-0.0], [-0.0]) and not V.same("draws1", [[0.0, -0.0]], [[0.0, 0.0]])
    assert V.same("accepts", np.array([3], dtype=np.int32), np.array([3], dtype=np.int64)) and not V.same("uniforms1", [3], [4])


@pytest.fixture(scope="module")
def oracle_runs():
    """every case on the oracle once: {(family, name): [record of chain 0, record of chain C - 1]}"""
    return {(f, n): [V.oracle_record(V.case(f, n)["spec"], ch) for ch in (0, V.CHAINS - 1)] for f, n in ALL}


@pytest.mark.parametrize("family,name", ALL)
def test_the_case_reaches_its_branch_and_is_alive_or_stuck_on_the_oracle(family, name, oracle_runs):
    c = V.case(family, name)
    with np.errstate(all="ignore"):
        c["reaches"](c["spec"])
    recs = oracle_runs[(family, name)]
    assert V.kind_holds(c["kind"], recs, c["spec"], c["components"]) is None, V.kind_holds(c["kind"], recs, c["spec"], c["components"])
    for r in recs:
        assert r["draws1"].shape == (24, c["spec"]["P"]) and r["draws2"].shape == (5, c["spec"]["P"])
        if c["kind"] in ("stuck", "frozen"):
            assert np.array_equal(r["state"], np.array(c["spec"]["init"])) and V.same("log_post2", r["log_post0"], r["log_post2"])
        else:
            assert np.isfinite(r["log_post2"]), r["log_post2"]


def test_what_the_oracle_says_of_single_cases(oracle_runs):
    lp = lambda f, n, k: [r[k] for r in oracle_runs[(f, n)]]
    # starts with log_post = -inf and recovers
    for f, n in (("normal", "f_outside_support"), ("beta_bern", "theta_init_0"), ("beta_bern", "theta_init_1"), ("hier_normal", "outside_support")):
        assert lp(f, n, "log_post0") == [-np.inf, -np.inf] and np.isfinite(lp(f, n, "log_post2")).all()
    # stuck at -inf / at NaN: every update is -inf - -inf or NaN - NaN
    for f, n in (("normal", "i_inf"), ("normal", "i_1e250"), ("beta_bern", "invalid_2.0"), ("beta_bern", "invalid_0.5"), ("pois_glm", "negative_count")):
        assert lp(f, n, "log_post0") == [-np.inf, -np.inf] and lp(f, n, "log_post2") == [-np.inf, -np.inf]
    assert np.isnan(lp("normal", "i_nan", "log_post0")).all() and np.isnan(lp("normal", "i_nan", "log_post2")).all()
    # magnitudes the issue names
    assert all(-4e4 < v < -3e4 for v in lp("normal", "a_one_out_of_mid_range", "log_post2"))
    assert all(abs(v) > 1e7 for v in lp("pois_glm", "count_1e6", "log_post0"))
    # int mu on centred data: one of the two chains ends at -0.0, the other at +0.0 -- the sign is part of the state
    ends = sorted(np.signbit(r["state"][0]) for r in oracle_runs[("normal", "h_int_mu_zero")])
    assert all(r["state"][0] == 0.0 for r in oracle_runs[("normal", "h_int_mu_zero")]) and ends == [False, True]
    # constant data: mu stays at the data's value, S2 == 0 exactly, sigma is driven towards its bound and proposals fall outside it
    for r in oracle_runs[("normal", "h_int_mu_constant_data")]:
        assert r["state"][0] == 3.0 and 0.0 < r["state"][1] < 0.05 and r["inbounds"][1] < V.STEPS
    # sigma without a lower bound: every proposal is inside the bounds, the negative ones among them give NaN and are rejected
    for r in oracle_runs[("normal", "g_sigma_unbounded")]:
        assert r["inbounds"].tolist() == [V.STEPS, V.STEPS] and r["state"][1] > 0.0
    # all counts zero: the betas' intercept runs negative; the change point's every proposal is accepted (why the alive condition is asked of the betas there)
    for r in oracle_runs[("pois_glm", "all_counts_zero")]:
        assert r["accepts"][8] == r["inbounds"][8] > 0
    # the stuck chains consume the uniforms of their bounds checks only: fewer than an alive chain of the same family
    assert all(r["uniforms2"] < 1100 for r in oracle_runs[("normal", "i_nan")])


def test_dataset_specs_share_the_sampler_and_differ_in_the_middle():
    for middle in ("a_one_out_of_mid_range", "f_outside_support"):
        specs = V.dataset_specs(middle)
        assert len(specs) == 3 and specs[1] is V.case("normal", middle)["spec"]
        for s in specs:
            assert s["init"] == specs[1]["init"] and s["comp_opts"] == specs[1]["comp_opts"] and s["params"] == specs[1]["params"] and s["n_obs"] == 200
        assert V.data_mid_range(specs[0]["data"]["x"]) and V.data_mid_range(specs[2]["data"]["x"])
        assert specs[0]["hyper"] == specs[2]["hyper"] == specs[1]["hyper"] != None      # noqa: E711  (shared: amwg_create_datasets refuses anything else)
