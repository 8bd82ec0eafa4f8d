"""-m gpu: every family's kernels on non-finite and out-of-range log_post (README.edges.md; the inputs and what each is aimed at: tests/value_edges_cases.py,
validated without a device by tests/test_value_edges_host.py).

The other sampling tests drive the kernels with unit-scale data, default priors and chains started inside the support: log_post is finite there and every
value stays inside the range the fast arithmetic needs.  Here it is not: an observation, den = 2 sigma^2 or mu outside mid_range (csrc/amwg_div.h), a start outside
the prior's support (lp = -inf, then dA = +inf), -inf - -inf and NaN in every update, eta beyond 690, a negative count.  The branches that exist for these inputs --
certified_test's verdict 0, the accept shortcuts of step_body and of the lean Normal stepper, pass_slow, has_invalid, the H > 690 guard -- decide every case.

References, for every case:
  1. the same sampler at ONE lane per chain with full_evaluation = 1 (the reference's expression in the reference's order in every update; for the Beta-Bernoulli
     family exact_division = 1: the term-by-term pass) -- all 100 chains, every bit: the draws of two sample() calls, the final state, every info() counter, the
     uniforms consumed, the named order and log_post after zero steps, between the two calls and at the end.  The kernel is asserted on both sides.
  2. oracle_lib.OracleChain for chain 0 and chain 99, in the sampler's summation order.
log_post compares as "both NaN, or the same bits" (the CPU and the device produce NaNs of different sign and payload for inf - inf); draws and states as bytes
(-0.0 is not +0.0).  No tolerance anywhere.  100 chains (a partial second wavefront), burn 50, sample(70, thin = 3), diag(), sample(5), diag().

Every case also asserts that it is what it says: "alive" -- on chains 0 and 99 every adapting component accepts and rejects --, "stuck" -- accepts == 0 on ALL
chains --, "frozen" -- every proposal equals the current value and is accepted --, and for X * 150 that some chain of the sampler accepts a beta."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SCRATCH = ["a_one_out_of_mid_range", "f_outside_support"]      # the cases of the child process (AMWG_WAVE_SCRATCH=0)

_refs, _oracles = {}, {}


def _V():
    import value_edges_cases
    return value_edges_cases


def _run(spec, kernel, lanes, **options):
    """-> (record, launch_info) of one sampler over the schedule; the kernel it ran is asserted"""
    import amwg_ctypes as A
    V = _V()
    s = A.Sampler(spec, chains=V.CHAINS, seed=V.SEED, lanes_per_chain=lanes, **options)
    li = s.launch_info()
    assert li["kernel"].startswith(kernel), (kernel, li)
    if lanes:
        assert li["lanes_per_chain"] == lanes, li
    if options.get("block_threads"):
        assert li["block_threads"] == options["block_threads"], li
    rec = V.sampler_record(s)
    s.close()
    return rec, li


def _reference(family, name, kernel, **options):
    """the one-lane sampler that evaluates the expression in every update: run once per case and shared, never changed"""
    if (family, name) not in _refs:
        rec, li = _run(_V().case(family, name)["spec"], kernel, 1, **options)
        assert "_cert" not in li["kernel"] and li["summation_order"] == 1, li
        _refs[(family, name)] = rec
    return _refs[(family, name)]


def _oracle(family, name, local, lanes=1, group_local=False):
    key = (family, name, local, lanes, group_local)
    if key not in _oracles:
        _oracles[key] = _V().oracle_record(_V().case(family, name)["spec"], local, lanes=lanes, group_local=group_local)
    return _oracles[key]


def _check(family, name, got, li, reference=None, oracle_lanes=1, group_local=False):
    """what differs from the reference sampler (all chains) and from the oracle (chains 0 and C - 1); then the case's own condition"""
    V = _V()
    c = V.case(family, name)
    bad = [] if reference is None else V.differences(got, reference)
    for local in (0, V.CHAINS - 1):
        bad += V.differences_from_oracle(got, _oracle(family, name, local, oracle_lanes, group_local), local)
    assert not bad, (family, name, bad, li)
    steps = V.STEPS
    assert (got["inbounds"] <= steps).all() and (got["accepts"] <= got["inbounds"]).all()
    ends = [{k: V.chain_of(got, k, local) for k in ("accepts", "inbounds")} for local in (0, V.CHAINS - 1)]
    if c["kind"] == "stuck":
        assert (got["accepts"] == 0).all(), got["accepts"]      # ALL chains
        assert np.array_equal(got["state"], np.repeat(np.array(c["spec"]["init"])[:, None], V.CHAINS, axis=1))
    elif c["kind"] == "frozen":
        assert (got["accepts"] == got["inbounds"]).all() and (got["inbounds"] > 0).all()
        assert np.array_equal(got["state"], np.repeat(np.array(c["spec"]["init"])[:, None], V.CHAINS, axis=1))
    elif c["kind"] == "alive_any":
        assert got["accepts"][:8].sum() > 0 and got["accepts"].sum() < got["inbounds"].sum(), got["accepts"]      # over the whole sampler: some chain accepts a beta
    else:
        assert V.kind_holds("alive", ends, c["spec"], c["components"]) is None, V.kind_holds("alive", ends, c["spec"], c["components"])
    return got


def test_every_case_of_the_list_is_run_here():
    """the parametrised tests below take their cases from EXPECTED: nothing is skipped, and the lists are the files' own"""
    V = _V()
    assert NORMAL == V.EXPECTED["normal"] and BERN == V.EXPECTED["beta_bern"] and POIS == V.EXPECTED["pois_glm"] and HIER == V.EXPECTED["hier_normal"]
    assert DAGGER == V.DAGGER and set(NO_SCRATCH) <= set(DAGGER)
    for fam in V.EXPECTED:
        assert [c["name"] for c in V.cases(fam)] == V.EXPECTED[fam]


# ---- Normal family
NORMAL = ["a_one_out_of_mid_range", "b_scale_1e-40", "b_scale_1e-155", "c_scale_1e40", "d_offset_1e15", "e_scale_1e-40_default_scale", "e_scale_1e40_default_scale",
          "e_offset_1e15_default_scale", "f_outside_support", "g_sigma_unbounded", "h_int_mu_zero", "h_int_mu_constant_data", "i_nan", "i_inf", "i_1e250",
          "a_2049_observations"]
DAGGER = ["a_one_out_of_mid_range", "d_offset_1e15", "f_outside_support"]
N_CERT, N_FULL = "amwg_step_kernel_cert<NormalModel,1,%d>", "amwg_step_kernel<NormalModel,1,"


def _normal(name, kernel=N_CERT % 256, **options):
    got, li = _run(_V().case("normal", name)["spec"], kernel, 1, **options)
    assert li["summation_order"] == 1, li
    return _check("normal", name, got, li, _reference("normal", name, N_FULL, full_evaluation=1))


@pytest.mark.parametrize("name", NORMAL)
def test_normal_lean_stepper(name):
    """amwg_step_kernel_cert<NormalModel,1,256>: normal_one_lane_body's copy of the accept shortcuts and certified_test on non-finite differences"""
    got = _normal(name)
    lp0 = got["log_post0"]
    if name == "f_outside_support":
        assert (lp0 == -np.inf).all() and np.isfinite(got["log_post2"]).all()      # after zero steps: -inf; the first proposal inside the support has dA = +inf
    elif name == "i_nan":
        assert np.isnan(lp0).all() and np.isnan(got["log_post2"]).all()
    elif name in ("i_inf", "i_1e250"):
        assert (lp0 == -np.inf).all() and (got["log_post2"] == -np.inf).all()
    elif name == "h_int_mu_zero":
        mu = got["state"][0]
        assert (mu == 0.0).all() and np.signbit(mu).any() and not np.signbit(mu).all()      # -0.0 and +0.0 both occur: the sign is compared (bytes)
    elif name == "g_sigma_unbounded":
        assert (got["inbounds"] == _V().STEPS).all() and (got["state"][1] > 0.0).all()      # (a negative sigma is inside the bounds, its log_post NaN: rejected)


@pytest.mark.parametrize("block", [512, 1024])
@pytest.mark.parametrize("name", DAGGER)
def test_normal_512_and_1024_thread_classes(name, block):
    _normal(name, N_CERT % block, block_threads=block)


@pytest.mark.parametrize("name", DAGGER)
def test_normal_sufficient_statistics(name):
    _normal(name, N_CERT % 256, sufficient_statistics=1)


@pytest.mark.parametrize("shift", [24, 40])
@pytest.mark.parametrize("name", DAGGER)
def test_normal_wide_bounds(name, shift):
    """test_bound_shift: certified_test_wide's guard (eta >= 2^9 at 40) on top of the non-finite values"""
    _normal(name, N_CERT % 256, test_bound_shift=shift)


@pytest.mark.parametrize("name", DAGGER)
def test_normal_sixty_four_lanes_against_the_oracle_in_that_order(name):
    """the plain lane-order kernel (not certified): every double against the oracle in summation_order"""
    got, li = _run(_V().case("normal", name)["spec"], "amwg_step_kernel<NormalModel,64,", 64)
    assert li["summation_order"] == 64, li
    _check("normal", name, got, li, None, oracle_lanes=64)


def test_normal_readlane_form_without_wave_scratch():
    """AMWG_WAVE_SCRATCH=0 in a fresh child process (this file run as a script): every case of NO_SCRATCH must report, and report no difference."""
    assert "AMWG_WAVE_SCRATCH" not in os.environ
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, AMWG_WAVE_SCRATCH="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert [c["case"] for c in rec] == NO_SCRATCH
    for c in rec:
        assert c["differs"] == [] and c["kernel"] == N_CERT % 256, c


@pytest.mark.parametrize("middle", ["a_one_out_of_mid_range", "f_outside_support"])
def test_normal_dataset_sampler_with_a_live_edge_case_in_the_middle(middle):
    """amwg_step_kernel_cert_ds: the middle dataset is case a (data_mid_range = 0 for it alone, alive) or case f (every dataset starts outside the support and
    recovers) -- each dataset against an ordinary sampler on it at its chain_offset."""
    from dataset_harness import against_twins
    specs = _V().dataset_specs(middle)
    got = against_twins(specs, 64, 1, 64, kernel="amwg_step_kernel_cert_ds<NormalModel,1,256>")
    acc, inb = got["info"]["accepts"][:, 64:128].sum(axis=1), got["info"]["inbounds"][:, 64:128].sum(axis=1)
    assert (acc > 0).all() and (acc < inb).all(), (acc, inb)      # alive: the middle dataset's chains accept and reject in both components
    assert np.isfinite(got["diag"]["log_post"][64:128]).all()


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_case_a_through_the_certified_tail_of_a_translated_closure():
    """tests/js/user_models.js edge_normal_one_out: bench_normal's closure with case a's priors as literals (the translator accepts them) on case a's data --
    amwg_user_step_cert against the closure evaluated in every update (amwg_user_step), against the hand-written family, and against the oracle"""
    import user_host
    V = _V()
    fam = V.case("normal", "a_one_out_of_mid_range")["spec"]
    src, arrays, meta = user_host.translated("edge_normal_one_out")
    assert meta["cert_tail_n"] == 200 and "kCertifiedTail = true" in src and arrays[0].tobytes() == fam["data"]["x"].tobytes()
    spec = {k: fam[k] for k in ("params", "P", "init", "comp_opts")}
    spec["user"] = user_host.user_spec_part(src, arrays, meta)
    want, li = _run(spec, "amwg_user_step", 1, full_evaluation=1)
    assert li["kernel"] == "amwg_user_step", li
    got, li = _run(spec, "amwg_user_step_cert", 1)
    assert li["kernel"] == "amwg_user_step_cert" and li["summation_order"] == 1, li
    assert not V.differences(got, want), V.differences(got, want)
    _check("normal", "a_one_out_of_mid_range", got, li, _reference("normal", "a_one_out_of_mid_range", N_FULL, full_evaluation=1))


# ---- Beta-Bernoulli family, n = 300
BERN = ["theta_init_0", "theta_init_1", "all_ones", "all_zeros_flat_prior", "hyper_half_half", "theta_unbounded", "invalid_2.0", "invalid_0.5"]
B_ONE = "amwg_step_kernel<BetaBernModel,1,"


@pytest.mark.parametrize("variant", ["fast_forward", "exact_division", "sixty_four_lanes"])
@pytest.mark.parametrize("name", BERN)
def test_beta_bernoulli(name, variant):
    """one lane (the two-valued fast-forward), exact_division = 1 (term by term) and 64 lanes: has_invalid, log_v8(0) at theta = 0 and 1, the flat prior's shortcut"""
    spec = _V().case("beta_bern", name)["spec"]
    if variant == "sixty_four_lanes":
        got, li = _run(spec, "amwg_step_kernel<BetaBernModel,64,", 64)
        got = _check("beta_bern", name, got, li, None, oracle_lanes=li["summation_order"])
    else:
        ref = _reference("beta_bern", name, B_ONE, exact_division=1, full_evaluation=1)
        got, li = _run(spec, B_ONE, 1, exact_division=1 if variant == "exact_division" else 0)
        got = _check("beta_bern", name, got, li, ref)
    if name.startswith("theta_init"):
        assert (got["log_post0"] == -np.inf).all() and np.isfinite(got["log_post2"]).all()
    if name.startswith("invalid"):
        assert (got["log_post0"] == -np.inf).all() and (got["log_post2"] == -np.inf).all()


# ---- Poisson GLM with a change point, n = 300
POIS = ["X_times_150", "zero_count_rows_times_600", "negative_count", "non_integer_count", "count_1e6", "all_counts_zero"]


@pytest.mark.parametrize("shift", [0, 18])
@pytest.mark.parametrize("name", POIS)
def test_poisson_sixteen_lane_certified_kernel(name, shift):
    """amwg_step_kernel_cert<PoisGlmModel,16,256>: H > 690, a negative count (F = +inf), lfactorial of a non-integer, |log_post| ~ 1e7; with the bound widened 2^18-fold too"""
    ref = _reference("pois_glm", name, "amwg_step_kernel<PoisGlmModel,1,", full_evaluation=1)
    got, li = _run(_V().case("pois_glm", name)["spec"], "amwg_step_kernel_cert<PoisGlmModel,16,256>", 16, test_bound_shift=shift)
    assert li["summation_order"] == 1, li
    got = _check("pois_glm", name, got, li, ref)
    if name == "negative_count":
        assert (got["log_post0"] == -np.inf).all() and (got["log_post2"] == -np.inf).all()
    if name == "count_1e6":
        assert (np.abs(got["log_post0"]) > 1e7).all()


# ---- hierarchical Normal, n = 640, G = 8
HIER = ["one_out_of_mid_range", "outside_support"]


@pytest.mark.parametrize("name", HIER)
def test_hierarchical_sweep_kernel(name):
    """amwg_sweep_kernel_cert<HierNormalModel,...> at 64 lanes: against one lane with the expression in every update, and the oracle in the reference's order"""
    ref = _reference("hier_normal", name, "amwg_step_kernel<HierNormalModel,1,", full_evaluation=1)
    got, li = _run(_V().case("hier_normal", name)["spec"], "amwg_sweep_kernel_cert<HierNormalModel", 64)
    assert li["summation_order"] == 1, li
    got = _check("hier_normal", name, got, li, ref)
    if name == "outside_support":
        assert (got["log_post0"] == -np.inf).all() and np.isfinite(got["log_post2"]).all()


@pytest.mark.parametrize("name", HIER)
def test_hierarchical_group_local(name):
    """options.group_local: its sums are in its own lane order, so its reference is its restatement in the oracle (gl_*), chains 0 and 99, every bit; and the
    one-lane sampler with the expression in every update in everything that is not a sum: the decisions' counters and the uniforms consumed"""
    V = _V()
    ref = _reference("hier_normal", name, "amwg_step_kernel<HierNormalModel,1,", full_evaluation=1)
    got, li = _run(V.case("hier_normal", name)["spec"], "amwg_gl_kernel", 0, group_local=1)
    assert li["lanes_per_chain"] == 64, li
    got = _check("hier_normal", name, got, li, None, oracle_lanes=64, group_local=True)
    print("group-local against one lane per chain (reported, two summation orders):", V.differences(got, ref))


def _child():
    for p in (ROOT, os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    try:
        import torch  # noqa: F401  (before the library, as tests/conftest.py does)
    except Exception:
        pass
    assert os.environ.get("AMWG_WAVE_SCRATCH") == "0"
    V = _V()
    out = []
    for name in NO_SCRATCH:
        spec = V.case("normal", name)["spec"]
        ref, _ = _run(spec, N_FULL, 1, full_evaluation=1)
        got, li = _run(spec, N_CERT % 256, 1)
        bad = V.differences(got, ref)
        for local in (0, V.CHAINS - 1):
            bad += V.differences_from_oracle(got, V.oracle_record(spec, local), local)
        out.append({"case": name, "differs": bad, "kernel": li["kernel"], "block_threads": li["block_threads"]})
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    _child()
