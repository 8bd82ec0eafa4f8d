"""Datasets of unequal sizes in one sampler (amwg_create_datasets_ragged; csrc/amwg_dataset.h), on the GPU.  The bar is the one of
tests/test_gpu_datasets.py, with the same harness (tests/dataset_harness.py): every bit.

Every dataset's chains against an ordinary sampler on that dataset with the parameters of the FIRST spec (the list constructor passes one params array
for the whole sampler).  The sizes are the smallest at which a per-dataset size can go wrong, one case per row of the table in
tests/README.ragged_datasets.md.  The Poisson family's sizes start at 2: with n = 1 the reference's own prior is log(1 / 0)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import dataset_harness
import gpu_util
import model_spec
import oracle_lib
from dataset_harness import BURN, SAMPLE, SEED, THIN, assert_same_bits, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def against_twins(case, specs, cpd, lanes, block, **kw):
    """through the ragged entry; the twins' runs are kept under the case's name"""
    return dataset_harness.against_twins(specs, cpd, lanes, block, case=case, ragged=True, **kw)


def ragged_specs(model, sizes, tweak=None):
    """one spec per size, data synth with a different data_seed per dataset; every spec carries the parameters, init and stepper options of the first"""
    out = []
    for d, n in enumerate(sizes):
        kw = {"exp": oracle_lib.lib().orc_exp} if model == "pois_glm" else {}
        data = model_spec.make_data(model, n, 900 + 11 * d, **kw)
        data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
        if tweak:
            tweak(d, data)
        spec = model_spec.build_spec(model, data)
        assert spec["n_obs"] == n
        if out:
            spec = dict(spec, params=out[0]["params"], P=out[0]["P"], init=out[0]["init"], comp_opts=out[0]["comp_opts"])
        out.append(spec)
    return out


NORMAL_ONE_LANE = (1, 2, 63, 64, 65, 1023, 1024, 1025, 1100)


NORMAL_ONE_LANE_512 = (1, 513, 1025)


@pytest.mark.parametrize("block,cpd", [(64, 64), (256, 256), (512, 512)])
def test_normal_certified_pass_one_lane(block, cpd):
    """Below a wavefront, either side of one row of 64, either side of one block of 16 rows, block + row + masked tail; an LDS tile of each dataset's own size
    in front of the stepper state; one-wavefront and 256-thread workgroups.  (512, 512): the 512-thread class, blocks of 8 rows -- below a wavefront, a block and a
    single observation, two blocks and one (the byte-parity companion of the class tests/test_gpu_value_audit.py audits per dataset)."""
    if block == 512:
        against_twins("n1_512", ragged_specs("normal", NORMAL_ONE_LANE_512), cpd, 1, block, kernel="amwg_step_kernel_cert_ds<NormalModel,1,512>")
        return
    against_twins("n1", ragged_specs("normal", NORMAL_ONE_LANE), cpd, 1, block, kernel="amwg_step_kernel_cert_ds<NormalModel,1,256>")


@pytest.mark.parametrize("opts", [{"full_evaluation": 1}, {"test_bound_shift": 14}, {"test_bound_shift": 40}, {"sufficient_statistics": 1}],
                         ids=["full_evaluation", "shift14", "shift40", "sufficient_statistics"])
def test_normal_one_lane_options(opts):
    """The expression in every update (the scalar-cache pass over the shifted global pointer), widened bounds (the epsilon of the certified value contains n),
    and the pass-free value n (xbar - mu)^2 + SS -- each against its twins, and all of them equal to the default: none may change a bit."""
    specs = ragged_specs("normal", (1, 65, 1025))
    plain = against_twins("n1o", specs, 64, 1, 64, kernel="amwg_step_kernel_cert_ds<")
    got = against_twins("n1o", specs, 64, 1, 64, kernel="amwg_step_kernel_ds<" if opts.get("full_evaluation") else "amwg_step_kernel_cert_ds<", **opts)
    assert_same_bits(plain, got, str(opts))


def test_normal_sixteen_lanes_with_lanes_without_an_observation():
    against_twins("n16", ragged_specs("normal", (5, 16, 17, 1100)), 4, 16, 64, kernel="amwg_step_kernel_ds<NormalModel,16,256>")


def test_normal_multi_wave_chain_with_fewer_observations_than_lanes():
    against_twins("n128", ragged_specs("normal", (100, 129, 1100)), 2, 128, 128, kernel="amwg_step_kernel_ds<NormalModel,128,256>")


def huge_in_the_smallest(d, data):
    if d == 0:
        data["x"][1] = 1e250      # data_mid_range = 0 for this dataset only


def test_normal_data_mid_range_of_the_smallest_dataset_only():
    against_twins("nhuge", ragged_specs("normal", (3, 65, 300), huge_in_the_smallest), 64, 1, 64, kernel="amwg_step_kernel_cert_ds<")


BERN_ONE_LANE = (1, 31, 32, 33, 64, 100, 2000)


@pytest.mark.parametrize("exact", [0, 1])
def test_beta_bernoulli_one_lane_word_boundaries(exact):
    """The 32-bit word boundary of the bit array and of the six tables, whose sizes are two_valued_words(n_d) per dataset."""
    against_twins("b1", ragged_specs("beta_bern", BERN_ONE_LANE), 256, 1, 256, kernel="amwg_step_kernel_ds<BetaBernModel,1,256>", exact_division=exact)


def test_beta_bernoulli_four_lanes():
    against_twins("b4", ragged_specs("beta_bern", (3, 33, 2000)), 16, 4, 64, kernel="amwg_step_kernel_ds<BetaBernModel,4,256>")


def one_half_in_the_middle(d, data):
    if d == 1:
        data["x"][17] = 0.5      # neither 0 nor 1: has_invalid for this dataset only


def test_beta_bernoulli_invalid_observation_in_one_dataset():
    against_twins("binv", ragged_specs("beta_bern", (3, 33, 100), one_half_in_the_middle), 64, 1, 64, kernel="amwg_step_kernel_ds<BetaBernModel,1,256>")


POIS_SIXTEEN = (2, 15, 16, 17, 47, 300, 301)


def test_poisson_glm_sixteen_lanes_certified():
    """The column stride of the design matrix [7][n_d], the prior ld.unif(cp, 0, n_d - 1) and the bound of the certified value, all per dataset; the shared
    bound of cp is the first dataset's (upper = 1)."""
    against_twins("p16", ragged_specs("pois_glm", POIS_SIXTEEN), 16, 16, 256, kernel="amwg_step_kernel_cert_ds<PoisGlmModel,16,256>")


def test_poisson_glm_sixteen_lanes_largest_first():
    """The same datasets in descending order: the shared bound of cp is then 300, so the change point moves left and right of every observation of the
    smaller datasets and beyond their end, where each dataset's own prior is -inf."""
    specs = ragged_specs("pois_glm", POIS_SIXTEEN[::-1])
    against_twins("p16d", specs, 16, 16, 256, kernel="amwg_step_kernel_cert_ds<PoisGlmModel,16,256>")


def test_poisson_glm_sixty_four_lanes():
    against_twins("p64", ragged_specs("pois_glm", (300, 17)), 4, 64, 256, kernel="amwg_step_kernel_ds<PoisGlmModel,64,256>")


@pytest.mark.parametrize("model,sizes,cpd,lanes,block", [("normal", (1, 65, 1025), 64, 1, 64), ("pois_glm", (301, 2, 17, 47), 16, 16, 256)])
def test_permuting_the_datasets_permutes_the_posteriors(model, sizes, cpd, lanes, block):
    """Dataset d of a permuted sampler equals its twin at the new offset: nothing but the place changes."""
    specs = ragged_specs(model, sizes)
    D = len(sizes)
    order = [(d * 2 + 1) % D for d in range(D)] if D % 2 else list(range(D))[::-1]
    assert sorted(order) == list(range(D)) and order != list(range(D))
    case = "perm-" + model
    against_twins(case, specs, cpd, lanes, block)
    against_twins(case, specs, cpd, lanes, block, order=order)


def test_steps_per_launch_cuts_the_run_without_changing_a_bit():
    specs = ragged_specs("normal", (1, 65, 1025))
    whole = against_twins("n1o", specs, 64, 1, 64)
    cut = amwg_ctypes.Sampler(specs, chains=192, seed=SEED, lanes_per_chain=1, block_threads=64, steps_per_launch=7, ragged=True)
    assert_same_bits(whole, run(cut), "steps_per_launch = 7")
    cut.close()


@pytest.mark.parametrize("model,sizes,d,cpd,lanes,block", [("normal", (1100, 2, 65), 1, 64, 1, 64), ("normal", (1100, 2, 65), 2, 64, 1, 64),
                                                           ("pois_glm", (300, 2, 17), 1, 16, 16, 256), ("pois_glm", (300, 2, 17), 2, 16, 16, 256)])
def test_chains_of_a_small_and_an_odd_sized_dataset_equal_the_oracle(model, sizes, d, cpd, lanes, block):
    """Anchor to the reference, independent of the library's own single-dataset path: chain 3 of dataset d (global id d * cpd + 3) against the CPU oracle in
    the reference's order (both kernels decide from certified values: summation order 1)."""
    specs = ragged_specs(model, sizes)
    ds = amwg_ctypes.Sampler(specs, chains=len(sizes) * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block, ragged=True)
    assert ds.launch_info()["summation_order"] == 1
    local = d * cpd + 3
    orc = oracle_lib.OracleChain(specs[d], SEED, local, lanes=1)
    schedule = [{"op": "burn", "n": BURN}, {"op": "sample", "n": SAMPLE, "thin": THIN}]
    gpu_util.assert_chain_equals_oracle(ds, local, orc, gpu_util.run_schedule(ds, schedule), gpu_util.run_schedule(orc, schedule))
    ds.close()


def test_summaries_per_dataset():
    """dataset_quantiles() == numpy's sort over each dataset's slice of sample() (R's type 7 rule, as tests/test_gpu_dataset_quantiles.py states it);
    dataset_moments()[d] equals the twin sampler's moments() byte for byte (the same kernel over the same values in the same order); dataset_n_obs()
    returns the sizes."""
    sizes = (2, 65, 300)
    specs = ragged_specs("normal", sizes)
    cpd = 64
    ds = amwg_ctypes.Sampler(specs, chains=3 * cpd, seed=SEED, lanes_per_chain=1, block_threads=64, ragged=True)
    assert ds.dataset_n_obs() == list(sizes)
    ds.burn(BURN)
    draws = ds.sample(SAMPLE * 4, THIN)
    mean, sd = ds.dataset_moments()
    probs = [0.025, 0.5, 0.975]
    q = ds.dataset_quantiles(probs)
    assert mean.shape == (3, 2) and q.shape == (3, 2, 3)
    for d in range(3):
        for p in range(2):
            v = np.sort(draws[:, p, d * cpd:(d + 1) * cpd].ravel())
            for j, pr in enumerate(probs):
                h = (v.size - 1) * pr
                lo = int(np.floor(h))
                want = v[lo] + (h - lo) * (v[min(lo + 1, v.size - 1)] - v[lo])
                assert q[d, p, j] == want, (d, p, pr, q[d, p, j], want)
        twin = amwg_ctypes.Sampler(specs[d], chains=cpd, seed=SEED, chain_offset=d * cpd, lanes_per_chain=1, block_threads=64)
        twin.burn(BURN)
        twin.sample(SAMPLE * 4, THIN)
        m, s = twin.moments()
        assert mean[d].tobytes() == m.tobytes() and sd[d].tobytes() == s.tobytes(), (d, mean[d], m, sd[d], s)
        twin.close()
    ds.close()


def test_equal_sizes_through_the_ragged_entry_are_the_dataset_sampler():
    """Equal sizes are the special case of ragged, not a second code path: both entries build the same sampler."""
    specs = ragged_specs("normal", (300, 300, 300))
    a = amwg_ctypes.Sampler(specs, chains=192, seed=SEED, lanes_per_chain=1, block_threads=64, ragged=True)
    b = amwg_ctypes.Sampler(specs, chains=192, seed=SEED, lanes_per_chain=1, block_threads=64)
    assert a.launch_info() == b.launch_info()
    assert_same_bits(run(a), run(b), "equal sizes")
    a.close()
    b.close()


def test_the_planner_fits_the_largest_dataset_and_names_it_when_it_cannot():
    """Left to the planner: one geometry whose workgroups serve whole datasets, with LDS for the largest.  Sixteen lanes stage all of a dataset's
    observations in LDS (8 bytes each): 30 000 of them fit no workgroup, and the refusal names that dataset."""
    specs = ragged_specs("normal", (5, 1100, 64))
    s = amwg_ctypes.Sampler(specs, chains=12, seed=SEED, ragged=True)      # cpd = 4
    li = s.launch_info()
    per_workgroup = 1 if li["lanes_per_chain"] > 64 else li["block_threads"] // li["lanes_per_chain"]
    assert 4 % per_workgroup == 0 and li["grid_blocks"] * per_workgroup == 12, li
    s.burn(10)
    s.close()
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(ragged_specs("normal", (5, 30000, 64)), chains=12, seed=SEED, lanes_per_chain=16, ragged=True)
    assert "amwg error -1" in str(ei.value) and "dataset 1" in str(ei.value) and "n_obs = 30000" in str(ei.value), str(ei.value)


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_ragged_datasets_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_ragged_datasets.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu ragged datasets ok" in p.stdout, p.stdout + "\n" + p.stderr
