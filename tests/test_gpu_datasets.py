"""Many datasets in one sampler (amwg_create_datasets; csrc/amwg_dataset.h), on the GPU.  The bar is the project's own: every bit.

Every dataset's chains against an ordinary sampler on that dataset, with the harness of tests/dataset_harness.py (which states what is compared and on
which schedule).  Data: synth with a different data_seed per dataset.  The shapes are the smallest at which the new code can still go wrong (one case per
row of the table in the pull request's issue).  Two chains are anchored to the CPU oracle directly, independent of the library's own single-dataset path."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import gpu_util
import model_spec
import oracle_lib
from dataset_harness import BURN, SAMPLE, SEED, THIN, against_twins, assert_same_bits, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dataset_specs(model, n_obs, D, tweak=None):
    out = []
    for d in range(D):
        kw = {"exp": oracle_lib.lib().orc_exp} if model == "pois_glm" else {}
        data = model_spec.make_data(model, n_obs, 500 + 7 * d, **kw)
        data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
        if tweak:
            tweak(d, data)
        out.append(model_spec.build_spec(model, data))
    return out


@pytest.mark.parametrize("block,cpd", [(256, 256), (64, 64)])
def test_normal_certified_pass_one_lane(block, cpd):
    """N = 1100: one block of 16 rows (1024 observations), one single row, a masked tail of 12; the LDS tile per workgroup; the wave scratch lines of
    12 (3) wavefronts.  256-thread workgroups, and one-wavefront workgroups."""
    against_twins(dataset_specs("normal", 1100, 3), cpd, 1, block, kernel="amwg_step_kernel_cert_ds<NormalModel,1,256>")


def test_steps_per_launch_cuts_the_run_without_changing_a_bit():
    specs = dataset_specs("normal", 1100, 3)
    whole = against_twins(specs, 64, 1, 64)
    cut = against_twins(specs, 64, 1, 64, steps_per_launch=7)
    assert_same_bits(whole, cut, "steps_per_launch = 7")


def huge_in_the_middle(d, data):
    if d == 1:
        data["x"][5] = 1e250      # data_mid_range = 0 for this dataset only


@pytest.mark.parametrize("full", [0, 1])
def test_normal_per_dataset_constants_differ(full):
    """The middle dataset's data_mid_range is 0, its neighbours' 1.  full_evaluation = 1: the scalar-cache pass over the global array, i.e. the shifted pointer."""
    specs = dataset_specs("normal", 300, 3, huge_in_the_middle)
    against_twins(specs, 64, 1, 64, kernel="amwg_step_kernel_ds<" if full else "amwg_step_kernel_cert_ds<", full_evaluation=full)


def test_normal_test_bound_shift_changes_nothing():
    specs = dataset_specs("normal", 1100, 3)
    plain = against_twins(specs, 64, 1, 64)
    ds = amwg_ctypes.Sampler(specs, chains=192, seed=SEED, lanes_per_chain=1, block_threads=64, test_bound_shift=14)
    assert_same_bits(plain, run(ds), "test_bound_shift = 14")
    ds.close()


def test_normal_sufficient_statistics_per_dataset():
    against_twins(dataset_specs("normal", 1100, 3), 64, 1, 64, kernel="amwg_step_kernel_cert_ds<", sufficient_statistics=1)


def test_normal_sixteen_lanes_four_chains_per_dataset():
    """The plain lane-order kernel: the four chains of a wavefront belong to the same dataset, five workgroups."""
    got = against_twins(dataset_specs("normal", 1100, 5), 4, 16, 64, kernel="amwg_step_kernel_ds<NormalModel,16,256>")
    assert got["draws"].shape[2] == 20


def test_normal_multi_wave_chain():
    against_twins(dataset_specs("normal", 1100, 3), 2, 128, 128, kernel="amwg_step_kernel_ds<NormalModel,128,256>")


def one_half(d, data):
    if d == 1:
        data["x"][17] = 0.5      # neither 0 nor 1: has_invalid for this dataset only


@pytest.mark.parametrize("exact", [0, 1])
def test_beta_bernoulli_tables_and_has_invalid_per_dataset(exact):
    against_twins(dataset_specs("beta_bern", 2000, 3, one_half), 256, 1, 256, kernel="amwg_step_kernel_ds<BetaBernModel,1,256>", exact_division=exact)


def negative_count(d, data):
    if d == 2:
        data["y"][11] = -1.0      # lfact = +inf: this dataset's data always takes the expression


@pytest.mark.parametrize("lanes,kernel", [(16, "amwg_step_kernel_cert_ds<PoisGlmModel,16,256>"), (64, "amwg_step_kernel_ds<PoisGlmModel,64,256>")])
def test_poisson_glm_constants_per_dataset(lanes, kernel):
    against_twins(dataset_specs("pois_glm", 300, 3, negative_count), 16, lanes, 256, kernel=kernel)


def test_planner_searches_only_geometries_that_serve_whole_datasets():
    specs = dataset_specs("normal", 1100, 3)
    s = amwg_ctypes.Sampler(specs, chains=12, seed=SEED)      # cpd = 4, lanes and block left to the planner
    li = s.launch_info()
    per_workgroup = 1 if li["lanes_per_chain"] > 64 else li["block_threads"] // li["lanes_per_chain"]
    assert 4 % per_workgroup == 0 and li["grid_blocks"] * per_workgroup == 12, li
    s.burn(10)
    s.close()
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(specs, chains=300, seed=SEED, lanes_per_chain=1, block_threads=256)      # cpd = 100
    assert "amwg error -1" in str(ei.value) and "cpd = 100" in str(ei.value) and "lanes 1" in str(ei.value) and "block 256" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("model,n_obs,cpd,lanes,block", [("normal", 1100, 64, 1, 64), ("pois_glm", 300, 16, 16, 256)])
def test_one_chain_of_dataset_one_equals_the_oracle(model, n_obs, cpd, lanes, block):
    """Anchor to the reference, independent of the library's own single-dataset path: chain 3 of dataset 1 (global id cpd + 3) against the CPU oracle in the
    reference's order (both kernels decide from certified values: summation order 1)."""
    tweak = negative_count if model == "pois_glm" else None
    specs = dataset_specs(model, n_obs, 3, tweak)
    ds = amwg_ctypes.Sampler(specs, chains=3 * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block)
    assert ds.launch_info()["summation_order"] == 1
    local = cpd + 3
    orc = oracle_lib.OracleChain(specs[1], SEED, local, lanes=1)
    schedule = [{"op": "burn", "n": BURN}, {"op": "sample", "n": SAMPLE, "thin": THIN}]
    gpu_util.assert_chain_equals_oracle(ds, local, orc, gpu_util.run_schedule(ds, schedule), gpu_util.run_schedule(orc, schedule))
    ds.close()


def test_summaries_per_dataset():
    """dataset_moments()[d] equals the twin sampler's moments() byte for byte: the same kernel over the same values in the same order.
    dataset_convergence()[d] against the twin's convergence(): two summation orders (the pooled call reduces on the host), the tolerances of
    tests/test_gpu_moments.py.  The pooled calls are refused."""
    specs = dataset_specs("normal", 300, 3)
    cpd = 64
    ds = amwg_ctypes.Sampler(specs, chains=3 * cpd, seed=SEED, lanes_per_chain=1, block_threads=64)
    ds.burn(BURN)
    ds.sample(SAMPLE * 4, THIN)
    mean, sd = ds.dataset_moments()
    rhat, ess = ds.dataset_convergence()
    assert mean.shape == (3, 2) and rhat.shape == (3, 2)
    for call in (ds.moments, ds.convergence, lambda: ds.quantiles([0.5])):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_last_sample_dataset_moments" in str(ei.value)
    for d in range(3):
        twin = amwg_ctypes.Sampler(specs[d], chains=cpd, seed=SEED, chain_offset=d * cpd, lanes_per_chain=1, block_threads=64)
        twin.burn(BURN)
        twin.sample(SAMPLE * 4, THIN)
        m, s = twin.moments()
        r, e = twin.convergence()
        assert mean[d].tobytes() == m.tobytes() and sd[d].tobytes() == s.tobytes(), (d, mean[d], m, sd[d], s)
        np.testing.assert_allclose(rhat[d], r, rtol=1e-10)
        np.testing.assert_allclose(ess[d], e, rtol=1e-10)
        twin.close()
    ds.close()


def test_one_dataset_is_amwg_create():
    specs = dataset_specs("normal", 1100, 1)
    a = amwg_ctypes.Sampler(specs, chains=64, seed=SEED, lanes_per_chain=1, block_threads=64)
    b = amwg_ctypes.Sampler(specs[0], chains=64, seed=SEED, lanes_per_chain=1, block_threads=64)
    assert a.D == 1 and a.launch_info() == b.launch_info()
    assert_same_bits(run(a), run(b), "n_datasets = 1")
    a.moments()      # (an ordinary sampler: the pooled summaries work)
    a.close()
    b.close()


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_datasets_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_datasets.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu datasets ok" in p.stdout, p.stdout + "\n" + p.stderr
