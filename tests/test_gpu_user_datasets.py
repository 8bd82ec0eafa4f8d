"""-m gpu: many datasets in one sampler for a TRANSLATED closure (amwg_create_user_datasets; csrc/amwg_user_dataset.h).  The bar is that of the built-in families'
dataset samplers (tests/dataset_harness.py): dataset d's chains equal, bit for bit and over ALL chains, an ordinary amwg_create_user sampler compiled from the same source
on dataset d's arrays with chain_offset = d * cpd at the same lanes_per_chain and block_threads -- existing code, whose chains other tests pin to the reference.  Schedule:
burn 120, sample(40, thin = 3); the draws (derived quantities included), info(), state() and diag() as bytes.  Closures: tests/js/dataset_models.js, D = 3."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import model_spec
import user_datasets_lib as udl
from dataset_harness import SEED, BURN, SAMPLE, THIN, assert_same_bits, run, slice_chains

pytestmark = [pytest.mark.gpu, pytest.mark.node, pytest.mark.skipif(udl.NODE is None, reason="node is not installed")]
ROOT = udl.ROOT
D = udl.D
_twins = {}


def twin_run(tag, d, cpd, offset, lanes, block, opts=()):
    """-> (run(), launch_info()) of the ordinary closure sampler on dataset d at one offset, once per case"""
    k = (tag, d, cpd, offset, lanes, block, tuple(sorted(dict(opts).items())))
    if k not in _twins:
        twin = amwg_ctypes.Sampler(udl.specs(tag)[d], chains=cpd, seed=SEED, chain_offset=offset, lanes_per_chain=lanes, block_threads=block, **dict(opts))
        assert twin.D == 1 and twin.dataset_n_obs() == [0]
        _twins[k] = (run(twin), twin.launch_info())
        twin.close()
    return _twins[k]


def same_launch(li, twin_li):
    """a closure's kernel is its hiprtc symbol: the twin's marker is a suffix"""
    assert li["kernel"].endswith("_ds") and li["kernel"][:-3] == twin_li["kernel"], (li["kernel"], twin_li["kernel"])
    for k in ("lanes_per_chain", "block_threads", "summation_order"):
        assert li[k] == twin_li[k], (k, li, twin_li)
    assert li["datasets"] > 1 and twin_li["datasets"] == 1


def against_twins(tag, cpd, lanes, block, kernel=None, order=None, **opts):
    specs = udl.specs(tag)
    order = list(range(D)) if order is None else list(order)
    ds = amwg_ctypes.Sampler([specs[d] for d in order], chains=D * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block, **opts)
    li = ds.launch_info()
    assert ds.D == D and li["datasets"] == D and ds.dataset_n_obs() == [0] * D
    if kernel:
        assert li["kernel"] == kernel, li
    got = run(ds)
    for j, d in enumerate(order):
        want, twin_li = twin_run(tag, d, cpd, j * cpd, li["lanes_per_chain"], li["block_threads"], opts)
        same_launch(li, twin_li)
        assert_same_bits(slice_chains(got, j * cpd, (j + 1) * cpd), want, "%s: dataset %d at offset %d" % (tag, d, j * cpd))
    ds.close()
    return got, li


@pytest.mark.parametrize("lanes,block,cpd", [(1, 64, 128), (16, 64, 8), (64, 256, 4)])
def test_scaled_normal_equals_its_twins(lanes, block, cpd):
    """(1, 64, 128) and (16, 64, 8): two workgroups per dataset -- a wrong d would show; (16, 64): chains sharing a wavefront"""
    got, li = against_twins("ds_scaled_normal", cpd, lanes, block, kernel="amwg_user_step_ds")
    per_workgroup = block // lanes
    assert li["grid_blocks"] == D * cpd // per_workgroup
    # the datasets differ, so their posteriors do
    mu = got["draws"][:, 0, :].reshape(-1, D, cpd).mean(axis=(0, 2))
    assert len(set(mu.tolist())) == D


def test_the_order_of_the_datasets_is_the_callers():
    against_twins("ds_scaled_normal", 128, 1, 64, order=[2, 0, 1])


def test_readme_normal_decides_from_its_certified_tail():
    """one lane per chain: the certified twin, summation order 1; against the ordinary sampler, against the built-in family's dataset sampler on the same data (the
    translated closure and the hand-written family are the same chains, as tests/test_gpu_user.py holds for one dataset), and against itself with inflated bounds"""
    tag, cpd = "ds_readme_normal", 256
    got, li = against_twins(tag, cpd, 1, 256, kernel="amwg_user_step_cert_ds")
    assert li["summation_order"] == 1
    _, _, sets = udl.load(tag)
    fam = [model_spec.build_spec("normal", {"x": np.asarray(arrays[0], dtype=np.float64)}) for arrays in sets]
    f = amwg_ctypes.Sampler(fam, chains=D * cpd, seed=SEED, lanes_per_chain=1, block_threads=256)
    assert f.launch_info()["kernel"].startswith("amwg_step_kernel_cert_ds")
    assert_same_bits(got, run(f), "translated closure against the built-in family, datasets")
    f.close()
    shifted = amwg_ctypes.Sampler(udl.specs(tag), chains=D * cpd, seed=SEED, lanes_per_chain=1, block_threads=256, test_bound_shift=14)
    assert_same_bits(got, run(shifted), "test_bound_shift = 14")
    shifted.close()


def type7(sorted_values, probs):
    n = sorted_values.size
    out = []
    for q in probs:
        h = (n - 1) * q
        lo = int(np.floor(h))
        hi = min(lo + 1, n - 1)
        out.append(sorted_values[lo] + (h - lo) * (sorted_values[hi] - sorted_values[lo]))
    return np.array(out)


@pytest.mark.parametrize("lanes", [1, 16])
def test_mixed_closure_equals_its_twins_and_is_summarised_per_dataset(lanes):
    """types u8 / i32 / f64 and label ranges that differ per dataset, a scalar that differs, a derived quantity, a log_post of -inf in dataset 2 (a negative count)"""
    tag, cpd, block = "ds_mixed", 64, 64
    got, li = against_twins(tag, cpd, lanes, block, kernel="amwg_user_step_ds")
    assert got["draws"].shape[1] == 5      # theta[3], b, and the derived spread
    lp2 = got["diag"]["log_post"][2 * cpd:]
    assert np.isneginf(lp2).all() and np.isfinite(got["diag"]["log_post"][: 2 * cpd]).all()
    spread = got["draws"][:, 4, :]
    assert spread.tobytes() == (got["draws"][:, 2, :] - got["draws"][:, 0, :]).tobytes()
    ds = amwg_ctypes.Sampler(udl.specs(tag), chains=D * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block)
    ds.burn(BURN)
    draws = ds.sample(SAMPLE * 4, THIN)
    mean, sd = ds.dataset_moments()
    rhat, ess = ds.dataset_convergence()
    probs = [0.025, 0.5, 0.975]
    q = ds.dataset_quantiles(probs)
    assert mean.shape == (D, 5) and rhat.shape == (D, 5) and q.shape == (D, 5, 3)
    for call in (ds.moments, ds.convergence, lambda: ds.quantiles([0.5])):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_last_sample_dataset_moments" in str(ei.value)
    for d in range(D):
        twin = amwg_ctypes.Sampler(udl.specs(tag)[d], chains=cpd, seed=SEED, chain_offset=d * cpd, lanes_per_chain=lanes, block_threads=block)
        twin.burn(BURN)
        twin.sample(SAMPLE * 4, THIN)
        m, s = twin.moments()
        r, e = twin.convergence()
        assert mean[d].tobytes() == m.tobytes() and sd[d].tobytes() == s.tobytes(), (d, mean[d], m, sd[d], s)
        np.testing.assert_allclose(rhat[d], r, rtol=1e-10)
        np.testing.assert_allclose(ess[d], e, rtol=1e-10)
        twin.close()
        for p in range(5):
            want = type7(np.sort(draws[:, p, d * cpd:(d + 1) * cpd].reshape(-1)), probs)
            assert q[d, p].tobytes() == want.tobytes(), (d, p, q[d, p], want)
    ds.close()


def test_more_arrays_than_inline_pointers():
    against_twins("ds_many_arrays", 64, 1, 64, kernel="amwg_user_step_ds")


def test_auto_geometry_constructs_and_equals_twins_at_the_geometry_it_reports():
    got, li = against_twins("ds_scaled_normal", 64, 0, 0)
    per_workgroup = 1 if li["lanes_per_chain"] > 64 else li["block_threads"] // li["lanes_per_chain"]
    assert 64 % per_workgroup == 0 and li["grid_blocks"] * per_workgroup == D * 64, li


def test_a_geometry_that_does_not_serve_whole_datasets_is_refused():
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(udl.specs("ds_scaled_normal"), chains=9, seed=SEED, lanes_per_chain=1, block_threads=64)      # cpd = 3
    assert "amwg error -1" in str(ei.value) and "cpd = 3" in str(ei.value) and "lanes 1" in str(ei.value) and "block 64" in str(ei.value), str(ei.value)


def test_one_lane_equals_each_datasets_own_default_translation():
    """The independent path: dataset d's chains against the ordinary sampler that the DEFAULT translation of datasets[d] alone gives -- its own source, storage types
    and plans.  One lane per chain is the reference's order in both."""
    tag, cpd = "ds_scaled_normal", 128
    ds = amwg_ctypes.Sampler(udl.specs(tag), chains=D * cpd, seed=SEED, lanes_per_chain=1, block_threads=64)
    got = run(ds)
    ds.close()
    for d in range(D):
        own = amwg_ctypes.Sampler(udl.own_spec(tag, d), chains=cpd, seed=SEED, chain_offset=d * cpd, lanes_per_chain=1, block_threads=64)
        assert_same_bits(slice_chains(got, d * cpd, (d + 1) * cpd), run(own), "dataset %d against its own translation" % d)
        own.close()


def test_one_dataset_is_amwg_create_user():
    spec = udl.specs("ds_scaled_normal")[1]
    a = amwg_ctypes.Sampler([spec], chains=64, seed=SEED, lanes_per_chain=1, block_threads=64)
    b = amwg_ctypes.Sampler(spec, chains=64, seed=SEED, lanes_per_chain=1, block_threads=64)
    assert a.D == 1 and a.launch_info() == b.launch_info()
    assert_same_bits(run(a), run(b), "n_datasets = 1")
    a.close()
    b.close()


def test_js_front_end_user_datasets_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_user_datasets.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu user datasets ok" in p.stdout, p.stdout + "\n" + p.stderr
