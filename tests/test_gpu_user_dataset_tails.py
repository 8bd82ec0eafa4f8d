"""-m gpu: the certified Poisson / logistic tails of a translated closure on MANY datasets (amwg_create_user_datasets on a source marked kTailPerDataset:
amwg_user_step_cert_ds at 16 lanes per chain, summation order 1).  The bar is every bit (tests/dataset_harness.py: burn 120, sample(40, thin 3); draws, info, state and
diag as bytes): dataset d's chains against an ordinary amwg_create_user sampler from the same source on dataset d's arrays, against the sampler that dataset d's OWN
default translation gives (literals in its text, its own storage types, the existing amwg_user_step_cert -- both are the reference's chain), and against the expression
in every update.  A wrong sum-of-lfactorial slot moves the certified value by hundreds: every chain would differ.  That each slot is the dataset's own is
tests/test_user_dataset_tails_host.py's to check; the audit here is the evidence beside it.  Closures: tests/js/dataset_tail_models.js, D = 3."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import amwg_ctypes
import user_dataset_tails_lib as tl
import user_datasets_lib as udl
from dataset_harness import SEED, assert_same_bits, run, slice_chains

pytestmark = [pytest.mark.gpu, pytest.mark.node, pytest.mark.skipif(udl.NODE is None, reason="node is not installed")]
ROOT, D = udl.ROOT, udl.D
KERNEL = "amwg_user_step_cert_ds"
OWN_PLAN = ["dst_logit", "dst_logit_weights", "dst_pois_linear"]      # (an ordinary translation has these plans from 64 observations on: not dst_pois_small's 37)


@pytest.mark.parametrize("tag", tl.MARKED)
@pytest.mark.parametrize("lanes,block,cpd", [(16, 64, 8), (16, 256, 16)])
def test_certified_tails_equal_their_twins(tag, lanes, block, cpd):
    """(16, 64, 8): two workgroups per dataset, four chains sharing a wavefront; (16, 256, 16): one workgroup per dataset"""
    got, li, _ = tl.against_twins(tag, cpd, lanes, block, kernel=KERNEL)
    assert li["summation_order"] == 1 and li["grid_blocks"] == D * cpd // (block // lanes)
    lp = got["diag"]["log_post"].reshape(D, cpd)
    assert len({float(v) for v in lp.mean(axis=1)}) == D      # (the datasets differ, so their posteriors do)


@pytest.mark.parametrize("tag", ["dst_logit_weights", "dst_pois_linear"])
def test_the_order_of_the_datasets_is_the_callers(tag):
    tl.against_twins(tag, 8, 16, 64, kernel=KERNEL, order=[2, 0, 1])


def test_constants_as_the_17th_array_travel_in_the_device_table():
    tl.against_twins("dst_logit_many", 8, 16, 64, kernel=KERNEL)


@pytest.mark.parametrize("tag", OWN_PLAN + ["dst_logit_many"])
def test_equal_to_each_datasets_own_default_translation(tag):
    cpd = 8
    ds = amwg_ctypes.Sampler(tl.specs(tag), chains=D * cpd, seed=SEED, lanes_per_chain=16, block_threads=64)
    assert ds.launch_info()["kernel"] == KERNEL
    got = run(ds)
    ds.close()
    for d in range(D):
        own = amwg_ctypes.Sampler(tl.own_spec(tag, d), chains=cpd, seed=SEED, chain_offset=d * cpd, lanes_per_chain=16, block_threads=64)
        assert own.launch_info()["kernel"] == "amwg_user_step_cert" and own.launch_info()["summation_order"] == 1
        assert_same_bits(slice_chains(got, d * cpd, (d + 1) * cpd), run(own), "%s: dataset %d against its own translation" % (tag, d))
        own.close()


@pytest.mark.parametrize("tag", tl.MARKED)
def test_equal_to_the_expression_in_every_update(tag):
    """one lane per chain with full_evaluation (the reference's order, no certified value anywhere), and the bounds inflated 2^12- and 2^30-fold (far more updates go
    to the expression): every byte, the cached log_post included"""
    cpd = 64
    kw = dict(chains=D * cpd, seed=SEED)
    base = amwg_ctypes.Sampler(tl.specs(tag), lanes_per_chain=16, block_threads=64, **kw)
    assert base.launch_info()["kernel"] == KERNEL
    want = run(base)
    base.close()
    for what, opts in (("one lane, full evaluation", dict(lanes_per_chain=1, block_threads=64, full_evaluation=1)),
                       ("test_bound_shift 12", dict(lanes_per_chain=16, block_threads=64, test_bound_shift=12)),
                       ("test_bound_shift 30", dict(lanes_per_chain=16, block_threads=64, test_bound_shift=30))):
        s = amwg_ctypes.Sampler(tl.specs(tag), **opts, **kw)
        assert_same_bits(want, run(s), tag + ": " + what)
        s.close()


@pytest.mark.parametrize("tag", ["dst_logit", "dst_pois_linear"])
def test_auto_geometry_constructs_and_equals_twins_at_the_geometry_it_reports(tag):
    got, li, _ = tl.against_twins(tag, 64, 0, 0)
    print(tag, li)
    per_workgroup = 1 if li["lanes_per_chain"] > 64 else li["block_threads"] // li["lanes_per_chain"]
    assert 64 % per_workgroup == 0 and li["grid_blocks"] * per_workgroup == D * 64, li


def test_a_geometry_that_does_not_serve_whole_datasets_is_refused():
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(tl.specs("dst_logit"), chains=3 * 6, seed=SEED, lanes_per_chain=16, block_threads=128)      # 8 chains per workgroup, cpd = 6
    assert "amwg error -1" in str(ei.value) and "cpd = 6" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("tag", ["dst_logit", "dst_pois_small"])
def test_per_dataset_moments_on_the_certified_sampler(tag):
    cpd = 8
    _, _, (mean, sd) = tl.against_twins(tag, cpd, 16, 64, kernel=KERNEL)
    for d in range(D):
        m, s = tl.twin_run(tag, d, cpd, d * cpd, 16, 64)[2]
        assert mean[d].tobytes() == m.tobytes() and sd[d].tobytes() == s.tobytes(), (d, mean[d], m, sd[d], s)


def test_one_dataset_under_a_marked_source_is_an_ordinary_sampler():
    """amwg_create_user takes the marked source: the constants are its one dataset's array"""
    spec = tl.specs("dst_pois_linear")[1]
    a = amwg_ctypes.Sampler(spec, chains=8, seed=SEED, lanes_per_chain=16, block_threads=64)
    assert a.launch_info()["kernel"] == "amwg_user_step_cert" and a.launch_info()["summation_order"] == 1
    a.close()


def test_js_front_end_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_user_dataset_tails.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu user dataset tails ok" in p.stdout, p.stdout + "\n" + p.stderr


def test_bounds_hold_per_dataset_in_the_audit_build(tmp_path):
    """tools/bound_audit.py --only dstail (the audit build evaluates the expression beside every certified value): every case on a _cert kernel, every dataset audited,
    not one wrong verdict, both ratios at most 0.5 per dataset -- the bar tests/test_gpu_bound_audit.py sets for every bound"""
    out = tmp_path / "audit.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bound_audit.py"), "--only", "dstail", "--out", str(out)], capture_output=True, text=True, timeout=900)
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    rec = json.load(open(out))
    assert {c["name"] for c in rec["cases"]} == {"dstail_" + t for t in tl.MARKED}
    for c in rec["cases"]:
        assert "_cert" in c["kernel"] and c["kernel"].endswith("_ds"), c
        assert c["wrong_verdicts"] == 0 and len(c["datasets"]) == D, c
        for q in c["datasets"]:
            print(c["name"], q)
            assert q["audited_decisions"] > 0 and q["wrong_verdicts"] == 0 and q["max_value_ratio"] <= 0.5 and q["max_difference_ratio"] <= 0.5, (c["name"], q)
