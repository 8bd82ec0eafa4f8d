"""TEST INFRASTRUCTURE for the certified Poisson / logistic tails of options.datasets with a translated closure: runs tests/js/translate_dataset_tails_cli.js once per session
(the product's translate_datasets over the closures of tests/js/dataset_tail_models.js, D = 3 datasets each) into user_datasets_lib's directory, so that its load(),
load_own(), specs(), own_spec() and HostEval serve these tags too (also `<tag>.notail`: translated with the caller's no_pois_tail / no_logit_tail), and holds what the GPU
tests share: the comparison of a dataset sampler with ordinary samplers on each dataset (the schedule and the bytes of tests/dataset_harness.py)."""
import json
import os
import subprocess

import amwg_ctypes
import user_datasets_lib as udl
from dataset_harness import SEED, assert_same_bits, run, slice_chains

ROOT, NODE, D = udl.ROOT, udl.NODE, udl.D
MARKED = ["dst_logit", "dst_logit_weights", "dst_pois_linear", "dst_pois_small"]      # come out with a certified tail in its per-dataset form
CLI = os.path.join(ROOT, "tests", "js", "translate_dataset_tails_cli.js")
_done = False
_extra = set()
_twins = {}


def workdir():
    global _done
    d = udl.workdir()
    if not _done:
        p = subprocess.run([NODE, CLI, d], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + "\n" + p.stderr
        _done = True
    return d


def use_dir(path):
    """keep the translations in `path` instead of a temporary directory (tools/time_user_dataset_tails.py --workdir: sized variants found there are not translated again)"""
    os.makedirs(path, exist_ok=True)
    udl._dir = path


def translate_sized(name, n_obs, n_datasets=D):
    """a closure of dataset_tail_models.js at another size and number of datasets (tools/time_user_dataset_tails.py); -> its tag"""
    tag = "%s_%d" % (name, n_obs)
    meta = os.path.join(workdir(), tag + ".notail.meta.json")
    if tag not in _extra and os.path.exists(meta) and json.load(open(meta))["n_datasets"] == n_datasets:
        _extra.add(tag)
    if tag not in _extra:
        p = subprocess.run([NODE, CLI, workdir(), "%s:%d:%d" % (name, n_obs, n_datasets)], cwd=ROOT, capture_output=True, text=True, timeout=1200)
        assert p.returncode == 0, p.stdout + "\n" + p.stderr
        _extra.add(tag)
    return tag


def load(tag):
    workdir()
    return udl.load(tag)


def load_own(tag, k):
    workdir()
    return udl.load_own(tag, k)


def specs(tag):
    workdir()
    return udl.specs(tag)


def own_spec(tag, k):
    workdir()
    return udl.own_spec(tag, k)


def forced_source(tag):
    return open(os.path.join(workdir(), tag + ".forced.hip")).read()


def host_eval(tag):
    workdir()
    return udl.HostEval(tag)


def twin_run(tag, d, cpd, offset, lanes, block, opts=()):
    """-> (run(), launch_info(), moments()) of the ordinary closure sampler from the ONE source on dataset d at one offset, once per case"""
    k = (tag, d, cpd, offset, lanes, block, tuple(sorted(dict(opts).items())))
    if k not in _twins:
        twin = amwg_ctypes.Sampler(specs(tag)[d], chains=cpd, seed=SEED, chain_offset=offset, lanes_per_chain=lanes, block_threads=block, **dict(opts))
        assert twin.D == 1
        got = run(twin)
        _twins[k] = (got, twin.launch_info(), twin.moments())
        twin.close()
    return _twins[k]


def against_twins(tag, cpd, lanes, block, kernel=None, order=None, **opts):
    """-> (run(), launch_info(), dataset_moments()) of the dataset sampler, after comparing every dataset's chains with its twin, bit for bit"""
    sp = specs(tag)
    order = list(range(D)) if order is None else list(order)
    ds = amwg_ctypes.Sampler([sp[d] for d in order], chains=D * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block, **opts)
    li = ds.launch_info()
    assert ds.D == D and li["datasets"] == D
    if kernel:
        assert li["kernel"] == kernel, li
    got = run(ds)
    moments = ds.dataset_moments()
    for j, d in enumerate(order):
        want, twin_li, _ = twin_run(tag, d, cpd, j * cpd, li["lanes_per_chain"], li["block_threads"], opts)
        assert li["kernel"].endswith("_ds") and li["kernel"][:-3] == twin_li["kernel"], (li["kernel"], twin_li["kernel"])
        for k in ("lanes_per_chain", "block_threads", "summation_order"):
            assert li[k] == twin_li[k], (k, li, twin_li)
        assert_same_bits(slice_chains(got, j * cpd, (j + 1) * cpd), want, "%s: dataset %d at offset %d" % (tag, d, j * cpd))
    ds.close()
    return got, li, moments
