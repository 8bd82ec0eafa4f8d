"""What the GPU tests of the dataset samplers share (tests/test_gpu_datasets.py: equal sizes; tests/test_gpu_ragged_datasets.py: unequal sizes).  The bar
is the project's own: every bit.

A sampler over D datasets is compared with D ordinary samplers (amwg_create), one per dataset, with chain_offset = d * cpd, the same seed and the same
lanes_per_chain and block_threads, over ALL chains: the draws as bytes, every array of info(), state(), and diag()'s uniforms, named_order and log_post.
Schedule: burn 120 (adaptation crosses two batches), then sample(40, thin=3).  launch_info() of the two sides must agree -- the kernel's name modulo the
twin's marker "_ds", lanes, block and summation order.  The spec builders stay with the files: their data seeds differ."""
import numpy as np

import amwg_ctypes

SEED = 20261018
BURN, SAMPLE, THIN = 120, 40, 3


def run(s):
    s.burn(BURN)
    draws = s.sample(SAMPLE, THIN)
    return {"draws": draws, "info": s.info(), "state": s.state(), "diag": s.diag()}


def assert_same_bits(a, b, what):
    assert a["draws"].tobytes() == b["draws"].tobytes(), what + ": draws"
    for k in a["info"]:
        assert a["info"][k].tobytes() == b["info"][k].tobytes(), what + ": info " + k
    assert a["state"].tobytes() == b["state"].tobytes(), what + ": state"
    for k in ("uniforms", "named_order", "log_post"):
        assert a["diag"][k].tobytes() == b["diag"][k].tobytes(), what + ": diag " + k


def slice_chains(r, c0, c1):
    return {"draws": np.ascontiguousarray(r["draws"][:, :, c0:c1]), "info": {k: np.ascontiguousarray(v[:, c0:c1]) for k, v in r["info"].items()},
            "state": np.ascontiguousarray(r["state"][:, c0:c1]), "diag": {k: np.ascontiguousarray(v[c0:c1]) for k, v in r["diag"].items()}}


def same_launch(li, twin_li):
    """launch_info() of a dataset sampler against that of the ordinary sampler on one of its datasets"""
    assert "_ds<" in li["kernel"] and li["kernel"].replace("_ds<", "<") == twin_li["kernel"], (li["kernel"], twin_li["kernel"])
    for k in ("lanes_per_chain", "block_threads", "summation_order"):
        assert li[k] == twin_li[k], (k, li, twin_li)
    assert li["datasets"] > 1 and twin_li["datasets"] == 1


_twin_runs = {}


def twin_run(case, spec, cpd, offset, lanes, block, opts):
    """-> (run(), launch_info()) of the ordinary sampler on one dataset at one offset.  With a `case` (a name for the spec: the caller vouches that the same
    name means the same data) it is run once per (case, offset, geometry, options) and shared by the tests that compare against it."""
    k = None if case is None else (case, cpd, offset, lanes, block, tuple(sorted(opts.items())))
    if k in _twin_runs:
        return _twin_runs[k]
    twin = amwg_ctypes.Sampler(spec, chains=cpd, seed=SEED, chain_offset=offset, lanes_per_chain=lanes, block_threads=block, **opts)
    assert twin.dataset_n_obs() == [spec["n_obs"]]
    got = (run(twin), twin.launch_info())
    twin.close()
    if k is not None:
        _twin_runs[k] = got
    return got


def against_twins(specs, cpd, lanes, block, kernel=None, case=None, order=None, ragged=False, **opts):
    """-> the dataset sampler's results, after comparing every dataset's chains with an ordinary sampler on that dataset.
    order: the datasets as the sampler gets them (a permutation of range(D)); dataset order[j] then sits at offset j * cpd, and so does its twin.
    ragged: through amwg_create_datasets_ragged.  case: the name under which the twins' runs are kept for later tests (twin_run)."""
    D = len(specs)
    order = list(range(D)) if order is None else list(order)
    extra = {"ragged": True} if ragged else {}
    ds = amwg_ctypes.Sampler([specs[d] for d in order], chains=D * cpd, seed=SEED, lanes_per_chain=lanes, block_threads=block, **extra, **opts)
    li = ds.launch_info()
    assert ds.D == D and li["datasets"] == D
    assert ds.dataset_n_obs() == [specs[d]["n_obs"] for d in order]
    if kernel:
        assert li["kernel"].startswith(kernel), li
    got = run(ds)
    for j, d in enumerate(order):
        want, twin_li = twin_run(None if case is None else (case, d), specs[d], cpd, j * cpd, lanes, block, opts)
        same_launch(li, twin_li)
        assert_same_bits(slice_chains(got, j * cpd, (j + 1) * cpd), want, "dataset %d (n_obs = %d) at offset %d" % (d, specs[d]["n_obs"], j * cpd))
    ds.close()
    return got
