"""Datasets of unequal sizes in one sampler (amwg_create_datasets_ragged), the part that needs no GPU: the two new names of the C ABI are mirrored in
the ctypes binding, the new entry refuses BEFORE a device is opened everything amwg_create_datasets refuses except unequal sizes (so these run on a machine
without a device, with the reason in amwg_last_error()), the old entry keeps its refusal of unequal sizes, and the JavaScript front end routes unequal
sizes to the new entry by itself."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import amwg_ctypes
import model_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed")
RAGGED = (40, 41, 7)


def specs(model="normal", n_obs=RAGGED, hyper=None, **kw):
    return [model_spec.build_spec(model, model_spec.make_data(model, n, 100 + d, **kw), hyper=(hyper[d] if hyper else None)) for d, n in enumerate(n_obs)]


def refused(spec_list, why, chains=12, ragged=True, **opts):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(spec_list, chains=chains, seed=1, ragged=ragged, **opts)
    msg = str(ei.value)
    assert "amwg error -1" in msg, msg      # AMWG_EINVAL: not AMWG_EHIP, i.e. before a device was needed
    assert re.search(why, msg), msg


def test_the_header_and_the_ctypes_exports_hold_the_two_new_names():
    hdr = open(os.path.join(ROOT, "include", "amwg.h")).read()
    declared = set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(amwg_ctypes.EXPORTS)
    L = amwg_ctypes.lib()
    for name in ("amwg_create_datasets_ragged", "amwg_dataset_n_obs"):
        assert name in declared and name in amwg_ctypes.EXPORTS and getattr(L, name) is not None


def test_dataset_n_obs_of_no_sampler_is_an_error_like_the_other_accessors_with_an_out_argument():
    L = amwg_ctypes.lib()
    out = (C.c_int32 * 1)(-5)
    assert L.amwg_dataset_n_obs(None, out) == -1 and b"amwg_dataset_n_obs" in L.amwg_last_error()
    assert out[0] == -5
    assert L.amwg_launch_info(None, None, None, None, None, None, None) == -1      # (the accessor it behaves like)


def test_no_datasets_is_refused():
    L = amwg_ctypes.lib()
    md, pa, oa, op, h = amwg_ctypes.ModelDesc(), (amwg_ctypes.ParamDesc * 2)(), (amwg_ctypes.CompOpt * 2)(), amwg_ctypes.Options(), C.c_void_p()
    init = (C.c_double * 2)(0.5, 0.5)
    op.chains = 12
    for n in (0, -3):
        assert L.amwg_create_datasets_ragged(C.byref(md), n, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1
        assert b"amwg_create_datasets_ragged: n_datasets must be >= 1" in L.amwg_last_error()
    assert L.amwg_create_datasets_ragged(None, 3, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1
    assert b"amwg_create_datasets_ragged: null argument" in L.amwg_last_error()


def test_chains_must_be_a_multiple_of_the_datasets():
    refused(specs(), r"amwg_create_datasets_ragged: chains \(13, the total\) must be a multiple of n_datasets \(3\)", chains=13)


def test_mismatched_model_is_refused():
    mixed = specs()
    mixed[2] = dict(specs("beta_bern")[2], params=mixed[0]["params"])
    refused(mixed, r"dataset 2 is of model 2, dataset 0 of model 1")


def test_mismatched_K_is_refused():
    mixed = specs()
    mixed[1] = dict(mixed[1], K=7)
    refused(mixed, r"dataset 1 has K = 7, G = 0, dataset 0 has K = 0, G = 0")


def test_mismatched_hyper_is_refused():
    refused(specs(hyper=[[0, 100, 0, 100], [0, 100, 0, 100], [0, 100, 0, 50]]), r"dataset 2 has hyper\[3\] = 50, dataset 0 has 100")


def test_hierarchical_family_is_refused():
    refused(specs("hier_normal", n_obs=(64, 128), G=4), r"the hierarchical family is not supported", chains=8)


def test_group_local_is_refused():
    refused(specs(), r"group_local is an evaluation of the hierarchical family", group_local=1)


def test_autotune_is_refused():
    refused(specs(), r"AMWG_LANES_AUTOTUNE is not supported", lanes_per_chain=-2)


def test_each_dataset_passes_the_check_of_its_family():
    """check_family_args runs per dataset: a null x in the LAST dataset only."""
    L = amwg_ctypes.lib()
    import numpy as np
    x = np.arange(8, dtype=np.float64)
    mds = (amwg_ctypes.ModelDesc * 2)()
    for k, n in enumerate((8, 5)):
        mds[k].model, mds[k].n_obs = 1, n
        for i, v in enumerate((0.0, 100.0, 0.0, 100.0)):
            mds[k].hyper[i] = v
    mds[0].x = x.ctypes.data_as(C.POINTER(C.c_double))
    pa, oa, op, h = (amwg_ctypes.ParamDesc * 2)(), (amwg_ctypes.CompOpt * 2)(), amwg_ctypes.Options(), C.c_void_p()
    for p in pa:
        p.type, p.len, p.top, p.multidim, p.lower, p.upper = 0, 1, 1, 0, -float("inf"), float("inf")
    init = (C.c_double * 2)(0.5, 0.5)
    op.chains = 8
    assert L.amwg_create_datasets_ragged(mds, 2, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1
    assert b"normal model: x is null" in L.amwg_last_error()
    mds[1].n_obs = -1
    assert L.amwg_create_datasets_ragged(mds, 2, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1
    assert b"n_obs < 0" in L.amwg_last_error()


def test_the_old_entry_still_refuses_unequal_sizes_and_points_to_the_new_one():
    refused(specs(n_obs=(40, 41, 40)), r"amwg_create_datasets: dataset 1 has n_obs = 41, dataset 0 has 40 \(ragged datasets are not supported\).*amwg_create_datasets_ragged", ragged=False)


def test_unequal_sizes_pass_every_check_of_the_new_entry():
    """What is left to fail without a device is the device: AMWG_EHIP (-2), after all the checks.  (With a device this constructs a sampler.)"""
    try:
        s = amwg_ctypes.Sampler(specs(), chains=12, seed=1, ragged=True)
    except amwg_ctypes.AmwgError as e:
        assert "amwg error -2" in str(e) and "no HIP device" in str(e), str(e)
    else:
        assert s.dataset_n_obs() == list(RAGGED)
        s.close()


JS_CASES = r"""
const mcmc = require('./bayes.js_amd/mcmc.js');
const ld = require('./bayes.js_amd/ld.js');
const params = { mu: { type: 'real' }, sigma: { type: 'real', lower: 0 } };
const log_post = function (state, data) {
  var lp = 0;
  lp += ld.norm(state.mu, 0, 100);
  lp += ld.unif(state.sigma, 0, 100);
  for (var i = 0; i < data.length; i++) lp += ld.norm(data[i], state.mu, state.sigma);
  return lp;
};
function thrown(f) { try { f(); } catch (e) { return String(e && e.message ? e.message : e); } return null; }
let s = null;
const m = thrown(() => { s = new mcmc.AmwgSampler(params, log_post, null, { datasets: [[1, 2, 3, 4], [2, 3, 4, 5, 6]], chains: 8, seed: 1 }); });
if (m !== null && (/ragged/.test(m) || /n_obs/.test(m))) { console.log('FAIL unequal sizes still stop at the size check: ' + m); process.exit(1); }
if (m !== null && !/no HIP device/.test(m)) { console.log('FAIL unequal sizes stop at something other than the device: ' + m); process.exit(1); }
if (m === null && String(s.dataset_n_obs) !== '4,5') { console.log('FAIL dataset_n_obs: ' + s.dataset_n_obs); process.exit(1); }
console.log('ragged frontend ok' + (m === null ? ' (sampler constructed)' : ' (stopped at: ' + m + ')'));
"""


@needs_node
@pytest.mark.node
def test_js_front_end_routes_unequal_sizes_to_the_ragged_entry(tmp_path):
    script = tmp_path / "ragged_cases.js"
    script.write_text(JS_CASES.replace("./bayes.js_amd/", os.path.join(ROOT, "bayes.js_amd") + "/"))
    p = subprocess.run([NODE, str(script)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ragged frontend ok" in p.stdout, p.stdout + "\n" + p.stderr
