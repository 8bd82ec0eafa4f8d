"""Many datasets in one sampler (amwg_create_datasets), the part that needs no GPU: the C ABI stays mirrored in the ctypes binding, every
call the library refuses is refused BEFORE a device is opened (so these run on a machine without one) with the reason in amwg_last_error(),
and the JavaScript front end refuses what it cannot serve (options.datasets beside a data argument; a closure that is no built-in family)."""
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


def specs(model="normal", n_obs=(40, 40, 40), hyper=None, **kw):
    return [model_spec.build_spec(model, model_spec.make_data(model, n, 100 + d, **kw), hyper=(hyper[d] if hyper else None)) for d, n in enumerate(n_obs)]


def refused(spec_list, why, chains=12, **opts):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(spec_list, chains=chains, seed=1, **opts)
    msg = str(ei.value)
    assert "amwg error -1" in msg, msg      # AMWG_EINVAL: not AMWG_EHIP, i.e. before a device was needed
    assert re.search(why, msg), msg


def test_header_declarations_equal_the_ctypes_exports():
    hdr = open(os.path.join(ROOT, "include", "amwg.h")).read()
    declared = set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(amwg_ctypes.EXPORTS)
    L = amwg_ctypes.lib()
    for name in ("amwg_create_datasets", "amwg_num_datasets", "amwg_last_sample_dataset_moments", "amwg_last_sample_dataset_diagnostics"):
        assert name in declared and getattr(L, name) is not None
    assert L.amwg_num_datasets(None) == 0


def test_no_datasets_is_refused():
    import ctypes as C
    L = amwg_ctypes.lib()
    md, pa, oa, op, h = amwg_ctypes.ModelDesc(), (amwg_ctypes.ParamDesc * 2)(), (amwg_ctypes.CompOpt * 2)(), amwg_ctypes.Options(), C.c_void_p()
    init = (C.c_double * 2)(0.5, 0.5)
    op.chains = 12
    for n in (0, -3):
        assert L.amwg_create_datasets(C.byref(md), n, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1
        assert b"n_datasets must be >= 1" in L.amwg_last_error()
    with pytest.raises(amwg_ctypes.AmwgError):
        amwg_ctypes.Sampler([], chains=12, seed=1)


def test_chains_must_be_a_multiple_of_the_datasets():
    refused(specs(), r"chains \(13, the total\) must be a multiple of n_datasets \(3\)", chains=13)


def test_mismatched_n_obs_is_refused():
    refused(specs(n_obs=(40, 41, 40)), r"dataset 1 has n_obs = 41, dataset 0 has 40 \(ragged datasets are not supported\)")


def test_mismatched_model_is_refused():
    mixed = specs()
    mixed[2] = dict(specs("beta_bern")[2], params=mixed[0]["params"])
    refused(mixed, r"dataset 2 is of model 2, dataset 0 of model 1")


def test_mismatched_hyper_is_refused():
    refused(specs(hyper=[[0, 100, 0, 100], [0, 100, 0, 100], [0, 100, 0, 50]]), r"dataset 2 has hyper\[3\] = 50, dataset 0 has 100")


def test_hierarchical_family_is_refused():
    refused(specs("hier_normal", n_obs=(64, 64), G=4), r"the hierarchical family is not supported", chains=8)


def test_group_local_is_refused():
    refused(specs(), r"group_local is an evaluation of the hierarchical family", group_local=1)


def test_autotune_is_refused():
    refused(specs(), r"AMWG_LANES_AUTOTUNE is not supported", lanes_per_chain=-2)


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
const datasets = [[1, 2, 3, 4], [2, 3, 4, 5]];
function thrown(f) { try { f(); } catch (e) { return String(e && e.message ? e.message : e); } return null; }
let m = thrown(() => new mcmc.AmwgSampler(params, log_post, [1, 2, 3], { datasets: datasets, chains: 8 }));
if (!m || !/options\.datasets/.test(m) || !/data/.test(m)) { console.log('FAIL data beside datasets: ' + m); process.exit(1); }
const odd = function (state, data) { var lp = ld.norm(state.mu, 0, 100) + ld.unif(state.sigma, 0, 100); for (var i = 0; i < data.length; i++) lp += ld.norm(data[i] * 2, state.mu, state.sigma); return lp; };
m = thrown(() => new mcmc.AmwgSampler(params, odd, null, { datasets: datasets, chains: 8 }));
if (!m || !/options\.datasets/.test(m) || !/built-in/.test(m)) { console.log('FAIL translated closure with datasets: ' + m); process.exit(1); }
console.log('datasets frontend ok');
"""


@needs_node
@pytest.mark.node
def test_js_front_end_refuses_data_beside_datasets_and_translated_closures(tmp_path):
    script = tmp_path / "datasets_cases.js"
    script.write_text(JS_CASES.replace("./bayes.js_amd/", os.path.join(ROOT, "bayes.js_amd") + "/"))
    p = subprocess.run([NODE, str(script)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "datasets frontend ok" in p.stdout, p.stdout + "\n" + p.stderr
