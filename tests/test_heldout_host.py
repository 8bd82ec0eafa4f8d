"""Held-out predictive density (amwg_last_sample_dataset_heldout; amwg_heldout_check in the test library), the part that needs no GPU: the calls are declared, mirrored
and exported; what they refuse for their arguments alone is refused BEFORE a device is opened -- on a device number that does not exist -- with the call's name;
heldout_splits restated; kfold_total under node.  tests/README.heldout.md says what each test pins."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
from test_waic_host import NO_DEVICE, ROOT, declared

CALL, CHECK = "amwg_last_sample_dataset_heldout", "amwg_heldout_check"


def test_calls_are_declared_mirrored_and_exported():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS and getattr(amwg_ctypes.lib(), CALL) is not None
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and not hasattr(amwg_ctypes.lib(), CHECK)
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    assert "amwg_heldout.hip" not in build_id.KERNEL_FILES and "amwg_heldout.h" not in build_id.KERNEL_FILES      # not a source of the step kernels
    L = amwg_ctypes.lib()      # null arguments are refused before any device call
    fake, summary, held = C.c_void_p(8), (C.c_double * 2)(), (amwg_ctypes.ModelDesc * 1)()      # (fake is never dereferenced: refused for another argument first)
    for args in ((None, held, None, summary, None), (fake, None, None, summary, None), (fake, held, None, None, None)):
        assert L.amwg_last_sample_dataset_heldout(*args) == -1, args
        assert CALL.encode() in L.amwg_last_error(), L.amwg_last_error()


X3 = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}
H3 = {"model": "hier_normal", "n_obs": 3, "G": 2, "data": {"x": np.zeros(3), "g": np.array([0, 1, 1], dtype=np.int32)}}
P3 = {"model": "pois_glm", "n_obs": 3, "K": 7, "data": {"x": np.zeros(21), "y": np.zeros(3)}}


@pytest.mark.parametrize("draws,specs,held,index,words", [
    (np.zeros((1, 2, 1)), [X3], [X3], None, "fewer than 2 draws"),
    (np.zeros((2, 1, 2)), [X3], [X3], None, "reads 2 components"),
    (np.zeros((2, 2, 2)), [X3], [dict(X3, model="beta_bern")], None, "is of model"),
    (np.zeros((2, 2, 2)), [X3], [dict(X3, n_obs=-1)], None, "n_obs < 0"),
    (np.zeros((2, 9, 2)), [P3], [dict(P3, K=6)], None, "K = 6"),
    (np.zeros((2, 9, 2)), [P3], [P3], [np.array([0, -1, 2])], "index[1] = -1"),
    (np.zeros((2, 4, 2)), [H3], [dict(H3, G=3)], None, "G = 3"),
    (np.zeros((2, 4, 2)), [H3], [dict(H3, data={"x": np.zeros(3), "g": np.array([0, 2, 1], dtype=np.int32)})], None, "outside 0..1"),
    (np.zeros((2, 4, 2)), [H3, H3], [H3, H3], None, "one dataset"),
])
def test_heldout_check_refuses_before_a_device_is_opened(draws, specs, held, index, words):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.heldout_check(draws, specs, held, index=index, device=NO_DEVICE)
    assert CHECK in str(ei.value) and words in str(ei.value), str(ei.value)      # (a call that reached the device would fail without the call's name)


def test_heldout_splits_restated():      # 2048 workgroups per dataset over the tiles of 64, a run of at least 256 draws
    lib = amwg_ctypes.selftest_lib()
    for S in (2, 255, 256, 511, 512, 4096, 256000, 1 << 22):
        for m in (0, 1, 64, 65, 130, 64 * 2048, 64 * 2048 + 1):
            tiles = (m + 63) // 64
            want = min(max(2048 // tiles if tiles else 1, 1), max(S // 256, 1))
            assert lib.amwg_heldout_splits_check(S, m) == want, (S, m)
    assert lib.amwg_heldout_splits_check(256000, 1) == 1000


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_kfold_total_under_node():
    script = r"""
const mcmc = require('./bayes.js_amd/mcmc.js');
const a = { pointwise: [-1.0, -2.5] }, b = { pointwise: [] }, c = { pointwise: [-0.5, -1.5, -3.25] };
const out = { abc: mcmc.kfold_total([a, b, c]), one: mcmc.kfold_total([{ pointwise: [-2] }]), none: mcmc.kfold_total([b]), throws: [] };
for (const bad of [[a, {}], null, [null]]) { try { mcmc.kfold_total(bad); out.throws.push(false); } catch (e) { out.throws.push(String(e)); } }
console.log(JSON.stringify(out, (k, v) => (typeof v === 'number' && isNaN(v) ? 'NaN' : v)));
"""
    p = subprocess.run([shutil.which("node"), "-e", script], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    out = json.loads(p.stdout)
    v = [-1.0, -2.5, -0.5, -1.5, -3.25]
    total = ss = 0.0
    for q in v:
        total += q
    for q in v:
        ss += (q - total / 5) * (q - total / 5)
    assert out["abc"] == {"elpd_kfold": total, "se": math.sqrt(5 * ss / 4), "n": 5}
    assert out["one"] == {"elpd_kfold": -2, "se": "NaN", "n": 1} and out["none"] == {"elpd_kfold": 0, "se": "NaN", "n": 0}
    assert all(isinstance(t, str) and "kfold_total" in t and "pointwise" in t for t in out["throws"])
