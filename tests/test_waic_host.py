"""WAIC per dataset (amwg_last_sample_dataset_waic), the part that needs no GPU: the call is declared in the header with its rule, mirrored in the ctypes binding and
exported by the product library; the entry point that drives the kernels on a caller's draws and data (amwg_waic_check) is in the test library only; what either
refuses for its arguments alone is refused BEFORE a device is opened -- on a device number that does not exist -- with the call's name in amwg_last_error(); the
reference against closed forms and the host twins; waic_totals, the finish restated; compare_waic under node.  tests/README.waic.md says what each test pins."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import waic_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "amwg_last_sample_dataset_waic"
CHECK = "amwg_waic_check"
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP (-2), not AMWG_EINVAL (-1)


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_call_is_declared_mirrored_and_exported():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.lib(), CALL) is not None
    for method in ("dataset_waic", "waic"):
        assert callable(getattr(amwg_ctypes.Sampler, method))
    assert callable(amwg_ctypes.waic_totals)
    header = " ".join(re.sub(r"(?m)^ \* ", " ", open(os.path.join(ROOT, "include", "amwg.h")).read()).split())      # (the comment's leading stars and line breaks removed)
    for words in ("lppd_i = m_i + log(sum_s exp(l_si - m_i)) - log S, with m_i = max_s l_si", "p_i = sum_s (l_si - mean_i)^2 / (S - 1)", "ld_norm(x_i, mu, sigma)",
                  "ld_bern(x_i, theta)", "ld_norm(y_i, theta[g_i], sigma)", "+ beta[7] from i >= cp on", "Priors are not part of l", "ACCUMULATIONS ARE NOT FIXED TO THE BIT",
                  "no floating-point atomics", "The exponential is exp_v8", "E = 8 (S + 16) u", "|lppd_i - exact| <= E + 4 u |exact|",
                  "E sqrt(V (V + mean_i^2)) + (E max_s |l_si|)^2", "lppd_i and p_i are NaN for that (d, i) only", "elpd_i = lppd_i - p_i", "NaN for n_d = 1",
                  "high[d] counts p_i > 0.4", "the pointwise terms of a closure are not known to the library; built-in families only", "256 MiB", "OUT OF SCOPE", "PSIS-LOO"):
        assert words in header, words      # the header states the rule
    summarize = header[header.index("Calls that need the draws themselves"):]
    assert CALL in summarize[:400]      # listed among the calls a summarising run refuses


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and callable(amwg_ctypes.waic_check)
    assert not hasattr(amwg_ctypes.lib(), CHECK)
    for internal in ("amwg_waic_launch", "amwg_waic_shape", "amwg_waic_totals", "amwg_waic_set_budget"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_the_waic_sources_are_not_among_the_step_kernels_sources():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    for f in ("amwg_waic.hip", "amwg_waic.h"):
        assert f not in build_id.KERNEL_FILES and os.path.exists(os.path.join(ROOT, "bayes.js_amd", "csrc", f)), f
    assert "waic" not in open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_sampler.h")).read().lower()
    hdr = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_waic.h")).read()
    assert "__global__" not in hdr and "__device__" not in hdr and "visibility push(hidden)" in hdr
    src = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_waic.hip")).read()
    assert "atomic" not in src.lower() and "exp_v8" in src      # deterministic accumulations; the exponential the header names


def test_sampler_call_refuses_null_arguments_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: the call is refused for the other argument first
    summary = (C.c_double * 4)()
    for args in ((None, summary, None, None), (fake, None, None, None), (None, None, None, None)):
        assert L.amwg_last_sample_dataset_waic(*args) == -1, args
        assert CALL.encode() in L.amwg_last_error(), L.amwg_last_error()


X3 = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}


@pytest.mark.parametrize("draws,specs,words", [
    (np.zeros((1, 2, 1)), [X3], "fewer than 2 draws"),
    (np.zeros((2, 1, 2)), [X3], "reads 2 components"),
    (np.zeros((2, 2, 3)), [X3, X3], "bad shape"),
    (np.zeros((2, 2, 2)), [X3, dict(X3, model="beta_bern")], "is of model"),
    (np.zeros((2, 2, 2)), [dict(X3, n_obs=0)], "n_obs 0"),
    (np.zeros((2, 9, 2)), [{"model": "pois_glm", "n_obs": 3, "K": 6, "data": {"x": np.zeros(21), "y": np.zeros(3)}}], "K = 7"),
    (np.zeros((2, 9, 2)), [{"model": "pois_glm", "n_obs": 3, "K": 7, "data": {"x": np.zeros(21)}}], "needs y"),
    (np.zeros((2, 4, 2)), [{"model": "hier_normal", "n_obs": 3, "G": 2, "data": {"x": np.zeros(3), "g": np.array([0, 2, 1], dtype=np.int32)}}], "outside 0..1"),
    (np.zeros((2, 4, 2)), [{"model": "hier_normal", "n_obs": 3, "G": 2, "data": {"x": np.zeros(3), "g": np.zeros(3, dtype=np.int32)}}] * 2, "one dataset"),
    (np.zeros((2, 3, 2)), [{"model": "hier_normal", "n_obs": 3, "G": 2, "data": {"x": np.zeros(3), "g": np.zeros(3, dtype=np.int32)}}], "reads 4 components"),
])
def test_waic_check_refuses_bad_shapes_before_a_device_is_opened(draws, specs, words):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.waic_check(draws, specs, device=NO_DEVICE)
    assert CHECK in str(ei.value) and words in str(ei.value), str(ei.value)


def test_waic_check_refuses_a_large_loglik_and_a_negative_budget():
    spec = {"model": "normal", "n_obs": 4097, "data": {"x": np.zeros(4097)}}
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.waic_check(np.zeros((64, 2, 64)), [spec], loglik=True, device=NO_DEVICE)      # 4096 draws x 4097 observations > 2^24
    assert CHECK in str(ei.value) and "2^24" in str(ei.value)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.waic_check(np.zeros((2, 2, 2)), [X3], scratch_bytes=-1, device=NO_DEVICE)
    assert CHECK in str(ei.value) and "scratch_bytes" in str(ei.value)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:      # a valid call reaches the device, and there is none of that number: AMWG_EHIP's words, not a refusal
        amwg_ctypes.waic_check(np.zeros((2, 2, 2)), [X3], device=NO_DEVICE)
    assert CHECK not in str(ei.value)


def test_the_reference_against_closed_forms_and_host_twins():
    wr.self_check()


def test_waic_totals_is_the_finish_as_stated():
    rng = np.random.default_rng(3)
    n = 37
    pw = np.stack([rng.normal(-2.0, 1.0, size=n), rng.uniform(0.0, 0.8, size=n)], axis=1)
    summary, high = amwg_ctypes.waic_totals(pw, n)
    elpd_i = pw[:, 0] - pw[:, 1]
    lppd = p = elpd = 0.0
    for i in range(n):      # Python floats: the same IEEE operations in the same order
        lppd, p, elpd = lppd + pw[i, 0], p + pw[i, 1], elpd + elpd_i[i]
    ss = 0.0
    for i in range(n):
        ss += (elpd_i[i] - elpd / n) * (elpd_i[i] - elpd / n)
    want = np.array([elpd, math.sqrt(n * ss / (n - 1)), p, lppd])
    assert summary.tobytes() == want.tobytes() and high == int((pw[:, 1] > 0.4).sum())
    assert abs(summary[0] - math.fsum(elpd_i)) < 1e-12 and abs(summary[1] - math.sqrt(n * np.var(elpd_i, ddof=1))) < 1e-12
    # rows beyond n_obs (NaN in the library's output) are not read; n = 1 has no standard error; a NaN pair makes the totals NaN
    padded = np.concatenate([pw, np.full((5, 2), np.nan)])
    assert amwg_ctypes.waic_totals(padded, n)[0].tobytes() == summary.tobytes()
    one, h1 = amwg_ctypes.waic_totals(pw[:1], 1)
    assert one[0] == elpd_i[0] and math.isnan(one[1]) and one[2] == pw[0, 1] and one[3] == pw[0, 0] and h1 == int(pw[0, 1] > 0.4)
    bad = pw.copy()
    bad[4] = np.nan
    assert np.isnan(amwg_ctypes.waic_totals(bad, n)[0]).all()


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_compare_waic_under_node():
    script = r"""
const mcmc = require('./bayes.js_amd/mcmc.js');
const a = { pointwise: [[-1.0, 0.2], [-2.5, 0.1], [-0.5, 0.3], [-1.5, 0.05]] }, b = { pointwise: [[-1.2, 0.1], [-2.0, 0.3], [-0.9, 0.2], [-1.0, 0.4]] };
const out = { ab: mcmc.compare_waic(a, b), ba: mcmc.compare_waic(b, a), aa: mcmc.compare_waic(a, a), throws: [] };
for (const bad of [[a, { pointwise: b.pointwise.slice(1) }], [a, {}], [null, b]]) { try { mcmc.compare_waic(bad[0], bad[1]); out.throws.push(false); } catch (e) { out.throws.push(String(e)); } }
console.log(JSON.stringify(out));
"""
    p = subprocess.run([shutil.which("node"), "-e", script], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    out = json.loads(p.stdout)
    ea = [-1.0 - 0.2, -2.5 - 0.1, -0.5 - 0.3, -1.5 - 0.05]
    eb = [-1.2 - 0.1, -2.0 - 0.3, -0.9 - 0.2, -1.0 - 0.4]
    diff = [x - y for x, y in zip(ea, eb)]
    total = 0.0
    for v in diff:
        total += v
    ss = 0.0
    for v in diff:
        ss += (v - total / 4) * (v - total / 4)
    assert out["ab"]["elpd_diff"] == total and out["ab"]["se_diff"] == math.sqrt(4 * ss / 3)
    assert out["ba"]["elpd_diff"] == -total and abs(out["ba"]["se_diff"] - out["ab"]["se_diff"]) < 1e-15
    assert out["aa"] == {"elpd_diff": 0, "se_diff": 0}
    assert "not the same data" in out["throws"][0] and "4 and 3" in out["throws"][0] and all(isinstance(t, str) and "compare_waic" in t for t in out["throws"])
