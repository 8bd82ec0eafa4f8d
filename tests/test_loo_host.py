"""PSIS-LOO per dataset (amwg_last_sample_dataset_loo), the part that needs no GPU: the call is declared in the header with its rule, mirrored in the ctypes binding
and exported by the product library; the entry point that drives the kernels on a caller's draws and data (amwg_loo_check) is in the test library only; what either
refuses for its arguments alone is refused BEFORE a device is opened -- on a device number that does not exist -- the cap on the tail length included; the tail
length; the reference against closed forms; the fp64 restatement of the rule against the extended-precision one over the very cases of tests/test_gpu_loo.py, within a
quarter of each bound; loo_totals, the finish restated; compare_loo under node.  tests/README.loo.md says what each test pins."""
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
import loo_reference as lr
import waic_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "amwg_last_sample_dataset_loo"
CHECK = "amwg_loo_check"
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP (-2), not AMWG_EINVAL (-1)


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_declared_and_mirrored():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.lib(), CALL) is not None
    for method in ("dataset_loo", "loo"):
        assert callable(getattr(amwg_ctypes.Sampler, method))
    assert callable(amwg_ctypes.loo_totals) and callable(amwg_ctypes.loo_tail_len)
    header = " ".join(re.sub(r"(?m)^ \* ", " ", open(os.path.join(ROOT, "include", "amwg.h")).read()).split())      # (the comment's leading stars and line breaks removed)
    for words in ("a_0 <= ... <= a_{S-1}", "M = min(floor(S / 5), m3), m3 the smallest integer with m3^2 >= 9 S", "if M < 5: khat_i = +inf",
                  "elpd_loo_i = a_0 + log S - log sum_t exp(a_0 - a_t)", "ec = exp_v8(a_0 - a_M)", "THE EXCESSES ARE PINNED TO THE BIT", "x_r = exp_v8(a_0 - a_{M-r}) - ec",
                  "mm = 30 + floor(sqrt(M))", "x* = x_{floor(M / 4 + 0.5)}", "theta_j = 1 / x_M + (1 - sqrt(mm / (j - 0.5))) / (3 x*)", "k_j = mean_r log1p(-theta_j x_r)",
                  "L_j = M (log(-theta_j / k_j) - k_j - 1)", "w_j = 1 / sum_i exp(L_i - L_j)", "sigma = -k' / theta^", "khat_i = (M k' + 5) / (M + 10)",
                  "If x* <= 0, or x_M <= 0, or khat is not finite: the raw route", "p_r = (r - 0.5) / M", "q_r = sigma expm1(-khat log1p(-p_r)) / khat",
                  "lw~_r = min(log(q_r + ec), 0)", "elpd_loo_i = a_0 + log((S - M) + sum_r exp(lw~_r - lw_r)) - log(B + sum_r exp(lw~_r)), with B = sum_{t >= M} exp(a_0 - a_t)",
                  "ties at the cutoff cannot change the result", "NOT PINNED TO THE BIT", "no floating-point atomics", "E_k = M (M + mm) u (1 + |khat|)",
                  "|elpd_loo_i - exact| <= E (1 + |exact|) + 4 ln(2 M) E_k", "NaN for that (d, i) only", "p_loo = lppd - elpd_loo", "NaN for n_d = 1",
                  "high[d] counts khat_i > 0.7, +inf included", "the pointwise terms of a closure are not known to the library; built-in families only", "M + 1 > 8192",
                  "8192 doubles (64 KB)", "256 MiB", "OUT OF SCOPE: LOO after amwg_sample_summarize", "moment matching", "r_eff", "a pooled LOO across devices", "tails beyond the LDS cap"):
        assert words in header, words      # the header states the rule
    waic_scope = header[header.index("OUT OF SCOPE: WAIC after"):][:300]
    assert "PSIS-LOO" not in waic_scope      # no longer out of WAIC's scope: it is the next call
    summarize = header[header.index("Calls that need the draws themselves"):]
    assert CALL in summarize[:450]      # listed among the calls a summarising run refuses


def test_selftest_call_is_in_the_test_library_only():
    for name in (CHECK, "amwg_loo_stats"):
        assert name in declared("amwg_selftest.h") and name in amwg_ctypes.SELFTEST_EXPORTS and name not in amwg_ctypes.EXPORTS
        assert getattr(amwg_ctypes.selftest_lib(), name) is not None and not hasattr(amwg_ctypes.lib(), name)
    assert callable(amwg_ctypes.loo_check) and callable(amwg_ctypes.loo_stats)
    for internal in ("amwg_loo_launch", "amwg_loo_shape", "amwg_loo_totals", "amwg_loo_set_budget", "amwg_loo_set_timing", "amwg_loo_last_stats", "amwg_waic_describe"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_the_loo_sources_are_not_among_the_step_kernels_sources():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    csrc = os.path.join(ROOT, "bayes.js_amd", "csrc")
    for f in ("amwg_loo.hip", "amwg_loo.h", "amwg_terms.h"):
        assert f not in build_id.KERNEL_FILES and os.path.exists(os.path.join(csrc, f)), f
    assert "amwg_loo" not in open(os.path.join(csrc, "amwg_sampler.h")).read().lower()
    hdr = open(os.path.join(csrc, "amwg_loo.h")).read()
    assert "__global__" not in hdr and "__device__" not in hdr and "visibility push(hidden)" in hdr
    src = open(os.path.join(csrc, "amwg_loo.hip")).read()
    for fn in ("exp_v8", "log_v8", "log1p_v8", "expm1_v8", "select_key"):
        assert fn in src, fn
    # the atomics count and place terms: every one of them is on an integer
    assert set(re.findall(r"\b(atomic[A-Za-z]+)\(", src)) == {"atomicAdd", "atomicMin", "atomicOr"}
    for target in re.findall(r"\batomic[A-Za-z]+\((?:\([^)]*\))?&(\w+)", src):
        assert target in ("cnt", "h", "state"), target      # LDS counters, the global counters, the state's integer fields
    assert 'amwg_loo.o' in open(os.path.join(csrc, "Makefile")).read().split("COMMON_OBJS =")[1].split("\n")[0]
    # both calls take their terms from the one header
    for f in ("amwg_loo.hip", "amwg_waic.hip"):
        assert '#include "amwg_terms.h"' in open(os.path.join(csrc, f)).read() and "struct Family" not in open(os.path.join(csrc, f)).read()


def test_sampler_call_refuses_null_arguments_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: the call is refused for the other argument first
    summary = (C.c_double * 4)()
    for args in ((None, summary, None, None), (fake, None, None, None), (None, None, None, None)):
        assert L.amwg_last_sample_dataset_loo(*args) == -1, args
        assert CALL.encode() in L.amwg_last_error(), L.amwg_last_error()


X3 = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}


@pytest.mark.parametrize("draws,specs,words", [
    (np.zeros((1, 2, 1)), [X3], "fewer than 2 draws"),
    (np.zeros((2, 1, 2)), [X3], "reads 2 components"),
    (np.zeros((2, 2, 3)), [X3, X3], "bad shape"),
    (np.zeros((2, 2, 2)), [X3, dict(X3, model="beta_bern")], "is of model"),
    (np.zeros((2, 2, 2)), [dict(X3, n_obs=0)], "n_obs 0"),
    (np.zeros((2, 9, 2)), [{"model": "pois_glm", "n_obs": 3, "K": 6, "data": {"x": np.zeros(21), "y": np.zeros(3)}}], "K = 7"),
    (np.zeros((2, 4, 2)), [{"model": "hier_normal", "n_obs": 3, "G": 2, "data": {"x": np.zeros(3), "g": np.array([0, 2, 1], dtype=np.int32)}}], "outside 0..1"),
    (np.zeros((2, 4, 2)), [{"model": "hier_normal", "n_obs": 3, "G": 2, "data": {"x": np.zeros(3), "g": np.zeros(3, dtype=np.int32)}}] * 2, "one dataset"),
])
def test_loo_check_refuses_bad_shapes_before_a_device_is_opened(draws, specs, words):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.loo_check(draws, specs, device=NO_DEVICE)
    assert CHECK in str(ei.value) and words in str(ei.value), str(ei.value)


def test_the_cap_on_the_tail_length_is_decided_from_the_shape():
    S = 1
    while lr.tail_len(S) + 1 <= 8192:      # the first S whose tail exceeds the cap, by doubling and bisection
        S *= 2
    lo, hi = S // 2, S
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lr.tail_len(mid) + 1 <= 8192 else (lo, mid)
    assert lr.tail_len(lo) == 8191 and lr.tail_len(hi) == 8192 and 7.4e6 < hi < 7.5e6, (lo, hi)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.loo_check(np.zeros((hi, 2, 1)), [X3], device=NO_DEVICE)      # (the pages of the array are never touched)
    assert CHECK in str(ei.value) and "8192 doubles (64 KB)" in str(ei.value) and str(hi) in str(ei.value), str(ei.value)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:      # one draw fewer is served: the call reaches the device, and there is none of that number
        amwg_ctypes.loo_check(np.zeros((lo, 2, 1)), [X3], device=NO_DEVICE)
    assert CHECK not in str(ei.value)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.loo_check(np.zeros((2, 2, 2)), [X3], scratch_bytes=-1, device=NO_DEVICE)
    assert CHECK in str(ei.value) and "scratch_bytes" in str(ei.value)
    spec = {"model": "normal", "n_obs": 90000, "data": {"x": np.zeros(90000)}}
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.loo_check(np.zeros((64, 2, 64)), [spec], tails=True, device=NO_DEVICE)      # 193 x 90000 > 2^24
    assert CHECK in str(ei.value) and "2^24" in str(ei.value)


@pytest.mark.parametrize("S,M", [(2, 0), (3, 0), (24, 4), (25, 5), (29, 5), (30, 6), (224, 44), (225, 45), (226, 45), (1088, 99), (4096, 192), (256000, 1518)])
def test_tail_len(S, M):
    assert lr.tail_len(S) == M == amwg_ctypes.loo_tail_len(S)
    m3 = next(m for m in range(0, 3 * S + 2) if m * m >= 9 * S)
    assert M == min(S // 5, m3)


def test_the_reference_against_closed_forms():
    lr.self_check()


def test_the_fp64_restatement_stays_within_a_quarter_of_each_bound():
    """the measurement the bounds of include/amwg.h rest on, over the cases of tests/test_gpu_loo.py: the rule in numpy fp64 against the rule in extended precision,
    both from the same pinned excesses.  The device's sums run in another order: the margin of four is theirs."""
    worst = {"elpd": (0.0, ""), "khat": (0.0, "")}
    fitted = raw = 0
    for name, draws, specs in lr.all_cases():
        D = len(specs)
        S = draws.shape[0] * draws.shape[2] // D
        for d, spec in enumerate(specs):
            ll = lr.loglik_of(spec, wr.draws_of_dataset(draws, D, d))
            ref_e, ref_k = lr.pointwise(ll)
            e64, k64 = lr.pointwise(ll, np.float64)
            re, rk = lr.ratios(e64, k64, ref_e, ref_k, S)
            fitted, raw = fitted + int(np.isfinite(ref_k).sum()), raw + int(np.isinf(ref_k).sum())
            for key, r in (("elpd", re), ("khat", rk)):
                if r > worst[key][0]:
                    worst[key] = (r, "%s, dataset %d, S = %d" % (name, d, S))
            assert re <= 0.25 and rk <= 0.25, (name, d, S, re, rk)
    print("fp64 against extended precision over %d fitted and %d unfitted observations: largest |elpd error| / bound %.3g (%s), largest |khat error| / bound %.3g (%s)"
          % (fitted, raw, worst["elpd"][0], worst["elpd"][1], worst["khat"][0], worst["khat"][1]))
    assert fitted > 1000 and raw > 500


def test_loo_totals_is_the_finish_as_stated():
    rng = np.random.default_rng(3)
    n = 37
    pw = np.stack([rng.normal(-2.2, 1.0, size=n), rng.normal(-2.0, 1.0, size=n), rng.uniform(-0.2, 1.2, size=n)], axis=1)
    pw[5, 2] = np.inf
    summary, high = amwg_ctypes.loo_totals(pw, n)
    elpd = lppd = 0.0
    for i in range(n):      # Python floats: the same IEEE operations in the same order
        elpd, lppd = elpd + pw[i, 0], lppd + pw[i, 1]
    ss = 0.0
    for i in range(n):
        ss += (pw[i, 0] - elpd / n) * (pw[i, 0] - elpd / n)
    want = np.array([elpd, math.sqrt(n * ss / (n - 1)), lppd - elpd, lppd])
    assert summary.tobytes() == want.tobytes() and high == int((pw[:, 2] > 0.7).sum()) and pw[5, 2] > 0.7
    assert abs(summary[0] - math.fsum(pw[:, 0])) < 1e-12 and abs(summary[1] - math.sqrt(n * np.var(pw[:, 0], ddof=1))) < 1e-12
    # rows beyond n_obs (NaN in the library's output) are not read; n = 1 has no standard error; a NaN triple makes the totals NaN
    padded = np.concatenate([pw, np.full((5, 3), np.nan)])
    assert amwg_ctypes.loo_totals(padded, n)[0].tobytes() == summary.tobytes()
    one, h1 = amwg_ctypes.loo_totals(pw[:1], 1)
    assert one[0] == pw[0, 0] and math.isnan(one[1]) and one[2] == pw[0, 1] - pw[0, 0] and one[3] == pw[0, 1] and h1 == int(pw[0, 2] > 0.7)
    bad = pw.copy()
    bad[4] = np.nan
    assert np.isnan(amwg_ctypes.loo_totals(bad, n)[0]).all()


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_compare_loo_under_node():
    script = r"""
const mcmc = require('./bayes.js_amd/mcmc.js');
const a = { pointwise: [[-1.2, -1.0, 0.2], [-2.6, -2.5, 0.1], [-0.8, -0.5, 0.9], [-1.55, -1.5, Infinity]] };
const b = { pointwise: [[-1.3, -1.2, 0.1], [-2.3, -2.0, 0.3], [-1.1, -0.9, 0.2], [-1.4, -1.0, 0.4]] };
const out = { ab: mcmc.compare_loo(a, b), ba: mcmc.compare_loo(b, a), aa: mcmc.compare_loo(a, a), throws: [] };
for (const bad of [[a, { pointwise: b.pointwise.slice(1) }], [a, {}], [null, b]]) { try { mcmc.compare_loo(bad[0], bad[1]); out.throws.push(false); } catch (e) { out.throws.push(String(e)); } }
console.log(JSON.stringify(out));
"""
    p = subprocess.run([shutil.which("node"), "-e", script], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    out = json.loads(p.stdout)
    ea, eb = [-1.2, -2.6, -0.8, -1.55], [-1.3, -2.3, -1.1, -1.4]
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
    assert "not the same data" in out["throws"][0] and "4 and 3" in out["throws"][0] and all(isinstance(t, str) and "compare_loo" in t for t in out["throws"])
