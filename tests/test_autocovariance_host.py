"""Autocovariance along the chains and the Geyer ESS (amwg_last_sample_dataset_autocovariance, amwg_set_autocovariance, amwg_autocovariance_info), the part that
needs no GPU: the calls are declared in the header, mirrored in the ctypes binding and exported by the product library; the entry point that drives the kernels on
a caller's array (amwg_autocovariance_check) is in the test library only; what either refuses for its arguments alone is refused BEFORE a device is opened -- on a
device number that does not exist -- with the call's name in amwg_last_error(); the restated order of the kernels against exact rational arithmetic (the
measurement behind the cap's factor F); and autocorrelation_ess(), a pure host function, in Python and in JavaScript.  tests/README.autocorrelation.md says what
each test pins."""
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
import autocovariance_reference as ar
import summary_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["amwg_last_sample_dataset_autocovariance", "amwg_set_autocovariance", "amwg_autocovariance_info"]
CHECK = "amwg_autocovariance_check"
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP (-2), not AMWG_EINVAL (-1)


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_calls_are_declared_mirrored_and_exported():
    for call in CALLS:
        assert call in declared("amwg.h") and call in amwg_ctypes.EXPORTS, call
        assert getattr(amwg_ctypes.lib(), call) is not None
    for method in ("set_autocovariance", "dataset_autocovariance", "autocovariance_info"):
        assert callable(getattr(amwg_ctypes.Sampler, method))
    assert callable(amwg_ctypes.autocorrelation_ess)
    header = open(os.path.join(ROOT, "include", "amwg.h")).read()
    for words in ("S_l += y_t * y_(t-l)", "gamma_l = ((S_l - ybar * ((Y - H_l) + (Y - T_l))) + (double)(n - l) * (ybar * ybar)) / (double)n", "m_c = a + ybar"):
        assert words in header, words      # the header states the arithmetic


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and callable(amwg_ctypes.autocovariance_check)
    assert not hasattr(amwg_ctypes.lib(), CHECK)
    for internal in ("amwg_autocov_window", "amwg_autocov_collect", "amwg_autocov_of_array", "amwg_autocov_shape", "amwg_autocov_lag_check", "amwg_autocov_state_elems",
                     "amwg_autocov_armed", "amwg_autocov_begin", "amwg_autocov_forget"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_the_autocovariance_sources_are_not_among_the_step_kernels_sources():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    assert "amwg_autocov.hip" not in build_id.KERNEL_FILES and "amwg_autocov.h" not in build_id.KERNEL_FILES
    sampler_h = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_sampler.h")).read().lower()
    assert "autocov" not in sampler_h      # the armed autocovariance lives beside the handle, not in it
    assert os.path.exists(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_autocov.hip"))


def test_sampler_calls_refuse_bad_arguments_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: each of these calls is refused for another argument first
    values, out = (C.c_int32 * 2)(0, 1), (C.c_double * 8)()
    name = b"amwg_last_sample_dataset_autocovariance"
    for args, why in (((None, values, 2, 1, out, out, out), b"null sampler"), ((fake, values, 2, 1, None, out, out), b"null acov"),
                      ((fake, values, 2, 1, out, None, out), b"null mean"), ((fake, values, 2, 1, out, out, None), b"null between"),
                      ((fake, values, 0, 1, out, out, out), b"0 values"), ((fake, values, -3, 1, out, out, out), b"-3 values"),
                      ((fake, values, 2, 0, out, out, out), b"max_lag 0"), ((fake, values, 2, 1025, out, out, out), b"max_lag 1025")):
        assert L.amwg_last_sample_dataset_autocovariance(*args) == -1, why
        assert name in L.amwg_last_error() and why in L.amwg_last_error(), L.amwg_last_error()
    assert L.amwg_set_autocovariance(None, values, 2, 3) == -1
    assert b"amwg_set_autocovariance" in L.amwg_last_error() and b"null sampler" in L.amwg_last_error()
    k = C.c_int32()
    assert L.amwg_autocovariance_info(None, C.byref(k), None, None) == -1
    assert b"amwg_autocovariance_info" in L.amwg_last_error()


def check_args(**change):
    """the arguments of amwg_autocovariance_check for a valid call of 3 rows x 3 values x 4 chains in 2 datasets over the values (2, 0) at lags 0 .. 2, with `change`"""
    keep = {"draws": np.zeros(36), "values": np.array([2, 0], dtype=np.int32), "acov": np.zeros(2 * 2 * 3), "mean": np.zeros(4), "between": np.zeros(4)}
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a = {"draws": dp(keep["draws"]), "rows": 3, "PR": 3, "C": 4, "D": 2, "values": keep["values"].ctypes.data_as(C.POINTER(C.c_int32)), "n_values": 2, "max_lag": 2,
         "window_rows": 0, "acov": dp(keep["acov"]), "mean": dp(keep["mean"]), "between": dp(keep["between"]), "device": NO_DEVICE}
    for k, v in change.items():
        if k == "value_list":
            keep["values"] = np.array(v, dtype=np.int32)
            a["values"], a["n_values"] = keep["values"].ctypes.data_as(C.POINTER(C.c_int32)), len(v)
        else:
            a[k] = v
    order = ("draws", "rows", "PR", "C", "D", "values", "n_values", "max_lag", "window_rows", "acov", "mean", "between", "device")
    return [a[k] for k in order], keep


@pytest.mark.parametrize("change,why", [
    (dict(draws=None), b"null argument"), (dict(values=None), b"null argument"), (dict(acov=None), b"null argument"), (dict(mean=None), b"null argument"),
    (dict(between=None), b"null argument"),
    (dict(n_values=0), b"0 values"), (dict(n_values=-1), b"-1 values"), (dict(value_list=[0, 1, 2, 1]), b"4 values"),      # n_values < 1, n_values > PR
    (dict(value_list=[0, 3]), b"outside the recorded values"), (dict(value_list=[-1, 0]), b"outside the recorded values"),
    (dict(value_list=[1, 1]), b"listed twice"), (dict(value_list=[2, 0, 2]), b"listed twice"),
    (dict(max_lag=0), b"max_lag 0"), (dict(max_lag=-1), b"max_lag -1"), (dict(max_lag=1025, rows=2000), b"max_lag 1025"),
    (dict(max_lag=3), b"max_lag 3 needs more than 3 kept draws"), (dict(max_lag=1, rows=1), b"needs more than 1 kept draws"),      # max_lag >= rows
    (dict(rows=2 ** 61, C=4), b"beyond size_t"), (dict(rows=3, C=2 ** 62, D=1), b"beyond size_t"),
    (dict(rows=0), b"bad shape"), (dict(PR=0), b"bad shape"), (dict(C=0), b"bad shape"), (dict(D=0), b"bad shape"), (dict(D=3), b"bad shape"),
    (dict(window_rows=-1), b"bad shape")])
def test_selftest_call_refuses_bad_arguments_before_any_device_call(change, why):
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_autocovariance_check(*args) == -1, change      # (-2 would be the device that does not exist)
    assert CHECK.encode() in T.amwg_last_error() and why in T.amwg_last_error(), T.amwg_last_error()


@pytest.mark.parametrize("change", [dict(), dict(value_list=[1]), dict(value_list=[2, 1, 0]), dict(window_rows=1), dict(max_lag=1), dict(rows=2, max_lag=1, C=2, D=2),
                                    dict(rows=1025, max_lag=1024)])
def test_a_valid_call_reaches_the_device_that_does_not_exist(change):
    """the control of the test above: with nothing to refuse, the same call gets as far as opening device 99 and fails THERE (AMWG_EHIP)"""
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_autocovariance_check(*args) == -2, T.amwg_last_error()


# ---- the restated order against exact: the measurement of the cap's factor F (tests/README.autocorrelation.md)

@pytest.mark.parametrize("rows,cpd", ar.HOST_SHAPES)
def test_the_restated_order_stays_under_a_quarter_of_the_cap(rows, cpd):
    worst = [0.0, ""]
    for pattern in sr.FINITE:
        a = ar.array(pattern, rows, cpd)
        for L in ar.host_lags(rows):
            ar.held_to_exact(a.want(L), a, L, "%s %dx%d L %d" % (pattern, rows, cpd, L), worst)
    print("restated order vs exact, %d x %d: largest |error| / cap = %.4f at %s" % (rows, cpd, worst[0], worst[1]))
    assert ar.CAP_FACTOR == 1.0 and worst[0] < 0.25, worst


@pytest.mark.parametrize("pattern", sr.W_ZERO + sr.NON_FINITE)
def test_constant_columns_are_exactly_zero_and_non_finite_ones_nan(pattern):
    a = ar.array(pattern, 9, 64)
    acov, mean, between = a.want(4)
    if pattern in sr.NON_FINITE:
        assert np.all(np.isnan(acov)) and np.all(np.isnan(mean)) and np.all(np.isnan(between))
    else:
        assert all(ar.quarter(a.segment(d, p)) for d in range(ar.D) for p in ar.VALUES)      # multiples of 1/4
        assert np.all(acov == 0.0)
        ar.held_to_exact((acov, mean, between), a, 4, pattern, [0.0, ""])
        for (d, k), (ea, em, eb, kap) in a.exact(4).items():
            assert mean[d, k] == em and between[d, k] == eb      # every sum of them is exact
    x = 3.0 + np.random.default_rng(1).standard_normal((9, 5))
    for bad in (np.nan, np.inf, -np.inf):
        for row in (0, 4, 8):      # the pilot, the middle, the last row
            y = x.copy()
            y[row, 2] = bad
            acov, mean, between = ar.kernel_order(y, 3)
            assert np.all(np.isnan(acov)) and math.isnan(mean) and math.isnan(between), (bad, row)


def test_exact_and_the_restated_order_on_hand_values():
    x = np.array([[1.0], [2.0], [4.0], [5.0]])      # mean 3: deviations -2, -1, 1, 2
    acov, mean, between = ar.exact(x, 3)
    assert list(acov) == [10.0 / 4, 3.0 / 4, -4.0 / 4, -4.0 / 4] and mean == 3.0 and between == 0.0
    got = ar.kernel_order(x, 3)
    assert list(got[0]) == list(acov) and got[1] == 3.0 and got[2] == 0.0
    two = np.concatenate([x, x + 2.0], axis=1)      # a second chain, moved by 2: the same autocovariance, chain means 3 and 5
    acov2, mean2, between2 = ar.kernel_order(two, 3)
    assert list(acov2) == list(acov) and mean2 == 4.0 and between2 == 2.0
    assert ar.exact(two, 3)[2] == 2.0
    rng = np.random.default_rng(3)
    z = rng.standard_normal((300, 7))
    want = [np.mean([np.sum((z[l:, c] - z[:, c].mean()) * (z[:300 - l, c] - z[:, c].mean())) / 300 for c in range(7)]) for l in range(6)]
    assert np.allclose(ar.kernel_order(z, 5)[0], want, rtol=1e-11, atol=1e-14) and np.allclose(ar.exact(z, 5)[0], want, rtol=1e-11, atol=1e-14)


# ---- autocorrelation_ess()

def geometric(phi, L):
    return [phi ** l for l in range(L + 1)]


def truncated_tau(phi, L):
    """tau of rho_l = phi^l summed over the pairs that fit into lags 0 .. L: -1 + 2 sum_(l < 2 floor((L + 1) / 2)) phi^l"""
    return -1.0 + 2.0 * sum(phi ** l for l in range(2 * ((L + 1) // 2)))


N_BIG = 10 ** 12      # n / (n - 1) = 1 to 1e-12
ESS_CASES = {      # name: (acov, between, rows, chains)
    "white": ([1.0] + [0.0] * 9, 0.0, N_BIG, 1),
    "geometric": (geometric(0.5, 40), 0.0, N_BIG, 1),
    "alternating": ([1.0, -0.9, 0.8, -0.7], 0.0, 3, 1),      # n / (n - 1) = 1.5: rho_1 = 1 - 1.5 x 1.9 = -1.85, so P_0 < 0
    "positive": (geometric(0.9, 9), 0.0, N_BIG, 1),
    "clamp": ([1.0, 0.5, 0.1, 0.1, 0.3, 0.3, -0.5, -0.5], 0.0, N_BIG, 1),
    "zero": ([0.0, 0.0, 0.0, 0.0], 0.0, 100, 1),
    "between_ignored": ([1.0, 0.5, 0.25, 0.125], 7.0, N_BIG, 1),
    "between_used": ([1.0, 0.5, 0.25, 0.125], 1.0, N_BIG, 4),
}


def check_ess_cases(res):
    """res: name -> dict with rho (list, None for NaN), tau, ess (None for NaN), truncated, lags_used"""
    r = res["white"]
    assert r["rho"][0] == 1.0 and abs(r["tau"] - 1.0) <= 1e-9 and abs(r["ess"] - N_BIG) <= 1e-9 * N_BIG
    assert r["truncated"] and r["lags_used"] == 2      # (rho_l = 1 - n / (n - 1) < 0 for l >= 1: the second pair is negative)
    r = res["geometric"]      # L = 40: 20 pairs + a last lag without a partner
    full = (1 + 0.5) / (1 - 0.5)
    tail = 2.0 * sum(0.5 ** l for l in range(40, 2000))
    assert abs(r["tau"] - (full - tail)) <= 1e-9 and abs(r["tau"] - truncated_tau(0.5, 40)) <= 1e-9 and not r["truncated"] and r["lags_used"] == 40
    r = res["alternating"]      # truncated at k = 0: nothing kept
    assert r["rho"][1] < -1.0 and r["truncated"] and r["lags_used"] == 0 and r["tau"] == -1.0
    r = res["positive"]
    assert not r["truncated"] and r["lags_used"] == 10 and abs(r["tau"] - truncated_tau(0.9, 9)) <= 1e-9
    r = res["clamp"]      # P = 1.5, 0.2, 0.6 -> clamped to 0.2, then -1.0 stops the sum
    assert r["truncated"] and r["lags_used"] == 6 and abs(r["tau"] - (-1.0 + 2.0 * (1.5 + 0.2 + 0.2))) <= 1e-9
    r = res["zero"]
    assert r["rho"][0] == 1.0 and all(v is None for v in r["rho"][1:]) and r["tau"] is None and r["ess"] is None and not r["truncated"]
    a, b = res["between_ignored"], res["between_used"]
    assert abs(a["rho"][1] - 0.5) <= 1e-9 and abs(b["rho"][1] - (1.0 - 0.5 / 2.0)) <= 1e-9      # var_plus = 1 against 1 + 1
    assert abs(a["ess"] - N_BIG / a["tau"]) <= 1e-9 * N_BIG and abs(b["ess"] - 4 * N_BIG / b["tau"]) <= 1e-9 * N_BIG


def plain(r):
    none = lambda v: None if v != v else float(v)
    return {"rho": [none(v) for v in r["rho"]], "tau": none(r["tau"]), "ess": none(r["ess"]), "truncated": bool(r["truncated"]), "lags_used": int(r["lags_used"])}


def test_autocorrelation_ess_hand_values():
    check_ess_cases({name: plain(amwg_ctypes.autocorrelation_ess(*args)) for name, args in ESS_CASES.items()})
    r = amwg_ctypes.autocorrelation_ess([2.0, 1.0], 0.0, 11, 1)      # n / (n - 1) = 1.1: rho_1 = 1 - 1.1 x 0.5
    assert abs(r["rho"][1] - 0.45) <= 1e-15 and r["lags_used"] == 2
    for bad in (math.nan, math.inf):
        r = amwg_ctypes.autocorrelation_ess([bad, 1.0], 0.0, 11, 1)
        assert r["rho"][0] == 1.0 and math.isnan(r["rho"][1]) and math.isnan(r["tau"]) and math.isnan(r["ess"])


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_autocorrelation_ess_hand_values():
    script = ("const mcmc = require(%r); const cases = %s; const out = {}; const none = (v) => Number.isNaN(v) ? null : v; "
              "for (const name of Object.keys(cases)) { const r = mcmc.autocorrelation_ess.apply(null, cases[name]); "
              "out[name] = {rho: r.rho.map(none), tau: none(r.tau), ess: none(r.ess), truncated: r.truncated, lags_used: r.lags_used}; } console.log(JSON.stringify(out));")
    p = subprocess.run([shutil.which("node"), "-e", script % (os.path.join(ROOT, "bayes.js_amd", "mcmc.js"), json.dumps(ESS_CASES))], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    check_ess_cases(got)
    want = {name: plain(amwg_ctypes.autocorrelation_ess(*args)) for name, args in ESS_CASES.items()}
    assert got == want      # the same arithmetic in the same order: the same doubles


@pytest.mark.parametrize("phi", [0.0, 0.5])
def test_the_restated_order_recovers_tau_of_an_ar1_series(phi):
    """M = 4, n = 50 000, L = 200: tau within 10 % of (1 + phi) / (1 - phi); its relative standard error there is about sqrt(2 x 21 / 200 000) = 1.4 %"""
    rng = np.random.default_rng([20261020, int(phi * 10)])
    n, M = 50000, 4
    e = rng.standard_normal((n, M))
    x = np.empty((n, M))
    x[0] = e[0] / math.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    acov, mean, between = ar.kernel_order(x + 10.0, 200)
    r = amwg_ctypes.autocorrelation_ess(acov, between, n, M)
    want = (1 + phi) / (1 - phi)
    print("AR(1) phi %.1f: tau %.4f (wanted %.4f), ess %.0f, lags used %d" % (phi, r["tau"], want, r["ess"], r["lags_used"]))
    assert r["truncated"] and abs(r["tau"] / want - 1.0) <= 0.10, r
