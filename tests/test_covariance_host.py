"""Posterior covariance and correlation (amwg_last_sample_dataset_covariance, amwg_set_covariance, amwg_covariance_info), the part that needs no GPU: the calls are
declared in the header, mirrored in the ctypes binding and exported by the product library; the entry point that drives the kernels on a caller's array
(amwg_covariance_check) is in the test library only; what either refuses for its arguments alone is refused BEFORE a device is opened -- on a device number that
does not exist -- with the call's name in amwg_last_error(); the restated order of the kernels against exact rational arithmetic (the measurement behind the cap's
factor F); and correlation(), a pure host function, in Python and in JavaScript.  tests/README.covariance.md says what each test pins."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import covariance_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["amwg_last_sample_dataset_covariance", "amwg_set_covariance", "amwg_covariance_info"]
CHECK = "amwg_covariance_check"
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP (-2), not AMWG_EINVAL (-1)


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_calls_are_declared_mirrored_and_exported():
    for call in CALLS:
        assert call in declared("amwg.h") and call in amwg_ctypes.EXPORTS, call
        assert getattr(amwg_ctypes.lib(), call) is not None
    for method in ("set_covariance", "dataset_covariance", "covariance_info"):
        assert callable(getattr(amwg_ctypes.Sampler, method))
    assert callable(amwg_ctypes.correlation)


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and callable(amwg_ctypes.covariance_check)
    assert not hasattr(amwg_ctypes.lib(), CHECK)
    for internal in ("amwg_comoment_window", "amwg_covariance_finish", "amwg_covariance_of_array", "amwg_covariance_shape", "amwg_covariance_values_check",
                     "amwg_covariance_order", "amwg_covariance_pairs", "amwg_covariance_armed", "amwg_covariance_begin", "amwg_covariance_forget"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_the_covariance_sources_are_not_among_the_step_kernels_sources():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    assert "amwg_covariance.hip" not in build_id.KERNEL_FILES and "amwg_covariance.h" not in build_id.KERNEL_FILES
    sampler_h = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_sampler.h")).read().lower()
    assert "covariance" not in sampler_h and "comoment" not in sampler_h      # the armed covariance lives beside the handle, not in it
    assert os.path.exists(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_covariance.hip"))


def test_sampler_calls_refuse_bad_arguments_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: each of these calls is refused for another argument first
    values, cov = (C.c_int32 * 2)(0, 1), (C.c_double * 4)()
    name = b"amwg_last_sample_dataset_covariance"
    for args, why in (((None, values, 2, cov), b"null sampler"), ((fake, values, 2, None), b"null cov"), ((fake, values, 0, cov), b"0 values"),
                      ((fake, values, -3, cov), b"-3 values")):
        assert L.amwg_last_sample_dataset_covariance(*args) == -1, why
        assert name in L.amwg_last_error() and why in L.amwg_last_error(), L.amwg_last_error()
    assert L.amwg_set_covariance(None, values, 2) == -1
    assert b"amwg_set_covariance" in L.amwg_last_error() and b"null sampler" in L.amwg_last_error()
    k = C.c_int32()
    assert L.amwg_covariance_info(None, C.byref(k), None) == -1
    assert b"amwg_covariance_info" in L.amwg_last_error()


def check_args(**change):
    """the arguments of amwg_covariance_check for a valid call of 2 rows x 3 values x 4 chains in 2 datasets over the values (2, 0), with `change` applied"""
    keep = {"draws": np.zeros(24), "values": np.array([2, 0], dtype=np.int32), "cov": np.zeros(2 * 4)}
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a = {"draws": dp(keep["draws"]), "rows": 2, "PR": 3, "C": 4, "D": 2, "values": keep["values"].ctypes.data_as(C.POINTER(C.c_int32)), "n_values": 2,
         "window_rows": 0, "cov": dp(keep["cov"]), "device": NO_DEVICE}
    for k, v in change.items():
        if k == "value_list":
            keep["values"] = np.array(v, dtype=np.int32)
            a["values"], a["n_values"] = keep["values"].ctypes.data_as(C.POINTER(C.c_int32)), len(v)
        else:
            a[k] = v
    order = ("draws", "rows", "PR", "C", "D", "values", "n_values", "window_rows", "cov", "device")
    return [a[k] for k in order], keep


@pytest.mark.parametrize("change,why", [
    (dict(draws=None), b"null argument"), (dict(values=None), b"null argument"), (dict(cov=None), b"null argument"),
    (dict(n_values=0), b"0 values"), (dict(n_values=-1), b"-1 values"), (dict(value_list=[0, 1, 2, 1]), b"4 values"),      # n_values < 1, n_values > PR
    (dict(value_list=[0, 3]), b"outside the recorded values"), (dict(value_list=[-1, 0]), b"outside the recorded values"),
    (dict(value_list=[1, 1]), b"listed twice"), (dict(value_list=[2, 0, 2]), b"listed twice"),
    (dict(rows=1, C=2, D=2), b"at least 2 draws"),      # rows x cpd < 2
    (dict(rows=2 ** 61, C=4), b"beyond size_t"), (dict(rows=2, C=2 ** 62, D=1), b"beyond size_t"),
    (dict(rows=0), b"bad shape"), (dict(PR=0), b"bad shape"), (dict(C=0), b"bad shape"), (dict(D=0), b"bad shape"), (dict(D=3), b"bad shape"),
    (dict(window_rows=-1), b"bad shape")])
def test_selftest_call_refuses_bad_arguments_before_any_device_call(change, why):
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_covariance_check(*args) == -1, change      # (-2 would be the device that does not exist)
    assert CHECK.encode() in T.amwg_last_error() and why in T.amwg_last_error(), T.amwg_last_error()


@pytest.mark.parametrize("change", [dict(), dict(value_list=[1]), dict(value_list=[2, 1, 0]), dict(window_rows=1), dict(rows=1, C=4, D=2), dict(rows=2, C=2, D=2)])
def test_a_valid_call_reaches_the_device_that_does_not_exist(change):
    """the control of the test above: with nothing to refuse, the same call gets as far as opening device 99 and fails THERE (AMWG_EHIP)"""
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_covariance_check(*args) == -2, T.amwg_last_error()


# ---- the restated order against exact: the measurement of the cap's factor F (tests/README.covariance.md)

_worst = [0.0, ""]


@pytest.mark.parametrize("rows,cpd", cr.SHAPES)
def test_the_restated_order_stays_under_a_quarter_of_the_cap(rows, cpd):
    worst = [0.0, ""]
    for pattern, kind in cr.CASES():
        a = cr.array(pattern, kind, rows, cpd)
        label = "%s/%s %dx%d" % (pattern, kind, rows, cpd)
        cr.held_to_exact(a.want, a, cr.D, label, worst)
        assert np.array_equal(a.want, np.transpose(a.want, (0, 2, 1)), equal_nan=True)
    print("restated order vs exact, %d x %d: largest |error| / cap = %.4f at %s" % (rows, cpd, worst[0], worst[1]))
    if worst[0] > _worst[0]:
        _worst[:] = worst
    assert cr.CAP_FACTOR == 1.0 and worst[0] < 0.25, worst


def test_exact_cov_and_the_restated_order_on_hand_values():
    x = np.array([[1.0, 2.0], [3.0, 6.0]])      # the values 1, 2, 3, 6: mean 3, sum of squares about it 14
    y = 2.0 * x
    assert cr.exact_cov(x, x) == 14.0 / 3.0 and cr.exact_cov(x, y) == 28.0 / 3.0 and cr.exact_cov(x, -x) == -14.0 / 3.0
    assert np.isnan(cr.exact_cov(x, np.array([[1.0, np.inf], [0.0, 0.0]])))
    assert cr.kernel_order_cov(x) == np.float64(14.0) / np.float64(3.0)
    assert cr.kernel_order_cov(x, y) == 2.0 * cr.kernel_order_cov(x)
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((2, 7, 300))
    want = np.cov(a.reshape(-1), b.reshape(-1))
    got = [[cr.kernel_order_cov(a), cr.kernel_order_cov(a, b)], [cr.kernel_order_cov(a, b), cr.kernel_order_cov(b)]]
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert np.allclose([[cr.exact_cov(a, a), cr.exact_cov(a, b)], [cr.exact_cov(a, b), cr.exact_cov(b, b)]], want, rtol=1e-12, atol=0)


# ---- correlation()

HAND = [      # (cov, the correlation wanted; None = NaN)
    ([[4.0, 2.0], [2.0, 9.0]], [[1.0, 1.0 / 3.0], [1.0 / 3.0, 1.0]]),
    ([[1.0, 2.0], [2.0, 4.0]], [[1.0, 1.0], [1.0, 1.0]]),                    # y = 2 x
    ([[1.0, -1.0], [-1.0, 1.0]], [[1.0, -1.0], [-1.0, 1.0]]),                # y = -x
    ([[0.0, 0.0], [0.0, 2.0]], [[None, None], [None, 1.0]]),                 # a zero variance
    ([[1.0, 1.0000000000000002], [1.0000000000000002, 1.0]], [[1.0, 1.0], [1.0, 1.0]]),      # rounding beyond 1 is clamped
    ([[float("inf"), 1.0], [1.0, 1.0]], [[None, None], [None, 1.0]]),        # a variance that is not finite
    ([[1.0, float("nan")], [float("nan"), 1.0]], [[1.0, None], [None, 1.0]]),
    ([[-1.0, 0.5], [0.5, 1.0]], [[None, None], [None, 1.0]]),
]


def as_array(want):
    return np.array([[np.nan if v is None else v for v in row] for row in want])


def test_correlation_hand_values():
    for cov, want in HAND:
        got = amwg_ctypes.correlation(np.array(cov))
        assert np.array_equal(got, as_array(want), equal_nan=True), (cov, got)
    stack = amwg_ctypes.correlation(np.array([HAND[0][0], HAND[3][0]]))      # [D][K][K]
    assert np.array_equal(stack, np.array([as_array(HAND[0][1]), as_array(HAND[3][1])]), equal_nan=True)
    with pytest.raises(amwg_ctypes.AmwgError):
        amwg_ctypes.correlation(np.zeros((2, 3)))


@pytest.mark.parametrize("n,k", [(5, 2), (40, 3), (300, 8)])
def test_correlation_against_np_corrcoef(n, k):
    rng = np.random.default_rng([20261020, n, k])
    x = rng.standard_normal((k, n)) @ rng.standard_normal((n, n)) * np.exp(rng.standard_normal(k))[:, None] * 10.0 ** rng.integers(-3, 4, k)[:, None]
    got = amwg_ctypes.correlation(np.cov(x))
    want = np.corrcoef(x)
    assert np.all(np.diagonal(got) == 1.0) and np.all(np.abs(got) <= 1.0)
    assert np.max(np.abs(got - want)) <= 8 * cr.U, np.max(np.abs(got - want))      # a quotient, a product and two square roots: a few u of a number <= 1
    assert np.array_equal(got, got.T)


@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_correlation_hand_values():
    script = ("const mcmc = require(%r); const cases = %s; "
              "console.log(JSON.stringify(cases.map(c => mcmc.correlation(c.map(r => r.map(v => v === 'inf' ? Infinity : v === 'nan' ? NaN : v)))"
              ".map(r => r.map(v => Number.isNaN(v) ? null : v)))));")
    enc = lambda v: "inf" if v == float("inf") else "nan" if v != v else v
    cases = [[[enc(v) for v in row] for row in cov] for cov, _ in HAND]
    p = subprocess.run([shutil.which("node"), "-e", script % (os.path.join(ROOT, "bayes.js_amd", "mcmc.js"), json.dumps(cases))], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got == [want for _, want in HAND], got
