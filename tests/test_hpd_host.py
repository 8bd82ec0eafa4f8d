"""Highest-density intervals per dataset (amwg_last_sample_dataset_hpd), the part that needs no GPU: the call is declared in the header with its rule, mirrored
in the ctypes binding and exported by the product library; the entry point that drives the kernels on a caller's array (amwg_hpd_check) is in the test library
only; what either refuses for its arguments alone is refused BEFORE a device is opened -- on a device number that does not exist -- with the call's name in
amwg_last_error(); the host reference on hand values; and the device's route restated (hpd_tails) against the full sort (hpd), as bytes.
tests/README.hpd.md says what each test pins."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import amwg_ctypes
import hpd_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "amwg_last_sample_dataset_hpd"
CHECK = "amwg_hpd_check"
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP (-2), not AMWG_EINVAL (-1)


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_call_is_declared_mirrored_and_exported():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.lib(), CALL) is not None
    for method in ("dataset_hpd", "hpd"):
        assert callable(getattr(amwg_ctypes.Sampler, method))
    header = " ".join(re.sub(r"(?m)^ \* ", " ", open(os.path.join(ROOT, "include", "amwg.h")).read()).split())      # (the comment's leading stars and line breaks removed)
    for words in ("with -0 before +0", "g = floor(p * (double)N), one IEEE fp64 multiply then floor, clamped to [1, N - 1]", "Set k = N - g",
                  "w_i = x_(i+g) - x_(i) in fp64, for i = 0 ... k - 1", "i* is the smallest i whose w_i is minimal, with widths compared as doubles",
                  "(x_(i*), x_(i*+g))", "Its bytes are those of two draws", "outside the open interval (0, 1) gives (NaN, NaN)",
                  "A NaN or +-inf anywhere among the N draws of (d, v) gives (NaN, NaN) for every probability of that (d, v), and nowhere else",
                  "out[D][P + derived][n_probs][2]", "256 MiB", "AS p -> 0 THE TAILS APPROACH THE WHOLE SLICE"):
        assert words in header, words      # the header states the rule
    summarize = header[header.index("Calls that need the draws themselves"):]
    assert CALL in summarize[:400]      # listed among the calls a summarising run refuses


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and callable(amwg_ctypes.hpd_check)
    assert not hasattr(amwg_ctypes.lib(), CHECK) and not hasattr(amwg_ctypes.lib(), "amwg_hpd_limits")
    for internal in ("amwg_hpd_launch", "amwg_hpd_shape", "amwg_hpd_lds_keys", "amwg_hpd_set_budget"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_the_hpd_sources_are_not_among_the_step_kernels_sources():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    for f in ("amwg_hpd.hip", "amwg_hpd.h", "amwg_select.h"):
        assert f not in build_id.KERNEL_FILES and os.path.exists(os.path.join(ROOT, "bayes.js_amd", "csrc", f)), f
    assert "hpd" not in open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_sampler.h")).read().lower()
    hdr = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_hpd.h")).read()
    assert "__global__" not in hdr and "__device__" not in hdr and "visibility push(hidden)" in hdr      # the launcher and the shape check only
    src = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_hpd.hip")).read()
    assert "hipcub" not in src and "rocprim" not in src and "hipMemcpyDeviceToHost" in src


def test_sampler_call_refuses_bad_arguments_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: each of these calls is refused for another argument first
    probs, out = (C.c_double * 2)(0.5, 0.95), (C.c_double * 64)()
    for args in ((None, probs, 2, out), (fake, None, 2, out), (fake, probs, 2, None), (fake, probs, 0, out), (fake, probs, -1, out)):
        assert L.amwg_last_sample_dataset_hpd(*args) == -1, args
        assert CALL.encode() in L.amwg_last_error(), L.amwg_last_error()


def check_args(**change):
    """the arguments of amwg_hpd_check for a valid call of 3 rows x 2 values x 4 chains in 2 datasets at two probabilities, with `change`"""
    keep = {"draws": np.zeros(24), "probs": np.array([0.5, 0.95]), "out": np.zeros(2 * 2 * 2 * 2)}
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a = {"device": NO_DEVICE, "draws": dp(keep["draws"]), "rows": 3, "PR": 2, "C": 4, "D": 2, "probs": dp(keep["probs"]), "n_probs": 2, "out": dp(keep["out"])}
    a.update(change)
    return [a[k] for k in ("device", "draws", "rows", "PR", "C", "D", "probs", "n_probs", "out")], keep


@pytest.mark.parametrize("change,why", [
    (dict(draws=None), b"null argument"), (dict(probs=None), b"null argument"), (dict(out=None), b"null argument"),
    (dict(n_probs=0), b"bad shape"), (dict(n_probs=-2), b"bad shape"), (dict(rows=0), b"bad shape"), (dict(PR=0), b"bad shape"), (dict(C=0), b"bad shape"),
    (dict(D=0), b"bad shape"), (dict(D=3), b"bad shape"), (dict(D=65536, C=65536), b"bad shape"),
    (dict(rows=2 ** 31, C=4), b"more than 2^31 - 1 values"), (dict(rows=2 ** 30, C=4, D=1), b"more than 2^31 - 1 values"),
    (dict(rows=1, C=2, D=2), b"fewer than 2 values"), (dict(rows=1, C=1, D=1), b"fewer than 2 values")])
def test_selftest_call_refuses_bad_arguments_before_any_device_call(change, why):
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_hpd_check(*args) == -1, change      # (-2 would be the device that does not exist)
    assert CHECK.encode() in T.amwg_last_error() and why in T.amwg_last_error(), T.amwg_last_error()


@pytest.mark.parametrize("change", [dict(), dict(n_probs=1), dict(rows=1, C=4, D=2), dict(rows=2, C=1, D=1), dict(D=1), dict(D=4)])
def test_a_valid_call_reaches_the_device_that_does_not_exist(change):
    """the control of the test above: with nothing to refuse, the same call gets as far as opening device 99 and fails THERE (AMWG_EHIP)"""
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_hpd_check(*args) == -2, T.amwg_last_error()


def test_the_scratch_budget_is_set_without_a_device_and_restored():
    T = amwg_ctypes.selftest_lib()
    assert T.amwg_hpd_limits(NO_DEVICE, -1, None, None) == -1 and b"amwg_hpd_limits" in T.amwg_last_error()
    keys, before = amwg_ctypes.hpd_limits(4096, lds=False)
    assert keys is None and before == 256 << 20      # the default the header states
    assert amwg_ctypes.hpd_limits(0, lds=False)[1] == 4096
    assert amwg_ctypes.hpd_limits(0, lds=False)[1] == 256 << 20
    assert T.amwg_hpd_limits(NO_DEVICE, 0, C.byref(C.c_int64()), None) == -2      # asking for the LDS size opens the device


# ---- the host reference on hand values

PROBS = (1e-9, 0.05, 0.29, 0.5, 0.9, 0.95, 1 - 1e-12)


def test_two_draws_give_min_and_max_for_every_p():
    for x in ([3.0, -1.0], [-1.0, 3.0], [0.0, -0.0], [5.0, 5.0]):
        for p in PROBS:
            lo, hi, g, k, i = hr.hpd(x, p)
            assert (g, k, i) == (1, 1, 0)
            assert hr.pair_bytes((lo, hi)) == hr.values(np.sort(hr.keys(x))).tobytes(), (x, p)


def test_all_widths_tie_on_an_even_grid_and_the_first_wins():
    x = np.arange(100, dtype=np.float64)[::-1] * 0.25      # exact arithmetic: every width of a given g is the same double
    for p in (0.05, 0.5, 0.9, 0.95):
        lo, hi, g, k, i = hr.hpd(x, p)
        assert i == 0 and lo == 0.0 and hi == 0.25 * g and g == int(p * 100) and k == 100 - g


def test_a_constant_slice_and_binary_slices():
    for p in PROBS:
        assert hr.hpd(np.full(37, 2.5), p)[:2] == (2.5, 2.5) and hr.hpd(np.full(37, 2.5), p)[4] == 0
    x = np.array([0.0] * 30 + [1.0] * 70)      # sorted: 30 zeros, 70 ones
    assert hr.hpd(x, 0.5)[:5] == (1.0, 1.0, 50, 50, 30)      # the first i with x_(i) = 1: width 0
    assert hr.hpd(x, 0.69)[:5] == (1.0, 1.0, 69, 31, 30)     # 69 ones apart: ranks 30 and 99
    assert hr.hpd(x, 0.9)[:5] == (0.0, 1.0, 90, 10, 0)       # every window of 91 spans both values: all widths 1, the first wins
    y = 1.0 - x      # 70 zeros, 30 ones
    assert hr.hpd(y, 0.5)[:5] == (0.0, 0.0, 50, 50, 0)
    assert hr.hpd(y, 0.9)[:5] == (0.0, 1.0, 90, 10, 0)


def test_the_product_just_below_an_integer_floors_down():
    assert 0.29 * 100.0 < 29.0 and hr.rank_g(0.29, 100) == 28      # the rule is what the fp64 product says
    x = np.random.default_rng(5).standard_normal(100)
    lo, hi, g, k, i = hr.hpd(x, 0.29)
    s = np.sort(x)
    assert (g, k) == (28, 72) and (lo, hi) == (s[i], s[i + 28]) and i == int(np.argmin(s[28:] - s[:72]))


def test_the_clamps_at_both_ends():
    x = np.random.default_rng(6).standard_normal(50)
    s = np.sort(x)
    lo, hi, g, k, i = hr.hpd(x, 1e-9)      # floor(5e-8) = 0 -> g = 1: the closest pair of neighbours
    assert (g, k) == (1, 49) and i == int(np.argmin(s[1:] - s[:-1])) and (lo, hi) == (s[i], s[i + 1])
    lo, hi, g, k, i = hr.hpd(x, 1 - 1e-12)      # floor(50 - 5e-11) = 49 = N - 1: one window, the range
    assert (g, k, i) == (49, 1, 0) and (lo, hi) == (s[0], s[-1])
    assert hr.rank_g(1 - 2.0 ** -53, 50) == 49
    for bad in (0.0, 1.0, -0.5, 1.5, math.nan, math.inf):
        r = hr.hpd(x, bad)
        assert math.isnan(r[0]) and math.isnan(r[1]) and hr.rank_g(bad, 50) is None
        r = hr.hpd_tails(x, bad)
        assert math.isnan(r[0]) and math.isnan(r[1])


def test_one_non_finite_draw_gives_nan_for_every_p():
    x = np.random.default_rng(7).standard_normal(40)
    for bad in (math.nan, math.inf, -math.inf):
        for at in (0, 17, 39):
            y = x.copy()
            y[at] = bad
            for p in PROBS:
                for f in (hr.hpd, hr.hpd_tails):
                    r = f(y, p)
                    assert math.isnan(r[0]) and math.isnan(r[1]), (bad, at, p)


def test_negative_zero_sorts_before_positive_zero():
    x = np.array([0.0, -0.0, 0.0, -0.0, 1.0])
    lo, hi, g, k, i = hr.hpd(x, 0.5)      # g = 2: sorted -0 -0 +0 +0 1; widths 0, 0, 1: i* = 0 -> (-0, +0)
    assert (g, i) == (2, 0) and math.copysign(1.0, lo) == -1.0 and math.copysign(1.0, hi) == 1.0
    assert hr.pair_bytes(hr.hpd_tails(x, 0.5)) == hr.pair_bytes((lo, hi))


@pytest.mark.parametrize("kind", hr.KINDS)
def test_the_two_tails_equal_the_full_sort_as_bytes(kind):
    """1000 small arrays of each of the four kinds, at a random p and at the probabilities people use: the same bytes, g, k and i*"""
    rng = np.random.default_rng([20261020, hr.KINDS.index(kind)])
    for trial in range(1000):
        n = int(rng.integers(2, 200))
        x = hr.draws_of(kind, n, rng)
        for p in (float(rng.random()), (0.5, 0.9, 0.95, 0.29, 1e-9, 1 - 1e-12)[trial % 6]):
            if not 0.0 < p < 1.0:
                continue
            a, b = hr.hpd(x, p), hr.hpd_tails(x, p)
            assert hr.pair_bytes(a) == hr.pair_bytes(b) and a[2:] == b[2:], (kind, n, p, a, b)
