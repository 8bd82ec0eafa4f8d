"""Posterior histograms over caller-given edges (amwg_last_sample_dataset_histogram, amwg_set_histogram, amwg_histogram_info), the part that needs no GPU: the calls
are declared in the header, mirrored in the ctypes binding and exported by the product library; the entry point that drives the kernel on a caller's array
(amwg_histogram_check) is in the test library only; what either refuses for its arguments alone is refused BEFORE a device is opened -- on a device number that does
not exist -- with the call's name in amwg_last_error(); and interval_brackets(), a pure host function, against a brute-force restatement and against np.quantile.
tests/README.histogram.md says what each test pins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amwg_ctypes
from histogram_reference import counts_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["amwg_last_sample_dataset_histogram", "amwg_set_histogram", "amwg_histogram_info"]
CHECK = "amwg_histogram_check"
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP (-2), not AMWG_EINVAL (-1)


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_calls_are_declared_mirrored_and_exported():
    for call in CALLS:
        assert call in declared("amwg.h") and call in amwg_ctypes.EXPORTS, call
        assert getattr(amwg_ctypes.lib(), call) is not None
    for method in ("set_histogram", "dataset_histogram", "histogram_info"):
        assert callable(getattr(amwg_ctypes.Sampler, method))
    assert callable(amwg_ctypes.interval_brackets)


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and callable(amwg_ctypes.histogram_check)
    assert not hasattr(amwg_ctypes.lib(), CHECK)
    for internal in ("amwg_histogram_launch", "amwg_histogram_shape", "amwg_histogram_edges_check", "amwg_histogram_grid", "amwg_histogram_armed", "amwg_histogram_begin",
                     "amwg_histogram_forget"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_the_histogram_sources_are_not_among_the_step_kernels_sources():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    assert "amwg_histogram.hip" not in build_id.KERNEL_FILES and "amwg_histogram.h" not in build_id.KERNEL_FILES
    sampler_h = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_sampler.h")).read()
    assert "histogram" not in sampler_h.lower()      # the armed histogram lives beside the handle, not in it


def test_sampler_calls_refuse_bad_arguments_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: each of these calls is refused for another argument first
    edges, counts = (C.c_double * 8)(*range(8)), (C.c_uint64 * 64)()
    name = b"amwg_last_sample_dataset_histogram"
    for args, why in (((None, edges, 4, counts), b"null sampler"), ((fake, edges, 4, None), b"null counts"), ((fake, edges, 0, counts), b"0 bins"),
                      ((fake, edges, 4097, counts), b"4097 bins"), ((fake, edges, -1, counts), b"-1 bins")):
        assert L.amwg_last_sample_dataset_histogram(*args) == -1, why
        assert name in L.amwg_last_error() and why in L.amwg_last_error(), L.amwg_last_error()
    for args, why in (((None, edges, 4), b"null sampler"), ((fake, None, 4), b"null edges"), ((fake, edges, 0), b"0 bins"), ((fake, edges, 4097), b"4097 bins")):
        assert L.amwg_set_histogram(*args) == -1, why
        assert b"amwg_set_histogram" in L.amwg_last_error() and why in L.amwg_last_error(), L.amwg_last_error()
    b = C.c_int32()
    assert L.amwg_histogram_info(None, C.byref(b), None) == -1
    assert b"amwg_histogram_info" in L.amwg_last_error()


def check_args(**change):
    """the arguments of amwg_histogram_check for a valid call of 2 rows x 1 value x 4 chains in 2 datasets under 3 bins, with `change` applied"""
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    keep = {"draws": np.zeros(8), "edges": np.array([0.0, 1.0, 2.0, 3.0]), "counts": np.zeros(2 * 6, dtype=np.uint64)}
    a = {"draws": dp(keep["draws"]), "rows": 2, "PR": 1, "C": 4, "D": 2, "edges": dp(keep["edges"]), "bins": 3, "window_rows": 0,
         "counts": keep["counts"].ctypes.data_as(C.POINTER(C.c_uint64)), "device": NO_DEVICE}
    for k, v in change.items():
        if k == "edge_values":
            keep["edges"] = np.array(v, dtype=np.float64)
            a["edges"] = dp(keep["edges"])
        else:
            a[k] = v
    order = ("draws", "rows", "PR", "C", "D", "edges", "bins", "window_rows", "counts", "device")
    return [a[k] for k in order], keep


@pytest.mark.parametrize("change,why", [
    (dict(draws=None), b"null argument"), (dict(edges=None), b"null argument"), (dict(counts=None), b"null argument"),
    (dict(bins=0), b"0 bins"), (dict(bins=4097), b"4097 bins"), (dict(bins=-3), b"-3 bins"),
    (dict(edge_values=[0.0, 2.0, 1.0, 3.0]), b"not strictly ascending"), (dict(edge_values=[0.0, 1.0, 1.0, 3.0]), b"not strictly ascending"),
    (dict(edge_values=[3.0, 2.0, 1.0, 0.0]), b"not strictly ascending"), (dict(edge_values=[0.0, float("nan"), 2.0, 3.0]), b"not finite"),
    (dict(edge_values=[0.0, 1.0, 2.0, float("inf")]), b"not finite"), (dict(edge_values=[float("-inf"), 1.0, 2.0, 3.0]), b"not finite"),
    (dict(rows=0), b"bad shape"), (dict(PR=0), b"bad shape"), (dict(C=0), b"bad shape"), (dict(D=0), b"bad shape"), (dict(D=3), b"bad shape"),
    (dict(window_rows=-1), b"bad shape")])
def test_selftest_call_refuses_bad_arguments_before_any_device_call(change, why):
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args(**change)
    assert T.amwg_histogram_check(*args) == -1, change      # (-2 would be the device that does not exist)
    assert CHECK.encode() in T.amwg_last_error() and why in T.amwg_last_error(), T.amwg_last_error()


def test_a_valid_call_reaches_the_device_that_does_not_exist():
    """the control of the test above: with nothing to refuse, the same call gets as far as opening device 99 and fails THERE (AMWG_EHIP)"""
    T = amwg_ctypes.selftest_lib()
    args, keep = check_args()
    assert T.amwg_histogram_check(*args) == -2, T.amwg_last_error()


# ---- interval_brackets

def brute_brackets(counts, edges, probs):
    """the definition, restated on an explicit sorted list of bin labels: -1 under, 0 .. bins - 1, bins over"""
    counts = [int(v) for v in counts]
    bins = len(edges) - 1
    labels = [-1] * counts[bins] + [i for i in range(bins) for _ in range(counts[i])] + [bins] * counts[bins + 1]
    n = len(labels)
    out = []
    for q in probs:
        if counts[bins + 2] > 0 or n == 0 or not (0.0 <= q <= 1.0):
            out.append((np.nan, np.nan))
            continue
        h = (n - 1) * q
        r0 = int(np.floor(h))
        r1 = min(r0 + 1, n - 1)
        a, b = labels[r0], labels[r1]
        out.append((-np.inf if a < 0 else edges[a], np.inf if b >= bins else edges[b + 1]))
    return np.array(out, dtype=np.float64).reshape(len(probs), 2)


EDGES = [0.0, 1.0, 2.5, 4.0, 8.0]      # 4 bins
PROBS = [0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0]


@pytest.mark.parametrize("counts", [
    [3, 4, 2, 1, 0, 0, 0],        # all in real bins
    [0, 0, 10, 0, 0, 0, 0],       # both ranks in one bin, empty bins around it
    [1, 1, 0, 0, 0, 0, 0],        # ranks in neighbouring bins (n = 2: every q in (0, 1) interpolates between the two)
    [5, 0, 0, 5, 0, 0, 0],        # ranks in bins far apart: q = 0.5 straddles the empty middle
    [2, 2, 2, 2, 6, 0, 0],        # ranks in under
    [2, 2, 2, 2, 0, 6, 0],        # ranks in over
    [0, 0, 0, 0, 4, 0, 0],        # everything under
    [0, 0, 0, 0, 0, 4, 0],        # everything over
    [1, 0, 0, 0, 3, 3, 0],        # under and over around one value
    [0, 1, 0, 0, 0, 0, 0],        # n = 1
    [0, 0, 0, 0, 1, 0, 0],        # n = 1, under
    [0, 0, 0, 0, 0, 0, 0],        # n = 0
    [3, 4, 2, 1, 0, 0, 1],        # a NaN was counted
    [10 ** 15, 2 * 10 ** 15, 7, 0, 5, 0, 0]])      # counts beyond 2^32
def test_interval_brackets_against_the_definition(counts):
    got = amwg_ctypes.interval_brackets(np.array(counts, dtype=np.uint64), EDGES, PROBS + [-0.1, 1.5, float("nan")])
    if sum(counts) < 10 ** 6:
        want = brute_brackets(counts, EDGES, PROBS + [-0.1, 1.5, float("nan")])
        assert np.array_equal(got, want, equal_nan=True), (counts, got, want)
    assert np.all(np.isnan(got[-3:]))
    if counts[6] > 0 or sum(counts[:6]) == 0:
        assert np.all(np.isnan(got))


def test_interval_brackets_hand_values():
    ib = amwg_ctypes.interval_brackets
    inf = np.inf
    assert ib([3, 4, 2, 1, 0, 0, 0], EDGES, [0.0, 0.5, 1.0]).tolist() == [[0.0, 1.0], [1.0, 2.5], [4.0, 8.0]]      # n = 10: ranks (0, 1), (4, 5), (9, 9)
    assert ib([1, 1, 0, 0, 0, 0, 0], EDGES, [0.5]).tolist() == [[0.0, 2.5]]                                        # ranks 0 and 1 in neighbouring bins
    assert ib([5, 0, 0, 5, 0, 0, 0], EDGES, [0.5]).tolist() == [[0.0, 8.0]]                                        # rank 4 in bin 0, rank 5 in bin 3
    assert ib([0, 1, 0, 0, 0, 0, 0], EDGES, [0.0, 0.3, 1.0]).tolist() == [[1.0, 2.5]] * 3                          # n = 1
    assert ib([2, 2, 2, 2, 6, 0, 0], EDGES, [0.0, 1.0]).tolist() == [[-inf, 0.0], [4.0, 8.0]]                      # both ranks under: hi = edges[0]
    assert ib([2, 2, 2, 2, 0, 6, 0], EDGES, [0.0, 1.0]).tolist() == [[0.0, 1.0], [8.0, inf]]                       # both ranks over: lo = edges[bins]
    assert ib([0, 0, 0, 0, 1, 1, 0], EDGES, [0.5]).tolist() == [[-inf, inf]]
    big = ib([10 ** 15, 2 * 10 ** 15, 7, 0, 5, 0, 0], EDGES, [0.0, 0.2, 0.5, 1.0]).tolist()
    assert big == [[-inf, 0.0], [0.0, 1.0], [1.0, 2.5], [2.5, 4.0]]


@pytest.mark.parametrize("n", [1, 2, 3, 10, 101, 1000])
@pytest.mark.parametrize("kind", ["normal", "ties_on_edges", "few_values", "with_under_and_over"])
def test_np_quantile_lies_in_the_bracket(n, kind):
    rng = np.random.default_rng([20261019, n, len(kind)])
    edges = np.linspace(-3.0, 3.0, 25)
    if kind == "normal":
        x = rng.standard_normal(n).clip(-2.99, 2.99)
    elif kind == "ties_on_edges":
        x = rng.choice(edges[:-1], size=n)      # every value exactly on an edge: it belongs to the bin that STARTS there
    elif kind == "few_values":
        x = rng.choice([-1.0, 0.1, 0.1000001, 2.0], size=n)
    else:
        x = 2.5 * rng.standard_normal(n)
    c = counts_of(x, edges)
    assert int(c.sum()) == n
    probs = [0.0, 0.025, 0.1, 0.5, 0.9, 0.975, 1.0] + rng.random(20).tolist()
    br = amwg_ctypes.interval_brackets(c, edges, probs)
    qs = np.quantile(x, probs)      # (numpy's default is R's type 7)
    for q, (lo, hi), v in zip(probs, br, qs):
        assert lo <= v <= hi, (kind, n, q, lo, v, hi)
    if kind in ("normal", "ties_on_edges"):
        assert c[-3] == c[-2] == 0 and np.all(np.isfinite(br))
