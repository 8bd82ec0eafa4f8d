"""The references of the on-device summaries (tests/summary_reference.py) held to each other, without a GPU; tests/test_gpu_summary_arrays.py holds the kernels to them.

(a) the kernels' order restated in numpy float64 (kernel_order, kernel_order_moments) against exact rational arithmetic, on every pattern x shape: inside the caps of
    tests/README.summaries.md -- the check that the caps are fair to the restated order ALONE, before any device is asked to meet them -- and exactly the NaNs
    the library's rule gives on degenerate columns.  The largest |error| / cap per quantity is printed (pytest -s).
(b) the torch twin (bayes.js_amd/shard.py pooled_convergence) on the same arrays, one dataset at a time and over all the chains: inside the same caps; on the two
    W = 0 patterns its present answers (NaN / +inf), which differ from the library's, are pinned as they are.
(c) what amwg_summaries_check refuses, by message, before a device is opened."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import amwg_ctypes
import summary_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = "amwg_summaries_check"
WORST = {}


def ids(shape):
    return "%dx%d" % shape


def figures(c):
    """(quantity, the restated order's figure, exact) of every segment of a case"""
    for d in range(R.D):
        for p in range(R.PR):
            e = c.exact[d][p]
            yield (d, p), [("rhat", c.rhat[d, p], e), ("ess", c.ess[d, p], e), ("mean", c.mean[d, p], e), ("sd", c.sd[d, p], e)]


# ---- (a)

@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("name", R.FINITE)
def test_restated_order_stays_inside_the_cap_on_finite_patterns(name, shape):
    rows, cpd = shape
    c = R.case(name, rows, cpd)
    for (d, p), got in figures(c):
        e = c.exact[d][p]
        if name != "integers":      # (small integers at the smallest shapes may give a constant half-chain set or equal chain means: NaN on both sides, held below)
            assert math.isfinite(e["rhat"]) and math.isfinite(e["ess"]), (name, shape, d, p, e)
        R.held_to_exact(got, rows // 2, cpd, rows * cpd, "%s %dx%d (d %d, p %d)" % (name, rows, cpd, d, p), WORST)
    # a quarter of the cap is the most the reference's own order may use: the device has to fit into the same cap (tests/README.summaries.md)
    for key, (ratio, label) in sorted(WORST.items()):
        print("largest |restated - exact| / cap so far: %-4s %.4f  at %s" % (key, ratio, label))
        assert ratio <= 0.25, (key, ratio, label)


def test_patterns_are_what_their_names_say():
    """R-hat far from 1 where the pattern means it, so that no case can quietly be a healthy one"""
    for rows, cpd in R.SHAPES:
        camps = [R.case("two_camps", rows, cpd).exact[d][p]["rhat"] for d in range(R.D) for p in range(R.PR)]
        assert min(camps) > 2.5, (rows, cpd, camps)
        if rows >= 8:
            trend = [R.case("trend", rows, cpd).exact[d][p]["rhat"] for d in range(R.D) for p in range(R.PR)]
            assert min(trend) > 1.3, (rows, cpd, trend)      # the halves differ by 2.5 sd: an unsplit R-hat would sit near 1
        healthy = [R.case("healthy", rows, cpd).exact[d][p]["rhat"] for d in range(R.D) for p in range(R.PR)]
        if rows * cpd >= 500:
            assert max(healthy) < 1.2, (rows, cpd, healthy)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_degenerate_patterns_give_exactly_the_documented_nans(shape):
    rows, cpd = shape
    for name in R.W_ZERO + R.NON_FINITE:
        c = R.case(name, rows, cpd)
        for (d, p), got in figures(c):
            e = c.exact[d][p]
            assert math.isnan(e["rhat"]) and math.isnan(c.rhat[d, p]), (name, shape, d, p)      # W = 0, or a used draw that is not finite
            if name == "constant_chains_that_differ":      # the chain means vary: ess is a number (var_plus = B / n), and is held to the cap
                assert math.isfinite(e["ess"]) and e["ess"] > 0
            else:
                assert math.isnan(e["ess"]) and math.isnan(c.ess[d, p]), (name, shape, d, p)
            if name in R.W_ZERO:
                R.held_to_exact(got, rows // 2, cpd, rows * cpd, "%s %dx%d (d %d, p %d)" % (name, rows, cpd, d, p), {})
            else:
                assert math.isnan(c.sd[d, p]) and math.isnan(e["sd"])
                assert (math.isnan(c.mean[d, p]) and math.isnan(e["mean"])) if name == "one_nan" else (c.mean[d, p] == math.inf == e["mean"])
        if name == "all_equal":
            assert np.all(c.sd == 0.0)


def test_an_odd_last_row_is_ignored_by_the_diagnostics_and_used_by_the_moments():
    c = R.case("healthy", 5, 3)
    x = R.segment(c.draws, 1, 1).copy()
    a, b = R.kernel_order(x), R.kernel_order(x[:4])
    assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
    e5, e4 = R.exact(x), R.exact(x[:4])
    assert e5["rhat"] == e4["rhat"] and e5["ess"] == e4["ess"] and e5["mean"] != e4["mean"]
    x[4, 0] = np.nan      # a NaN in the ignored row: the diagnostics stay numbers, the moments do not
    e = R.exact(x)
    assert e["rhat"] == e4["rhat"] and math.isnan(e["mean"]) and math.isfinite(R.kernel_order(x)[0])


# ---- (b)

def shard_figures(draws):
    import torch
    import shard
    r, e = shard.pooled_convergence(None, torch.from_numpy(np.array(draws, order="C")))
    return r.numpy(), e.numpy()


def shard_held_to_exact(r, e, ref, half, cpd, n, label, worst):
    """a figure whose exact value is NaN by the library's rule (a zero variance in the denominator: `integers` at the smallest shapes) is a division by zero in
    shard.py: anything but a finite number.  Every other figure is held to the cap."""
    got = []
    for key, g in (("rhat", r), ("ess", e)):
        if math.isnan(ref[key]):
            assert not math.isfinite(g), (label, key, g)
        else:
            got.append((key, g, ref))
    R.held_to_exact(got, half, cpd, n, label, worst)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("name", R.FINITE)
def test_torch_twin_stays_inside_the_cap(name, shape):
    rows, cpd = shape
    c = R.case(name, rows, cpd)
    worst = {}
    for d in range(R.D):
        r, e = shard_figures(c.draws[:, :, d * cpd:(d + 1) * cpd])
        for p in range(R.PR):
            shard_held_to_exact(r[p], e[p], c.exact[d][p], rows // 2, cpd, rows * cpd, "shard %s %dx%d (d %d, p %d)" % (name, rows, cpd, d, p), worst)
    r, e = shard_figures(c.draws)
    for p in range(R.PR):
        shard_held_to_exact(r[p], e[p], c.pooled[p], rows // 2, R.D * cpd, rows * R.D * cpd, "shard %s %dx%d (pooled, p %d)" % (name, rows, cpd, p), worst)
    print("shard.py, largest |error| / cap:", worst)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_torch_twin_on_degenerate_columns_as_it_is_today(shape):
    """W = 0: the library answers NaN; shard.py divides: sqrt(0 / 0) = NaN where B = 0 too, sqrt(B / 0) = +inf where the constant chains differ.  Pinned, not endorsed:
    shard.py is not changed here (bench.py imports it)."""
    rows, cpd = shape
    for d in range(R.D):
        r, e = shard_figures(R.case("all_equal", rows, cpd).draws[:, :, d * cpd:(d + 1) * cpd])
        assert np.all(np.isnan(r)) and np.all(np.isnan(e)), (shape, d, r, e)
        c = R.case("constant_chains_that_differ", rows, cpd)
        r, e = shard_figures(c.draws[:, :, d * cpd:(d + 1) * cpd])
        assert np.all(r == np.inf), (shape, d, r)
        for p in range(R.PR):
            R.held_to_exact([("ess", e[p], c.exact[d][p])], rows // 2, cpd, rows * cpd, "shard constant_chains_that_differ %dx%d (d %d, p %d)" % (rows, cpd, d, p), {})
        for name in R.NON_FINITE:
            r, e = shard_figures(R.case(name, rows, cpd).draws[:, :, d * cpd:(d + 1) * cpd])
            assert np.all(np.isnan(r)) and np.all(np.isnan(e)), (name, shape, d, r, e)


# ---- (c)

def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and not hasattr(amwg_ctypes.lib(), CHECK)
    for internal in ("amwg_moments_launch", "amwg_dataset_diagnostics_launch", "amwg_pooled_diagnostics", "amwg_diagnostics_refusal", "amwg_chain_halves"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal)
    assert callable(amwg_ctypes.summaries_check)


def test_refusals_come_before_any_device_call_with_the_products_words():
    T = amwg_ctypes.selftest_lib()
    x, o = (C.c_double * 64)(), [(C.c_double * 16)() for _ in range(6)]

    def refused(device, draws, rows, pr, chains, datasets, window_rows, outs=o):
        assert T.amwg_summaries_check(device, draws, rows, pr, chains, datasets, window_rows, *outs) == -1
        msg = T.amwg_last_error().decode()
        assert msg.startswith(CHECK + ": "), msg
        return msg
    # (device 1 000 000 does not exist: a call that reached use_device would say so instead)
    assert "null argument" in refused(1000000, None, 4, 1, 4, 1, 0)
    for k in range(6):
        assert "null argument" in refused(1000000, x, 4, 1, 4, 1, 0, o[:k] + [None] + o[k + 1:])
    for rows, pr, chains, datasets, window_rows in ((0, 1, 4, 1, 0), (4, 0, 4, 1, 0), (4, 65536, 4, 1, 0), (4, 1, 0, 1, 0), (4, 1, 4, 0, 0), (4, 1, 4, 65536, 0), (4, 1, 4, 3, 0), (4, 1, 4, 1, -1)):
        assert "bad shape" in refused(1000000, x, rows, pr, chains, datasets, window_rows)
    # the product's refusal, word for word (amwg_last_sample_dataset_diagnostics): fewer than 4 kept draws, fewer than 2 chains per dataset
    for rows, chains, datasets in ((3, 4, 1), (1, 4, 2), (4, 1, 1), (4, 3, 3), (8, 2, 2)):
        assert refused(1000000, x, rows, 1, chains, datasets, 0) == CHECK + ": needs a sample() of >= 4 kept draws on >= 2 chains per dataset"
    assert "array too large" in refused(1000000, x, 1 << 40, 1 << 10, 1 << 20, 1, 0)
    with pytest.raises(amwg_ctypes.AmwgError, match="needs a sample\\(\\) of >= 4 kept draws on >= 2 chains per dataset"):
        amwg_ctypes.summaries_check(np.zeros((3, 2, 4)), 2)


def test_the_header_documents_the_degenerate_columns():
    hdr = open(os.path.join(ROOT, "include", "amwg.h")).read()
    at = hdr.index("int amwg_last_sample_diagnostics(")
    doc = hdr[hdr.rindex("/*", 0, at):at]
    assert "NaN when W = 0" in doc and "not finite" in doc and "chain means do not" in doc and "odd number of kept draws the last one is ignored" in doc
