"""Summaries without stored draws (amwg_sample_summarize), the part that needs no GPU: the three calls are declared in the header, mirrored in the ctypes binding
and exported by the product library; the entry point that drives the fold on a caller's array (amwg_fold_check) is in the test library only; and what either refuses
for its arguments alone is refused BEFORE a device is opened, with the call's name in amwg_last_error()."""
import ctypes as C
import os
import re

import amwg_ctypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["amwg_sample_summarize_async", "amwg_sample_summarize", "amwg_summary_info"]
CHECK = "amwg_fold_check"


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_calls_are_declared_mirrored_and_exported():
    for call in CALLS:
        assert call in declared("amwg.h") and call in amwg_ctypes.EXPORTS, call
        assert getattr(amwg_ctypes.lib(), call) is not None
    assert callable(amwg_ctypes.Sampler.summarize) and callable(amwg_ctypes.Sampler.summary_info)


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and callable(amwg_ctypes.fold_check)
    assert not hasattr(amwg_ctypes.lib(), CHECK)
    for internal in ("amwg_fold_window", "amwg_fold_halves", "amwg_fold_moments", "amwg_chain_halves", "amwg_summarised", "amwg_summary_of", "amwg_refuse_summarised"):
        assert not hasattr(amwg_ctypes.lib(), internal) and not hasattr(amwg_ctypes.selftest_lib(), internal), internal


def test_bad_arguments_are_refused_before_any_device_call():
    L = amwg_ctypes.lib()
    fake = C.c_void_p(8)      # never dereferenced: each of these calls is refused for another argument first
    for fn in (L.amwg_sample_summarize, L.amwg_sample_summarize_async):
        for args, why in (((None, 10, 1, 0), b"null sampler"), ((fake, -1, 1, 0), b"n < 0"), ((fake, 10, 0, 0), b"thin < 1"), ((fake, 10, -3, 0), b"thin < 1"),
                          ((fake, 10, 1, -1), b"window_rows < 0")):
            assert fn(*args) == -1
            assert b"amwg_sample_summarize" in L.amwg_last_error() and why in L.amwg_last_error(), L.amwg_last_error()
    r = C.c_int64()
    assert L.amwg_summary_info(None, C.byref(r), None, None, None, None) == -1
    assert b"amwg_summary_info" in L.amwg_last_error()


def test_selftest_call_refuses_bad_arguments_before_any_device_call():
    T = amwg_ctypes.selftest_lib()
    draws, out = (C.c_double * 8)(), (C.c_double * 32)()
    good = [0, draws, 2, 1, 4, 2, 1, out, out, out, out]      # device, draws, rows, PR, C, D, window_rows, halves_folded, halves_direct, mean, sd
    for at, bad in ((1, None), (7, None), (8, None), (9, None), (10, None), (2, 0), (2, -1), (3, 0), (4, 0), (5, 0), (5, 3), (6, 0), (6, -2)):
        args = list(good)
        args[at] = bad
        assert T.amwg_fold_check(*args) == -1, (at, bad)
        assert CHECK.encode() in T.amwg_last_error()
    assert b"bad shape" in T.amwg_last_error()      # (the last one: window_rows < 1)
