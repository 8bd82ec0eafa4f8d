"""Per-dataset quantiles (amwg_last_sample_dataset_quantiles), the part that needs no GPU: the call is declared in the header, mirrored in the ctypes binding
and exported by the product library; the entry point that drives its kernel on a caller's array (amwg_dataset_quantiles_check) is in the test library only;
and what either refuses for its arguments alone is refused BEFORE a device is opened, with the call's name in amwg_last_error()."""
import ctypes as C
import os
import re

import amwg_ctypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "amwg_last_sample_dataset_quantiles"
CHECK = "amwg_dataset_quantiles_check"


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_call_is_declared_mirrored_and_exported():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.lib(), CALL) is not None
    assert callable(amwg_ctypes.Sampler.dataset_quantiles)
    hdr = open(os.path.join(ROOT, "include", "amwg.h")).read()
    assert "are not provided" not in hdr


def test_selftest_call_is_in_the_test_library_only():
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None
    assert not hasattr(amwg_ctypes.lib(), CHECK)
    assert not hasattr(amwg_ctypes.lib(), "amwg_dataset_quantiles_launch") and not hasattr(amwg_ctypes.selftest_lib(), "amwg_dataset_quantiles_launch")      # (internal)


def test_bad_arguments_are_refused_before_any_device_call():
    L = amwg_ctypes.lib()
    probs, out = (C.c_double * 1)(0.5), (C.c_double * 4)()
    fake = C.c_void_p(8)      # never dereferenced: each of these calls is refused for another argument first
    for args in ((fake, None, 1, out), (fake, probs, 1, None), (fake, probs, 0, out), (fake, probs, -2, out), (None, probs, 1, out)):
        assert L.amwg_last_sample_dataset_quantiles(*args) == -1
        assert CALL.encode() in L.amwg_last_error()


def test_selftest_call_refuses_bad_arguments_before_any_device_call():
    T = amwg_ctypes.selftest_lib()
    draws, probs, out = (C.c_double * 4)(), (C.c_double * 1)(0.5), (C.c_double * 4)()
    for args in ((0, None, 1, 1, 4, 1, probs, 1, out), (0, draws, 1, 1, 4, 1, None, 1, out), (0, draws, 1, 1, 4, 1, probs, 1, None),
                 (0, draws, 1, 1, 4, 1, probs, 0, out), (0, draws, 0, 1, 4, 1, probs, 1, out), (0, draws, 1, 0, 4, 1, probs, 1, out),
                 (0, draws, 1, 1, 0, 1, probs, 1, out), (0, draws, 1, 1, 4, 0, probs, 1, out)):
        assert T.amwg_dataset_quantiles_check(*args) == -1
        assert CHECK.encode() in T.amwg_last_error()


def test_shapes_the_kernel_cannot_serve_are_refused_from_the_shape_alone():
    """More than 2^31 - 1 values per dataset and component, or datasets that do not divide the chains: refused before a device is opened and before the
    array is touched (the array handed over is tiny)."""
    T = amwg_ctypes.selftest_lib()
    small, probs, out = (C.c_double * 8)(), (C.c_double * 1)(0.5), (C.c_double * 8)()
    assert T.amwg_dataset_quantiles_check(0, small, 1 << 31, 1, 1, 1, probs, 1, out) == -1
    assert b"2^31 - 1" in T.amwg_last_error() and CHECK.encode() in T.amwg_last_error()
    assert T.amwg_dataset_quantiles_check(0, small, 1 << 20, 1, 1 << 12, 2, probs, 1, out) == -1      # 2^20 rows x 2^11 chains per dataset = 2^31
    assert b"2^31 - 1" in T.amwg_last_error()
    assert T.amwg_dataset_quantiles_check(0, small, 2, 1, 4, 3, probs, 1, out) == -1      # 3 datasets do not divide 4 chains
    assert b"bad shape" in T.amwg_last_error()
