"""WAIC without stored draws (amwg_set_waic, amwg_waic_info; amwg_waic_fold_check in the test library), the part that needs no GPU: the calls are declared,
mirrored and exported; what they refuse for their arguments alone is refused before a device is opened, with the call's name; a closure's pointwise program
compiles for gfx950 with the fold's entry in its code object.  tests/README.waic_fold.md says what each test pins."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import amwg_ctypes as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP, not AMWG_EINVAL
X3 = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_calls_are_declared_mirrored_and_exported():
    for call in ("amwg_set_waic", "amwg_waic_info"):
        assert call in declared("amwg.h") and call in A.EXPORTS and getattr(A.lib(), call) is not None
    check = "amwg_waic_fold_check"
    assert check in declared("amwg_selftest.h") and check in A.SELFTEST_EXPORTS and check not in A.EXPORTS
    assert getattr(A.selftest_lib(), check) is not None and not hasattr(A.lib(), check) and callable(A.waic_fold_check)
    for method in ("set_waic", "waic_info"):
        assert callable(getattr(A.Sampler, method))
    for internal in ("amwg_waic_fold_begin", "amwg_waic_fold_window", "amwg_waic_fold_finish", "amwg_waic_begin", "amwg_waic_armed"):
        assert not hasattr(A.lib(), internal), internal
    header = " ".join(re.sub(r"(?m)^ \* ", " ", open(os.path.join(ROOT, "include", "amwg.h")).read()).split())
    for words in ("NOT promised to equal the stored run's bytes", "(rows, C / D) and window_rows", "THE SAME BOUNDS hold", "amwg_last_sample_dataset_loo keeps refusing"):
        assert words in header, words
    assert "WAIC after amwg_sample_summarize" not in header


def test_null_arguments_are_refused_before_any_device_call():
    L = A.lib()
    for on in (0, 1):
        assert L.amwg_set_waic(None, on) == -1 and b"amwg_set_waic" in L.amwg_last_error()
    armed, n = C.c_int32(), C.c_size_t()
    assert L.amwg_waic_info(None, C.byref(armed), C.byref(n)) == -1 and b"amwg_waic_info" in L.amwg_last_error()


@pytest.mark.parametrize("draws,specs,window_rows,words", [
    (np.zeros((2, 2, 2)), [X3], 0, "window_rows 0"),
    (np.zeros((1, 2, 1)), [X3], 1, "fewer than 2 draws"),
    (np.zeros((2, 1, 2)), [X3], 1, "reads 2 components"),
    (np.zeros((2, 2, 3)), [X3, X3], 1, "bad shape"),
])
def test_fold_check_refuses_bad_arguments_before_a_device_is_opened(draws, specs, window_rows, words):
    with pytest.raises(A.AmwgError) as ei:
        A.waic_fold_check(draws, specs, window_rows, device=NO_DEVICE)
    assert "amwg_waic_fold_check" in str(ei.value) and words in str(ei.value), str(ei.value)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_a_pointwise_program_compiles_for_gfx950_with_the_fold_entry(tmp_path, monkeypatch):
    import pointwise_lib as pl
    m = pl.fixtures(5, 2, ("normal",))["models"]["normal"]
    dump = tmp_path / "pw.hsaco"
    monkeypatch.setenv("AMWG_DUMP_CODE_OBJECT", str(dump))
    assert A.compile_pointwise(m["source"], m["terms_source"], "gfx950") > 10000
    code = dump.read_bytes()
    for entry in (b"amwg_pw_waic_partial", b"amwg_pw_waic_fold"):
        assert entry in code, entry
