"""PSIS-LOO predictive calibration (amwg_last_sample_dataset_loo_predictive), the part that needs no GPU.  tests/README.loo_predictive.md says what each test pins."""
import ctypes as C

import numpy as np
import pytest

import amwg_ctypes
import loo_predictive_reference as lpr
import loo_reference as lr
from test_loo_host import NO_DEVICE, X3, declared

CALL, CHECK = "amwg_last_sample_dataset_loo_predictive", "amwg_loo_predictive_check"


def test_the_two_names_are_declared_and_exported():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS and getattr(amwg_ctypes.lib(), CALL) is not None
    assert CHECK in declared("amwg_selftest.h") and CHECK in amwg_ctypes.SELFTEST_EXPORTS and CHECK not in amwg_ctypes.EXPORTS
    assert getattr(amwg_ctypes.selftest_lib(), CHECK) is not None and not hasattr(amwg_ctypes.lib(), CHECK)


def test_refusals_name_the_call_before_any_device_call():
    L = amwg_ctypes.lib()
    fake, summary = C.c_void_p(8), (C.c_double * 4)()      # (fake is never dereferenced: refused for the other argument first)
    for args in ((None, summary, None, None), (fake, None, None, None)):
        assert L.amwg_last_sample_dataset_loo_predictive(*args) == -1 and CALL.encode() in L.amwg_last_error(), L.amwg_last_error()
    bare = amwg_ctypes.Sampler.__new__(amwg_ctypes.Sampler)      # no handle: the binding refuses held with loo before it asks the library
    with pytest.raises(amwg_ctypes.AmwgError, match=CALL):
        bare.dataset_predictive([X3], loo=True)
    for draws, specs, words in ((np.zeros((1, 2, 1)), [X3], "fewer than 2 draws"), (np.zeros((2, 1, 2)), [X3], "reads 2 components"), (None, [X3], "draws must be")):
        with pytest.raises(amwg_ctypes.AmwgError, match="loo_predictive_check") as ei:
            amwg_ctypes.loo_predictive_check(draws, specs, device=NO_DEVICE)
        assert words in str(ei.value), str(ei.value)


@pytest.mark.parametrize("col", [
    np.linspace(-3.0, -1.0, 20) ** 3,                                                        # M = 4: the raw route
    -np.sqrt(np.arange(1.0, 26.0)),                                                          # M = 5, distinct terms
    np.repeat(-np.sqrt(np.arange(1.0, 11.0))[::-1], [2, 3, 3, 4, 3, 3, 3, 3, 3, 3]),      # S = 30, M = 6: the third class holds positions 5, 6, 7
], ids=["raw", "distinct", "ties_across_M"])
def test_the_weight_rule_against_its_plain_restatement(col):
    col = col[np.random.default_rng(5).permutation(len(col))]
    w, khat, denominator = lpr.weights(col)
    assert np.isfinite(khat) == (lr.tail_len(len(col)) >= 5)
    assert np.allclose(np.asarray(w, dtype=np.float64), np.asarray(lpr.brute_weights(col), dtype=np.float64), rtol=1e-15, atol=0)
    assert abs(float(w.sum() / denominator) - 1.0) <= 1e-15      # the weights sum to the denominator of LOO's elpd_loo_i
    for v in np.unique(col):      # equal terms, equal weights
        assert len(set(np.asarray(w)[col == v].tolist())) == 1
