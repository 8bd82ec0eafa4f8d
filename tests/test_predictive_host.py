"""Posterior predictive calibration (amwg_last_sample_dataset_predictive), the part that needs no GPU.  tests/README.predictive.md says what each test pins."""
import ctypes as C

import numpy as np
import pytest

import amwg_ctypes
from test_heldout_host import H3, P3, X3
from test_waic_host import NO_DEVICE, declared

CALL, CHECK = "amwg_last_sample_dataset_predictive", "amwg_predictive_check"


def test_calls_are_declared_mirrored_and_exported():
    assert CALL in declared("amwg.h") and CALL in amwg_ctypes.EXPORTS and getattr(amwg_ctypes.lib(), CALL) is not None
    for check in (CHECK, "amwg_predictive_totals_check"):
        assert check in declared("amwg_selftest.h") and check in amwg_ctypes.SELFTEST_EXPORTS and check not in amwg_ctypes.EXPORTS
        assert getattr(amwg_ctypes.selftest_lib(), check) is not None and not hasattr(amwg_ctypes.lib(), check) and callable(amwg_ctypes.Sampler.dataset_predictive)
    L = amwg_ctypes.lib()      # null arguments are refused before any device call (held may be NULL: in-sample)
    fake, summary = C.c_void_p(8), (C.c_double * 4)()      # (fake is never dereferenced: refused for another argument first)
    for args in ((None, None, None, summary, None), (fake, None, None, None, None)):
        assert L.amwg_last_sample_dataset_predictive(*args) == -1, args
        assert CALL.encode() in L.amwg_last_error(), L.amwg_last_error()


@pytest.mark.parametrize("draws,specs,held,index,words", [
    (np.zeros((1, 2, 1)), [X3], None, None, "fewer than 2 draws"),
    (np.zeros((2, 1, 2)), [X3], None, None, "reads 2 components"),
    (np.zeros((2, 2, 2)), [X3], [dict(X3, model="beta_bern")], None, "is of model"),
    (np.zeros((2, 2, 2)), [X3], [dict(X3, n_obs=-1)], None, "n_obs < 0"),
    (np.zeros((2, 9, 2)), [P3], [P3], [np.array([0, -1, 2])], "index[1] = -1"),
    (np.zeros((2, 4, 2)), [H3], [dict(H3, G=3)], None, "G = 3"),
    (np.zeros((2, 4, 2)), [H3, H3], None, None, "one dataset"),
])
def test_predictive_check_refuses_before_a_device_is_opened(draws, specs, held, index, words):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.predictive_check(draws, specs, held, index=index, device=NO_DEVICE)
    assert CHECK in str(ei.value) and words in str(ei.value), str(ei.value)      # (a call that reached the device would fail without the call's name)


@pytest.mark.parametrize("mids,y,mean,want", [      # want: cover50, cover90, rmse; mean_mid is the running sum of the mids over m
    ([0.25, 0.75, 0.05, 0.95], [1.0, 2.0, 3.0, 5.0], [1.0, 2.0, 3.0, 3.0], [0.5, 1.0, 1.0]),                  # the edges are inside, both of them
    ([0.2499999999999999, 0.7500000000000002, 0.04, 0.96], [0.0] * 4, [0.0] * 4, [0.0, 0.5, 0.0]),            # ... and a step beyond them is outside
    ([], [], [], [float("nan")] * 3),                                                                          # m_d = 0
    ([0.5, float("nan"), 0.5], [0.0] * 3, [0.0] * 3, [float("nan")] * 3),                                      # a NaN observation: the four values
])
def test_the_finish_on_hand_made_arrays(mids, y, mean, want):
    pw = np.array([[m, m, mu, 1.0] for m, mu in zip(mids, mean)]).reshape(-1, 4)      # (pit_hi = pit_lo = m: mid_j is m itself)
    total = 0.0
    for m in mids:
        total += m
    assert np.array_equal(amwg_ctypes.predictive_totals(pw, y), np.array(want + [total / len(mids) if want[0] == want[0] else float("nan")]), equal_nan=True)
