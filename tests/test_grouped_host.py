"""WAIC and PSIS-LOO over groups of observations, the part that needs no GPU: the calls are declared, mirrored and exported; what the arguments alone decide is
refused before a device is opened, with the call's name; the groups and the order they are dealt to the tiles in are a function of the labels alone.
tests/README.grouped.md says what each test pins."""
import os
import re

import numpy as np
import pytest

import amwg_ctypes as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 99      # a device number that does not exist: a call that reached the device would fail with AMWG_EHIP, not AMWG_EINVAL
X3 = {"model": "normal", "n_obs": 3, "data": {"x": np.zeros(3)}}
CHECKS = ("amwg_waic_grouped_check", "amwg_loo_grouped_check", "amwg_user_waic_grouped_check", "amwg_user_loo_grouped_check", "amwg_group_csr_check")


def declared(header):
    return set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_calls_are_declared_mirrored_and_exported():
    for call in ("amwg_last_sample_dataset_waic_grouped", "amwg_last_sample_dataset_loo_grouped"):
        assert call in declared("amwg.h") and call in A.EXPORTS and getattr(A.lib(), call) is not None
    for check in CHECKS:
        assert check in declared("amwg_selftest.h") and check in A.SELFTEST_EXPORTS and getattr(A.selftest_lib(), check) is not None and not hasattr(A.lib(), check)


@pytest.mark.parametrize("check", [A.waic_check, A.loo_check])
def test_refused_before_a_device_call(check):
    name = "amwg_waic_grouped_check" if check is A.waic_check else "amwg_loo_grouped_check"
    with pytest.raises(A.AmwgError) as ei:
        check(np.zeros((1, 2, 1)), [X3], device=NO_DEVICE, groups=[np.arange(3)])
    assert name in str(ei.value) and "fewer than 2 draws per dataset" in str(ei.value), str(ei.value)
    L, pi32 = A.selftest_lib(), A.C.POINTER(A.C.c_int32)
    mds, keep = A._model_descs([X3])
    call = getattr(L, name)
    assert call(NO_DEVICE, A._dp(np.zeros((4, 2, 1))), 4, 2, 1, 1, mds, pi32(), 0, A._dp(np.empty(4)), None, None, None, None) == -1
    assert (name + ": NULL labels") in L.amwg_last_error().decode()
    for product in ("amwg_last_sample_dataset_waic_grouped", "amwg_last_sample_dataset_loo_grouped"):
        assert getattr(A.lib(), product)(None, pi32(), None, None, None, None) == -1 and (product + ": null argument") in A.lib().amwg_last_error().decode()


def test_the_groups_are_a_function_of_the_labels_alone():
    labels = np.array([40, -3, 40, 7, 7, 40, 1000, -3, 40, 5], dtype=np.int32)      # groups -3, 5, 7, 40, 1000 of sizes 2, 1, 2, 4, 1
    start, member, deal = A.group_csr(labels)
    assert start.tolist() == [0, 2, 3, 5, 9, 10]
    assert member.tolist() == [1, 7, 9, 3, 4, 0, 2, 5, 8, 6]      # by (label, observation index)
    assert deal.tolist() == [3, 0, 2, 1, 4]                        # by falling size, equal sizes by rising group number
    start, member, deal = A.group_csr(np.arange(70)[::-1])          # singletons: the identity deal, the members reversed
    assert start.tolist() == list(range(71)) and member.tolist() == list(range(69, -1, -1)) and deal.tolist() == list(range(70))
