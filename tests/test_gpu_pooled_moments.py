"""-m gpu: the pooled moments() of an ordinary sampler, to the bit.  tests/test_gpu_moments.py holds them to the reference within tolerances; this file
pins the ORDER of the sums, restated in numpy float64: the kernel is the one behind dataset_moments() (csrc/amwg_diag.hip dataset_moments_kernel) run as one
dataset of all the chains, so per recorded value, over v = draws[:, p, :].reshape(-1) (row after row, n = rows x chains values):

    1024 partial sums, thread t over v[t], v[t + 1024], ...; a halving tree over them (512, 256, ..., 1); m = s / n;
    second pass in the same order: dlt = x - m, ss += dlt * dlt (a product, then a sum: the library is built with -ffp-contract=off);
    sd = sqrt(tot / (n - 1)), 0 for n = 1.  A thread without an element adds nothing.

The shapes are the smallest at which that order can go wrong."""
import numpy as np
import pytest

import amwg_ctypes
import model_spec
from summary_reference import kernel_order_moments      # (tree_sum and strided_sums over 1 024 threads: the restated order lives there, shared)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("chains,rows", [(1, 1), (64, 3), (192, 7)], ids=["n1_sd_is_0", "n192_idle_threads", "n1344_two_rounds"])
def test_pooled_moments_follow_the_kernels_order_bit_for_bit(chains, rows):
    """n = 1: the sd = 0 branch; n = 192 < 1024: idle threads in the tree; n = 1344: the first 320 threads hold two elements, the rest one."""
    spec = model_spec.build_spec("normal", model_spec.make_data("normal", 50, 20261019))
    s = amwg_ctypes.Sampler(spec, chains=chains, seed=20261019, lanes_per_chain=1)
    s.burn(120)
    draws = s.sample(rows, 1)      # [rows][P][chains]
    assert draws.shape == (rows, 2, chains)
    mean, sd = s.moments()
    s.close()
    for p in range(draws.shape[1]):
        want_m, want_sd = kernel_order_moments(np.ascontiguousarray(draws[:, p, :]).reshape(-1))
        print("component %d: mean %r (numpy %r), sd %r (numpy %r)" % (p, mean[p], want_m, sd[p], want_sd))
        assert np.float64(mean[p]).tobytes() == np.float64(want_m).tobytes(), (p, mean[p], want_m)
        assert np.float64(sd[p]).tobytes() == np.float64(want_sd).tobytes(), (p, sd[p], want_sd)
