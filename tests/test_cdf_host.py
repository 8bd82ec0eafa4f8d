"""No GPU: csrc/amwg_cdf.h compiled for the host (tests/host/cdf_host.cpp) against mpmath at 50 digits, on the grids of tests/README.predictive.md.  The bounds asserted
are the header's (kErfcRel, kPoisRel): 4 x the largest error these grids showed, rounded up to a power of two.  Each test prints the largest error it saw."""
import ctypes as C
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from predictive_reference import ERFC_REL, POIS_REL      # csrc/amwg_cdf.h: kErfcRel, kPoisRel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp.mp.dps = 50
TINY, STEP, U = 2.0 ** -1022, 2.0 ** -1074, 2.0 ** -53      # the smallest normal double; one subnormal step; the rounding of 1 - Q
EDGES = [float(np.nextafter(b, s)) for b in (0.5, 1.5, 3.0, 6.0, 600.0 ** 0.5, 28.0) for s in (-np.inf, b, np.inf)]      # the piece boundaries and a step either side
ERFC_X = [0.0, 5e-324, 1e-300, 2.0 ** -60, 1.0, 2.25, 5.0, 10.0, 20.0, 26.0, 26.5, 27.0, 27.2, 27.3, 40.0, np.inf, np.nan] + EDGES
LAMS = [1e-300, 1e-3, 0.5, 1.0, 50.0, 745.2, 1e3, 1e5]
POIS = [(y, lam) for y in (0.0, 1.0, 2.0, 50.0, 1000.0, 1e5) for lam in LAMS] + \
       [(max(0.0, float(round(lam + k * 5 * lam ** 0.5))), lam) for lam in LAMS for k in (-1, 1)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """-> run(name, width, *columns): the entry `name` of cdf_host.cpp over equally long columns -> [n][width]"""
    so = os.path.join(str(tmp_path_factory.mktemp("cdf_host")), "cdf_host.so")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "cdf_host.cpp"), "-o", so], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lib, pd = C.CDLL(so), C.POINTER(C.c_double)

    def run(name, width, *columns):
        cols, out = [np.array(c, dtype=np.float64) for c in columns], np.empty((len(columns[0]), width))
        getattr(lib, name)(C.c_long(len(out)), *[c.ctypes.data_as(pd) for c in cols + [out]])
        return out
    return run


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_erfc_against_mpmath(host, sign):
    xs, worst = [sign * x for x in ERFC_X], 0.0
    for x, g in zip(xs, host("cdf_erfc", 1, xs)[:, 0]):
        exact = mp.erfc(mp.mpf(x))
        if x != x or exact == 0 or exact == 2:      # NaN stays NaN; at the infinities the value itself
            assert (np.isnan(g) if x != x else g == float(exact)), (x, g)
        elif exact >= TINY:
            worst = max(worst, float(abs(mp.mpf(g) - exact) / exact))
        else:                                       # (27.3 and beyond: 0 for a value below half a subnormal step)
            assert abs(mp.mpf(g) - exact) <= STEP, (x, g)
    print("erfc, sign %+d: largest relative error %.3g = 2^%.1f (stated 2^%d)" % (sign, worst, np.log2(worst), np.log2(ERFC_REL)))
    assert worst <= ERFC_REL


def test_poisson_pair_against_mpmath(host):
    """the header's bound on each of F, Fm and the complement Q: |value - exact| <= kPoisRel min(exact, 1 - exact) + 2^-53"""
    worst = 0.0
    for (yi, li), (F, Fm, Q) in zip(POIS, host("cdf_poisson", 3, *zip(*POIS))):
        L = mp.mpf(li)
        exact = [mp.gammainc(yi + 1, L, mp.inf, regularized=True), mp.gammainc(yi, L, mp.inf, regularized=True) if yi > 0 else mp.mpf(0), mp.gammainc(yi + 1, 0, L, regularized=True)]
        for g, e in zip((F, Fm, Q), exact):
            err, tail = abs(mp.mpf(g) - e) - U, min(e, 1 - e)
            if tail >= TINY:
                worst = max(worst, float(err / tail))
            else:
                assert err <= STEP, (yi, li, g)
    print("Poisson pair: largest relative error %.3g = 2^%.1f (stated 2^%d)" % (worst, np.log2(worst), np.log2(POIS_REL)))
    assert worst <= POIS_REL


def test_poisson_pair_refuses_what_is_no_count(host):
    out = host("cdf_poisson", 3, [-1.0, 0.5, np.nan, np.inf, 3.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0, np.nan, np.inf, 0.0, 0.0])
    assert np.isnan(out[:6]).all() and out[6].tolist() == [1.0, 1.0, 0.0] and out[7].tolist() == [1.0, 0.0, 0.0]
