"""No GPU: the host twin of tests/test_gpu_twoval.py (README.twoval.md).  csrc/amwg_twoval.h compiled with g++ (tests/host/twoval_eval_host.cpp) gives, on every
lane of every case of tests/twoval_cases.py, the bits of the plain sequential sum -- and the cases are shown to ARRIVE where the header is intricate: the census
conditions are asserted here, on the inputs.  The restated table recipe, the plain sum and the census are themselves checked on cases small enough to do by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import twoval_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host(out_dir, header_dir=None):
    """twoval_eval_host.so from csrc/amwg_twoval.h -- or from the amwg_twoval.h of header_dir (tools/twoval_mutations.py: a mutated copy) -- -> eval(...) -> sums [m]"""
    so = os.path.join(str(out_dir), "twoval_eval_host.so")
    inc = (["-I", str(header_dir)] if header_dir else []) + ["-I", os.path.join(ROOT, "bayes.js_amd", "csrc")]
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + inc + [os.path.join(ROOT, "tests", "host", "twoval_eval_host.cpp"), "-o", so]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lib = C.CDLL(so)
    pd = C.POINTER(C.c_double)
    lib.twoval_eval.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.c_long, pd, pd, pd, pd]

    def run(n, tab, acc0, l1, l0):
        tab = np.ascontiguousarray(tab, dtype=np.uint32)
        acc0, l1, l0 = (np.ascontiguousarray(v, dtype=np.float64) for v in (acc0, l1, l0))
        assert l1.shape == acc0.shape == l0.shape and tab.size == 6 * V.words(n)
        out = np.empty(acc0.size)
        assert lib.twoval_eval(tab.ctypes.data_as(C.POINTER(C.c_uint32)), n, acc0.size, acc0.ctypes.data_as(pd), l1.ctypes.data_as(pd), l0.ctypes.data_as(pd),
                               out.ctypes.data_as(pd)) == 0
        return out
    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("twoval_host"))


def test_case_list_is_the_issues():
    assert V.SHAPES == [0, 1, 31, 32, 33, 63, 64, 65, 777, 4099, 8192, 20000] and V.M == 2048 and len(V.case_list()) == len(V.SHAPES) * len(V.KINDS)
    for n, kind in V.case_list():
        c = V.case(n, kind)
        x = c["x"]
        assert x.shape == (n,) and x.dtype == np.uint8 and (n == 0 or x.max() <= 1)
        assert c["acc0"].shape == c["l1"].shape == c["l0"].shape == (V.M,) and c["tab"].shape == (6 * (n // 32 + 2),)
        if n >= 777:
            runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[2], x, [2]]).astype(int))))      # the lengths of the runs of equal observations
            edges = np.flatnonzero(np.diff(x.astype(int))) + 1                                      # where a new run begins
            if kind.startswith("iid_"):
                p = int(kind[4:]) / 100
                assert abs(x.mean() - p) < 4 * (p * (1 - p) / n) ** 0.5      # four standard deviations of a mean of n draws
            elif kind == "runs":
                assert runs.max() <= V.RUN_MAX and (runs[:-1] % 32 != 0).all() and len(set(runs.tolist())) > 5
            elif kind == "runs_32k":      # runs that end before, on and behind a word boundary
                assert set((runs[:-1] % 32).tolist()) == {31, 0, 1} and set((edges % 32).tolist()) == {31, 0, 1}
            elif kind == "alternating":
                assert (runs == 1).all()
            elif kind.startswith("period"):
                p, one = int(kind[6]), int(kind.endswith("_one"))
                assert (x[p:] == x[:-p]).all() and int((x[:p] == one).sum()) == 1
            elif kind in ("all_ones", "all_zeros"):
                assert (x == (kind == "all_ones")).all()
            else:
                assert np.flatnonzero(x == (kind == "sparse_ones")).tolist() == [0, 31, 32, n - 1]
        # the lanes the issue fixes
        j = np.arange(V.M)
        assert all(abs(v) == 2.0 ** p for v, p in zip(c["acc0"][V.STALL][:45], range(40, 85))) and (c["acc0"][V.STALL] < 0).all()
        nf = len(V.FALLBACK_ADDENDS)
        assert V.same_bits(c["l1"][V.FALLBACK0:V.FALLBACK0 + nf], V.FALLBACK_ADDENDS).all() and V.same_bits(c["l0"][V.FALLBACK0 + nf:V.FALLBACK0 + 2 * nf], V.FALLBACK_ADDENDS).all()
        assert np.array_equal(np.flatnonzero(c["flags"]["fallback"]), j[V.FALLBACK0:V.FALLBACK0 + 2 * nf])
        assert (c["l1"][V.EQUAL] == c["l0"][V.EQUAL]).all()
        ratio = c["l0"][V.RATIO] / c["l1"][V.RATIO]
        assert (np.log2(ratio) == np.round(np.log2(ratio))).all() and (ratio != 1).all()
        assert (np.frexp(c["l1"][V.POWERS])[0] == -0.5).all() and (np.frexp(c["l0"][V.POWERS])[0] == -0.5).all()
        assert c["acc0"][V.ACC0_FIXED0:V.ACC0_FIXED0 + 4].tobytes() == np.array(V.ACC0_FIXED).tobytes()
        below = c["acc0"][V.BELOW_POW2]
        up = np.ldexp(1.0, np.frexp(below)[1])      # the power of two above |start|
        assert (below < 0).all() and ((up + below) / np.spacing(-below) <= 4).all() and ((up + below) > 0).all()


def test_the_planted_cases_of_the_issue_are_among_the_lanes():
    """The three cases that each kill one mutation which the random fuzz let live: they are lanes of the cases, in >= 8 variants each."""
    # saturation: 8 192 ones, -2.0 + 8 192 x -1.0: the first probe's product is 8 192 x 2^51 = 2^64
    c = V.case(8192, "all_ones")
    lane = V.SATURATION.start + 1
    assert (c["acc0"][lane], c["l1"][lane]) == (-2.0, -1.0) and c["want"][lane] == -8194.0
    hit = 0
    for n, kind in V.case_list():
        c, n1 = V.case(n, kind), int(V.case(n, kind)["x"].sum())
        for v, lane in enumerate(range(V.SATURATION.start, V.SATURATION.stop)):
            N, l = (n1, c["l1"][lane]) if v & 1 else (n - n1, c["l0"][lane])
            _, e, sig = V.addend_parts(np.array([l]))
            _, ea, _ = V.addend_parts(np.array([c["acc0"][lane]]))
            if N >= 4097 and ea[0] == e[0] + 1 and (N * (int(sig[0]) >> 1)) >> 64:      # n d >= 2^64 in the binade right above the addend
                assert (N * (int(sig[0]) >> 1)) % (1 << 64) < 1 << 32
                hit += 1
    assert hit >= 8, hit
    # half an ulp on a stalled sum: -(2^53 + 2) + 40 x -1.0 beside -0.25 rounds to even ONCE
    x = np.ones(40, dtype=np.uint8)
    assert V.plain_sum(x, [-(2.0 ** 53 + 2)], [-1.0], [-0.25])[0] == -(2.0 ** 53 + 4)
    c = V.case(64, "all_ones")
    lane = V.HALF_ULP.start + 1      # the ones tie, A odd, the other addend a quarter of an ulp
    assert (c["acc0"][lane], c["l1"][lane], c["l0"][lane], c["want"][lane]) == (-(2.0 ** 53 + 2), -1.0, -0.25, -(2.0 ** 53 + 4))
    moved = sum(int((V.case(*k)["want"][V.HALF_ULP] != V.case(*k)["acc0"][V.HALF_ULP]).sum()) for k in V.case_list())
    assert moved >= 8 * 20, moved
    # landing: alternating, n = 64, -4 and -2 from -(2^54 - 192) ends on -2^54 exactly
    c = V.case(64, "alternating")
    lane = [q for q in range(V.LANDING.start, V.LANDING.stop) if (c["l1"][q], c["l0"][q], c["acc0"][q]) == (-4.0, -2.0, -(2.0 ** 54 - 192))]
    assert lane and (c["want"][lane] == -2.0 ** 54).all()
    for n, kind in V.case_list():
        if n >= 31:
            assert V.case(n, kind)["flags"]["landing"][V.LANDING].sum() >= 32, (n, kind)


def test_the_restated_table_recipe_against_a_double_loop():
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 2, n).astype(np.uint8) for n in (0, 1, 32, 70, 97, 200)] + [V.case(65, k)["x"] for k in ("runs", "alternating", "sparse_zeros", "all_ones", "period3_zero")]
    for x in seqs:
        n, W = x.size, x.size // 32 + 2
        want = np.zeros((6, W), dtype=np.uint32)
        for w in range(W):
            want[0, w] = sum(1 << (i - 32 * w) for i in range(32 * w, min(32 * w + 32, n)) if x[i] == 1)
            want[1, w] = sum(1 for i in range(min(32 * w, n)) if x[i] == 1)
        for row, sym in ((2, 1), (4, 0)):
            odd = []
            for i in range(n):      # the run of the other value right in front of observation i
                run = 0
                while i - 1 - run >= 0 and x[i - 1 - run] != sym:
                    run += 1
                odd.append(x[i] == sym and run % 2 == 1)
            for w in range(W):
                want[row, w] = sum(1 << (i - 32 * w) for i in range(32 * w, min(32 * w + 32, n)) if odd[i])
                want[row + 1, w] = sum(1 for i in range(min(32 * w, n)) if odd[i])
        got = V.tables(x)
        assert len(got) == 6 and all(g.dtype == np.uint32 and g.shape == (W,) for g in got)
        assert np.stack(got).tobytes() == want.tobytes() and V.tables_flat(x).tobytes() == want.tobytes()


def test_the_plain_sum_is_the_sequential_loop():
    c = V.case(777, "runs")
    for j in (0, 77, 129, 137, 161, 163, 200, 262, 270, 300, 1000, 2047):
        acc = float(c["acc0"][j])
        for v in c["x"].tolist():
            acc = acc + float(c["l1"][j] if v else c["l0"][j])
        assert V.same_bits(acc, c["want"][j]), j
    assert not V.same_bits(0.0, -0.0) and V.same_bits(np.nan, -np.nan) and not V.same_bits(1.0, np.nextafter(1.0, 2.0))


def test_the_census_on_visits_done_by_hand():
    def one(x, acc0, l1, l0):
        return {k for k, v in V.census(np.array(x, dtype=np.uint8), np.array([acc0]), np.array([l1]), np.array([l0]))[1].items() if v[0]}
    ones = [1] * 100
    # -4 + 100 x -1.0: binades [4, 8) of 4 observations, [8, 16) of 8, ... [64, 128) of the last 40; a power of two never ties above s = 0 and below s = 53; every
    # binade is entered ON a power of two; the other addend (2^-60) moves nothing there
    assert one(ones, -4.0, -1.0, -2.0 ** -60) == {"mode0_lt32", "mode0_32_63", "tie_free", "one_increment_zero", "landing"}
    # ulp 2: the zeros' -1.0 is half an ulp (q = 0, a tie), the ones' -2.0 moves the significand by 1, an odd increment: mode 3 for all 100 observations (the sum
    # stays far below 2^54), and no zero follows in the data.  A = 2^52 is even; from -(2^53 + 2) it is odd: the same classes but the parity
    assert one(ones, -2.0 ** 53, -2.0, -1.0) == {"mode3_ge64", "mode3_absent", "mode3_two_boundaries", "half_ulp_tie_even", "one_increment_zero"}
    assert one(ones, -(2.0 ** 53 + 2), -2.0, -1.0) == {"mode3_ge64", "mode3_absent", "mode3_two_boundaries", "half_ulp_tie_odd", "one_increment_zero"}
    # the other addend -4.0: increment 2, even -> mode 2 with no tying symbol in the visit
    assert one(ones, -2.0 ** 53, -4.0, -1.0) == {"mode2_ge64", "mode2_no_tying_symbol", "half_ulp_tie_even", "one_increment_zero"}
    # both half an ulp: mode 1; both a quarter: stalled
    assert one(ones, -2.0 ** 53, -1.0, -1.0) == {"mode1_ge64", "half_ulp_tie_even"}
    assert one(ones, -2.0 ** 54, -1.0, -1.0) == {"mode0_ge64", "stalled"}
    # ulp 2, the zeros tie with q = 1 (-3.0 = 1.5 ulps), the ones add 1: mode 3.  Data 1 0 | 1 1 0 | 1 0 ...: the first zero is observation 1 (not the visit's
    # first); behind it a zero after the even run 1 1 and one after the odd run 1: both kinds of mark; 7 observations cross no word boundary
    assert one([1, 0, 1, 1, 0, 1, 0], -2.0 ** 53, -2.0, -3.0) == {"mode3_lt32", "mode3_odd_and_even"}
    assert one([0, 1, 0, 1, 0], -2.0 ** 53, -2.0, -3.0) == {"mode3_lt32", "mode3_first_at_start"}      # every later zero after a run of one: odd marks only
    # 40 observations from observation 0 cross ONE word boundary, 65 cross two
    assert "mode3_two_boundaries" not in one([1, 0] * 20, -2.0 ** 53, -2.0, -3.0) and "mode3_two_boundaries" in one([1, 0] * 33, -2.0 ** 53, -2.0, -3.0)
    # an odd significand ties where s = 1: sums in [2, 4), left after at most two observations; from s = 2 on its remainder is below half
    f = one(ones, -2.0, -(1.0 + 2.0 ** -52), -(1.0 + 2.0 ** -52))
    assert "mode1_lt32" in f and "tie_free" in f and "mode1_ge64" not in f
    # exponent equal to the addend's: term by term until the sum is -2.0; a start at 0.0 or above; -0.0 is no such start; a positive addend
    assert "tie_free" in one(ones, -1.0, -1.0, -1.0)
    assert {"starts_nonneg", "tie_free"} <= one(ones, 3.0, -1.0, -1.0) and "starts_nonneg" in one(ones, 0.0, -1.0, -1.0) and "starts_nonneg" not in one(ones, -0.0, -1.0, -1.0)
    assert one(ones, -4.0, 0.25, -1.0) == {"fallback"}
    # the landing of the issue: alternating, 64 observations of -4 and -2 from -(2^54 - 192): one visit, no tie, and the FINAL sum is -2^54
    assert one([1, 0] * 32, -(2.0 ** 54 - 192), -4.0, -2.0) == {"mode0_ge64", "tie_free", "landing"}
    assert "landing" not in one([1, 0] * 32, -(2.0 ** 54 - 196), -4.0, -2.0)


def test_census_conditions():
    V.check_census_conditions()
    assert V.SUITE_MIN["mode1_ge64"] == V.SUITE_MIN["mode2_ge64"] == V.SUITE_MIN["mode3_ge64"] == 500 and all(v >= 100 for v in V.SUITE_MIN.values()) and len(V.SUITE_MIN) == 13
    assert V.SHARE_MIN == {"tie_free": 0.80, "mode3_ge64": 0.05}


@pytest.mark.parametrize("n,kind", V.case_list())
def test_host_build_equals_the_plain_sum(host, n, kind):
    c = V.case(n, kind)
    got = host(n, c["tab"], c["acc0"], c["l1"], c["l0"])
    bad = np.nonzero(~V.same_bits(got, c["want"]))[0]
    assert bad.size == 0, (bad.size, bad[:5], c["acc0"][bad[:5]], c["l1"][bad[:5]].view(np.uint64), c["l0"][bad[:5]].view(np.uint64), got[bad[:5]], c["want"][bad[:5]],
                           {f: int(v[bad].sum()) for f, v in c["flags"].items() if v[bad].any()})
