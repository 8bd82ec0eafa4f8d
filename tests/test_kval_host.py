"""No GPU: the host twin of tests/test_gpu_kval.py (README.kval.md).  csrc/amwg_kval.h compiled with g++ (tests/host/kval_eval_host.cpp) gives, on every lane of
every case of tests/kval_cases.py, the bits of the plain sequential sum -- and the cases are shown to ARRIVE where the header is intricate: the census conditions
are asserted here, on the inputs.  The restated recipe, the plain sum and the census are themselves checked on cases small enough to do by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kval_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host(out_dir, header_dir=None):
    """kval_eval_host.so from csrc/amwg_kval.h -- or from the amwg_kval.h of header_dir (tools/kval_mutations.py: a mutated copy) -- -> eval(case) -> sums [m]"""
    so = os.path.join(str(out_dir), "kval_eval_host.so")
    inc = (["-I", str(header_dir)] if header_dir else []) + ["-I", os.path.join(ROOT, "bayes.js_amd", "csrc")]
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + inc + [os.path.join(ROOT, "tests", "host", "kval_eval_host.cpp"), "-o", so]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lib = C.CDLL(so)
    pd = C.POINTER(C.c_double)
    lib.kval_eval.argtypes = [C.c_int, C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_uint32), C.c_long, pd, pd, pd]

    def run(K, idx, tab, acc0, c):
        idx, tab = np.ascontiguousarray(idx, dtype=np.uint8), np.ascontiguousarray(tab, dtype=np.uint32)
        acc0, c = np.ascontiguousarray(acc0, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
        assert c.shape == (acc0.size, K) and tab.size == 2 * K * V.words(idx.size)
        out = np.empty(acc0.size)
        assert lib.kval_eval(K, idx.ctypes.data_as(C.POINTER(C.c_uint8)), idx.size, tab.ctypes.data_as(C.POINTER(C.c_uint32)), acc0.size,
                             acc0.ctypes.data_as(pd), c.ctypes.data_as(pd), out.ctypes.data_as(pd)) == 0
        return out
    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("kval_host"))


def test_case_list_is_the_issues():
    assert V.SHAPES == [(0, 2), (1, 1), (31, 2), (32, 3), (33, 2), (64, 3), (777, 3), (777, 5), (4099, 13), (5000, 8), (20000, 16)] and V.M == 2048
    assert all(K in V.INSTANTIATED for _, K in V.SHAPES)
    for n, K in V.SHAPES:
        kinds = [k for (nn, KK, k) in V.case_list() if (nn, KK) == (n, K)]
        assert len(kinds) >= 2 and (kinds == list(V.KINDS) or K == 1)
    for key in V.case_list():
        c = V.case(*key)
        n, K = c["n"], c["K"]
        assert c["idx"].shape == (n,) and c["idx"].dtype == np.uint8 and (n == 0 or c["idx"].max() < K)
        assert c["acc0"].shape == (V.M,) and c["c"].shape == (V.M, K) and c["tab"].shape == (2 * K * (n // 32 + 2),)
        if n >= 777:
            seen = set(c["idx"].tolist())
            assert (len(seen) == 1) == (c["kind"] == "one_value")
            if c["kind"] == "absent_value":
                assert 0 not in seen
            if c["kind"] == "block_edges":      # value 0 at the first and last observation of its blocks and nowhere else
                at = np.nonzero(c["idx"] == 0)[0]
                assert at.size and set((at & 31).tolist()) == {0, 31}
            if c["kind"] == "runs":
                edges = np.nonzero(np.diff(c["idx"].astype(int)))[0]
                assert edges.size and (np.diff(edges) % 32 != 0).any()
        # the lanes the issue fixes
        assert c["acc0"][V.ACC0_FIXED0:V.ACC0_FIXED0 + 4].tobytes() == np.array(V.ACC0_FIXED).tobytes()
        assert all(abs(v) == 2.0 ** p for v, p in zip(c["acc0"][V.STALL][:45], range(40, 85))) and (c["acc0"][V.STALL] < 0).all()
        assert c["c"][V.POWERS_LANE, 0] == -1.0 and (K == 1 or c["c"][V.POWERS_LANE, K - 1] == -0.5)
        j = np.arange(V.M)
        ordinary = (j >= V.ORDINARY0) & (j % 8 == 1)
        mult = np.sort(c["c"][ordinary], axis=1)[:, ::-1]      # (sorted by magnitude: the one_value sequences move the largest addend to the value that occurs)
        assert np.array_equal(mult, mult[:, :1] * np.arange(1, K + 1))
    cp = V.case(*V.COPIES_SHAPE, "iid_skewed")
    assert (cp["c"][:64] == cp["c"][V.COPY_OF]).all() and (cp["acc0"][:64] == cp["acc0"][V.COPY_OF]).all() and V.COPY_OF % 8 not in (1, 2)


def test_the_restated_table_recipe_against_a_loop():
    rng = np.random.default_rng(5)
    for n, K in ((0, 1), (1, 2), (32, 2), (70, 3), (97, 16)):
        idx = rng.integers(0, K, n).astype(np.uint8)
        W = n // 32 + 2
        want = np.zeros((W, 2 * K), dtype=np.uint32)
        for w in range(W):
            for k in range(K):
                want[w, k] = sum(1 for i in range(min(32 * w, n)) if idx[i] == k)
                want[w, K + k] = sum(1 << (i - 32 * w) for i in range(32 * w, min(32 * w + 32, n)) if idx[i] == k)
        assert V.tables(idx, K).tobytes() == want.tobytes()


def test_the_plain_sum_is_the_sequential_loop():
    c = V.case(777, 5, "runs")
    for j in (0, 77, 129, 131, 136, 139, 1000, 2047):
        acc = float(c["acc0"][j])
        for v in c["idx"].tolist():
            acc = acc + float(c["c"][j, v])
        assert V.same_bits(acc, c["want"][j]), j
    assert not V.same_bits(0.0, -0.0) and V.same_bits(np.nan, -np.nan) and not V.same_bits(1.0, np.nextafter(1.0, 2.0))


def test_the_census_on_cases_done_by_hand():
    idx = np.zeros(100, dtype=np.uint8)
    one = lambda acc0, c: {k: bool(v[0]) for k, v in V.census(idx, np.array([acc0]), np.array([[c]]))[1].items()}
    f = one(-4.0, -1.0)                       # s = 2, 3, ...: a power of two never ties below s = 53, and d = 2^(52 - s) != 0
    assert f["tie_free"] and not (f["one_tie_ge64"] or f["one_tie_lt32"] or f["several_ties"] or f["stalled"] or f["starts_nonneg"])
    f = one(-2.0 ** 53, -1.0)                 # ulp 2: every -1.0 is half an ulp (d = 0, a tie); ties to even leave the sum where it is for all 100 observations
    assert f["one_tie_ge64"] and not f["tie_free"] and not f["stalled"]
    f = one(-2.0 ** 54, -1.0)                 # ulp 4: a quarter of an ulp, nothing moves
    assert f["stalled"] and not f["tie_free"] and not f["one_tie_ge64"]
    f = one(-1.0, -1.0)                       # exponent equal to the addend's: term by term until the sum is -2.0
    assert f["tie_free"]
    f = one(-2.0, -(1.0 + 2.0 ** -52))        # an odd significand ties where s = 1: sums in [2, 4), left after two observations; from s = 2 on its remainder is below half
    assert f["one_tie_lt32"] and f["tie_free"] and not f["one_tie_ge64"]
    f = one(-2.0 ** 53, -3.0)                 # ulp 2: 1.5 ulp, a tie with d = 1, for all 100 observations
    assert f["one_tie_ge64"] and not f["one_tie_lt32"] and not f["tie_free"]
    f = one(3.0, -1.0)
    assert f["starts_nonneg"] and f["tie_free"]
    assert one(0.0, -1.0)["starts_nonneg"] and not one(-0.0, -1.0)["starts_nonneg"]
    f = one(-4.0, 0.25)
    assert f["fallback"] and not f["tie_free"]
    two = V.census(idx, np.array([-2.0 ** 53, -2.0 ** 60]), np.array([[-3.0, -1.0], [-2.0 ** 8, -1.0]]))[1]      # 1.5 and 0.5 ulp: two ties | d = 1 and 0 at ulp 2^8
    assert two["several_ties"][0] and two["partial_zero"][1] and not two["several_ties"][1] and two["tie_free"][1]
    assert two["partial_zero"][0]      # (a tying addend's d is its floor: 0 for the half ulp beside the 1 of the 1.5 ulp)


def test_census_conditions():
    for n, K in V.SHAPES:
        if n >= 777:
            for flag, least in V.SHARE_MIN.items():
                assert V.shape_share(n, K, flag) >= least, (n, K, flag, V.shape_share(n, K, flag))
    for flag, least in V.SUITE_MIN.items():
        assert V.suite_count(flag) >= least, (flag, V.suite_count(flag))
    assert set().union(*[V.case(*k)["kinds"] for k in V.case_list()]) == V.FALLBACK_KINDS
    j = np.arange(V.M)
    for key in V.case_list():      # the fallback lanes are the fixed ones
        assert np.array_equal(np.nonzero(V.case(*key)["flags"]["fallback"])[0], j[V.FALLBACK0:V.FALLBACK0 + len(V.FALLBACK_ADDENDS)])


@pytest.mark.parametrize("n,K,kind", V.case_list())
def test_host_build_equals_the_plain_sum(host, n, K, kind):
    c = V.case(n, K, kind)
    got = host(K, c["idx"], c["tab"], c["acc0"], c["c"])
    bad = np.nonzero(~V.same_bits(got, c["want"]))[0]
    assert bad.size == 0, (bad.size, bad[:5], c["acc0"][bad[:5]], c["c"][bad[:5]].view(np.uint64), got[bad[:5]], c["want"][bad[:5]],
                           {f: int(v[bad].sum()) for f, v in c["flags"].items()})
    if (n, K) == V.COPIES_SHAPE:
        assert (got[:64].view(np.uint64) == got[V.COPY_OF:V.COPY_OF + 1].view(np.uint64)).all()
