"""-m gpu: the K-valued exact fast-forward (csrc/amwg_kval.h k_valued_sum<K>) ON THE DEVICE against the plain sequential sum (README.kval.md).

* The building block (amwg_k_valued_sum_check, lane j = thread j of 64-thread workgroups: every wavefront holds 64 different cases): device fast-forward ==
  device plain loop == numpy plain sum, the same bits or both NaN, on every lane of every case of tests/kval_cases.py -- the cases tests/test_kval_host.py runs
  through the host build, whose census conditions are asserted there and here.  Per case m = 2 048 lanes:
    addends -exp(U(-12, 3)) with z < 40 trailing significand bits cleared and bit z set in half of them; one lane in eight exact multiples c, 2c, 3c, ...; one in
    eight wide addends -exp(U(-80, 3)); starting sums half N(0, 3), half -exp(U(-5, 25)); lanes 64 .. 127 start at -2^(40 .. 84); lanes 128 .. 133 have an addend
    -inf, NaN, +0.25, 0.0, -5e-324, -1e-310; lane 134 has -1.0 and -0.5 together; lanes 136 .. 139 start at 0.0, -0.0, 1e300, -1e300; lanes 140 .. 171 land exactly
    on a power of two at or beside a block boundary; lanes 0 .. 63 of the shape (4 099, 13) are 64 copies of lane 203.
* The translator's own tables (translate.js kValuedTables, the arrays under the #aux:kval: keys) equal the restated recipe as bytes, and go through the check entry.
* The product's route: a closure with and without the shortcut ({"no_fast_forward": true}), two samplers at one lane per chain, every chain compared."""
import ctypes as C
import math
import re
import shutil
import time

import numpy as np
import pytest

import amwg_ctypes as A
import golden_io
import kval_cases as V
import user_host

pytestmark = pytest.mark.gpu
EINVAL = -1      # include/amwg.h AMWG_EINVAL
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


@pytest.mark.parametrize("n,K,kind", V.case_list())
def test_device_fast_forward_equals_device_loop_equals_plain_sum(n, K, kind):
    c = V.case(n, K, kind)
    ff, seq = A.k_valued_sum_check(K, c["idx"], c["tab"], c["acc0"], c["c"])
    for what, got in (("device plain loop", seq), ("device fast-forward", ff)):
        bad = np.nonzero(~V.same_bits(got, c["want"]))[0]
        assert bad.size == 0, (what, bad.size, bad[:5], c["acc0"][bad[:5]], c["c"][bad[:5]].view(np.uint64), got[bad[:5]], c["want"][bad[:5]],
                               {f: int(v[bad].sum()) for f, v in c["flags"].items()})
    assert V.same_bits(ff, seq).all()
    if (n, K) == V.COPIES_SHAPE:      # a wavefront in uniform control flow gives what the same case gives in its divergent place
        assert (ff[:64].view(np.uint64) == ff[V.COPY_OF:V.COPY_OF + 1].view(np.uint64)).all() and (seq[:64].view(np.uint64) == seq[V.COPY_OF:V.COPY_OF + 1].view(np.uint64)).all()


def test_census_conditions():
    """the cases arrive where the header is intricate (conditions on the inputs, computed on the CPU; tests/test_kval_host.py asserts the same)"""
    for n, K in V.SHAPES:
        if n >= 777:
            for flag, least in V.SHARE_MIN.items():
                assert V.shape_share(n, K, flag) >= least, (n, K, flag, V.shape_share(n, K, flag))
    for flag, least in V.SUITE_MIN.items():
        assert V.suite_count(flag) >= least, (flag, V.suite_count(flag))
    assert set().union(*[V.case(*k)["kinds"] for k in V.case_list()]) == V.FALLBACK_KINDS


def test_lanes_in_a_partial_wavefront_and_no_lanes():
    c = V.case(777, 5, "runs")
    for m in (1, 63, 65, 100):
        ff, seq = A.k_valued_sum_check(5, c["idx"], c["tab"], c["acc0"][:m], c["c"][:m])
        assert V.same_bits(ff, c["want"][:m]).all() and V.same_bits(seq, c["want"][:m]).all()
    ff, seq = A.k_valued_sum_check(5, c["idx"], c["tab"], c["acc0"][:0], c["c"][:0])
    assert ff.size == 0 and seq.size == 0
    e = V.case(0, 2, "iid_skewed")      # no observations: the sums are the starting sums
    ff, seq = A.k_valued_sum_check(2, e["idx"], e["tab"], e["acc0"], e["c"])
    assert V.same_bits(ff, e["acc0"]).all() and V.same_bits(seq, e["acc0"]).all()


def test_bad_arguments_are_refused():
    L = A.selftest_lib()
    c = V.case(33, 2, "runs")
    m = 4
    idx, tab, acc0, cc = c["idx"].copy(), c["tab"].copy(), c["acc0"][:m].copy(), np.ascontiguousarray(c["c"][:m])
    ff, seq = np.empty(m), np.empty(m)
    pb, pw, pd = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    call = lambda K=2, i=pb(idx), n=33, t=pw(tab), lanes=m, a=pd(acc0), q=pd(cc), o1=pd(ff), o2=pd(seq): L.amwg_k_valued_sum_check(0, K, i, n, t, lanes, a, q, o1, o2)
    assert call() == 0
    for K in (0, 4, 6, 7, 12, 14, 17, -1):
        assert call(K=K) == EINVAL and b"not instantiated" in L.amwg_last_error()
    for kw in (dict(i=None), dict(t=None), dict(a=None), dict(q=None), dict(o1=None), dict(o2=None), dict(n=-1), dict(lanes=-1)):
        assert call(**kw) == EINVAL, kw
    high = idx.copy()
    high[17] = 2
    assert call(i=pb(high)) == EINVAL and b"idx[17] = 2" in L.amwg_last_error()
    assert call(lanes=0) == 0 and call(n=0) == 0
    with pytest.raises(A.AmwgError):
        A.k_valued_sum_check(2, idx, tab[:-1], acc0, cc)


# ---- the translator's own tables

def translators_tables(name):
    """-> (y, idx, tab, K) of a closure whose loop the translator hands to k_valued_sum: the data array and the two arrays under its #aux:kval: keys"""
    src, arrays, meta = user_host.translated(name)
    keys = meta["array_keys"]
    t = [j for j, k in enumerate(keys) if k.startswith("#aux:kval:") and k.endswith(":tab")]
    i = [j for j, k in enumerate(keys) if k.startswith("#aux:kval:") and k.endswith(":idx")]
    assert len(t) == 1 and len(i) == 1
    y = arrays[int(keys[t[0]].split(":")[2])]
    assert meta["array_types"][t[0]] == 2 and meta["array_types"][i[0]] == 1      # i32 words, bytes
    tab = (arrays[t[0]].astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    return y, arrays[i[0]].astype(np.uint8), tab, int(re.search(r"kval_loop_one_lane<(\d+)>", src).group(1))


def restated_index(y):
    """the value index of every observation: distinct values numbered in the order of their first occurrence"""
    slot = {}
    return np.array([slot.setdefault(v, len(slot)) for v in y.tolist()], dtype=np.uint8), list(slot)


@needs_node
@pytest.mark.parametrize("name,K", [("pois_const_rate", 13), ("binom_const_size", 8)])
def test_translators_tables_equal_the_recipe_and_pass_the_check(name, K):
    y, idx, tab, k_src = translators_tables(name)
    want_idx, values = restated_index(y)
    assert k_src == K == len(values)
    assert idx.tobytes() == want_idx.tobytes()
    assert tab.tobytes() == V.tables(want_idx, K).tobytes()
    # the terms of 256 parameter values spread over the prior's range (the comparison is between fast-forward and plain loop on the SAME addends)
    lf = np.array([math.lgamma(v + 1) for v in values])
    v = np.array(values)
    if name == "pois_const_rate":
        rate = np.exp(np.linspace(math.log(1e-4), math.log(60.0), 256))
        c = v[None, :] * np.log(rate)[:, None] - rate[:, None] - lf[None, :]
    else:
        p = np.linspace(0.0005, 0.9995, 256)
        c = (math.lgamma(8) - lf - np.array([math.lgamma(7 - x + 1) for x in values]))[None, :] + v[None, :] * np.log(p)[:, None] + (7 - v)[None, :] * np.log1p(-p)[:, None]
    acc0 = np.where(np.arange(256) % 2 == 0, -1.5, 0.25) * np.linspace(0.1, 9.0, 256)      # a prior's log density, either sign
    want, flags, _ = V.census(want_idx, acc0, c)
    assert flags["tie_free"].mean() >= 0.9 and not flags["fallback"].any()
    ff, seq = A.k_valued_sum_check(K, idx, tab, acc0, c)
    assert V.same_bits(seq, want).all()
    bad = np.nonzero(~V.same_bits(ff, want))[0]
    assert bad.size == 0, (bad[:5], c[bad[:5]].view(np.uint64), ff[bad[:5]], want[bad[:5]])


# ---- the product's route

BURN, SAMPLE = 70, 50      # 120 updates per parameter and chain (the issue asks for at least 40), across two adaptation batches; README.kval.md has the twins' measured times
CHAINS = 250               # a partial fourth wavefront


def _spec(golden, translated):
    rec = golden_io.load("user_" + golden)["chains"][0]
    params, init, opts = [], [], []
    for p in rec["params_completed"]:
        ln = int(np.prod(p["dim"]))
        params.append({"type": p["type"], "len": ln, "top": p["dim"][0], "multidim": 0 if p["dim"] == [1] else 1, "lower": p["lower"], "upper": p["upper"]})
        init += p["init"]
    for o in rec["comp_opts"]:
        opts.append({"prop_log_scale": o.get("prop_log_scale", 0.0), "max_adaptation": o.get("max_adaptation", 0.33), "initial_adaptation": o.get("initial_adaptation", 1.0),
                     "target_accept_rate": o.get("target_accept_rate", 0.44), "batch_size": o.get("batch_size", 50), "is_adapting": o.get("is_adapting", True)})
    return {"user": user_host.user_spec_part(*translated), "params": params, "P": len(init), "init": init, "comp_opts": opts}


@needs_node
@pytest.mark.parametrize("name,golden,marker", [("pois_const_rate", "pois_const_rate", "kval_loop_one_lane<"), ("binom_const_size", "binom_const_size", "kval_loop_one_lane<"),
                                                ("readme_bern", "readme_bern", "bern_loop_one_lane("), ("bench_bern", "readme_bern", "bern_loop_one_lane("),
                                                ("multi_bern", "multi_bern", None)])
def test_closure_equals_its_term_by_term_twin_in_every_chain(name, golden, marker):
    """hiprtc's build of the header, the JavaScript tables and the generated addends against a term-by-term sum of the same closure: the same seed, so the same
    uniforms -- one differing bit in one log_post changes an accept decision and with it the draws.  (bench_bern: readme_bern's closure and parameters over 10^5
    observations.  multi_bern has no data loop -- four binary parameters and `return expr` --, so neither translation of it calls a fast-forward; it stays in the
    list as the closure on which the option must change nothing at all.)"""
    fast, plain = user_host.translated(name), user_host.translated_with(name, {"no_fast_forward": True})
    for m in ("kval_loop_one_lane<", "bern_loop_one_lane("):
        assert (m in fast[0]) == (m == marker) and m not in plain[0]
    if marker is None:
        assert fast[0] == plain[0]
    got = []
    for tr in (fast, plain):
        t0 = time.time()
        s = A.Sampler(_spec(golden, tr), chains=CHAINS, seed=20261021, lanes_per_chain=1)
        assert s.launch_info()["lanes_per_chain"] == 1
        t1 = time.time()
        s.burn(BURN)
        draws = s.sample(SAMPLE, 1)
        got.append((draws, s.state(), s.info()["accepts"], s.diag()["log_post"]))
        print("%s %s: create %.2f s, %d updates x %d chains %.2f s" % (name, "fast-forward" if tr is fast else "term by term", t1 - t0, BURN + SAMPLE, CHAINS, time.time() - t1))
        s.close()
    (da, sa, aa, la), (db, sb, ab, lb) = got
    assert da.shape[0] == SAMPLE and da.shape[2] == CHAINS
    assert da.tobytes() == db.tobytes(), np.nonzero((da != db).any(axis=(0, 1)))[0][:8]
    assert sa.tobytes() == sb.tobytes() and aa.tobytes() == ab.tobytes()
    assert V.same_bits(la, lb).all(), np.nonzero(~V.same_bits(la, lb))[0][:8]
    assert np.isfinite(la).all() and (aa.sum(axis=0) > 0).mean() > 0.9      # (nearly) every chain accepted something: decisions were there to differ in
    if marker:      # real parameters: the chains moved, each its own way
        assert len(set(sa[0].tolist())) > CHAINS // 2
