"""-m gpu: the two-valued exact fast-forward (csrc/amwg_twoval.h two_valued_sum) ON THE DEVICE against the plain sequential sum (README.twoval.md).

* The building block (amwg_two_valued_sum_check, lane j = thread j of 64-thread workgroups: every wavefront holds 64 different cases): device fast-forward ==
  device plain loop == numpy plain sum, the same bits or both NaN, on every lane of every case of tests/twoval_cases.py -- the cases tests/test_twoval_host.py
  runs through the host build, whose census conditions are asserted there and here -- and the same lanes through amwg_k_valued_sum_check at K = 2 on
  kval_cases.tables: a fourth implementation, written independently.  Per case m = 2 048 lanes:
      0 ..   63   addends -exp(U(-12, 3)) with floor(52 u^2) trailing significand bits cleared and the bit above set in half of them (one lane in eight: addends
                  -exp(U(-80, 3))); starting sums half N(0, 3), half -exp(U(-5, 25)) -- as are all lanes not listed below
     64 ..  127   start at -2^(40 .. 84): stalls
    128 ..  141   an addend -inf, NaN, +0.25, 0.0, -0.0, -5e-324, -1e-310: as l1 (128 .. 134), as l0 (135 .. 141) -- summed term by term by the header
    142 ..  147   equal addends              148 .. 153   addends in the ratio 2^(+-1 .. 3)              154 .. 159   both addends powers of two
    160 ..  163   start at 0.0, -0.0, 1e300, -1e300
    164 ..  195   start 1 .. 4 ulps below a power of two, 1 .. 12 binades above the larger addend
    196 ..  259   land EXACTLY on 2^54 (ulp 2, addends -1 .. -6) after 32, 64, 33, 31, 1, 96, 1000, n, n - 1, ... observations: without a tie and in modes 1, 2, 3
    260 ..  267   the product n * d of the first probe is k 2^64 + a little (where the data has >= 4 097 of a value)
    268 ..  291   a tying addend of exactly half an ulp on a sum that otherwise stalls: either value, A odd and even, beside 1/4 ulp, 2^-70 of it, or itself
    292 .. 1315   CONSTRUCTED for a visit of >= 64 observations in mode 1 (lane - 292 = 0 mod 4), mode 2 (1 mod 4) or mode 3 (2, 3 mod 4), either value tying
   1316 .. 2047   as 0 .. 63
* Every copy of the table recipe -- the library's (amwg_create.hip), the translator's (translate.js, the #aux:twoval: arrays) and the restated one -- gives the
  same bytes.
* The Beta-Bernoulli family at one lane per chain with its tables in LDS and, beyond kFfLdsLimit, in HBM, against its term-by-term twin.
* A `ld.bern` closure on structured data against its no_fast_forward twin, every chain."""
import shutil
import time

import numpy as np
import pytest

import amwg_ctypes as A
import kval_cases
import model_spec
import twoval_cases as V
import user_host
from test_gpu_kval import _spec

pytestmark = pytest.mark.gpu
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


@pytest.mark.parametrize("n,kind", V.case_list())
def test_device_fast_forward_equals_device_loop_equals_plain_sum(n, kind):
    c = V.case(n, kind)
    ff, seq = A.two_valued_sum_check(c["x"], c["acc0"], c["l1"], c["l0"])
    # K = 2 of the K-valued header: value index = the observation, addends (l0, l1), the K-valued tables restated in tests/kval_cases.py
    kff, kseq = A.k_valued_sum_check(2, c["x"], kval_cases.tables(c["x"], 2), c["acc0"], np.stack([c["l0"], c["l1"]], axis=1))
    for what, got in (("device plain loop", seq), ("device fast-forward", ff), ("K-valued plain loop", kseq), ("K-valued fast-forward at K = 2", kff)):
        bad = np.nonzero(~V.same_bits(got, c["want"]))[0]
        assert bad.size == 0, (what, bad.size, bad[:5], c["acc0"][bad[:5]], c["l1"][bad[:5]].view(np.uint64), c["l0"][bad[:5]].view(np.uint64), got[bad[:5]], c["want"][bad[:5]],
                               {f: int(v[bad].sum()) for f, v in c["flags"].items() if v[bad].any()})
    assert V.same_bits(ff, seq).all() and V.same_bits(ff, kff).all()


def test_census_conditions():
    """the cases arrive where the header is intricate (conditions on the inputs, computed on the CPU; tests/test_twoval_host.py asserts the same)"""
    V.check_census_conditions()


def test_lanes_in_a_partial_wavefront_and_no_lanes():
    c = V.case(777, "runs_32k")
    for m in (1, 63, 65, 100):
        ff, seq = A.two_valued_sum_check(c["x"], c["acc0"][:m], c["l1"][:m], c["l0"][:m])
        assert V.same_bits(ff, c["want"][:m]).all() and V.same_bits(seq, c["want"][:m]).all()
    sl = slice(V.CONSTRUCTED.start, V.CONSTRUCTED.start + 100)      # a partial second wavefront of constructed lanes
    ff, seq = A.two_valued_sum_check(c["x"], c["acc0"][sl], c["l1"][sl], c["l0"][sl])
    assert V.same_bits(ff, c["want"][sl]).all() and V.same_bits(seq, c["want"][sl]).all()
    ff, seq = A.two_valued_sum_check(c["x"], c["acc0"][:0], c["l1"][:0], c["l0"][:0])
    assert ff.size == 0 and seq.size == 0


# ---- the table recipe, three times

def translators_tables(name):
    """-> (x, tab) of a closure whose loop the translator hands to two_valued_sum: the data array and the array under its #aux:twoval: key"""
    src, arrays, meta = user_host.translated(name)
    keys = meta["array_keys"]
    t = [j for j, k in enumerate(keys) if k.startswith("#aux:twoval:")]
    assert len(t) == 1 and meta["array_types"][t[0]] == 2 and "bern_loop_one_lane(" in src      # i32 words
    x = arrays[int(keys[t[0]].split(":")[2])]
    assert set(x.tolist()) <= {0.0, 1.0}
    return x.astype(np.uint8), (arrays[t[0]].astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def test_every_copy_of_the_table_recipe_gives_the_same_bytes():
    for n, kind in V.case_list():      # the library's own (what the samplers and the check entry upload) against the restated recipe
        c = V.case(n, kind)
        got = A.two_valued_tables(c["x"])
        assert got.dtype == np.uint32 and got.tobytes() == c["tab"].tobytes(), (n, kind, np.nonzero(got != c["tab"])[0][:5])
    assert A.two_valued_tables(np.array([0, 7, 255, 1], dtype=np.uint8)).tobytes() == V.tables_flat(np.array([0, 1, 1, 1], dtype=np.uint8)).tobytes()      # non-zero = 1
    if shutil.which("node") is None:
        pytest.skip("node is not installed: the translator's copy was not compared")
    for name, n in (("readme_bern", 2000), ("bench_bern", 100000), ("bern_alternating", 777), ("bern_runs_32k", 777)):
        x, tab = translators_tables(name)
        assert x.size == n and tab.tobytes() == V.tables_flat(x).tobytes() and tab.tobytes() == A.two_valued_tables(x).tobytes(), name


# ---- the family: tables in LDS and in HBM

LDS_LIMIT = 120 * 1024      # csrc/amwg_models.h BetaBernModel::kFfLdsLimit
table_bytes = lambda n: 6 * (n // 32 + 2) * 4
N_LAST_LDS = max(n for n in range(163000, 165000) if table_bytes(n) <= LDS_LIMIT)      # 163 807: the last size whose six tables fit


def _family_data(n, kind):
    return V.sequence(n, kind, np.random.default_rng([17, n, V.KINDS.index(kind)])).astype(np.float64)


@pytest.mark.parametrize("n,kind,chains", [(N_LAST_LDS, "iid_50", 128), (N_LAST_LDS, "runs_32k", 100), (N_LAST_LDS + 1, "iid_50", 100), (N_LAST_LDS + 1, "runs_32k", 128),
                                           (200000, "iid_50", 128), (200000, "runs_32k", 100)])
def test_family_tables_in_lds_and_in_hbm(n, kind, chains):
    """Beta-Bernoulli, one lane per chain: up to n = 163 807 the six tables are staged into LDS, from 163 808 on they stay in HBM (lds_bytes returns 0, stage returns
    early) -- the branch no other sampler of the suite reaches (the largest has n = 10^5).  Either side against the term-by-term twin (exact_division = 1), chain by
    chain, from ordinary and extreme starting points; 100 chains: a partial second wavefront."""
    assert N_LAST_LDS == 163807 and table_bytes(N_LAST_LDS) == LDS_LIMIT and table_bytes(N_LAST_LDS + 1) > LDS_LIMIT
    spec = model_spec.build_spec("beta_bern", {"x": _family_data(n, kind)}, hyper=[2, 2])
    t0 = time.time()
    a = A.Sampler(spec, chains=chains, seed=5, lanes_per_chain=1)
    b = A.Sampler(spec, chains=chains, seed=5, lanes_per_chain=1, exact_division=1)
    ia = a.launch_info()
    assert ia["lanes_per_chain"] == 1
    if n <= N_LAST_LDS:      # the workgroup's dynamic LDS holds the tables -- or it cannot
        assert ia["lds_bytes"] >= table_bytes(n), ia
    else:
        assert ia["lds_bytes"] < table_bytes(N_LAST_LDS), ia
    rng = np.random.default_rng(1)
    start = rng.uniform(0, 1, (1, chains))
    start[0, :12] = [0.0, 1.0, 1e-300, 1e-12, 1 - 1e-12, 0.5, 2.0 ** -30, 1 - 2.0 ** -30, 0.3, 5e-324, np.nextafter(1.0, 0), np.nextafter(0.0, 1)]
    for s in (a, b):
        s.set_state(start)
        s.burn(0)
    la, lb = a.diag()["log_post"], b.diag()["log_post"]
    same = V.same_bits(la, lb)
    assert same.all(), (np.where(~same)[0][:5], la[~same][:5], lb[~same][:5], start[0, ~same][:5])
    ready, took = time.time() - t0, []
    for s in (a, b):
        t1 = time.time()
        s.burn(60)
        d = s.sample(40, 2)
        took.append((time.time() - t1, d))
    print("n = %d %s, %d chains, lds_bytes %d (tables %d bytes): create both + first log_post %.2f s, 140 updates fast-forward %.3f s, term by term %.3f s"
          % (n, kind, chains, ia["lds_bytes"], table_bytes(n), ready, took[0][0], took[1][0]))
    assert took[0][1].tobytes() == took[1][1].tobytes()
    assert a.info()["accepts"].tolist() == b.info()["accepts"].tolist()
    assert a.diag()["log_post"].tobytes() == b.diag()["log_post"].tobytes()
    assert (a.info()["accepts"].sum(axis=0) > 0).mean() > 0.9      # decisions were there to differ in
    a.close()
    b.close()


# ---- the closure route on structured data

CHAINS = 250      # a partial fourth wavefront


@needs_node
@pytest.mark.parametrize("name", ["bern_alternating", "bern_runs_32k"])
def test_closure_on_structured_data_equals_its_term_by_term_twin_in_every_chain(name):
    """hiprtc's build of the header and the JavaScript tables on data whose run parities the one-tie closed form depends on: 777 observations strictly alternating,
    and in runs that end one before, on and one behind a word boundary (tests/js/user_models.js).  tests/test_gpu_kval.py has the same leg on independent draws."""
    fast, plain = user_host.translated(name), user_host.translated_with(name, {"no_fast_forward": True})
    assert "bern_loop_one_lane(" in fast[0] and "bern_loop_one_lane(" not in plain[0]
    x = fast[1][0].astype(np.int64)
    assert x.size == 777
    if name == "bern_alternating":
        assert (np.diff(x) != 0).all()
    else:
        edges = np.flatnonzero(np.diff(x)) + 1
        runs = np.diff(np.concatenate([[0], edges]))
        assert set((edges % 32).tolist()) == {31, 0, 1} and set((runs % 32).tolist()) == {31, 0, 1}
    got = []
    for tr in (fast, plain):
        s = A.Sampler(_spec("readme_bern", tr), chains=CHAINS, seed=20261021, lanes_per_chain=1)
        assert s.launch_info()["lanes_per_chain"] == 1
        s.burn(70)
        draws = s.sample(50, 1)
        got.append((draws, s.state(), s.info()["accepts"], s.diag()["log_post"]))
        s.close()
    (da, sa, aa, la), (db, sb, ab, lb) = got
    assert da.shape[0] == 50 and da.shape[2] == CHAINS
    assert da.tobytes() == db.tobytes(), np.nonzero((da != db).any(axis=(0, 1)))[0][:8]
    assert sa.tobytes() == sb.tobytes() and aa.tobytes() == ab.tobytes()
    assert V.same_bits(la, lb).all(), np.nonzero(~V.same_bits(la, lb))[0][:8]
    assert np.isfinite(la).all() and (aa.sum(axis=0) > 0).mean() > 0.9 and len(set(sa[0].tolist())) > CHAINS // 2
