"""-m gpu: the uniform stream under keys, chain ids and positions that need all six words of the Philox counter and key (tests/README.stream.md).

Block b of chain c under seed s is philox4x32_10({b_lo, b_hi, c_lo, c_hi}, {s_lo, s_hi}) (csrc/amwg_philox.h).  Stream level: the product's own stream classes,
driven one by one through amwg_stream_check (include/amwg_selftest.h), against the numpy twin synth.uniforms -- bytes.  Sampler level: every kernel kind under
KEY and OFFSET, every chain against its oracle chain.  No tolerance anywhere: every comparison is equality of bytes or of integers."""
import shutil

import numpy as np
import pytest

import amwg_ctypes as A
import model_spec
import oracle_lib
import stream_reference as R
from gpu_util import assert_chain_equals_oracle, run_schedule
from stream_reference import KEY, OFFSET, POSITIONS

pytestmark = pytest.mark.gpu
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")

N_DRAWS = 2 * 64 * 3 + 5      # three refills of the widest stream (128 uniforms per fill), and an odd count
NEXT_KINDS = [A.STREAM_CHAIN, 1, 2, 4, 8, 16, 32, 64, A.STREAM_WINDOW]


def _chains_of(kind):
    """every position of POSITIONS at least once, more than two wavefronts where chains share one, and a last wavefront that is not full"""
    lanes = kind if 1 <= kind <= 64 else (1 if kind in (A.STREAM_CHAIN, A.STREAM_PAIRS) else 64)
    return max(len(POSITIONS), 2 * (64 // lanes) + 3)


def _starts(n_chains, shift=0):
    """every chain at another position: the first 23 at POSITIONS themselves, the next 23 twelve uniforms on, ... -- the chains that share a wavefront are of mixed
    parity, some on either side of the block carry"""
    return [POSITIONS[(i + shift) % len(POSITIONS)] + 12 * (i // len(POSITIONS)) for i in range(n_chains)]


def _assert_draws(got, seed, chain0, starts, n_draws, what):
    for i, c0 in enumerate(starts):
        want = R.uniforms(seed, chain0 + i, c0, n_draws)
        assert np.ascontiguousarray(got["draws"][i]).tobytes() == want.tobytes(), (what, "chain", i, "from", c0)
    assert got["consumed"].tolist() == [c0 + n_draws for c0 in starts], what


def test_the_numpy_twin_equals_the_oracle_at_full_words():
    """the reference of this file against oracle/amwg_oracle.c, at an odd start, past the block carry and near 2^62"""
    L = oracle_lib.lib()
    for seed, chain, start in [(KEY, OFFSET + 5, 0), (2 ** 64 - 1, 2 ** 63 + 5, 2 * (2 ** 32 - 2) + 1), (2 ** 32, OFFSET, 2 ** 62 - 3), (7, 3, 129)]:
        u = R.uniforms(seed, chain, start, 9)
        assert u.tobytes() == np.array([L.orc_uniform(seed, chain, start + i) for i in range(9)]).tobytes(), (seed, chain, start)


KEY_CASES = [(s, 5) for s in R.SEEDS] + [(7, c) for c in R.CHAIN0S] + [(s, c) for s in R.SEEDS for c in R.CHAIN0S]


@pytest.mark.parametrize("kind", NEXT_KINDS)
def test_every_stream_class_under_64_bit_seeds_chain_ids_and_positions(kind):
    """next() of ChainStream, CoopStream<1 .. 64> and WindowStream: a high seed word alone, a high chain word alone (chain0 = 2^32 - 3: the carry into c3 falls
    between local chains 2 and 3 of one wavefront), both, and in each the chains of a wavefront at the positions of stream_reference.POSITIONS -- b_hi != 0 in
    some lanes of a fill and not in others."""
    n = _chains_of(kind)
    for j, (seed, chain0) in enumerate(KEY_CASES):
        starts = _starts(n, shift=j)
        _assert_draws(A.stream_check(kind, seed, chain0, starts, N_DRAWS), seed, chain0, starts, N_DRAWS, (kind, hex(seed), hex(chain0)))


def test_the_positions_cross_the_block_carry_inside_a_fill():
    """what the positions are chosen for (no GPU work: the arithmetic of tests/README.stream.md): the block number passes 2^32 inside one fill of a chain on
    2, 4, 8 and 64 lanes, exactly between two fills, inside the window's half B, and inside the half B computed after a shift()"""
    b0 = [p >> 1 for p in POSITIONS]
    for lanes in (2, 4, 8, 16, 32, 64):
        assert any(b < 2 ** 32 < b + lanes for b in b0), lanes
    assert any(b + 64 == 2 ** 32 for b in b0) and any(b + 64 < 2 ** 32 < b + 128 for b in b0) and any(b + 128 < 2 ** 32 < b + 192 for b in b0)
    assert {p & 1 for p in POSITIONS} == {0, 1} and any(p > 2 ** 61 for p in POSITIONS)
    for kind in NEXT_KINDS + [A.STREAM_PAIRS]:      # no two chains of a launch, let alone of a wavefront, start alike
        for shift in range(len(KEY_CASES)):
            starts = _starts(_chains_of(kind), shift)
            assert len(set(starts)) == len(starts)
            per_wave = 1 if kind == A.STREAM_WINDOW else 64 // (kind if 1 <= kind <= 64 else 1)
            for w in range(0, len(starts) - per_wave + 1, per_wave) if per_wave >= 8 else ():      # (eight chains or more to a wavefront: both parities, far from the carry and about to pass it)
                wave = starts[w:w + per_wave]
                assert {p & 1 for p in wave} == {0, 1} and min(wave) < 2 ** 33 - 300 and any(2 ** 33 - 300 < p < 2 ** 33 for p in wave), (kind, shift, w)


def _pair_positions(calls, parity):
    """the positions (amwg_philox.h stream_next_pair: 0, 1, or 2 = the next draw refills) at which the calls find the one-lane stream"""
    pos, seen = parity, set()
    for c in calls:
        seen.add((int(c), pos))
        pos = (1 if pos == 1 else 2) if c else (1 if pos == 2 else pos + 1)
    return seen


def test_one_lane_stream_under_mixed_single_and_pair_draws():
    """CoopStream<1>::next_pair (stream_next_pair: the refill at one call site) mixed with next(): the values are the plain sequence, the count is singles + 2 x pairs,
    and both calls meet the stream at each of its three positions"""
    rng = np.random.default_rng(20261020)
    patterns = {"alternating": np.tile([0, 1], 130), "pairs": np.ones(195, dtype=np.uint8), "single first": np.concatenate([[0], np.ones(194)])}
    for k in range(3):
        patterns["random %d" % k] = rng.integers(0, 2, 300)
    n, seen = _chains_of(A.STREAM_PAIRS), set()
    for j, (name, calls) in enumerate(patterns.items()):
        calls = np.asarray(calls, dtype=np.uint8)
        n_draws = int(calls.size + calls.sum())
        assert n_draws >= N_DRAWS
        seed, chain0 = R.SEEDS[j % 4], R.CHAIN0S[j % 2]
        starts = _starts(n, shift=j)
        _assert_draws(A.stream_check(A.STREAM_PAIRS, seed, chain0, starts, n_draws, calls=calls), seed, chain0, starts, n_draws, name)
        seen |= _pair_positions(calls, 0) | _pair_positions(calls, 1)
    assert seen == {(c, p) for c in (0, 1) for p in (0, 1, 2)}


@pytest.mark.parametrize("n_draws", [N_DRAWS, 300, 331])      # the sweep begins 5 / 6, 44 / 45 and 75 / 76 uniforms into half A
def test_window_reads_ahead_and_flags_pairs_as_rnorm_decides_them(n_draws):
    """WindowStream as a sweep uses it: after n_draws next() calls, position(), ensure_b(), per-lane at() over the 128 uniforms ahead; then shift(), ensure_b() and
    the whole window.  E? bit j: rnorm (mcmc.js:44-53) accepts the pair at the even position 2j of that half, O? bit j: at the odd position 2j + 1; OA bit 63 is the
    pair that straddles the halves, OB bit 63 is clear.  Starts: POSITIONS -- the carry of the block number between the halves, inside half B, and inside the half B that
    follows the shift()."""
    seed, chain0 = KEY, OFFSET
    starts = _starts(len(POSITIONS))
    got = A.stream_check(A.STREAM_WINDOW_AT, seed, chain0, starts, n_draws)
    _assert_draws(got, seed, chain0, starts, n_draws, "window")
    for i, c0 in enumerate(starts):
        b0, p = R.window_after(seed, chain0 + i, c0, n_draws)
        w = R.uniforms(seed, chain0 + i, 2 * b0, 512)
        a, b, c = w[:128], w[128:256], w[256:384]
        assert np.ascontiguousarray(got["ahead"][i]).tobytes() == w[p:p + 128].tobytes(), ("at() ahead", i, c0)
        assert np.ascontiguousarray(got["window"][i]).tobytes() == w[128:384].tobytes(), ("window after shift()", i, c0)
        ea, oa = R.half_flags(a, b[0])
        eb, ob = R.half_flags(b)
        f = [[int(v) for v in row] for row in got["flags"][i]]
        assert f[0] == [ea, oa, eb, ob], ("flags after ensure_b()", i, c0, [hex(v) for v in f[0]], [hex(v) for v in (ea, oa, eb, ob)])
        assert ob >> 63 == 0
        assert f[1][:2] == [eb, ob], ("flags after shift()", i, c0)
        ec, oc = R.half_flags(c)
        assert f[2] == [eb, R.half_flags(b, c[0])[1], ec, oc], ("flags after shift() and ensure_b()", i, c0)


# ---- sampler level: every kernel kind under a full key.  Every chain against oracle_lib.OracleChain(spec, KEY, OFFSET + c, lanes = the kernel's summation order)

SCHEDULE = [{"op": "burn", "n": 60}, {"op": "sample", "n": 60, "thin": 3}, {"op": "burn", "n": 7}, {"op": "sample", "n": 10, "thin": 1}]
SPL = 17      # (steps per launch, odd: the launches resume at both parities of the stream)


def _against_oracle(s, oracle_spec, chains, offset=OFFSET, group_local=False, P=None):
    order = s.launch_info()["summation_order"]
    segs = run_schedule(s, SCHEDULE)
    if P is not None:
        segs = [g[:, :P, :] for g in segs]
    for c in range(chains):
        o = oracle_lib.OracleChain(oracle_spec, KEY, offset + c, lanes=order, group_local=group_local)
        assert_chain_equals_oracle(s, c, o, segs, run_schedule(o, SCHEDULE))
    return segs


def _launch(s, kernel, lanes, block, grid, order):
    li = s.launch_info()
    assert li["kernel"].startswith(kernel), li
    assert (li["lanes_per_chain"], li["block_threads"], li["grid_blocks"], li["summation_order"]) == (lanes, block, grid, order), li


def _hier_spec(n_obs, G):
    """labels that repeat with the lane stride (g_i = (i mod 64) mod G): what the row layout of the sweep kernels needs"""
    rng = np.random.default_rng(330)
    g = ((np.arange(n_obs) % 64) % G).astype(np.int32)
    x = rng.normal(5.0, 3.0, G)[g] + rng.normal(0.0, 2.0, n_obs)
    return model_spec.build_spec("hier_normal", {"x": x, "g": g, "G": G})


def _family_cases():
    normal = lambda n: model_spec.build_spec("normal", model_spec.make_data("normal", n, 41))
    glm = lambda: model_spec.build_spec("pois_glm", model_spec.make_data("pois_glm", 240, 43, exp=oracle_lib.lib().orc_exp))
    bern = lambda: model_spec.build_spec("beta_bern", model_spec.make_data("beta_bern", 300, 42))
    hier = lambda: _hier_spec(330, 5)
    # id: (spec, chains, options, kernel, lanes, block, grid, summation order, group-local oracle)
    return {
        "normal_cert": (lambda: normal(100), 16, dict(lanes_per_chain=1, block_threads=64), "amwg_step_kernel_cert<NormalModel,1,256>", 1, 64, 1, 1, False),
        "normal_sufficient": (lambda: normal(100), 16, dict(lanes_per_chain=1, block_threads=64, sufficient_statistics=1), "amwg_step_kernel_cert<NormalModel,1,256>", 1, 64, 1, 1, False),
        "normal_expression": (lambda: normal(100), 16, dict(lanes_per_chain=1, block_threads=64, full_evaluation=1), "amwg_step_kernel<NormalModel,1,256>", 1, 64, 1, 1, False),
        "normal_two_wavefronts": (lambda: normal(1000), 8, dict(lanes_per_chain=128), "amwg_step_kernel<NormalModel,128,", 128, 128, 8, 128, False),
        "bern_fast_forward": (bern, 16, dict(lanes_per_chain=1, block_threads=64), "amwg_step_kernel<BetaBernModel,1,", 1, 64, 1, 1, False),
        "glm_cert_16": (glm, 16, dict(lanes_per_chain=16, block_threads=64), "amwg_step_kernel_cert<PoisGlmModel,16,256>", 16, 64, 4, 1, False),
        "hier_sweep": (hier, 8, dict(lanes_per_chain=64, block_threads=64), "amwg_sweep_kernel_cert<HierNormalModel", 64, 64, 8, 1, False),
        "hier_sweep_expression": (hier, 8, dict(lanes_per_chain=64, block_threads=64, full_evaluation=2), "amwg_sweep_kernel<HierNormalModel", 64, 64, 8, 64, False),
        "hier_group_local": (hier, 8, dict(group_local=1, block_threads=64), "amwg_gl_kernel<HierGlModel", 64, 64, 8, 64, True),
    }


@pytest.mark.parametrize("case", list(_family_cases()))
def test_every_family_kernel_under_a_full_key_equals_the_oracle_in_every_chain(case):
    """seed KEY, chain ids OFFSET + c (c3 = 1 from local chain 3 on), launches of 17 steps: draws, counters, scales, state, uniforms consumed, named_order and log_post
    of every chain.  Each case asserts the kernel and the geometry it ran."""
    make, chains, opts, kernel, lanes, block, grid, order, gl = _family_cases()[case]
    spec = make()
    s = A.Sampler(spec, chains=chains, seed=KEY, chain_offset=OFFSET, steps_per_launch=SPL, **opts)
    _launch(s, kernel, lanes, block, grid, order)
    _against_oracle(s, spec, chains, group_local=gl)
    s.close()


@needs_node
def test_a_translated_closure_at_one_lane_under_a_full_key_equals_the_oracle_in_every_chain():
    """a hiprtc build: the key passes through another compilation of the same headers.  Oracle: its stepper over the host build of the closure's generated text."""
    from test_gpu_user import spec_for
    from test_translate import oracle_spec
    spec, m, _ = spec_for("modern_js")
    assert m.meta.get("cert_tail_n", 0) == 0
    s = A.Sampler(spec, chains=16, seed=KEY, chain_offset=OFFSET, lanes_per_chain=1, block_threads=64, steps_per_launch=SPL)
    li = s.launch_info()
    assert (li["kernel"], li["lanes_per_chain"], li["block_threads"], li["grid_blocks"], li["summation_order"]) == ("amwg_user_step", 1, 64, 1, 1), li
    _against_oracle(s, oracle_spec("modern_js")[0], 16, P=s.P)
    s.close()


@needs_node
def test_a_closure_with_a_certified_tail_under_a_full_key_equals_the_oracle_in_every_chain():
    from test_gpu_geometry import _user
    import user_host
    fam = model_spec.build_spec("normal", {"x": user_host.translated("bench_normal_n65")[1][0]})
    spec, oracle_spec, arrays, meta, _ = _user("bench_normal_n65", fam["params"], fam["init"])
    assert meta["cert_tail_n"] == len(arrays[0]) == 65
    s = A.Sampler(spec, chains=16, seed=KEY, chain_offset=OFFSET, lanes_per_chain=1, block_threads=64, steps_per_launch=SPL)
    li = s.launch_info()
    assert (li["kernel"], li["lanes_per_chain"], li["block_threads"], li["grid_blocks"], li["summation_order"]) == ("amwg_user_step_cert", 1, 64, 1, 1), li
    _against_oracle(s, oracle_spec, 16, P=s.P)
    s.close()


def test_a_dataset_sampler_whose_chain_ids_carry_inside_a_dataset():
    """Normal, 3 datasets x 16 chains from chain id 2^32 - 20: the carry into c3 falls on local chain 20, inside dataset 1 (and inside its wavefront).  A workgroup
    serves one dataset, so 16 chains per dataset are 4 lanes per chain in one-wavefront workgroups.  Every chain against the oracle chain on its dataset; and the same
    run through summarize() leaves state(), info() and diag() as the stored run's."""
    off, cpd, D = 2 ** 32 - 20, 16, 3
    specs = [model_spec.build_spec("normal", model_spec.make_data("normal", 100, 50 + d)) for d in range(D)]
    kw = dict(chains=D * cpd, seed=KEY, chain_offset=off, lanes_per_chain=4, block_threads=64, steps_per_launch=SPL)
    s = A.Sampler(specs, **kw)
    li = s.launch_info()
    assert li["kernel"] == "amwg_step_kernel_ds<NormalModel,4,256>" and (li["datasets"], li["block_threads"], li["grid_blocks"], li["summation_order"]) == (D, 64, D, 4), li
    segs = run_schedule(s, SCHEDULE)
    for c in range(D * cpd):
        o = oracle_lib.OracleChain(specs[c // cpd], KEY, off + c, lanes=4)
        assert_chain_equals_oracle(s, c, o, segs, run_schedule(o, SCHEDULE))
    t = A.Sampler(specs, **kw)
    thin = 1
    for seg in SCHEDULE:
        if seg["op"] == "burn":
            t.burn(seg["n"])
        else:
            thin = seg.get("thin", thin)
            assert t.summarize(seg["n"], thin) == -(-seg["n"] // thin)
    assert t.state().tobytes() == s.state().tobytes()
    for k, v in s.info().items():
        assert t.info()[k].tobytes() == v.tobytes(), k
    for k, v in s.diag().items():
        assert t.diag()[k].tobytes() == v.tobytes(), k
    s.close()
    t.close()
