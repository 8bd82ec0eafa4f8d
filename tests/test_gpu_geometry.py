"""-m gpu: the certified kernels in every launch geometry the host can launch them in.

The certified kernels (csrc/amwg_kernel.h "certified decisions") decide an accept test from a cheaper value of log_post and a bound, and fall back
to the reference's expression inside the bound: every bit of every chain must be what the expression gives.  The parity tests check that at the
geometries their chain counts happen to produce; here every workgroup class is asked for explicitly (options.block_threads), chain counts leave the
last wavefront and workgroup partly filled (the dead lanes shadow chain C - 1: csrc/amwg_kernel.h), and data sizes sit on either side of the pass's
blocks and of the LDS tile's limit.

Reference of every case: the same spec at one lane per chain in 64-thread workgroups with options.full_evaluation = 1 -- the expression in the
reference's order in every update.  Independent check: two chains per case (one of them C - 1) against the CPU oracle.  Every case asserts the
kernel, class and geometry it ran (launch_info): a case that silently falls back to another kernel fails."""
import os
import shutil

import numpy as np
import pytest

import amwg_ctypes as A
import model_spec
import oracle_lib
from gpu_util import assert_chain_equals_oracle

pytestmark = pytest.mark.gpu

SEED, OFFSET, SPL = 8, 3, 13      # (SPL: steps per launch, odd -- a launch ends by evaluating the expression, mid-schedule)
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def _schedule(s, steps, oracle=False):
    """sample with thin, burn, adaptation off and on, a state overwritten from the host (chains c = 1 mod 3 but the last, param 0), burn, sample.
    The oracle has no set_state: it runs the same schedule without it, and is compared only at chains the overwrite leaves alone."""
    seq = [s.sample(steps // 4, 3)]
    s.burn(steps // 2)
    s.set_adapting(False)
    seq.append(s.sample(steps // 8, 1))
    s.set_adapting(True)
    if not oracle:
        st = s.state()
        st[0, 1:s.C - 1:3] += 0.25
        s.set_state(st)
    s.burn(steps // 8)
    seq.append(s.sample(steps // 8 + 4, 2))
    return seq


def _run(s, steps):
    seq = _schedule(s, steps)
    return {"draws": [x.tobytes() for x in seq], "info": {k: v.tobytes() for k, v in s.info().items()}, "uniforms": s.diag()["uniforms"].tobytes(),
            "log_post": s.diag()["log_post"].tobytes(), "state": s.state().tobytes(), "segs": seq}


def _assert_same(got, want):
    for i, (x, y) in enumerate(zip(got["draws"], want["draws"])):
        assert x == y, "draws of sample call %d" % i
    for k in want["info"]:
        assert got["info"][k] == want["info"][k], k
    assert got["uniforms"] == want["uniforms"], "uniforms"
    assert got["log_post"] == want["log_post"], "cached log_post"
    assert got["state"] == want["state"], "state"


def _oracle_chains(C):
    """two chains the host overwrite leaves alone, one of them C - 1: the chain the dead lanes of a partial wavefront shadow"""
    mid = C // 2
    while mid % 3 == 1:
        mid += 1
    return sorted({C - 1, mid})


def _check_oracle(s, spec, C, segs, steps, oracles):
    """s against the CPU oracle (summation order 1) at _oracle_chains(C); `oracles` caches the oracle runs by chain"""
    for local in _oracle_chains(C):
        if local not in oracles:
            o = oracle_lib.OracleChain(spec, SEED, OFFSET + local, lanes=1)
            oracles[local] = (o, _schedule(o, steps, oracle=True))
        o, osegs = oracles[local]
        assert_chain_equals_oracle(s, local, o, segs, osegs)


def _geometry(s, kernel, block, grid):
    li = s.launch_info()
    assert (li["kernel"], li["block_threads"], li["grid_blocks"], li["summation_order"]) == (kernel, block, grid, 1), li
    assert li["lanes_per_chain"] == 1 or "PoisGlmModel,16" in kernel, li


def _grid(C, per_block):
    return -(-C // per_block)


# ---- Normal family, one lane per chain

NOBS = [1, 7, 511, 512, 513, 1023, 1024, 1025, 12288, 12289, 30000]    # around 8 x 64 and 16 x 64 (the 512- / 256-class blocks), the LDS tile's limit (12 288), global memory
BLOCKS = [64, 128, 256, 512, 1024]
CHAINS = [2113, 37, 1]        # 64 * 33 + 1: a partial last wavefront and workgroup in every class
STEPS = 400


def _normal_cases():
    cases = []
    for bi, bt in enumerate(BLOCKS):
        for ni, n in enumerate(NOBS):
            C = CHAINS[(bi + ni) % 3]
            if bt == 512 and n in (513, 12289, 30000):
                C = 2113
            cases.append((bt, C, n, ""))
    for n in (7, 513, 1025, 12289, 30000):
        cases += [(256, 2113, n, "no_scratch"), (512, 2113, n, "no_scratch"), (512, 2113, n, "sufficient"), (1024, 2113, n, "sufficient"),
                  (512, 2113, n, "shift14"), (512, 2113, n, "shift40")]
    return sorted(cases, key=lambda c: (c[2], c[1], c[0], c[3]))      # (cases that share a reference run one after the other)


_normal_refs = {}


def _normal_spec(n):
    return model_spec.build_spec("normal", model_spec.make_data("normal", n, 31))


def _normal_ref(C, n):
    """the expression in the reference's order at one lane in 64-thread workgroups; the oracle runs of two of its chains"""
    key = (C, n)
    if key not in _normal_refs:
        _normal_refs.clear()
        spec = _normal_spec(n)
        r = A.Sampler(spec, chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, block_threads=64, steps_per_launch=SPL, full_evaluation=1)
        _geometry(r, "amwg_step_kernel<NormalModel,1,256>", 64, _grid(C, 64))
        out = _run(r, STEPS)
        r.close()
        _normal_refs[key] = (spec, out, {})
    return _normal_refs[key]


@pytest.mark.parametrize("block,chains,n_obs,variant", _normal_cases())
def test_certified_normal_kernel_equals_the_expression_in_every_geometry(block, chains, n_obs, variant):
    """amwg_step_kernel_cert<NormalModel,1,{256,512,1024}> -- the wavefront's pass with blocks of 16 / 8 observations, the scalar-path pass of the 1024-thread
    class -- in every workgroup size, with and without the wave scratch (AMWG_WAVE_SCRATCH=0: v_readlane), with sufficient statistics, with the bound widened
    2^14- and 2^40-fold: every bit of every chain equals the expression's."""
    spec, ref, oracles = _normal_ref(chains, n_obs)
    kw = dict(chains=chains, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, block_threads=block, steps_per_launch=SPL)
    if variant == "no_scratch":
        os.environ["AMWG_WAVE_SCRATCH"] = "0"
        try:
            s = A.Sampler(spec, **kw)
        finally:
            del os.environ["AMWG_WAVE_SCRATCH"]
    else:
        s = A.Sampler(spec, sufficient_statistics=int(variant == "sufficient"), test_bound_shift={"shift14": 14, "shift40": 40}.get(variant, 0), **kw)
    _geometry(s, "amwg_step_kernel_cert<NormalModel,1,%d>" % max(block, 256), block, _grid(chains, block))
    got = _run(s, STEPS)
    _assert_same(got, ref)
    _check_oracle(s, spec, chains, got["segs"], STEPS, oracles)
    s.close()


def test_auto_geometry_at_131109_chains_is_the_512_class_and_equals_the_expression():
    """From 131 072 chains on the host picks 512-thread workgroups by itself (at least one per CU): the certified kernel with blocks of 8
    (csrc/amwg_plan.hip choose_geometry).  131 072 + 37 chains: the last workgroup holds one partial wavefront."""
    C, n, steps = 131072 + 37, 1000, 48
    spec = _normal_spec(n)
    s = A.Sampler(spec, chains=C, seed=SEED, chain_offset=OFFSET, steps_per_launch=SPL)
    _geometry(s, "amwg_step_kernel_cert<NormalModel,1,512>", 512, _grid(C, 512))
    r = A.Sampler(spec, chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, steps_per_launch=SPL, full_evaluation=1)
    assert r.launch_info()["kernel"].startswith("amwg_step_kernel<NormalModel,1,") and r.launch_info()["summation_order"] == 1
    got, want = _run(s, steps), _run(r, steps)
    _assert_same(got, want)
    _check_oracle(s, spec, C, got["segs"], steps, {})
    s.close()
    r.close()


# ---- Poisson family, 16 lanes per chain (four chains to a wavefront): partial wavefronts

@pytest.mark.parametrize("block,chains,n_obs", [(b, c, n) for b in (64, 256) for c in (3, 1027) for n in (61, 449)])
def test_certified_poisson_kernel_with_a_partial_wavefront_equals_the_expression(block, chains, n_obs):
    """amwg_step_kernel_cert<PoisGlmModel,16,256> with a wavefront that holds fewer than its four chains: the rows the four chains share are still
    read for the dead ones.  Reference: one lane per chain, the expression in every update (summation order 1)."""
    spec = model_spec.build_spec("pois_glm", model_spec.make_data("pois_glm", n_obs, 123, exp=oracle_lib.lib().orc_exp))
    kw = dict(chains=chains, seed=SEED, chain_offset=OFFSET, steps_per_launch=SPL)
    s = A.Sampler(spec, lanes_per_chain=16, block_threads=block, **kw)
    _geometry(s, "amwg_step_kernel_cert<PoisGlmModel,16,256>", block, _grid(chains, block // 16))
    r = A.Sampler(spec, lanes_per_chain=1, block_threads=64, full_evaluation=1, **kw)
    _geometry(r, "amwg_step_kernel<PoisGlmModel,1,256>", 64, _grid(chains, 64))
    steps = 300
    got, want = _run(s, steps), _run(r, steps)
    _assert_same(got, want)
    _check_oracle(s, spec, chains, got["segs"], steps, {})
    s.close()
    r.close()


# ---- translated closures with a certified tail (translate.js tailPlan, csrc/amwg_user.h)

def _user(name, params, init):
    import user_host
    src, arrays, meta = user_host.translated(name)
    opt = dict(model_spec.DEFAULT_OPT)
    spec = {"user": user_host.user_spec_part(src, arrays, meta), "P": len(init), "init": list(init), "comp_opts": [dict(opt) for _ in init], "params": params}
    m = user_host.host_model(name)
    oracle_spec = {"log_post_fn": lambda st, lanes: m.eval(st, 1), "params": params, "P": len(init), "init": list(init), "comp_opts": spec["comp_opts"]}
    return spec, oracle_spec, arrays, meta, m


_tail_refs = {}
TAIL_STEPS = 200


def _tail_ref(name, C):
    """the closure with full_evaluation = 1 at one lane in 64-thread workgroups; the hand-written Normal family on the same data gives the same bits"""
    key = (name, C)
    if key not in _tail_refs:
        _tail_refs.clear()
        import user_host
        fam = model_spec.build_spec("normal", {"x": user_host.translated(name)[1][0]})
        spec, oracle_spec, arrays, meta, _ = _user(name, fam["params"], fam["init"])
        assert meta["cert_tail_n"] == len(arrays[0])
        kw = dict(chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, block_threads=64, steps_per_launch=SPL)
        r = A.Sampler(spec, full_evaluation=1, **kw)
        _geometry(r, "amwg_user_step", 64, _grid(C, 64))
        f = A.Sampler(fam, **kw)
        _geometry(f, "amwg_step_kernel_cert<NormalModel,1,256>", 64, _grid(C, 64))
        out, fout = _run(r, TAIL_STEPS), _run(f, TAIL_STEPS)
        _assert_same(fout, out)
        r.close()
        f.close()
        _tail_refs[key] = (spec, oracle_spec, out, {})
    return _tail_refs[key]


@needs_node
@pytest.mark.parametrize("name,block,chains", [(nm, b, c) for nm in ("bench_normal", "bench_normal_n65") for c in (1, 65, 2113) for b in (64, 256, 512, 1024)])
def test_certified_tail_of_a_closure_equals_the_expression_in_every_geometry(name, block, chains):
    """amwg_user_step_cert at one lane per chain: the wavefront's pass in workgroups of up to 256 threads, the uniform pass over tail_x_global above
    (csrc/amwg_user.h) -- every bit of every chain equals the closure evaluated in every update, and the hand-written family's.  bench_normal's 80 KB of
    observations and the state of 1 024 chains do not fit one CU's LDS together: that workgroup size is refused, not replaced by another."""
    spec, oracle_spec, ref, oracles = _tail_ref(name, chains)
    kw = dict(chains=chains, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, block_threads=block, steps_per_launch=SPL)
    if name == "bench_normal" and block == 1024:
        with pytest.raises(A.AmwgError, match="no launch geometry fits"):
            A.Sampler(spec, **kw)
        return
    s = A.Sampler(spec, **kw)
    _geometry(s, "amwg_user_step_cert", block, _grid(chains, block))
    got = _run(s, TAIL_STEPS)
    _assert_same(got, ref)
    _check_oracle(s, oracle_spec, chains, got["segs"], TAIL_STEPS, oracles)
    s.close()


# ---- the replica fallback with a certified tail: 64-thread workgroups of fewer than 64 chains

INF = float("inf")
REPLICA_PARAMS = [{"type": "real", "len": 300, "top": 300, "multidim": 1, "lower": -INF, "upper": INF},
                  {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": -INF, "upper": INF},
                  {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": 0.0, "upper": INF}]
REPLICA_INIT = [0.0] * 300 + [0.5, 0.5]


@needs_node
def test_replica_fallback_with_a_certified_tail_has_a_scratch_line_per_wavefront():
    """theta of dim [300]: 64 chains' LDS state does not fit, so the host launches 64-thread workgroups that hold fewer chains each (the replica fallback,
    StepArgs::cpb) -- C / cpb wavefronts, each with its line of the wave scratch (csrc/amwg_pass.h wave_scratch_of).  Sized for C / 64 + 64 lines, as it was,
    the buffer was too small for this launch; the host now sizes it per geometry and refuses a launch it does not cover.  Every bit against the closure
    evaluated in every update and against the bound widened 2^40-fold; cached log_post against the host build of the same text; two chains against the oracle."""
    C, steps = 8205, 24
    spec, oracle_spec, arrays, meta, m = _user("bench_replica_tail", REPLICA_PARAMS, REPLICA_INIT)
    assert meta["cert_tail_n"] == 1000 and len(arrays[0]) == 1000
    kw = dict(chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, steps_per_launch=SPL)
    s = A.Sampler(spec, **kw)
    li = s.launch_info()
    assert (li["kernel"], li["block_threads"], li["summation_order"]) == ("amwg_user_step_cert", 64, 1), li
    assert li["grid_blocks"] > C // 64 + 64, li          # more wavefronts than the old C / 64 + 64 lines
    runs = [s, A.Sampler(spec, full_evaluation=1, **kw), A.Sampler(spec, test_bound_shift=40, **kw)]
    assert [q.launch_info()["kernel"] for q in runs] == ["amwg_user_step_cert", "amwg_user_step", "amwg_user_step_cert"]
    assert all(q.launch_info()["grid_blocks"] == li["grid_blocks"] for q in runs)
    outs = [_run(q, steps) for q in runs]
    for o in outs[1:]:
        _assert_same(o, outs[0])
    st, lp = s.state(), s.diag()["log_post"]
    for c in range(0, C, 97):
        assert np.float64(lp[c]).tobytes() == np.float64(m.eval(st[:, c], 1)).tobytes(), c
    _check_oracle(s, oracle_spec, C, outs[0]["segs"], steps, {})
    for q in runs:
        q.close()


@needs_node
def test_autotune_times_the_replica_candidate_and_leaves_no_trace():
    """AMWG_LANES_AUTOTUNE (-2) times every lane count -- the one-lane replica candidate included, whose launch needs more scratch lines than any earlier
    allocation held -- and then runs exactly what a plain sampler at the lane count it picked runs."""
    C = 8205
    spec, _, _, _, _ = _user("bench_replica_tail", REPLICA_PARAMS, REPLICA_INIT)
    tuned = A.Sampler(spec, chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=-2)
    cands = tuned.tuning()
    assert 1 in [l for l, _ in cands] and all(ms > 0 for _, ms in cands), cands      # (a candidate whose launch failed is not listed)
    lanes = tuned.launch_info()["lanes_per_chain"]
    plain = A.Sampler(spec, chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=lanes)
    assert tuned.launch_info()["kernel"] == plain.launch_info()["kernel"] and tuned.launch_info()["grid_blocks"] == plain.launch_info()["grid_blocks"]
    _assert_same(_run(tuned, 16), _run(plain, 16))
    tuned.close()
    plain.close()


# ---- contract

def test_sufficient_statistics_refuses_autotune_and_takes_one_lane_when_asked_for_the_fastest():
    """include/amwg.h: sufficient_statistics decides from the one-lane certified kernel.  AMWG_LANES_AUTOTUNE could keep a multi-lane kernel, which never reads
    the statistics: AMWG_EINVAL.  AMWG_LANES_FASTEST (-1) gets the one-lane certified kernel."""
    spec = _normal_spec(1000)
    with pytest.raises(A.AmwgError, match="sufficient_statistics decides from the one-lane certified kernel"):
        A.Sampler(spec, chains=256, seed=SEED, lanes_per_chain=-2, sufficient_statistics=1)
    s = A.Sampler(spec, chains=256, seed=SEED, lanes_per_chain=-1, sufficient_statistics=1)
    li = s.launch_info()
    assert li["lanes_per_chain"] == 1 and li["kernel"].startswith("amwg_step_kernel_cert<NormalModel,1,") and li["summation_order"] == 1, li
    s.close()
