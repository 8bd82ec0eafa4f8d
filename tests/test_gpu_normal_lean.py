"""-m gpu: the Normal family's own stepper at one lane per chain (csrc/amwg_normal1.h), which runs under the certified kernel's name
amwg_step_kernel_cert<NormalModel,1,BT> in place of the generic step_body.

Every case runs the default sampler (certified decisions: the lean stepper) and compares it, bit for bit, with
  * the same sampler with full_evaluation = 1 -- amwg_step_kernel<NormalModel,1,BT>: step_body, the expression in every update --, all chains;
  * oracle_lib.OracleChain for the first and the last chain of the case.
Compared: the draws of two sample() calls, the final state, log_post and the order of the named steppers (diag(), asked once between the two calls -- a
finalize launch in mid-run -- and once at the end), every info() counter (accepts, inbounds, acceptance_count, iterations_since_adaption, batch_count,
prop_log_scale) and the uniforms consumed.  The second sample() call follows the first one's last step, so a wrong `perm` or stream position left behind by
a launch shows in its draws.  Every case asserts the kernel it ran and summation_order == 1.

ROWS against the pass's blocks -- 16 rows (1 024 observations) as built, 32 (2 048) with -DAMWG_LEAN_WAVE_BLOCK=32; the list straddles both --: nothing but
leftovers (1, 63), one row and one row + 1 (64, 65), one observation short of a block, exactly one, one + 1 (1 023, 1 024, 1 025; 2 047, 2 048, 2 049: every
remainder part and 63 leftovers), 60 rows (3 840: 3 blocks + the parts 8 + 4; or one + 16 + 8 + 4), 95 rows and 63 leftovers (6 143), and the array in
global memory instead of the LDS tile (12 304).
GEOMETRY at 3 903 observations (60 rows, 63 leftovers): 64 chains; 100 (dead lanes); 320 in workgroups of 256 (a partial second
workgroup, three of its wavefronts all dead lanes); workgroups of 64; the 512 and the 1 024 class; and, in a fresh child process with AMWG_WAVE_SCRATCH=0
(the library reads it when a sampler is made), the v_readlane form of the pass.
STEPPER: mu of type int inside [2, 4] and sigma with lower = 0 started at 0.05 (proposals outside their bounds draw no accept uniform: asserted to occur);
is_adapting false for one component; 120 steps cut into launches of 1, 7 and 100 steps (the pair (lpA, epsA) crosses launches, a launch ends in mid-batch);
sample(n, thin = 3) after burn; chain_offset != 0; sufficient_statistics = 1; test_bound_shift = 24 and 40, which widen the certified test's bound until
the expression decides -- at 40 every update (eta beyond the wide test's range: the proposal's value), at 24 a part of them, between certified accepts that
leave a cheap value standing in for the current state (then the expression is evaluated for the current state as well)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 23
CERT, FULL = "amwg_step_kernel_cert<NormalModel,1,", "amwg_step_kernel<NormalModel,1,"
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 2048 + 28 * 64, 2 * 2048 + 31 * 64 + 63, 12304]
N_GEO = 2048 + 28 * 64 + 63
GEOMETRY = [(64, 0), (100, 0), (320, 256), (128, 64), (512, 512), (1024, 1024)]      # (chains, block_threads; 0: the host's choice)
NO_SCRATCH = [(65, 64, 0), (2048 + 28 * 64, 64, 0), (2 * 2048 + 31 * 64 + 63, 100, 0), (12304, 64, 0)]      # (n_obs, chains, block_threads) of the child process


def _spec(n_obs, params=None, frozen=None):
    import model_spec
    spec = model_spec.build_spec("normal", model_spec.make_data("normal", n_obs, 31), params=params)
    if frozen is not None:
        spec["comp_opts"][frozen]["is_adapting"] = False
    return spec


def _schedule(s, burn, n1, thin):
    """burn, sample with `thin`, diag (a finalize launch), five more steps, diag: -> everything that is compared, as bytes / lists"""
    s.burn(burn)
    d1 = s.sample(n1, thin)
    g1 = s.diag()
    d2 = s.sample(5, 1)
    g2 = s.diag()
    out = {"draws1": d1, "draws2": d2, "state": s.state(), "log_post1": g1["log_post"], "log_post2": g2["log_post"], "order1": g1["named_order"], "order2": g2["named_order"],
           "uniforms1": g1["uniforms"], "uniforms2": g2["uniforms"]}
    out.update(s.info())
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def _oracle(spec, chain, burn, n1, thin):
    import oracle_lib
    o = oracle_lib.OracleChain(spec, SEED, chain, lanes=1)
    o.burn(burn)
    d1 = o.sample(n1, thin)
    lp1, or1, un1 = o.log_post(), o.named_order().copy(), o.uniforms()
    d2 = o.sample(5, 1)
    out = {"draws1": d1, "draws2": d2, "state": o.state(), "log_post1": lp1, "log_post2": o.log_post(), "order1": or1, "order2": o.named_order().copy(), "uniforms1": un1, "uniforms2": o.uniforms()}
    out.update(o.info())
    return out


def _chain_of(got, k, local):
    """what `got` (a sampler's record) holds for its chain `local`, in the oracle's shapes"""
    v = got[k]
    if k.startswith("draws"):
        return v[:, :, local]
    if k.startswith("order"):
        return v[local]
    if v.ndim == 2:
        return v[:, local]
    return v[local]


def _compare(spec, chains, block=0, burn=20, n1=40, thin=1, chain_offset=0, reference=None, **options):
    """-> (what differs from full_evaluation = 1 / from the oracle, the default sampler's record, its launch_info, the reference's record)"""
    import amwg_ctypes as A
    geo = dict(chains=chains, seed=SEED, lanes_per_chain=1, chain_offset=chain_offset)
    if block:
        geo["block_threads"] = block
    if reference is None:
        r = A.Sampler(spec, full_evaluation=1, **geo)
        lr = r.launch_info()
        assert lr["kernel"].startswith(FULL) and lr["lanes_per_chain"] == 1, lr
        reference = _schedule(r, burn, n1, thin)
        r.close()
    s = A.Sampler(spec, **geo, **options)
    li = s.launch_info()
    assert li["kernel"].startswith(CERT) and li["lanes_per_chain"] == 1 and li["summation_order"] == 1, li
    if block:
        assert li["block_threads"] == block, li
    got = _schedule(s, burn, n1, thin)
    s.close()
    bad = [k for k in reference if got[k].tobytes() != reference[k].tobytes()]
    for local in (0, chains - 1):
        want = _oracle(spec, chain_offset + local, burn, n1, thin)
        for k, w in want.items():
            g = _chain_of(got, k, local)
            same = np.array_equal(np.asarray(g, dtype=np.float64).view(np.uint64), np.asarray(w, dtype=np.float64).view(np.uint64)) if k in ("draws1", "draws2", "state", "log_post1", "log_post2", "prop_log_scale") \
                else np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64))
            if not same:
                bad.append("oracle chain %d: %s" % (local, k))
    return bad, got, li, reference


@pytest.mark.parametrize("n_obs", ROWS)
def test_rows_against_the_blocks_of_the_pass(n_obs):
    assert "AMWG_WAVE_SCRATCH" not in os.environ
    bad, _, li, _ = _compare(_spec(n_obs), 64)
    assert li["block_threads"] <= 256, li
    assert not bad, (bad, li)


@pytest.mark.parametrize("chains,block", GEOMETRY)
def test_geometry(chains, block):
    bad, _, li, _ = _compare(_spec(N_GEO), chains, block)
    assert not bad, (bad, li)


def test_readlane_form_without_wave_scratch():
    """AMWG_WAVE_SCRATCH=0 in a fresh child process (this file run as a script): every case of NO_SCRATCH must report, and report no difference."""
    env = dict(os.environ, AMWG_WAVE_SCRATCH="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert [tuple(c["case"]) for c in rec] == NO_SCRATCH
    for c in rec:
        assert c["differs"] == [] and c["kernel"].startswith(CERT), c


def _bounded_params():
    inf = float("inf")
    return [{"type": "int", "len": 1, "top": 1, "multidim": 0, "lower": 2.0, "upper": 4.0, "init": [3.0]},
            {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": 0.0, "upper": inf, "init": [0.05]}]


def test_int_mu_with_bounds_and_sigma_started_at_its_lower_bound():
    bad, got, li, _ = _compare(_spec(2049, params=_bounded_params()), 100, burn=50, n1=70, thin=3)
    assert not bad, (bad, li)
    steps = 50 + 70 + 5
    assert (got["inbounds"] < steps).any(axis=1).all() and (got["inbounds"] > 0).all(), got["inbounds"]      # (both components proposed outside their bounds, and inside)
    assert np.array_equal(got["state"][0], np.round(got["state"][0])) and (got["state"][1] > 0).all()


@pytest.mark.parametrize("frozen", [0, 1])
def test_one_component_not_adapting(frozen):
    bad, got, li, _ = _compare(_spec(2049, frozen=frozen), 64, burn=50, n1=70, thin=3)
    assert not bad, (bad, li)
    assert (got["batch_count"][frozen] == 0).all() and (got["batch_count"][1 - frozen] == 2).all(), got["batch_count"]


def test_launches_of_1_7_and_100_steps_and_a_chain_offset():
    """120 + 5 steps, adaptation on (batches of 50 close inside launches, launches end in mid-batch), chains 1 000 .. 1 099 of the seed"""
    spec, ref = _spec(2049), None
    for spl in (1, 7, 100):
        bad, got, li, ref = _compare(spec, 100, burn=50, n1=70, thin=3, chain_offset=1000, reference=ref, steps_per_launch=spl)
        assert not bad, (spl, bad, li)
        assert (got["batch_count"] == 2).all()


def test_sufficient_statistics():
    bad, _, li, _ = _compare(_spec(N_GEO), 100, burn=50, n1=70, thin=3, sufficient_statistics=1)
    assert not bad, (bad, li)


@pytest.mark.parametrize("shift", [24, 40])
def test_bounds_so_wide_that_the_expression_decides(shift):
    """(2 n + 64) u mag 1.25 is ~6e-9 here (n = 2 049, mag ~1e4): times 2^24 the test's eta is ~0.1 -- the wide test certifies the clear cases and hands the rest
    to the expression, for the current state too when a certified accept came before --; times 2^40 it is beyond 2^9 and every update is the expression's."""
    bad, _, li, _ = _compare(_spec(2049), 100, burn=50, n1=70, thin=3, test_bound_shift=shift)
    assert not bad, (bad, li)


def _child():
    for p in (ROOT, os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    try:
        import torch  # noqa: F401  (before the library, as tests/conftest.py does)
    except Exception:
        pass
    assert os.environ.get("AMWG_WAVE_SCRATCH") == "0"
    out = []
    for n, c, b in NO_SCRATCH:
        bad, _, li, _ = _compare(_spec(n), c, b)
        out.append({"case": [n, c, b], "differs": bad, "kernel": li["kernel"], "block_threads": li["block_threads"]})
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    _child()
