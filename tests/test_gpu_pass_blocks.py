"""-m gpu: the block structure of the wavefront's certified pass (csrc/amwg_pass.h norm_sq_pass_wave, scalar-means path).

The pass walks the data in full blocks of B rows (a row = 64 observations; B = 16 in workgroups of up to 256 threads, 8 in the 512-thread class) whose register
set is refilled in place -- the next block's rows are requested during the last group of the block before -- while every group requests the means of the group
after it, across block boundaries too; the rows after the last full block are ONE set of reads, worked through as the parts B/2, .., 1 and the partly filled row
(pass_rows).  The smallest shapes at which that can go wrong: one, two and three full blocks (a refill that is used, one that is not), every remainder length
1 .. 15 with a partly filled row, remainders without one, and both sides of the LDS tile's limit (12 288 observations: the ds_read and the global-memory
instantiations).

Every draw, info counter, uniform count, cached log_post and state must be byte-equal to the same spec with the expression in every update
(full_evaluation = 1) at one lane per chain in 64-thread workgroups; each case asserts the kernel and geometry it ran.  The VALUE of the pass -- not only the
decisions taken from it -- is checked through the audit build (tools/bound_audit.py run_case, libamwg_audit.so): |A - E| / eps and |dA - dE| / eta at most 0.5,
the factor of two the derivation in NormalModel::log_post_approx leaves."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import amwg_ctypes as A
import model_spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, OFFSET, SPL = 8, 3, 13      # (SPL: steps per launch, odd -- a launch ends by evaluating the expression, mid-schedule)
STEPS = 120
NOBS = sorted({1023, 1024, 1025, 2047, 2048, 2049, 3072, 3137} | {2048 + 64 * r + 5 for r in range(1, 16)} | {12288, 12289})
BLOCKS = [256, 512]
CHAINS = [37, 300]
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def _schedule(s, steps):
    """sample with thin, burn, adaptation off and on, a state overwritten from the host (chains c = 1 mod 3 but the last, param 0), burn, sample"""
    seq = [s.sample(steps // 4, 3)]
    s.burn(steps // 2)
    s.set_adapting(False)
    seq.append(s.sample(steps // 8, 1))
    s.set_adapting(True)
    st = s.state()
    st[0, 1:s.C - 1:3] += 0.25
    s.set_state(st)
    s.burn(steps // 8)
    seq.append(s.sample(steps // 8 + 4, 2))
    return seq


def _run(s, steps):
    seq = _schedule(s, steps)
    return {"draws": [x.tobytes() for x in seq], "info": {k: v.tobytes() for k, v in s.info().items()}, "uniforms": s.diag()["uniforms"].tobytes(),
            "log_post": s.diag()["log_post"].tobytes(), "state": s.state().tobytes()}


def _assert_same(got, want):
    for i, (x, y) in enumerate(zip(got["draws"], want["draws"])):
        assert x == y, "draws of sample call %d" % i
    for k in want["info"]:
        assert got["info"][k] == want["info"][k], k
    assert got["uniforms"] == want["uniforms"], "uniforms"
    assert got["log_post"] == want["log_post"], "cached log_post"
    assert got["state"] == want["state"], "state"


def _geometry(s, kernel, block, grid):
    li = s.launch_info()
    assert (li["kernel"], li["block_threads"], li["grid_blocks"], li["summation_order"], li["lanes_per_chain"]) == (kernel, block, grid, 1, 1), li


def _grid(C, per_block):
    return -(-C // per_block)


_refs = {}


def _ref(C, n):
    """the expression in the reference's order in every update, one lane per chain in 64-thread workgroups: computed once per (chains, n_obs), shared by the classes"""
    key = (C, n)
    if key not in _refs:
        _refs.clear()
        spec = model_spec.build_spec("normal", model_spec.make_data("normal", n, 31))
        r = A.Sampler(spec, chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, block_threads=64, steps_per_launch=SPL, full_evaluation=1)
        _geometry(r, "amwg_step_kernel<NormalModel,1,256>", 64, _grid(C, 64))
        out = _run(r, STEPS)
        r.close()
        _refs[key] = (spec, out)
    return _refs[key]


@pytest.mark.parametrize("n_obs,chains,block", [(n, c, b) for n in NOBS for c in CHAINS for b in BLOCKS])      # (cases that share a reference run one after the other)
def test_certified_normal_pass_equals_the_expression_at_every_block_count_and_remainder(n_obs, chains, block):
    """amwg_step_kernel_cert<NormalModel,1,{256,512}>: 1 .. 3 full blocks of 16 (2 .. 6 of 8, 12 and 24 at the tile's limit), remainders of 0 .. 15 full rows with
    and without a partly filled one, the tile in LDS and (12 289 observations) the array in global memory: every bit of every chain equals the expression's."""
    spec, ref = _ref(chains, n_obs)
    s = A.Sampler(spec, chains=chains, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, block_threads=block, steps_per_launch=SPL)
    _geometry(s, "amwg_step_kernel_cert<NormalModel,1,%d>" % block, block, _grid(chains, block))
    _assert_same(_run(s, STEPS), ref)
    s.close()


@needs_node
def test_certified_tail_of_a_closure_with_a_thirteen_row_remainder_equals_the_expression():
    """bench_normal's closure over its first 2 048 + 64 * 13 + 5 observations (two full blocks, the parts 8 and 4 and a partly filled row; the array staged in LDS,
    so the pass is the ds_read instantiation compiled by hiprtc): amwg_user_step_cert in 256-thread workgroups against the closure evaluated in every update."""
    import user_host
    n, name = 2048 + 64 * 13 + 5, "bench_normal_n2885"
    d = user_host.workdir()
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "translate_truncated_cli.js"), d, "bench_normal", str(n), name], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    src, arrays, meta = user_host.translated(name)
    assert meta["cert_tail_n"] == n == len(arrays[0]) and "kTailXLds = true" in src
    fam = model_spec.build_spec("normal", {"x": arrays[0]})
    opt = dict(model_spec.DEFAULT_OPT)
    spec = {"user": user_host.user_spec_part(src, arrays, meta), "P": 2, "init": list(fam["init"]), "comp_opts": [dict(opt), dict(opt)], "params": fam["params"]}
    C = 300
    kw = dict(chains=C, seed=SEED, chain_offset=OFFSET, lanes_per_chain=1, steps_per_launch=SPL)
    r = A.Sampler(spec, full_evaluation=1, block_threads=64, **kw)
    _geometry(r, "amwg_user_step", 64, _grid(C, 64))
    s = A.Sampler(spec, block_threads=256, **kw)
    _geometry(s, "amwg_user_step_cert", 256, _grid(C, 256))
    want, got = _run(r, STEPS), _run(s, STEPS)
    _assert_same(got, want)
    r.close()
    s.close()


AUDIT_N = [2049, 3137, 2048 + 64 * 13 + 5]
_AUDIT_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import bound_audit as B      # (points the binding at libamwg_audit.so before it is imported)
import numpy as np
import model_spec
out = []
for n in json.loads(sys.argv[2]):
    c = B.normal_case("normal_n%d" % n, model_spec.make_data("normal", n, 31)["x"], 256, 300)
    r = B.run_case(c)
    per = r["per"]
    out.append({"n": n, "kernel": r["kernel"], "audited_decisions": int(per[2].sum()), "wrong_verdicts": int(per[3].sum()), "nan": bool(np.isnan(per[0]).any() or np.isnan(per[1]).any()),
                "max_value_ratio": float(np.nanmax(per[0])), "max_difference_ratio": float(np.nanmax(per[1]))})
print("RESULT " + json.dumps(out))
"""


def test_the_value_of_the_pass_stays_within_half_its_bound():
    """The audit build evaluates the reference's expression E beside the pass's value A in every update: max |A - E| / eps <= 0.5 and max |dA - dE| / eta <= 0.5 (the
    existing gate's numbers: the derivation's factor of two), not one wrong verdict, at n = 2 049 (two blocks and a single partly filled row), 3 137 (three blocks, one
    full row and a partly filled one) and 2 885 (a thirteen-row remainder).  One child process: the audit library is a different libamwg than the one this process holds."""
    p = subprocess.run([sys.executable, "-c", _AUDIT_SCRIPT, os.path.join(ROOT, "tools"), json.dumps(AUDIT_N)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert [c["n"] for c in rec] == AUDIT_N
    for c in rec:
        print(c)
        assert c["kernel"] == "amwg_step_kernel_cert<NormalModel,1,256>", c
        assert c["audited_decisions"] > 0 and c["wrong_verdicts"] == 0 and not c["nan"], c
        assert c["max_value_ratio"] <= 0.5 and c["max_difference_ratio"] <= 0.5, c
