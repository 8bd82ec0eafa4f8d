"""-m gpu: certified decisions for closures that end in a logistic-regression loop (translate.js glmTailPlan, csrc/amwg_gtail.h): the 16-lane certified kernel
decides like the expression in the REFERENCE's order -- every byte of the one-lane run that evaluates the expression in every update, the reference's golden
chains for logit_n10k --, on and off the pass's fast path, beyond the reference's straight-line range and beyond the bound's cut-off; the device's
softplus_bounded is the host's; the bound audited on the device (tools/bound_audit.py --only logit)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import amwg_ctypes as A
import golden_io
import logit_host
import user_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_softplus_bounded_equals_the_host_build(tmp_path):
    """softplus_bounded (csrc/amwg_math.h) on the device, with literal coefficients and with the register form the pass uses, against the host build on the argument
    set of tests/host/softplus_bounded_fuzz.cpp -- bit for bit: the quotient without the general division's exponent juggling is the correctly rounded one."""
    exe = tmp_path / "softplus_bounded_fuzz"
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "host", "softplus_bounded_fuzz.cpp"), "-lquadmath"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    pairs = tmp_path / "pairs.bin"
    r = subprocess.run([str(exe), "200000", str(pairs)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    a = np.fromfile(pairs, dtype="<f8").reshape(-1, 2)
    assert a.shape[0] > 1_000_000
    x, want = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    for op in (36, 37):
        got = A.device_eval(op, x)
        bad = got.view(np.uint64) != want.view(np.uint64)
        assert not bad.any(), (op, int(bad.sum()), x[bad][:5], got[bad][:5], want[bad][:5])


def _golden_spec(name):
    """Sampler spec from the golden's completed params (what the reference built) + the translated model."""
    gold = golden_io.load("user_" + name)
    rec = gold["chains"][0]
    src, arrays, meta = user_host.translated(name)
    params, init, opts = [], [], []
    for p in rec["params_completed"]:
        ln = int(np.prod(p["dim"]))
        params.append({"type": p["type"], "len": ln, "top": p["dim"][0], "multidim": 0 if p["dim"] == [1] else 1, "lower": p["lower"], "upper": p["upper"]})
        init += p["init"]
    for o in rec["comp_opts"]:
        opts.append({"prop_log_scale": o.get("prop_log_scale", 0.0), "max_adaptation": o.get("max_adaptation", 0.33), "initial_adaptation": o.get("initial_adaptation", 1.0),
                     "target_accept_rate": o.get("target_accept_rate", 0.44), "batch_size": o.get("batch_size", 50), "is_adapting": o.get("is_adapting", True)})
    return {"user": user_host.user_spec_part(src, arrays, meta), "params": params, "P": len(init), "init": init, "comp_opts": opts}, src, gold


def _everything(q):
    return (q.state().tobytes(), q.info()["accepts"].tobytes(), q.info()["prop_log_scale"].tobytes(), q.diag()["uniforms"].tobytes(), q.diag()["log_post"].tobytes())


def test_certified_logistic_tail_of_a_translated_closure_reproduces_the_reference_and_the_full_evaluation():
    """logit_n10k (`lp += y[i] * eta - Math.log1p(Math.exp(eta))`, N = 1e4) runs amwg_user_step_cert at 16 lanes per chain (four chains of a wavefront share every
    row).  Its decisions are the expression's in the REFERENCE's order: chain by chain the reference's golden trajectory, and every bit of the run that evaluates the
    expression in every update at one lane per chain; widened and narrowed bounds change nothing."""
    from gpu_util import run_schedule
    spec, src, gold = _golden_spec("logit_n10k")
    for token in ("kLogitTail = true", "kCertifiedLanes = 16", "kTailN = 10000", "kTailUniformState = true", "kTailRows = true"):
        assert token in src, token
    sched = gold["case"]["schedule"]
    seed = gold["case"]["seed"]
    auto = A.Sampler(spec, chains=8192, seed=seed)
    li = auto.launch_info()
    assert (li["lanes_per_chain"], li["kernel"], li["summation_order"]) == (16, "amwg_user_step_cert", 1), li
    auto.close()
    kw = dict(chains=64, seed=seed, steps_per_launch=23)
    runs = [A.Sampler(spec, lanes_per_chain=16, **kw), A.Sampler(spec, lanes_per_chain=1, full_evaluation=1, **kw),
            A.Sampler(spec, lanes_per_chain=16, test_bound_shift=12, **kw), A.Sampler(spec, lanes_per_chain=16, test_bound_shift=30, **kw)]
    assert [q.launch_info()["kernel"] for q in runs] == ["amwg_user_step_cert", "amwg_user_step", "amwg_user_step_cert", "amwg_user_step_cert"]
    assert runs[0].launch_info()["summation_order"] == 1
    outs = []
    for q in runs:
        segs = run_schedule(q, sched)
        outs.append((b"".join(g.tobytes() for g in segs),) + _everything(q))
    assert all(o == outs[0] for o in outs[1:]), [[x == y for x, y in zip(o, outs[0])] for o in outs[1:]]
    for rec in gold["chains"]:      # the reference's own chains
        c = rec["chain"]
        assert runs[0].info()["accepts"][:, c].tolist() == rec["accepts"]
        assert runs[0].state()[:, c].tolist() == rec["final_state"]
        assert float(runs[0].diag()["log_post"][c]) == rec["log_post"]      # (the expression in the reference's order: the reference's own double)
    for q in runs:
        q.close()


def _four_runs_agree(spec, kw, shifts=(10, 34)):
    runs = [A.Sampler(spec, lanes_per_chain=16, **kw), A.Sampler(spec, lanes_per_chain=1, full_evaluation=1, **kw),
            A.Sampler(spec, lanes_per_chain=16, test_bound_shift=shifts[0], **kw), A.Sampler(spec, lanes_per_chain=16, test_bound_shift=shifts[1], **kw)]
    assert [q.launch_info()["kernel"] for q in runs] == ["amwg_user_step_cert", "amwg_user_step", "amwg_user_step_cert", "amwg_user_step_cert"]
    assert runs[0].launch_info()["summation_order"] == 1
    outs = []
    for q in runs:
        d1 = q.sample(70, 2)
        q.burn(110)
        d2 = q.sample(25, 1)
        outs.append((d1.tobytes(), d2.tobytes()) + _everything(q))
        q.close()
    assert all(o == outs[0] for o in outs[1:]), [[x == y for x, y in zip(o, outs[0])] for o in outs[1:]]
    state = np.frombuffer(outs[0][2], dtype=np.float64)
    assert np.isfinite(state).all() and np.isfinite(np.frombuffer(outs[0][6], dtype=np.float64)).all()
    return state


@pytest.mark.parametrize("label,flags", [("logit_tail_gather", ("false", "false", "false")), ("logit_tail_next_row", ("true", "false", "false")),
                                         ("logit_tail_small", ("true", "true", "false")), ("logit_tail_weights", ("true", "true", "false"))])
def test_certified_logistic_tail_fallback_paths_equal_the_expression(label, flags):
    """csrc/amwg_gtail.h off its fast path -- a coefficient gathered by the data (per-lane LDS reads of the state, the plain loop), a read of the next observation's
    row (no row cache) --, 517 observations (a ragged last round) and real-valued weights in the place of y: the 16-lane certified kernel against the same closure at
    ONE lane per chain with the expression in every update, and against narrowed / widened bounds: every bit of every chain, cached log_post included."""
    spec, src, meta = logit_host.spec(label)
    assert meta["logit_tail_n"] == 517 and "kLogitTail = true" in src
    got = tuple(re.search(k + r" = (true|false)", src).group(1) for k in ("kTailUniformState", "kTailRows", "kTailLinear"))
    assert got == flags, got
    _four_runs_agree(spec, dict(chains=96, seed=11, chain_offset=5, steps_per_launch=19))


@pytest.mark.parametrize("init,beyond", [((0.0, 30.0, 0.0, 0.0), 36.0), ((0.0, 350.0, 0.0, 0.0), 690.0)])
def test_certified_logistic_tail_beyond_the_straight_line_and_beyond_the_cut_off(init, beyond):
    """A start state that puts max |eta| = 2 |b1| beyond 36 (where the reference's log1p_exp_v8 leaves its straight line for the full functions) and one that puts
    it beyond 690 (the bound is infinite: the expression decides until the chain has come back): the same equality, and chains that are finite at the end."""
    assert 2.0 * init[1] > beyond
    spec, src, meta = logit_host.spec("logit_tail_small", init=init)
    _four_runs_agree(spec, dict(chains=64, seed=23, steps_per_launch=17))


def test_certified_logistic_bounds_hold_with_a_factor_of_two(tmp_path):
    """tools/bound_audit.py --only logit (the audit build evaluates the expression beside every certified value): every case on a _cert kernel, audited, not one
    wrong verdict, both ratios below 0.5 -- the bar tests/test_gpu_bound_audit.py sets for every bound.  Only the case built to exceed H = 690 may have nothing to audit."""
    out = tmp_path / "audit.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bound_audit.py"), "--only", "logit", "--out", str(out)], capture_output=True, text=True, timeout=900)
    print(p.stdout[-4000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    rec = json.loads(out.read_text())
    assert rec["summary"]["bounds_hold_with_factor_two"] and rec["summary"]["wrong_verdicts"] == 0
    by = {c["name"]: c for c in rec["cases"]}
    assert set(by) >= {"logit_n64", "logit_n65", "logit_n517", "logit_eta_36", "logit_eta_minus_36", "logit_H_689", "logit_H_691", "logit_all_zero_y", "logit_all_one_y"}
    for name, c in by.items():
        assert "_cert" in c["kernel"], (name, c["kernel"])
        assert c["wrong_verdicts"] == 0, c
        if name != "logit_H_691":
            assert c["audited_decisions"] > 0, c
        if c["audited_decisions"] > 0:
            assert c["max_value_ratio"] <= 0.5 and c["max_difference_ratio"] <= 0.5, c
