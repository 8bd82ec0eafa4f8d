"""Certified decisions for closures that end in a logistic-regression loop, without a GPU: the translator's plan (translate.js glmTailPlan) is found where it
must be and refused where it must be, the generated sources compile for gfx950 (hiprtc needs no device), softplus_bounded keeps the absolute error its comment
derives (tests/host/softplus_bounded_fuzz.cpp against __float128) and the bound of csrc/amwg_gtail.h holds with a factor of two when its derivation is replayed in
quad precision (tests/host/logit_bound_replay.cpp)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import amwg_ctypes as A
import logit_host
import user_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags(src):
    return tuple((re.search(k + r" = (true|false)", src) or [None, None])[1] for k in ("kTailUniformState", "kTailRows", "kTailLinear"))


def test_logit_n10k_gets_the_certified_logistic_tail():
    src, _, _ = user_host.translated("logit_n10k")
    for token in ("kLogitTail = true, kCertified = true, kReferenceOrder = true", "kCertifiedLanes = 16, kTailN = 10000, kStateN = 4", "kTailUniformState = true", "kTailRows = true",
                  "glm_tail_approx<UserModel, LogitLink, G, BT>", "glm_tail_reference<UserModel, LogitLink, G>", "gtail_sum_y() { return 4366.0; }",
                  "struct TailRow { uint8_t a0[1]; double a1[1]; double a2[1]; double a3[1]; };"):
        assert token in src, token
    assert "kPoisTail" not in src and "kCertifiedTail" not in src and "@LTAIL" not in src
    # the lane-split loop of the expression is emitted as it was: one device function for the softplus, its branch-free form in the unrolled body
    assert "log1p_exp_v8_open(rr_, v_eta)" in src and "log1p_exp_cold(v_eta)" in src
    # eta is the closure's own statements, never the fused form
    assert "gtail_eta_fused" not in src and "(((S(0) + (S(1) * R.a1[(0) - 0])) + (S(2) * R.a2[(0) - 0])) + (S(3) * R.a3[(0) - 0]))" in src


@pytest.mark.parametrize("name", ["logit_bern_n10k", "logistic_softplus", "records_logistic"])
def test_other_logistic_spellings_and_loops_that_are_not_last_get_no_plan(name):
    src, _, _ = user_host.translated(name)
    assert "kLogitTail" not in src and "LogitLink" not in src and "@LTAIL" not in src


def test_the_poisson_closure_keeps_its_own_plan():
    src, _, meta = user_host.translated("pois_glm_closure")
    assert "kPoisTail = true" in src and meta["pois_tail_n"] == 500 and "kLogitTail" not in src


@pytest.mark.parametrize("label,flags,n", [("logit_tail_small", ("true", "true", "false"), 517), ("logit_tail_small@64", ("true", "true", "false"), 64),
                                           ("logit_tail_gather", ("false", "false", "false"), 517), ("logit_tail_next_row", ("true", "false", "false"), 517),
                                           ("logit_tail_weights", ("true", "true", "false"), 517)])
def test_fixture_closures_get_the_plan_on_the_path_they_were_written_for_and_compile(label, flags, n):
    src, _, meta = logit_host.translated(label)
    assert meta["logit_tail_n"] == n and meta["pois_tail_n"] == 0 and meta["cert_tail_n"] == 0
    assert "kLogitTail = true" in src and ("kTailN = %d," % n) in src and _flags(src) == flags
    size = C.c_size_t(0)
    L = A.lib()
    assert L.amwg_compile_user(src.encode(), 16, 256, b"gfx950", C.byref(size)) == 0, L.amwg_last_error().decode()[-3000:]
    assert size.value > 0


def test_logit_n10k_compiles_for_gfx950_at_16_lanes():
    src, _, _ = user_host.translated("logit_n10k")
    size = C.c_size_t(0)
    L = A.lib()
    assert L.amwg_compile_user(src.encode(), 16, 256, b"gfx950", C.byref(size)) == 0, L.amwg_last_error().decode()[-3000:]


@pytest.mark.parametrize("label,opts", [("logit_not_last", None), ("logit_derived", None), ("logit_two_etas", None),
                                        ("logit_tail_small", {"no_logit_tail": True}), ("logit_tail_small", {"no_cert_tail": True})])
def test_no_plan_where_the_conditions_fail_or_it_is_switched_off(label, opts):
    src, _, meta = logit_host.translated(label, opts)
    assert meta["logit_tail_n"] == 0 and "kLogitTail" not in src and "kCertified" not in src and "@LTAIL" not in src


def test_no_plan_for_a_binary_parameter_or_a_non_finite_y(tmp_path):
    js = r"""
const t = require(process.argv[2]); global.ld = require(process.argv[3]); const lm = require(process.argv[4]);
const d = lm.data(517);
const P = { b: { type: 'real', dim: [4], lower: -Infinity, upper: Infinity, init: [0, 0, 0, 0] } };
const PB = Object.assign({ z: { type: 'binary', dim: [1], lower: 0, upper: 1, init: 1 } }, P);
const loop = 'for (var i = 0; i < d.w.length; i++) { var eta = s.b[0] + s.b[1] * d.x1[i]; lp += d.w[i] * eta - Math.log1p(Math.exp(eta)); } return lp; }';
const plain = 'function (s, d) { var lp = 0; for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10); ' + loop;
const binary = 'function (s, d) { var lp = ld.bern(s.z, 0.5); for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10); ' + loop;
const out = {};
const run = (k, text, params, data) => { const r = t.translate(text, params, data, {}); out[k] = [r.logit_tail_n, /kLogitTail/.test(r.source)]; };
run('plain', plain, P, d);
run('binary', binary, PB, d);
run('infinite_y', plain, P, Object.assign({}, d, { w: d.w.map((v, i) => (i === 9 ? Infinity : v)) }));
run('nan_y', plain, P, Object.assign({}, d, { w: d.w.map((v, i) => (i === 300 ? NaN : v)) }));
console.log(JSON.stringify(out));
"""
    import json
    f = tmp_path / "probe.js"
    f.write_text(js)
    p = subprocess.run(["node", str(f), os.path.join(ROOT, "bayes.js_amd", "translate.js"), os.path.join(ROOT, "bayes.js_amd", "ld.js"), os.path.join(ROOT, "tests", "js", "logit_models.js")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["plain"] == [517, True]
    assert out["binary"] == [0, False] and out["infinite_y"] == [0, False] and out["nan_y"] == [0, False]


def _build_host(tmp_path, name):
    exe = tmp_path / name
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "host", name + ".cpp"), "-lquadmath"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_softplus_bounded_keeps_its_derived_absolute_error(tmp_path):
    """max |softplus_bounded(x) - softplus(x)| over the fuzz's arguments, |x| <= 690, against __float128: at most kSoftplusBoundedAbs (the program's exit status), and
    the constant is the 2^-46 the comment in amwg_math.h derives."""
    exe = _build_host(tmp_path, "softplus_bounded_fuzz")
    r = subprocess.run([str(exe), "250000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r"arguments=(\d+) max_abs_error=(\S+) at .* kSoftplusBoundedAbs=(\S+) regs_vs_literals_mismatches=(\d+)", r.stdout)
    assert m and int(m.group(1)) > 1_000_000 and int(m.group(4)) == 0
    assert float.fromhex(m.group(3)) == 2.0 ** -46 and 0.0 < float(m.group(2)) <= 2.0 ** -46


def test_logistic_tail_bound_holds_with_a_factor_of_two_in_quad_precision(tmp_path):
    """the derivation of csrc/amwg_gtail.h replayed in __float128 on random and adversarial inputs: both halves hold, the pieces add up to no more than eps, and the
    worst |A - E| / eps is at most 0.5"""
    exe = _build_host(tmp_path, "logit_bound_replay")
    r = subprocess.run([str(exe), "8"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"cases=(\d+) skipped_nonfinite=(\d+) worst \|E-R\|/bE=(\S+) worst \|A-R\|/bA=(\S+) worst \|A-E\|/eps=(\S+) .* pieces_over_eps=(\d+) violations=(\d+)", r.stdout)
    assert m and int(m.group(1)) >= 1000 and int(m.group(6)) == 0 and int(m.group(7)) == 0
    assert float(m.group(3)) <= 1.0 and float(m.group(4)) <= 1.0 and float(m.group(5)) <= 0.5
