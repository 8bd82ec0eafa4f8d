"""options.pointwise -- WAIC and PSIS-LOO for translated closures -- the part that needs no GPU.  tests/README.pointwise.md says what each test pins.

The translator's plan on the fixtures of tests/js/pointwise_models.js: `source` is the same bytes with and without { pointwise: true } for every closure of
tests/js/user_models.js and of the new file; under V8 the head's value plus the sequential sum of term(i) is log_post(state), bit for bit; the host build of the
generated make_draw + term gives Node's term(i) as bytes; the pointwise program compiles for gfx950 (amwg_compile_pointwise); the refusals by their sentences, in
the translator and in both front ends; what the header says."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes as A
import pointwise_lib as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
N = 65
STATES = 36      # a few dozen states per closure


def test_source_is_the_same_bytes_with_and_without_the_flag():
    rec = pl.fixtures(N, STATES)
    assert len(rec["identity"]) >= 50 and set(rec["models"]) == set(pl.NAMES)
    for name, r in list(rec["identity"].items()) + list(rec["models"].items()) + list(rec["rejected"].items()):
        assert "error" not in r and r["identical"] is True, (name, r.get("error"))
    assert sum(1 for r in rec["identity"].values() if r["planned"]) >= 15      # (the plan is no rarity among ordinary closures)
    for r in rec["identity"].values():
        assert r["planned"] or r["why"].startswith("options.pointwise: ")


@pytest.mark.parametrize("name", pl.NAMES)
def test_every_fixture_has_a_plan_and_its_two_writings_agree_under_v8(name):
    m = pl.fixtures(N, STATES)["models"][name]
    assert m["why"] is None and m["n_obs"] == N and m["start"] == 0
    assert len(m["tie"]) == STATES and all(m["tie"])      # head + the sequential sum of term(i) == log_post(state), as bytes
    assert "struct UserTerms" in m["terms_source"] and "kTermN = %d" % N in m["terms_source"] and "kStateN = %d" % m["P"] in m["terms_source"]
    assert "log1p_exp_v8_open" not in m["terms_source"] and "log1p_exp_cold" not in m["terms_source"]      # the full softplus: the open / cold pair is the step loop's


@pytest.mark.parametrize("name", pl.NAMES)
def test_host_build_of_make_draw_and_term_gives_nodes_terms_as_bytes(name, tmp_path):
    m = pl.fixtures(N, STATES)["models"][name]
    (tmp_path / "m.hip").write_text(m["source"])
    (tmp_path / "m.terms.hip").write_text(m["terms_source"])
    so = str(tmp_path / "pw.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"),
                           "-DAMWG_USER_SOURCE=\"%s\"" % (tmp_path / "m.hip"), "-DAMWG_TERMS_SOURCE=\"%s\"" % (tmp_path / "m.terms.hip"), "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "host", "pointwise_eval_host.cpp")])
    lib = C.CDLL(so)
    assert lib.pointwise_n_obs() == N and lib.pointwise_state_n() == m["P"]
    arrs = [np.concatenate([a, np.zeros(16)]).astype(pl.DTYPES[t]) for a, t in zip(m["arrays"], m["array_types"])]      # (device-typed, with the spare elements of an upload)
    ptrs = (C.c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    out = np.empty(N)
    for s in range(STATES):
        st = np.ascontiguousarray(m["states"][s])
        lib.pointwise_terms(st.ctypes.data_as(C.POINTER(C.c_double)), ptrs, len(arrs), out.ctypes.data_as(C.POINTER(C.c_double)))
        assert pl.same_bytes(out, m["terms"][s]), (name, s, int(np.argmax(out.view(np.uint64) != m["terms"][s].view(np.uint64))))
    draw = lib.pointwise_draw_bytes()
    if name == "wide_state":
        assert draw > 48 * 1024 // 256      # a Draw large enough to shorten the staged run
    if name in ("normal", "pois_glm"):
        assert draw * 256 <= 48 * 1024      # the twins keep kStage = 256, as their families do


@pytest.mark.parametrize("name", pl.NAMES)
def test_pointwise_program_compiles_for_gfx950(name):
    m = pl.fixtures(N, STATES)["models"][name]
    assert A.compile_pointwise(m["source"], m["terms_source"], "gfx950") > 10000


def test_a_text_that_does_not_compile_is_refused_with_the_log():
    m = pl.fixtures(N, STATES)["models"]["normal"]
    with pytest.raises(A.AmwgError, match="pointwise terms of the translated log_post did not compile"):
        A.compile_pointwise(m["source"], m["terms_source"].replace("return w;", "return w_;"), "gfx950")


def test_the_plans_of_ordinary_closures_compile_for_gfx950():
    """every closure of tests/js/user_models.js that has a plan -- heads with staged and fast-forwarded loops, helpers, constants, forms the new fixtures lack"""
    planned = {k: r for k, r in pl.fixtures(N, STATES)["identity"].items() if r["planned"]}
    assert len(planned) >= 15
    for name, r in planned.items():
        try:
            assert A.compile_pointwise(r["source"], r["terms_source"], "gfx950") > 10000, name
        except A.AmwgError as e:
            raise AssertionError("%s: %s" % (name, str(e)[-3000:]))


@pytest.mark.parametrize("name", pl.REJECTED)
def test_rejected_closures_say_why(name):
    r = pl.fixtures(N, STATES)["rejected"][name]
    assert r["pointwise"] is None and r["expect"] in r["why"], r


def test_front_ends_refuse_by_message():
    js = """
      const { mcmc, ld } = require('./bayes.js_amd'); global.ld = ld;
      const pm = require('./tests/js/pointwise_models.js'), um = require('./tests/js/user_models.js');
      const out = [];
      const m = pm.build('has_break', 10);
      try { new mcmc.AmwgSampler(m.params, m.log_post, m.data, { translate: true, pointwise: true, chains: 64 }); out.push('no throw'); } catch (e) { out.push(String(e)); }
      const f = um.build('readme_normal');
      try { new mcmc.AmwgSampler(f.params, f.log_post, f.data, { pointwise: true, chains: 64 }); out.push('no throw'); } catch (e) { out.push(String(e)); }
      console.log(JSON.stringify(out));
    """
    p = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    import json
    got = json.loads(p.stdout)
    assert "options.pointwise: the final loop has a break" in got[0]
    assert "a built-in family needs no flag" in got[1]


def test_header_and_bindings_state_the_rule():
    declared = set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "amwg.h")).read()))
    for call in ("amwg_set_pointwise", "amwg_compile_pointwise", "amwg_pointwise_n_obs"):
        assert call in declared and call in A.EXPORTS and getattr(A.lib(), call) is not None
    checks = set(re.findall(r"\b(amwg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "amwg_selftest.h")).read()))
    for call in ("amwg_user_waic_check", "amwg_user_loo_check"):
        assert call in checks and call in A.SELFTEST_EXPORTS and call not in A.EXPORTS and not hasattr(A.lib(), call)
    header = " ".join(re.sub(r"(?m)^ \* ", " ", open(os.path.join(ROOT, "include", "amwg.h")).read()).split())
    for words in ("THE OBSERVATIONS OF A CLOSURE are the iterations of its FINAL LOOP", "Everything before the loop counts as prior and is no part of l",
                  "gets the WAIC of the final loop's observations only", "kStage = 256 at a time wherever 256 of the closure's Draw",
                  "otherwise the largest multiple of 4 that fits", "a function of sizeof(Draw) alone", "a built-in family needs no text",
                  "the pointwise terms of a closure are not known to the library; built-in families only"):
        assert words in header, words
    for scope in ("OUT OF SCOPE: WAIC after", "OUT OF SCOPE: LOO after"):
        assert "translated closures" not in header[header.index(scope):][:420]


def test_the_shared_kernels_keep_their_atomics_on_integers_and_stay_out_of_the_step_kernels():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_id
    csrc = os.path.join(ROOT, "bayes.js_amd", "csrc")
    assert "amwg_pointwise.h" not in build_id.KERNEL_FILES
    src = "\n".join(ln.split("//")[0] for ln in open(os.path.join(csrc, "amwg_pointwise.h")).read().split("\n"))      # (code only: no comments)
    assert set(re.findall(r"\b(atomic[A-Za-z]+)\(", src)) == {"atomicAdd", "atomicMin", "atomicOr"}
    for target in re.findall(r"\batomic[A-Za-z]+\((?:\([^)]*\))?&(\w+)", src):
        assert target in ("cnt", "h", "state"), target
    for f in ("amwg_waic.hip", "amwg_loo.hip"):      # the model-dependent kernels are the header's: the units hold wrappers only
        text = open(os.path.join(csrc, f)).read()
        assert "_body<Family<MODEL>" in text and "F::term" not in text
    rtc = open(os.path.join(csrc, "amwg_rtc_headers.c")).read()
    assert '"amwg_pointwise.h"' in rtc and '"amwg_select.h"' in rtc
