"""-m gpu: the edges of the wavefront's certified pass (csrc/amwg_pass.h norm_sq_pass_wave) -- the leftover observations behind the last full row.

n_obs % 64 observations do not fill a row.  The pass leaves them out of its rows: each chain adds them to its own sum after the butterfly, one read of the
leftovers (lane l: leftover l) requested before it, observation k then taken out of lane k.  Shapes: nothing but leftovers (1, 63), exactly one row and one
row + 1 (64, 65: no full block), one block and nothing else (1 024), one block + 16 leftovers (1 040), the flagship's row plan in small (1 808 = a block, the
parts 8 and 4, 16 leftovers), a twelve-row remainder with 63 leftovers (1 855), and the array in global memory instead of the LDS tile (12 304, 16 leftovers).

The default sampler (certified decisions) against the expression in every update (full_evaluation = 1), both at one lane per chain, 64 and 128 chains, default
workgroup size, 60 steps with adaptation on (burn 20 + sample 40: across the first batch of 50): draws, final state, every info counter (accepts, in-bounds
counts, prop_log_scale, ...) and the uniforms consumed, bit for bit.  Once with the wave scratch (means through the scalar memory path) and once, in a fresh
child process with AMWG_WAVE_SCRATCH=0 (read while a sampler is constructed), through the v_readlane form.  Every case asserts the kernel it ran."""
import json
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
NOBS = [1, 63, 64, 65, 1024, 1040, 1808, 1855, 12304]
CHAINS = [64, 128]
CASES = [(n, c) for n in NOBS for c in CHAINS]


def _run(s):
    s.burn(20)
    draws = s.sample(40, 1)
    info = s.info()
    return {"draws": draws.tobytes(), "state": s.state().tobytes(), "uniforms": s.diag()["uniforms"].tobytes(), "info": {k: v.tobytes() for k, v in info.items()}}


def _differences(got, want):
    bad = [k for k in ("draws", "state", "uniforms") if got[k] != want[k]]
    assert set(want["info"]) >= {"accepts", "inbounds", "prop_log_scale"}
    return bad + [k for k in want["info"] if got["info"][k] != want["info"][k]]


def _case(A, spec, chains, cert_kernel_prefix, ref_kernel_prefix):
    """-> (names of what differs between the default sampler and full_evaluation = 1, the default sampler's launch_info)"""
    r = A.Sampler(spec, chains=chains, seed=SEED, lanes_per_chain=1, full_evaluation=1)
    lr = r.launch_info()
    assert lr["kernel"].startswith(ref_kernel_prefix) and "_cert" not in lr["kernel"] and lr["lanes_per_chain"] == 1, lr
    want = _run(r)
    r.close()
    s = A.Sampler(spec, chains=chains, seed=SEED, lanes_per_chain=1)
    li = s.launch_info()
    assert li["kernel"].startswith(cert_kernel_prefix) and li["lanes_per_chain"] == 1 and li["block_threads"] <= 256, li      # (the wavefront's pass with blocks of 16 rows)
    got = _run(s)
    s.close()
    return _differences(got, want), li


def _normal_case(n_obs, chains):
    import amwg_ctypes as A
    import model_spec
    spec = model_spec.build_spec("normal", model_spec.make_data("normal", n_obs, 31))
    return _case(A, spec, chains, "amwg_step_kernel_cert<NormalModel,1,", "amwg_step_kernel<NormalModel,1,")


@pytest.mark.parametrize("n_obs,chains", CASES)
def test_leftover_observations_after_the_butterfly_decide_as_the_expression_does(n_obs, chains):
    """the scalar-means form of the pass (the wave scratch is allocated by default)"""
    assert "AMWG_WAVE_SCRATCH" not in os.environ
    bad, li = _normal_case(n_obs, chains)
    assert not bad, (bad, li)


def test_the_same_cases_through_the_readlane_form_without_wave_scratch():
    """AMWG_WAVE_SCRATCH=0 in a fresh child process (this file run as a script): every case of the list above must report, and report no difference."""
    env = dict(os.environ, AMWG_WAVE_SCRATCH="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert [(c["n_obs"], c["chains"]) for c in rec] == CASES
    for c in rec:
        assert c["differs"] == [], c


def test_certified_tail_of_a_closure_with_sixteen_leftover_observations_equals_the_expression():
    """bench_normal's closure over its first 1 040 observations (one block + 16 leftovers; hiprtc compiles the same pass for the closure's certified tail):
    amwg_user_step_cert against the closure evaluated in every update."""
    if shutil.which("node") is None:
        pytest.skip("node is not installed")
    import amwg_ctypes as A
    import model_spec
    import user_host
    n, name = 1040, "bench_normal_n1040"
    p = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "translate_truncated_cli.js"), user_host.workdir(), "bench_normal", str(n), name], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    src, arrays, meta = user_host.translated(name)
    assert meta["cert_tail_n"] == n == len(arrays[0])
    fam = model_spec.build_spec("normal", {"x": arrays[0]})
    opt = dict(model_spec.DEFAULT_OPT)
    spec = {"user": user_host.user_spec_part(src, arrays, meta), "P": 2, "init": list(fam["init"]), "comp_opts": [dict(opt), dict(opt)], "params": fam["params"]}
    bad, li = _case(A, spec, 128, "amwg_user_step_cert", "amwg_user_step")
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
    for n, c in CASES:
        bad, li = _normal_case(n, c)
        out.append({"n_obs": n, "chains": c, "differs": bad, "kernel": li["kernel"], "block_threads": li["block_threads"]})
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    _child()
