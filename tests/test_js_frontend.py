"""The JavaScript host side (north_star: host code stays JavaScript over an N-API addon).

test_frontend.js: parameter completion KATs, option merging, model recognition, errors (no GPU).
test_gpu.js (-m gpu): the README programs, verbatim, through bayes.js_amd on the GPU reproduce the
seeded reference runs of tests/golden/ bit for bit.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed")


def run_node(script, timeout):
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", script)], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + "\n" + p.stderr
    return p.stdout


@needs_node
def test_js_frontend_host_logic():
    assert "frontend ok" in run_node("test_frontend.js", 120)


@needs_node
@pytest.mark.gpu
def test_js_frontend_on_gpu_matches_reference_goldens():
    out = run_node("test_gpu.js", 600)
    assert "gpu frontend ok" in out
    # test_gpu.js section 8: the Normal family on normal_key64's data under the BigInt key 2^64 - 1 from chain id 2^32 - 3, 8 chains, burn 30, sample 5 -- the same
    # sampler made through the C ABI from Python gives the same uniform counts and draws, and its chains are the oracle's (chain 5: c3 = 1)
    import json
    import amwg_ctypes as A
    import golden_io
    import model_spec
    import oracle_lib
    js = json.loads(next(l for l in out.splitlines() if l.startswith("key64 "))[6:])
    spec = model_spec.spec_from_golden(golden_io.load("normal_key64"))
    seed, off = 2 ** 64 - 1, 2 ** 32 - 3
    s = A.Sampler(spec, chains=8, seed=seed, chain_offset=off, lanes_per_chain=1)
    s.burn(30)
    d = s.sample(5)
    assert js["uniforms"] == s.diag()["uniforms"].tolist()
    assert js["mu"] == d[:, 0, :].reshape(-1).tolist() and js["sigma"] == d[:, 1, :].reshape(-1).tolist()
    for c in (0, 5):
        o = oracle_lib.OracleChain(spec, seed, off + c, lanes=1)
        o.burn(30)
        assert d[:, :, c].tobytes() == o.sample(5).tobytes() and int(s.diag()["uniforms"][c]) == o.uniforms()
    s.close()


@needs_node
@pytest.mark.gpu
def test_translated_closures_on_gpu_match_reference_goldens():
    """Arbitrary user closures (real/int/binary params, every scalar ld.*, derived quantities) through translate.js + hiprtc."""
    assert "gpu user models ok" in run_node("test_gpu_user.js", 1200)
