"""TEST INFRASTRUCTURE: the closures of tests/js/logit_models.js translated with the product's translator (node tests/js/translate_logit_cli.js), and the
sampler spec they all share (four real coefficients)."""
import json
import os
import shutil
import subprocess
import tempfile

import user_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
_dir = None


def translated(label, opts=None):
    """label: name[@n[@ymode]] of tests/js/logit_models.js -> (source, arrays, meta); opts: extra translator options"""
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="amwg_logit_")
    d = _dir if not opts else tempfile.mkdtemp(prefix="amwg_logit_opts_")
    stem = os.path.join(d, label.replace("@", "_"))
    if not os.path.exists(stem + ".hip"):
        env = dict(os.environ, AMWG_TRANSLATE_OPTS=json.dumps(opts or {}))
        p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "translate_logit_cli.js"), d, label], cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout + "\n" + p.stderr
    return open(stem + ".hip").read(), user_host.read_arrays(stem + ".arrays.bin"), json.load(open(stem + ".meta.json"))


def spec(label, init=(0.0, 0.0, 0.0, 0.0)):
    """-> (sampler spec, source, meta)"""
    src, arrays, meta = translated(label)
    opt = {"prop_log_scale": 0.0, "batch_size": 50, "max_adaptation": 0.33, "initial_adaptation": 1.0, "target_accept_rate": 0.44, "is_adapting": True}
    params = [{"type": "real", "len": 4, "top": 4, "multidim": 1, "lower": -INF, "upper": INF}]
    return {"user": user_host.user_spec_part(src, arrays, meta), "params": params, "P": 4, "init": list(init), "comp_opts": [dict(opt) for _ in range(4)], "n_obs": meta["logit_tail_n"]}, src, meta
