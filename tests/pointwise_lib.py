"""What the options.pointwise tests share: the fixtures of tests/js/pointwise_models.js as tests/js/pointwise_cli.js writes them (translated by the product's
translator, with Node's own term values as the truth), decoded once per (n, states) and left unchanged."""
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["normal", "bern", "hier", "pois_glm", "logistic", "locals", "head_local", "derived_int", "wide_state", "minus_inf"]
REJECTED = ["loop_not_last", "acc_twice", "has_break", "early_return", "under_if", "derived_in_loop", "draw_too_large"]
DTYPES = {0: np.float64, 1: np.uint8, 2: np.int32}      # AMWG_F64, AMWG_U8, AMWG_I32


def unhex(h):
    return np.frombuffer(bytes.fromhex(h), dtype=np.float64).copy()


@functools.lru_cache(maxsize=None)
def fixtures(n, n_states=4, names=()):
    """-> the CLI's record for n observations: models{name: {...}}, rejected{}, identity{} (the last two only when no names are given)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pw.json")
        subprocess.run(["node", os.path.join(ROOT, "tests", "js", "pointwise_cli.js"), out, str(n), str(n_states)] + list(names), check=True, timeout=300, cwd=ROOT)
        rec = json.load(open(out))
    for m in rec["models"].values():
        if "source" not in m:
            continue
        m["arrays"] = [unhex(a) for a in m["arrays"]]
        m["states"] = np.array([unhex(s) for s in m["states"]])      # [n_states][P]
        m["terms"] = np.array([unhex(t) for t in m["terms"]])        # [n_states][n_obs]
    return rec


def user_spec(m):
    """the closure as amwg_ctypes takes it (Sampler's spec["user"]; user_waic_check's `users` entry)"""
    return {"source": m["source"], "arrays": m["arrays"], "array_types": m["array_types"], "n_derived": m["n_derived"], "lds_bytes": m["lds_bytes"],
            "lds_bytes_one_lane": m["lds_bytes_one_lane"], "parallel": m["parallel"], "max_threads": m["max_threads"], "work_per_eval": m["work_per_eval"],
            "work_one_lane": m["work_one_lane"]}


def draws_of(m, rows, chains, PR=None):
    """synthetic draws [rows][PR][chains] whose draw s = row * chains + chain is state s % n_states of the fixture (derived components: zeros)"""
    st = m["states"]
    PR = m["P"] + m["n_derived"] if PR is None else PR
    dr = np.zeros((rows, PR, chains))
    for r in range(rows):
        for c in range(chains):
            dr[r, :m["P"], c] = st[(r * chains + c) % len(st)]
    return dr


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
