"""TEST INFRASTRUCTURE for options.datasets with a translated closure: runs tests/js/translate_datasets_cli.js once per session (the product's translate_datasets over the
closures of tests/js/dataset_models.js, D = 3 datasets each) and hands out what it wrote -- the one source, its meta, every dataset's arrays, every dataset's own default
translation -- and the specs amwg_ctypes.Sampler takes."""
import ctypes as C
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

import model_spec
import user_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
D = 3
_dir = None
_extra = set()


def workdir():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="amwg_user_ds_")
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "translate_datasets_cli.js"), _dir], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + "\n" + p.stderr
    return _dir


def translate_sized(name, n_obs, n_datasets=D):
    """a closure of dataset_models.js at another size and number of datasets (tools/time_user_datasets.py); -> its tag"""
    tag = "%s_%d" % (name, n_obs)
    if tag not in _extra:
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "translate_datasets_cli.js"), workdir(), "%s:%d:%d" % (name, n_obs, n_datasets)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + "\n" + p.stderr
        _extra.add(tag)
    return tag


def refusals():
    return json.load(open(os.path.join(workdir(), "refusals.json")))


def load(tag):
    """-> (source, meta, [arrays of dataset d])"""
    d = workdir()
    meta = json.load(open(os.path.join(d, tag + ".meta.json")))
    return (open(os.path.join(d, tag + ".hip")).read(), meta, [user_host.read_arrays(os.path.join(d, "%s.d%d.arrays.bin" % (tag, k))) for k in range(meta["n_datasets"])])


def load_own(tag, k):
    """the default translation of dataset k alone: -> (source, meta, arrays)"""
    d = workdir()
    stem = os.path.join(d, "%s.own%d" % (tag, k))
    return open(stem + ".hip").read(), json.load(open(stem + ".meta.json")), user_host.read_arrays(stem + ".arrays.bin")


def spec_of(source, meta, arrays, params_meta):
    """one amwg_ctypes.Sampler spec: the closure's source on one dataset's arrays"""
    init = [float(v) for v in params_meta["init"]]
    params = [dict(p, lower=float("-inf") if p["lower"] is None else float(p["lower"]), upper=float("inf") if p["upper"] is None else float(p["upper"])) for p in params_meta["params"]]
    return {"user": user_host.user_spec_part(source, arrays, meta), "params": params, "P": len(init), "init": init, "comp_opts": [dict(model_spec.DEFAULT_OPT) for _ in init]}


def specs(tag):
    """-> [spec of dataset d] under the ONE source"""
    source, meta, sets = load(tag)
    return [spec_of(source, meta, arrays, meta) for arrays in sets]


def own_spec(tag, k):
    source, meta, arrays = load_own(tag, k)
    return spec_of(source, meta, arrays, load(tag)[1])


class HostEval:
    """The one source compiled for the host (tests/host/user_eval_host.cpp, as tests/user_host.py builds it), evaluated on any dataset's arrays."""

    def __init__(self, tag):
        d = workdir()
        self.source, self.meta, self.sets = load(tag)
        so = os.path.join(d, tag + ".so")
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"),
               '-DAMWG_USER_SOURCE="%s"' % os.path.join(d, tag + ".hip"), "-o", so, os.path.join(ROOT, "tests", "host", "user_eval_host.cpp")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-4000:]
        self.lib = C.CDLL(so)
        self.lib.user_eval.restype = C.c_double
        self.lib.user_eval.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_double)]
        self.n_derived = self.lib.user_num_derived()

    def eval(self, k, state, lanes=1):
        """-> (log_post, [derived]) on dataset k"""
        typed = [a.astype([np.float64, np.uint8, np.int32][t]) for a, t in zip(self.sets[k], self.meta["array_types"])]
        ptrs = (C.c_void_p * max(1, len(typed)))(*[a.ctypes.data for a in typed])
        st = np.ascontiguousarray(state, dtype=np.float64)
        dv = np.zeros(max(1, self.n_derived))
        v = self.lib.user_eval(st.ctypes.data_as(C.POINTER(C.c_double)), ptrs, len(typed), lanes, dv.ctypes.data_as(C.POINTER(C.c_double)))
        return v, dv[: self.n_derived].tolist()
