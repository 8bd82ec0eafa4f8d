"""Development tool (GPU box; not part of the test suite): what dataset_waic() and dataset_loo() of a TRANSLATED CLOSURE (options.pointwise; csrc/amwg_pointwise.h
instantiated by hiprtc for the closure's UserTerms) cost beside the built-in family's, in one run, at 256 datasets x 256 chains x 1 000 kept draws x 1 000 observations:
  family    the Normal family on the data of the `normal` fixture of tests/js/pointwise_models.js: dataset_waic(), dataset_loo()
  twin      the README Normal closure on the same data: the same two calls, and their ratio to the family's
  logistic  the logistic-regression fixture, which has no family to stand beside: the same two calls
  compile   the first dataset_waic() of the twin in a fresh process on an empty code cache (a miss: hiprtc compiles the pointwise program) and again in a fresh
            process on the cache it left (a hit), each beside a steady call of the same process: first - steady is what the first call pays
Every step is a child process of its own under its own time limit; the steps are chained, and nothing is started after one that failed.  Host clock around each
call -- each ends in a stream synchronise --, one untimed warm-up, five timings of WAIC and three of LOO: median [min - max] in milliseconds.
    python tools/time_pointwise.py [--json profiles/pointwise.json] [--small]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BURN = 20261021, 100
STEP_LIMIT_S = 420


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms}


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def translated(name, D, n, tmp):
    import numpy as np
    out = os.path.join(tmp, "%s.json" % name)
    subprocess.run(["node", os.path.join(ROOT, "tools", "time_pointwise_translate.js"), out, name, str(D), str(n)], check=True, timeout=300, cwd=ROOT)
    t = json.load(open(out))
    unhex = lambda h: np.frombuffer(bytes.fromhex(h), dtype=np.float64).copy()
    t["arrays"] = [[unhex(a) for a in row] for row in t["arrays"]]
    t["data"] = [unhex(d) if d is not None else None for d in t["data"]]
    return t


def closure_specs(t, params, init):
    import model_spec
    specs = []
    for row in t["arrays"]:
        user = {"source": t["source"], "arrays": row, "array_types": t["array_types"], "n_derived": t["n_derived"], "lds_bytes": t["lds_bytes"],
                "lds_bytes_one_lane": t["lds_bytes_one_lane"], "parallel": t["parallel"], "max_threads": t["max_threads"], "work_per_eval": t["work_per_eval"],
                "work_one_lane": t["work_one_lane"], "pointwise": t["terms_source"]}
        specs.append({"user": user, "params": params, "P": len(init), "init": init, "comp_opts": [dict(model_spec.DEFAULT_OPT) for _ in init]})
    return specs


def step(name, D, cpd, kept, n_obs):
    """one measurement, in this process -> dict"""
    sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
    try:
        import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
    except Exception:
        pass
    import numpy as np
    import amwg_ctypes as A
    import model_spec
    inf = float("inf")
    real = lambda lower=-inf: {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": lower, "upper": inf}
    with tempfile.TemporaryDirectory() as tmp:
        if name == "family":
            t = translated("normal", D, n_obs, tmp)
            specs = [model_spec.build_spec("normal", {"x": x}) for x in t["data"]]
        elif name in ("twin", "compile_miss", "compile_hit"):
            t = translated("normal", D, n_obs, tmp)
            fam = model_spec.build_spec("normal", {"x": t["data"][0]})
            specs = closure_specs(t, fam["params"], fam["init"])
        else:
            t = translated("logistic", D, n_obs, tmp)
            specs = closure_specs(t, [real(), real()], [0.5, 0.5])
    s = A.Sampler(specs if D > 1 else specs[0], chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    out = {"library": A.lib().amwg_version().decode(), "kernel": s.kernel_name() if hasattr(s, "kernel_name") else None}
    if name.startswith("compile"):
        out["first_dataset_waic_ms"] = clocked(lambda: s.dataset_waic())
        out["steady_dataset_waic"] = summary([clocked(lambda: s.dataset_waic()) for _ in range(3)])
        out["first_minus_steady_ms"] = out["first_dataset_waic_ms"] - out["steady_dataset_waic"]["median_ms"]
    else:
        w = s.dataset_waic()      # warm-up (a closure: the compile)
        out["dataset_waic"] = summary([clocked(lambda: s.dataset_waic()) for _ in range(5)])
        l = s.dataset_loo()
        out["dataset_loo"] = summary([clocked(lambda: s.dataset_loo()) for _ in range(3)])
        out["elpd_waic_dataset0"], out["elpd_loo_dataset0"] = float(w["summary"][0][0]), float(l["summary"][0][0])
        assert np.isfinite(w["summary"]).all() and np.isfinite(l["summary"]).all()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 4 datasets x 64 chains x 40 draws x 100 observations")
    ap.add_argument("--step", help="(internal) run one step in this process and print its JSON")
    ap.add_argument("--shape", help="(internal) D,cpd,kept,n_obs")
    a = ap.parse_args()
    if a.step:
        D, cpd, kept, n_obs = (int(v) for v in a.shape.split(","))
        print("RESULT " + json.dumps(step(a.step, D, cpd, kept, n_obs)), flush=True)
        return
    shape = (4, 64, 40, 100) if a.small else (256, 256, 1000, 1000)
    out = {"shape": dict(zip(("datasets", "chains_per_dataset", "kept", "n_obs"), shape)), "results": {}}
    R = out["results"]
    with tempfile.TemporaryDirectory() as cache:
        for name in ("family", "twin", "logistic", "compile_miss", "compile_hit"):
            env = dict(os.environ)
            if name.startswith("compile"):
                env["AMWG_CACHE_DIR"] = cache      # empty for the miss; what the miss left for the hit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--shape", ",".join(str(v) for v in shape)], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S, env=env, cwd=ROOT)
            lines = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                print("step %s failed (exit %d); nothing further is started\n%s" % (name, p.returncode, p.stderr[-3000:]), flush=True)
                sys.exit(1)
            R[name] = json.loads(lines[-1][len("RESULT "):])
            print("%s: %s" % (name, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in R[name].items() if k != "library"})), flush=True)
    out["ratios"] = {"twin_over_family_dataset_waic": R["twin"]["dataset_waic"]["median_ms"] / R["family"]["dataset_waic"]["median_ms"],
                     "twin_over_family_dataset_loo": R["twin"]["dataset_loo"]["median_ms"] / R["family"]["dataset_loo"]["median_ms"]}
    print("ratios: %s" % json.dumps(out["ratios"]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
