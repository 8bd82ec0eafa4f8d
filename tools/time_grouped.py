"""Development tool (GPU box; not part of the test suite): what WAIC and PSIS-LOO over GROUPS of observations (dataset_waic(groups=), dataset_loo(groups=);
csrc/amwg_pointwise.h, GROUPS OF OBSERVATIONS) cost beside the ungrouped calls of the same run, which perform the same S x n term evaluations.
  datasets  one Normal dataset sampler, 256 datasets x 256 chains x 1 000 kept draws x 1 000 observations, three pairs of timings on the same stored draws:
            ungrouped; 50 groups of 20; 4 groups of 250 (the select kernel spreads the four groups over the wavefront, the other two walking kernels do not);
            grouped / ungrouped for WAIC and for LOO; the select passes of each, from the same kernels over the fetched draws through the test library
  hier      one hierarchical sampler (8 groups, 4 096 chains x 250 kept draws x 4 000 observations), ungrouped beside grouped by its own group array
Every step is a child process of its own under its own time limit; the steps are chained, and nothing is started after one that failed.  Host clock around each call
-- each ends in a stream synchronise --, one untimed warm-up, five timings of WAIC and three of LOO: median [min - max] in milliseconds.
    python tools/time_grouped.py [--json profiles/grouped.json] [--small]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BURN = 20261126, 100
STEP_LIMIT_S = 540


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms}


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


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

    def spec_of(model, n, seed, **kw):
        data = model_spec.make_data(model, n, seed, **kw)
        return model_spec.build_spec(model, {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype != np.int32 else v) for k, v in data.items()}, **kw)

    if name == "datasets":
        specs = [spec_of("normal", n_obs, SEED + d) for d in range(D)]
        layouts = {"ungrouped": None, "groups_50": [np.arange(n_obs, dtype=np.int32) % (n_obs // 20)] * D, "groups_4": [np.arange(n_obs, dtype=np.int32) % 4] * D}
    else:
        specs = [spec_of("hier_normal", n_obs, SEED, G=8)]
        layouts = {"ungrouped": None, "own_groups": [np.asarray(specs[0]["data"]["g"], dtype=np.int32)]}
    s = A.Sampler(specs if len(specs) > 1 else specs[0], chains=len(specs) * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    out = {"library": A.lib().amwg_version().decode()}
    draws0 = None
    for label, groups in layouts.items():
        w = s.dataset_waic(groups=groups)      # warm-up
        r = {"dataset_waic": summary([clocked(lambda: s.dataset_waic(groups=groups)) for _ in range(5)])}
        l = s.dataset_loo(groups=groups)
        r["dataset_loo"] = summary([clocked(lambda: s.dataset_loo(groups=groups)) for _ in range(3)])
        r["elpd_waic_dataset0"], r["elpd_loo_dataset0"] = float(w["summary"][0][0]), float(l["summary"][0][0])
        if groups is not None:
            r["n_groups_dataset0"] = int(l["n_groups"][0])
        assert np.isfinite(w["summary"]).all() and np.isfinite(l["summary"]).all()
        # the select passes: the same kernels over dataset 0's fetched draws through the test library (the product library does not count them)
        if draws0 is None:
            draws0 = np.ascontiguousarray(s.fetch_draws()[:, :, :cpd])
        A.loo_check(draws0, specs[:1], pointwise=False, groups=None if groups is None else groups[:1])
        r["select_passes_dataset0"] = A.loo_stats()[0]
        out[label] = r
    for label in layouts:
        if label != "ungrouped":
            out[label]["waic_over_ungrouped"] = out[label]["dataset_waic"]["median_ms"] / out["ungrouped"]["dataset_waic"]["median_ms"]
            out[label]["loo_over_ungrouped"] = out[label]["dataset_loo"]["median_ms"] / out["ungrouped"]["dataset_loo"]["median_ms"]
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
    shapes = {"datasets": (4, 64, 40, 100), "hier": (1, 64, 40, 400)} if a.small else {"datasets": (256, 256, 1000, 1000), "hier": (1, 4096, 250, 4000)}
    out = {"shapes": {k: dict(zip(("datasets", "chains_per_dataset", "kept", "n_obs"), v)) for k, v in shapes.items()}, "results": {}}
    for name, shape in shapes.items():
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--shape", ",".join(str(v) for v in shape)], capture_output=True, text=True,
                           timeout=STEP_LIMIT_S, cwd=ROOT)
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print("step %s failed (exit %d); nothing further is started\n%s" % (name, p.returncode, p.stderr[-3000:]), flush=True)
            sys.exit(1)
        R = out["results"][name] = json.loads(lines[-1][len("RESULT "):])
        for label, r in R.items():
            if isinstance(r, dict):
                print("%s %s: dataset_waic %.1f ms, dataset_loo %.1f ms, %d select passes%s" % (name, label, r["dataset_waic"]["median_ms"], r["dataset_loo"]["median_ms"],
                      r["select_passes_dataset0"], "; grouped / ungrouped: WAIC %.2f, LOO %.2f" % (r["waic_over_ungrouped"], r["loo_over_ungrouped"]) if "loo_over_ungrouped" in r else ""), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
