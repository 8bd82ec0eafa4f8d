"""Development tool (GPU box; not part of the test suite): what the WAIC fold of an armed summarize() costs (csrc/amwg_waic_fold.hip, waic_fold_body) and beside what.
Every step is a process of its own under its own time limit (this file run again with --step); the parent only collects their JSON lines.
  unarmed  a dataset sampler of 256 datasets x 256 chains (the Normal family, n_obs = 1 000): summarize(1 000)
  armed    the same after set_waic(): summarize(1 000), the records' bytes, the windows, and dataset_waic() (the finish) apart
  stored   the same sampler holding the 1 000 kept draws: sample_async + sync, then dataset_waic() -- the yardstick: the fold evaluates the same S x n terms
  long     a shape too long to store at the same rate of work: 64 datasets x 64 chains x 200 000 kept draws x 200 observations, armed; one timing
Host clock around each call -- each ends in a stream synchronise --, one untimed warm-up, five timings; median [min - max] in milliseconds.  The figure of
interest is (armed - unarmed) / stored, with the spread of each beside it.
    python tools/time_waic_fold.py [--json profiles/waic_fold.json] [--small]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BURN, REPEATS = 20261126, 300, 5
LIMIT_S = {"unarmed": 240, "armed": 240, "stored": 240, "long": 600}


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms}


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def step(name, small):
    sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
    try:
        import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
    except Exception:
        pass
    import numpy as np
    import amwg_ctypes as A
    import model_spec

    def normal_spec(n_obs, seed):
        data = model_spec.make_data("normal", n_obs, seed)
        return model_spec.build_spec("normal", {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()})

    D, cpd, kept, n_obs = (8, 64, 50, 100) if small else (256, 256, 1000, 1000)
    if name == "long":
        D, cpd, kept, n_obs = (8, 64, 2000, 100) if small else (64, 64, 200000, 200)
    s = A.Sampler([normal_spec(n_obs, 500 + d) for d in range(D)], chains=D * cpd, seed=SEED)
    s.burn(BURN)
    out = {"library": A.lib().amwg_version().decode(), "shape": {"datasets": D, "chains_per_dataset": cpd, "kept": kept, "n_obs": n_obs}}
    if name == "stored":
        s.sample_async(kept)
        s.sync()
        s.dataset_waic()
        out["dataset_waic"] = summary([clocked(s.dataset_waic) for _ in range(REPEATS)])
    else:
        if name != "unarmed":
            s.set_waic()
        if name != "long":
            s.summarize(kept)
        out["summarize"] = summary([clocked(lambda: s.summarize(kept)) for _ in range(1 if name == "long" else REPEATS)])
        out["summary_info"] = s.summary_info()
        if name != "unarmed":
            out["waic_info"] = s.waic_info()
            got = s.dataset_waic()
            assert not np.isnan(got["summary"]).any()
            out["finish"] = summary([clocked(s.dataset_waic) for _ in range(REPEATS)])
            out["elpd_waic_dataset_0"] = float(got["summary"][0][0])
    s.close()
    print("STEP " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 8 datasets x 64 chains x 50 draws x 100 observations")
    ap.add_argument("--step", choices=sorted(LIMIT_S))
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.small)
    R = {}
    for name in ("unarmed", "armed", "stored", "long"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + (["--small"] if a.small else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[name])      # (a step that faults or runs out of time ends the tool: nothing runs after it)
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("STEP ")]
        if p.returncode != 0 or not lines:
            raise SystemExit("step %s failed (exit %d):\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
        R[name] = json.loads(lines[-1][5:])
        t = R[name].get("summarize") or R[name]["dataset_waic"]
        print("(%s) %.3f ms [%.3f - %.3f]  %s" % (name, t["median_ms"], t["min_ms"], t["max_ms"], json.dumps(R[name]["shape"])), flush=True)
    un, ar, st = R["unarmed"]["summarize"], R["armed"]["summarize"], R["stored"]["dataset_waic"]
    added = ar["median_ms"] - un["median_ms"]
    out = {"results": R, "fold_added_ms": added, "stored_dataset_waic_ms": st["median_ms"], "added_over_stored": added / st["median_ms"],
           "spread_ms": {"unarmed": un["max_ms"] - un["min_ms"], "armed": ar["max_ms"] - ar["min_ms"], "stored": st["max_ms"] - st["min_ms"]}}
    print("armed - unarmed = %.3f ms; stored dataset_waic() %.3f ms; ratio %.3f; spreads %s; finish %.3f ms; records %d bytes in %d windows" %
          (added, st["median_ms"], out["added_over_stored"], json.dumps(out["spread_ms"]), R["armed"]["finish"]["median_ms"], R["armed"]["waic_info"]["bytes"],
           R["armed"]["summary_info"]["windows"]), flush=True)
    print("long: %.1f ms for %s, records %d bytes, %d windows" % (R["long"]["summarize"]["median_ms"], json.dumps(R["long"]["shape"]), R["long"]["waic_info"]["bytes"],
                                                                  R["long"]["summary_info"]["windows"]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
