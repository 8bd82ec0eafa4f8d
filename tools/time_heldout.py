"""Development tool (GPU box; not part of the test suite): what the held-out predictive density (dataset_heldout; csrc/amwg_heldout.hip) costs.
One Normal dataset sampler, 256 datasets x 256 chains x 1 000 kept draws x 1 000 observations; two steps on stored draws:
  fold  m = 200 held-out observations per dataset (5-fold of 1 000): dataset_heldout beside dataset_waic() of the same run scaled by 200 / 1 000, and beside the
        route a caller had before -- fetch_draws and numpy -- on 2 datasets, EXTRAPOLATED to all of them and labelled so
  one   m = 1 per dataset (an exact refit): dataset_heldout over all datasets; then, through the test library on the fetched draws of 8 datasets, the new kernel
        (heldout_check) beside WAIC's kernel on a 1-observation dataset (waic_check) -- both calls upload the same draws, so a call with no held-out observation at
        all (the upload alone) is timed too and subtracted from both: kernel_ratio = (waic - upload) / (heldout - upload)
Every step is a child process of its own under its own time limit; the steps are chained, and nothing is started after one that failed.  Host clock around each call
-- each ends in a stream synchronise --, one untimed warm-up, five timings: median [min - max] in milliseconds.
    python tools/time_heldout.py [--json profiles/heldout.json] [--small]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_grouped import BURN, SEED, STEP_LIMIT_S, clocked, summary  # noqa: E402


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

    def spec_of(n, seed):
        data = model_spec.make_data("normal", n, seed)
        return model_spec.build_spec("normal", {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()})

    m = n_obs // 5 if name == "fold" else 1
    specs = [spec_of(n_obs, SEED + d) for d in range(D)]
    held = [spec_of(m, SEED + 5000 + d) for d in range(D)]
    s = A.Sampler(specs, chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    out = {"library": A.lib().amwg_version().decode(), "held_out_per_dataset": m, "block_R": "group_block<F>(): 8 for the Normal family (taken, not searched)"}
    h = s.dataset_heldout(held)
    assert np.isfinite(h["summary"][:, 0]).all()
    out["dataset_heldout"] = summary([clocked(lambda: s.dataset_heldout(held)) for _ in range(5)])
    if name == "fold":
        s.dataset_waic()
        out["dataset_waic"] = summary([clocked(lambda: s.dataset_waic()) for _ in range(5)])
        out["waic_scaled_ms"] = out["dataset_waic"]["median_ms"] * m / n_obs
        out["heldout_over_scaled_waic"] = out["dataset_heldout"]["median_ms"] / out["waic_scaled_ms"]

        def by_numpy():      # the caller's route: the draws to the host, the likelihood in numpy (2 datasets)
            dr = s.fetch_draws()
            for d in range(2):
                mu, sg = dr[:, 0, d * cpd:(d + 1) * cpd].reshape(-1), dr[:, 1, d * cpd:(d + 1) * cpd].reshape(-1)
                ll = -0.5 * np.log(2 * np.pi) - np.log(sg)[:, None] - (held[d]["data"]["x"][None, :] - mu[:, None]) ** 2 / (2 * sg * sg)[:, None]
                top = ll.max(axis=0)
                (top + np.log(np.exp(ll - top).sum(axis=0)) - np.log(ll.shape[0])).sum()
        out["fetch_and_numpy_2_datasets"] = summary([clocked(by_numpy) for _ in range(3)])
        out["fetch_and_numpy_extrapolated_ms"] = out["fetch_and_numpy_2_datasets"]["median_ms"] * D / 2
        out["extrapolated_numpy_over_heldout"] = out["fetch_and_numpy_extrapolated_ms"] / out["dataset_heldout"]["median_ms"]
    else:
        Dk = min(D, 8)
        dr = np.ascontiguousarray(s.fetch_draws()[:, :, :Dk * cpd])
        none = [{"model": "normal", "n_obs": 0, "data": {"x": np.zeros(0)}}] * Dk
        calls = {"upload_only": lambda: A.heldout_check(dr, specs[:Dk], none, pointwise=False), "heldout_check": lambda: A.heldout_check(dr, specs[:Dk], held[:Dk], pointwise=False),
                 "waic_check_1_observation": lambda: A.waic_check(dr, held[:Dk], pointwise=False)}
        for k, c in calls.items():
            c()
            out[k] = summary([clocked(c) for _ in range(5)])
        up = out["upload_only"]["median_ms"]
        out["check_datasets"] = Dk
        out["heldout_kernels_ms"], out["waic_kernels_ms"] = out["heldout_check"]["median_ms"] - up, out["waic_check_1_observation"]["median_ms"] - up
        out["kernel_ratio_waic_over_heldout"] = out["waic_kernels_ms"] / out["heldout_kernels_ms"] if out["heldout_kernels_ms"] > 0 else None
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
        print("RESULT " + json.dumps(step(a.step, *(int(v) for v in a.shape.split(",")))), flush=True)
        return
    shape = (4, 64, 40, 100) if a.small else (256, 256, 1000, 1000)
    out = {"shape": dict(zip(("datasets", "chains_per_dataset", "kept", "n_obs"), shape)), "results": {}}
    for name in ("fold", "one"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--shape", ",".join(str(v) for v in shape)], capture_output=True, text=True,
                           timeout=STEP_LIMIT_S, cwd=ROOT)
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print("step %s failed (exit %d); nothing further is started\n%s" % (name, p.returncode, p.stderr[-3000:]), flush=True)
            sys.exit(1)
        R = out["results"][name] = json.loads(lines[-1][len("RESULT "):])
        print("%s: %s" % (name, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in R.items() if k != "library"})), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
