"""Development tool (GPU box; not part of the test suite): what posterior predictive calibration (dataset_predictive; csrc/amwg_predictive.hip) costs.
One Normal dataset sampler, 256 datasets x 256 chains x 1 000 kept draws x 1 000 observations; three steps on stored draws:
  own   in-sample, 1 000 observations per dataset: dataset_predictive() beside dataset_waic() of the same run, and beside the route a caller had before --
        fetch_draws and scipy's norm.cdf -- on 2 datasets, EXTRAPOLATED to all of them and labelled so
  fold  m = 200 held-out observations per dataset: dataset_predictive(held) beside dataset_heldout(held) of the same run
  one   m = 1 per dataset: dataset_predictive(held) beside dataset_heldout(held)
Every step is a child process of its own under its own time limit; the steps are chained, and nothing is started after one that failed.  Host clock around each call
-- each ends in a stream synchronise --, one untimed warm-up, five timings: median [min - max] in milliseconds.
    python tools/time_predictive.py [--json profiles/predictive.json] [--small]"""
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

    m = {"own": n_obs, "fold": n_obs // 5, "one": 1}[name]
    specs = [spec_of(n_obs, SEED + d) for d in range(D)]
    held = None if name == "own" else [spec_of(m, SEED + 5000 + d) for d in range(D)]
    s = A.Sampler(specs, chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    out = {"library": A.lib().amwg_version().decode(), "observations_per_dataset": m}
    first = s.dataset_predictive(held, pointwise=False)
    assert np.isfinite(first["summary"]).all()
    out["cover50_cover90_of_dataset_0"] = first["summary"][0][:2].tolist()
    out["dataset_predictive"] = summary([clocked(lambda: s.dataset_predictive(held, pointwise=False)) for _ in range(5)])
    if name == "own":
        s.dataset_waic()
        out["dataset_waic"] = summary([clocked(lambda: s.dataset_waic()) for _ in range(5)])
        out["predictive_over_waic"] = out["dataset_predictive"]["median_ms"] / out["dataset_waic"]["median_ms"]

        def by_scipy():      # the caller's route: the draws to the host, the CDF in scipy (2 datasets)
            from scipy.stats import norm
            dr = s.fetch_draws()
            for d in range(2):
                mu, sg = dr[:, 0, d * cpd:(d + 1) * cpd].reshape(-1), dr[:, 1, d * cpd:(d + 1) * cpd].reshape(-1)
                norm.cdf((specs[d]["data"]["x"][None, :] - mu[:, None]) / sg[:, None]).mean(axis=0)
                np.sqrt((sg * sg).mean() + mu.var())
        out["fetch_and_scipy_2_datasets"] = summary([clocked(by_scipy) for _ in range(3)])
        out["fetch_and_scipy_extrapolated_ms"] = out["fetch_and_scipy_2_datasets"]["median_ms"] * D / 2
        out["extrapolated_scipy_over_predictive"] = out["fetch_and_scipy_extrapolated_ms"] / out["dataset_predictive"]["median_ms"]
    else:
        s.dataset_heldout(held)
        out["dataset_heldout"] = summary([clocked(lambda: s.dataset_heldout(held)) for _ in range(5)])
        out["predictive_over_heldout"] = out["dataset_predictive"]["median_ms"] / out["dataset_heldout"]["median_ms"]
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
    for name in ("own", "fold", "one"):
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
