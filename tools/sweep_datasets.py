"""Development tool (GPU box; not part of the test suite): what many datasets in one sampler cost and buy, at cfg2's shape -- the Normal family, N = 10^4
observations, 65 536 chains, one lane per chain, 256-thread workgroups.  Three lines, each after one untimed warm-up launch, at least five launches of 100 steps:
  (a) the ordinary sampler on ONE dataset (the parent's kernel): kernel_ms of amwg_launch_info per launch;
  (b) a dataset sampler, 256 datasets x 256 chains (amwg_create_datasets, the kernel's twin): kernel_ms likewise;
  (c) what a user has without it for the job of (b): 64 ordinary samplers x 1024 chains, launched side by side as tests/gpu_util.run_schedule_many does
      (burn_async on every sampler, then sync on every sampler), timed wall-clock around the joint launches.
Median, min and max in milliseconds per 100 steps.
    python tools/sweep_datasets.py [--launches 7] [--json profiles/datasets_sweep.json]
(b) and (a) execute the same instructions per update once the tile is staged; (b) against (c) is the comparison a user cares about."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
except Exception:
    pass
import amwg_ctypes as A  # noqa: E402
import model_spec  # noqa: E402

N_OBS, CHAINS, STEPS, SEED = 10000, 65536, 100, 20261018


def spec_of(d):
    return model_spec.build_spec("normal", model_spec.make_data("normal", N_OBS, 3000 + d))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms), "all_ms": ms}


def kernel_times(s, launches):
    s.burn(STEPS)      # untimed: log_post(init), first staging, instruction cache
    out = []
    for _ in range(launches):
        s.burn(STEPS)
        out.append(s.launch_info()["kernel_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "datasets_sweep.json"))
    args = ap.parse_args()
    launches = max(5, args.launches)
    geometry = dict(lanes_per_chain=1, block_threads=256, steps_per_launch=STEPS)
    res = {"shape": {"model": "normal", "n_obs": N_OBS, "chains": CHAINS, "steps_per_launch": STEPS, "lanes_per_chain": 1, "block_threads": 256},
           "library": A.lib().amwg_version().decode()}

    s = A.Sampler(spec_of(0), chains=CHAINS, seed=SEED, **geometry)
    res["a_one_dataset"] = dict(summary(kernel_times(s, launches)), kernel=s.launch_info()["kernel"], what="ordinary sampler, 1 dataset x 65536 chains, kernel_ms")
    s.close()
    print("(a)", json.dumps({k: v for k, v in res["a_one_dataset"].items() if k != "all_ms"}), flush=True)

    specs = [spec_of(d) for d in range(256)]
    s = A.Sampler(specs, chains=CHAINS, seed=SEED, **geometry)
    res["b_dataset_sampler"] = dict(summary(kernel_times(s, launches)), kernel=s.launch_info()["kernel"], what="dataset sampler, 256 datasets x 256 chains, kernel_ms")
    s.close()
    print("(b)", json.dumps({k: v for k, v in res["b_dataset_sampler"].items() if k != "all_ms"}), flush=True)

    many = [A.Sampler(specs[d], chains=1024, seed=SEED, chain_offset=1024 * d, **geometry) for d in range(64)]

    def joint():
        t0 = time.perf_counter()
        for q in many:
            q.burn_async(STEPS)
        for q in many:
            q.sync()
        return (time.perf_counter() - t0) * 1e3
    joint()
    res["c_64_samplers"] = dict(summary([joint() for _ in range(launches)]), kernel=many[0].launch_info()["kernel"],
                                what="64 ordinary samplers x 1024 chains launched side by side, wall-clock around the joint launches")
    for q in many:
        q.close()
    print("(c)", json.dumps({k: v for k, v in res["c_64_samplers"].items() if k != "all_ms"}), flush=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
    print("wrote", args.json)


if __name__ == "__main__":
    main()
