"""Development tool (GPU box; not part of the test suite): what one sampler over many datasets buys for a TRANSLATED closure -- ds_scaled_normal of
tests/js/dataset_models.js (`ld.norm(x[i] * 2, mu, sigma)`: no built-in family) at N = 1 000, 256 datasets x 256 chains.
  (a) the dataset sampler (amwg_create_user_datasets), burn(1000): one launch;
  (b) the way without it: 256 ordinary amwg_create_user samplers of 256 chains (chain_offset d * 256), burn(1000) on each in a loop -- (b1) one after the other,
      as a user's loop over segments does it, (b2) queued side by side (burn_async on each, then sync).
Both sides at the geometry the planner gives each of them (lanes_per_chain = 0, block_threads = 0): that is what a caller gets.  (a), (b1), (b2) alternate in one
process: one untimed warm-up each, then nine wall-clock timings each, median [min - max] in milliseconds; the constructors are timed separately (the first one of each
kind compiles or loads the code object, the others find it in the process).  The library's version string carries the kernel id.
    python tools/time_user_datasets.py [--json profiles/user_datasets.json]
    python tools/time_user_datasets.py --rehearse          # tiny shapes"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, CPD, N_OBS, STEPS, REPS, SEED = 256, 256, 1000, 1000, 9, 20261018


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms}


def fmt(r):
    return "%.1f ms [%.1f - %.1f]" % (r["median_ms"], r["min_ms"], r["max_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "user_datasets.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    n_datasets, cpd, n_obs, steps = (4, 64, 50, 20) if args.rehearse else (D, CPD, N_OBS, STEPS)
    sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
    try:
        import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
    except Exception:
        pass
    import amwg_ctypes as A
    import user_datasets_lib as udl
    t0 = time.perf_counter()
    tag = udl.translate_sized("ds_scaled_normal", n_obs, n_datasets)
    specs = udl.specs(tag)
    translate_ms = (time.perf_counter() - t0) * 1e3
    assert len(specs) == n_datasets
    res = {"shape": {"closure": "ds_scaled_normal", "n_obs": n_obs, "datasets": n_datasets, "chains_per_dataset": cpd, "steps": steps, "timings": REPS},
           "command": "python tools/time_user_datasets.py", "library": A.lib().amwg_version().decode(), "translate_datasets_and_load_ms": translate_ms}

    t0 = time.perf_counter()
    ds = A.Sampler(specs, chains=n_datasets * cpd, seed=SEED)
    res["a_constructor_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    many = [A.Sampler(specs[d], chains=cpd, seed=SEED, chain_offset=d * cpd) for d in range(n_datasets)]
    res["b_constructors_ms"] = (time.perf_counter() - t0) * 1e3
    res["a_launch"], res["b_launch"] = ds.launch_info(), many[0].launch_info()

    def a():
        t = time.perf_counter()
        ds.burn(steps)
        return (time.perf_counter() - t) * 1e3

    def b1():
        t = time.perf_counter()
        for q in many:
            q.burn(steps)
        return (time.perf_counter() - t) * 1e3

    def b2():
        t = time.perf_counter()
        for q in many:
            q.burn_async(steps)
        for q in many:
            q.sync()
        return (time.perf_counter() - t) * 1e3

    runs = {"a_dataset_sampler": a, "b1_one_sampler_per_dataset_in_turn": b1, "b2_one_sampler_per_dataset_side_by_side": b2}
    times = {k: [] for k in runs}
    for rep in range(REPS + 1):      # (the first round is the warm-up: log_post(init), first staging)
        for k, f in runs.items():
            ms = f()
            if rep:
                times[k].append(ms)
    for k in runs:
        res[k] = summary(times[k])
        print("%-42s %s" % (k, fmt(res[k])), flush=True)
    print("constructors: (a) %.0f ms, (b) %.0f ms for %d samplers; kernels: (a) %s %d lanes x %d, (b) %s %d lanes x %d" % (
        res["a_constructor_ms"], res["b_constructors_ms"], n_datasets, res["a_launch"]["kernel"], res["a_launch"]["lanes_per_chain"], res["a_launch"]["block_threads"],
        res["b_launch"]["kernel"], res["b_launch"]["lanes_per_chain"], res["b_launch"]["block_threads"]), flush=True)
    ds.close()
    for q in many:
        q.close()
    if not args.rehearse:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
