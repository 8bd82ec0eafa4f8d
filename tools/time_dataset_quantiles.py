"""Development tool (GPU box; not part of the test suite): what per-dataset quantiles cost beside the pooled call, on the same number of values -- the Normal
family, N = 10^4 observations, 65 536 chains, sample(1000), probabilities [0.025, 0.5, 0.975]:
  (a) a dataset sampler, 256 datasets x 256 chains: dataset_quantiles -- the radix select, one workgroup per (recorded value, dataset), nothing moved or sorted;
  (b) an ordinary sampler of 65 536 chains: the pooled quantiles -- gather, hipCUB radix sort, pick.
Both samplers are built and sampled once (the draws stay on the device); then (a) and (b) alternate in this one process, one untimed warm-up each and nine
timings each, host clock around the call (which ends in a stream synchronise).  Median [min - max] in milliseconds, and the kernel id of the library.
    python tools/time_dataset_quantiles.py [--json profiles/dataset_quantiles.json]
The margin of the comparison is (b)'s own min-max spread: `a_within_margin` says whether (a)'s median exceeds (b)'s median by more than that."""
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

N_OBS, CHAINS, DATASETS, BURN, SAMPLE, SEED, TIMINGS = 10000, 65536, 256, 300, 1000, 20261018, 9
PROBS = [0.025, 0.5, 0.975]


def spec_of(d):
    return model_spec.build_spec("normal", model_spec.make_data("normal", N_OBS, 3000 + d))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "timings": len(ms), "all_ms": ms}


def sampled(spec):
    s = A.Sampler(spec, chains=CHAINS, seed=SEED, lanes_per_chain=1, block_threads=256)
    s.burn(BURN)
    s.sample_async(SAMPLE)      # the draws stay in the library's device buffer: the summaries read them there
    s.sync()
    return s


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dataset_quantiles.json"))
    args = ap.parse_args()
    version = A.lib().amwg_version().decode()
    a = sampled([spec_of(d) for d in range(DATASETS)])
    b = sampled(spec_of(0))
    calls = {"a": lambda: a.dataset_quantiles(PROBS), "b": lambda: b.quantiles(PROBS)}
    ms = {"a": [], "b": []}
    for k in ("a", "b"):
        calls[k]()      # warm-up, untimed
    for _ in range(TIMINGS):
        for k in ("a", "b"):
            ms[k].append(clocked(calls[k]))
    a.close()
    b.close()
    res = {"shape": {"model": "normal", "n_obs": N_OBS, "chains": CHAINS, "kept_draws": SAMPLE, "recorded_values": 2, "probs": PROBS},
           "library": version, "kernel_id": version.split("kernels ")[-1],
           "a_dataset_quantiles": dict(summary(ms["a"]), what="dataset sampler, %d datasets x %d chains: dataset_quantiles (radix select in place)" % (DATASETS, CHAINS // DATASETS)),
           "b_pooled_quantiles": dict(summary(ms["b"]), what="ordinary sampler, %d chains: quantiles (gather + hipCUB radix sort + pick)" % CHAINS)}
    sa, sb = res["a_dataset_quantiles"], res["b_pooled_quantiles"]
    res["a_within_margin"] = sa["median_ms"] <= sb["median_ms"] + sb["spread_ms"]
    for k in ("a_dataset_quantiles", "b_pooled_quantiles"):
        r = res[k]
        print("(%s) %.3f ms [%.3f - %.3f]  %s" % (k[0], r["median_ms"], r["min_ms"], r["max_ms"], r["what"]), flush=True)
    print("kernel id %s; (a) within (b)'s median + spread: %s" % (res["kernel_id"], res["a_within_margin"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
    print("wrote", args.json)


if __name__ == "__main__":
    main()
