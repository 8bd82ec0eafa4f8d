"""Development tool (GPU box; not part of the test suite): what folding the kept draws costs beside storing them, at the cfg2 shape -- the Normal family,
N = 10^4 observations, 65 536 chains, 1 000 steps, thin 1:
  (a) sample_async + sync: the draws stored (1.05 GB on the device);
  (b) summarize: the draws folded window by window into per-chain accumulators (the default window, 64 MiB).
Two samplers of the same seed, burnt in alike; one untimed warm-up call each, then (a) and (b) alternate in this one process, five timings each.  The time is
launch_info()'s kernel_ms: HIP events around everything the call enqueued, the folds included.  Median [min - max] in milliseconds.
    python tools/summarize_cost.py [--json profiles/streaming_summaries.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
except Exception:
    pass
import amwg_ctypes as A  # noqa: E402
import model_spec  # noqa: E402

N_OBS, CHAINS, BURN, STEPS, SEED, TIMINGS = 10000, 65536, 300, 1000, 20261018, 5


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "timings": len(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "streaming_summaries.json"))
    args = ap.parse_args()
    version = A.lib().amwg_version().decode()
    spec = model_spec.build_spec("normal", model_spec.make_data("normal", N_OBS, 3000))
    a = A.Sampler(spec, chains=CHAINS, seed=SEED)
    b = A.Sampler(spec, chains=CHAINS, seed=SEED)
    for s in (a, b):
        s.burn(BURN)

    def stored():
        a.sample_async(STEPS)
        a.sync()
        return a.launch_info()

    def folded():
        b.summarize(STEPS)
        return b.launch_info()

    calls = {"a": stored, "b": folded}
    ms, launches = {"a": [], "b": []}, {}
    for k in ("a", "b"):
        calls[k]()      # warm-up, untimed
    for _ in range(TIMINGS):
        for k in ("a", "b"):
            li = calls[k]()
            ms[k].append(li["kernel_ms"])
            launches[k] = li["n_launches"]
    info = b.summary_info()
    kernel = a.launch_info()["kernel"]
    a.close()
    b.close()
    res = {"shape": {"model": "normal", "n_obs": N_OBS, "chains": CHAINS, "steps": STEPS, "thin": 1, "recorded_values": 2}, "library": version,
           "kernel_id": version.split("kernels ")[-1], "kernel": kernel,
           "a_stored": dict(summary(ms["a"]), launches=launches["a"], what="sample_async + sync: %d kept draws stored on the device" % STEPS),
           "b_summarize": dict(summary(ms["b"]), launches=launches["b"], what="summarize: the kept draws folded into per-chain accumulators, default window"),
           "summary_info": info}
    sa, sb = res["a_stored"], res["b_summarize"]
    res["b_over_a"] = sb["median_ms"] / sa["median_ms"]
    for k in ("a_stored", "b_summarize"):
        r = res[k]
        print("(%s) %.3f ms [%.3f - %.3f] in %d launches  %s" % (k[0], r["median_ms"], r["min_ms"], r["max_ms"], r["launches"], r["what"]), flush=True)
    print("kernel id %s; (b) / (a) = %.4f; summary_info %s" % (res["kernel_id"], res["b_over_a"], info))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
    print("wrote", args.json)


if __name__ == "__main__":
    main()
