"""Development tool (GPU box; not part of the test suite): what posterior histograms cost (csrc/amwg_histogram.hip), the Normal family, N = 10^4 observations:
  (a) cfg2's shape, 65 536 chains, 1 000 steps: summarize with 256 uniform bins armed (set_histogram) against summarize without.  Two samplers of the same seed,
      burnt in alike; one untimed warm-up call each, then the two alternate in this one process, five timings each.  The time is launch_info()'s kernel_ms: HIP
      events around everything the call enqueued, the folds and the histogram kernels included.
  (b) the stored path, a dataset sampler of 256 datasets x 256 chains x 1 000 kept draws: dataset_histogram at 256 and at 4 096 bins beside dataset_quantiles at
      three probabilities on the same draws; host clock around the call (which ends in a stream synchronise), one warm-up and nine timings each, alternating.
  (c) the contended case on the draws of (b): 256 bins placed so that every dataset's draws fall into <= 4 of them, against 256 bins spread over the draws' range.
Median [min - max] in milliseconds, and the kernel id of the library.
    python tools/histogram_cost.py [--json profiles/histogram_cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
except Exception:
    pass
import amwg_ctypes as A  # noqa: E402
import model_spec  # noqa: E402

N_OBS, CHAINS, DATASETS, BURN, STEPS, SEED = 10000, 65536, 256, 300, 1000, 20261019
PROBS = [0.025, 0.5, 0.975]


def spec_of(d):
    return model_spec.build_spec("normal", model_spec.make_data("normal", N_OBS, 3000 + d))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "timings": len(ms), "all_ms": ms}


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def alternate(calls, timings, value):
    ms = {k: [] for k in calls}
    for k in calls:
        calls[k]()      # warm-up, untimed
    for _ in range(timings):
        for k in calls:
            ms[k].append(value(calls[k]))
    return {k: summary(v) for k, v in ms.items()}


def show(tag, r, what):
    print("(%s) %.3f ms [%.3f - %.3f]  %s" % (tag, r["median_ms"], r["min_ms"], r["max_ms"], what), flush=True)


def part_a():
    spec = spec_of(0)
    plain = A.Sampler(spec, chains=CHAINS, seed=SEED)
    armed = A.Sampler(spec, chains=CHAINS, seed=SEED)
    for s in (plain, armed):
        s.burn(BURN)
    armed.sample_async(50)      # a pilot places the edges: the pilot's range widened by its own width on either side
    armed.sync()
    plain.sample_async(50)
    plain.sync()
    q = armed.quantiles([0.0, 1.0])
    edges = np.array([np.linspace(lo - (hi - lo), hi + (hi - lo), 257) for lo, hi in q])
    armed.set_histogram(edges)

    def run(s):
        s.summarize(STEPS)
        return s.launch_info()["kernel_ms"]

    res = alternate({"unarmed": lambda: run(plain), "armed": lambda: run(armed)}, 5, lambda call: call())
    counts = armed.dataset_histogram()
    res["armed"]["what"] = "summarize, 256 uniform bins armed: every 64 MiB window is read once more by the histogram kernel"
    res["unarmed"]["what"] = "summarize without a histogram"
    res["armed_minus_unarmed_ms"] = res["armed"]["median_ms"] - res["unarmed"]["median_ms"]
    res["fits_in_unarmed_spread"] = res["armed_minus_unarmed_ms"] <= res["unarmed"]["spread_ms"]
    res["histogram_info"], res["summary_info"] = armed.histogram_info(), armed.summary_info()
    res["counted"], res["outside_the_edges"] = int(counts.sum()), int(counts[:, :, 256:].sum())
    res["shape"] = {"model": "normal", "n_obs": N_OBS, "chains": CHAINS, "steps": STEPS, "thin": 1, "recorded_values": 2, "bins": 256}
    plain.close()
    armed.close()
    for k in ("unarmed", "armed"):
        show("a " + k, res[k], res[k]["what"])
    print("(a) armed - unarmed = %.3f ms; unarmed spread %.3f ms; fits: %s" % (res["armed_minus_unarmed_ms"], res["unarmed"]["spread_ms"], res["fits_in_unarmed_spread"]), flush=True)
    return res


def part_bc():
    s = A.Sampler([spec_of(d) for d in range(DATASETS)], chains=CHAINS, seed=SEED, lanes_per_chain=1, block_threads=256)
    s.burn(BURN)
    s.sample_async(STEPS)      # the draws stay in the library's device buffer: the summaries read them there
    s.sync()
    q = s.dataset_quantiles([0.0, 1.0])      # [D][PR][2]
    lo, hi = q[:, :, 0].min(axis=0), q[:, :, 1].max(axis=0)
    spread = {bins: np.array([np.linspace(lo[p] - 1e-9, hi[p] + 1e-9, bins + 1) for p in range(s.PR)]) for bins in (256, 4096)}
    # every dataset's draws in <= 4 bins: bins as wide as the widest dataset's range, so that a range straddles at most two; the rest of the 256 bins lie beyond
    width = (q[:, :, 1] - q[:, :, 0]).max(axis=0)
    few = np.array([lo[p] - 1e-9 + width[p] * np.arange(257) for p in range(s.PR)])
    calls = {"hist_256": lambda: s.dataset_histogram(spread[256]), "hist_4096": lambda: s.dataset_histogram(spread[4096]), "quantiles_3": lambda: s.dataset_quantiles(PROBS),
             "hist_256_few_bins": lambda: s.dataset_histogram(few)}
    res = alternate(calls, 9, clocked)
    c_few, c_spread = s.dataset_histogram(few), s.dataset_histogram(spread[256])
    res["bins_hit_per_cell_few"] = int(np.count_nonzero(c_few[:, :, :256], axis=2).max())
    res["bins_hit_per_cell_spread"] = int(np.count_nonzero(c_spread[:, :, :256], axis=2).max())
    assert int(c_few.sum()) == int(c_spread.sum()) == DATASETS * s.PR * STEPS * (CHAINS // DATASETS) and res["bins_hit_per_cell_few"] <= 4
    res["shape"] = {"model": "normal", "n_obs": N_OBS, "datasets": DATASETS, "chains_per_dataset": CHAINS // DATASETS, "kept_draws": STEPS, "recorded_values": 2, "probs": PROBS}
    res["reference_point_ms"] = 7.39      # profiles/dataset_quantiles.json: dataset_quantiles at three probabilities on this shape, another build
    s.close()
    what = {"hist_256": "dataset_histogram, 256 bins over the draws' range", "hist_4096": "dataset_histogram, 4 096 bins over the draws' range",
            "quantiles_3": "dataset_quantiles at three probabilities (radix select) on the same draws",
            "hist_256_few_bins": "dataset_histogram, 256 bins of which every dataset's draws reach <= %d (contended: most lanes of a wave name one counter)" % res["bins_hit_per_cell_few"]}
    for k in calls:
        res[k]["what"] = what[k]
        show(("c " if k.endswith("few_bins") else "b ") + k, res[k], what[k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "histogram_cost.json"))
    args = ap.parse_args()
    version = A.lib().amwg_version().decode()
    res = {"library": version, "kernel_id": version.split("kernels ")[-1], "a_summarize": part_a(), "bc_stored": part_bc()}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
    print("kernel id %s; wrote %s" % (res["kernel_id"], args.json))


if __name__ == "__main__":
    main()
