"""Development tool (GPU box; not part of the test suite): what posterior covariance costs (csrc/amwg_covariance.hip).
  (a) summarize with the covariance armed (set_covariance) against summarize without, at three shapes: the flagship's (Normal, 65 536 chains x 2 values, K = 2), a
      cfg5-like one (Poisson GLM, 8 192 chains x 9 values, K = 8: the coefficients) and a hierarchical-sized one (hierarchical Normal of 64 groups, 2 048 chains,
      K = 66).  Two samplers of the same seed, burnt in alike; one untimed warm-up call each, then the two alternate in this one process, five timings each.  The time
      is launch_info()'s kernel_ms: HIP events around everything the call enqueued, the folds and the co-moment kernels included.  The unarmed call is the path the
      library had before the covariance and is the baseline.
  (b) the stored path over 1 000 kept draws at the first two shapes: dataset_covariance over K values against dataset_covariance over ONE value, host clock around
      the call (which ends in a stream synchronise), one warm-up and seven timings each, alternating.  K = 1 has no pair: it runs the memset, fold_window_kernel over
      the whole array and the finishing kernel; K values add the co-moment kernel over the same array.  So K = 1 times the fold and the difference times the
      co-moment kernel, each over bytes that are known: their bytes per second stand side by side, from the same run.
Median [min - max] in milliseconds, and the kernel id of the library.
    python tools/covariance_cost.py [--json profiles/covariance_cost.json]"""
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

SEED, BURN = 20261020, 200
# name -> (model, n_obs, G, chains, steps of a summarising call, the values of the covariance)
SHAPES = {
    "flagship_K2": ("normal", 10000, None, 65536, 1000, [0, 1]),
    "cfg5_like_K8": ("pois_glm", 2000, None, 8192, 200, list(range(8))),
    "hierarchical_K66": ("hier_normal", 2000, 64, 2048, 200, list(range(66))),
}
STORED = {"flagship_K2": 1000, "cfg5_like_K8": 1000}      # kept draws of the stored path


def spec_of(model, n_obs, G):
    data = model_spec.make_data(model, n_obs, 3000) if G is None else model_spec.make_data(model, n_obs, 3000, G=G)
    return model_spec.build_spec(model, data)


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


def part_a(name):
    model, n_obs, G, chains, steps, values = SHAPES[name]
    spec = spec_of(model, n_obs, G)
    plain = A.Sampler(spec, chains=chains, seed=SEED)
    armed = A.Sampler(spec, chains=chains, seed=SEED)
    for s in (plain, armed):
        s.burn(BURN)
    armed.set_covariance(values)

    def run(s):
        s.summarize(steps)
        return s.launch_info()["kernel_ms"]

    res = alternate({"unarmed": lambda: run(plain), "armed": lambda: run(armed)}, 5, lambda call: call())
    K, PR = len(values), armed.PR
    res["armed_minus_unarmed_ms"] = res["armed"]["median_ms"] - res["unarmed"]["median_ms"]
    res["fits_in_unarmed_spread"] = res["armed_minus_unarmed_ms"] <= res["unarmed"]["spread_ms"]
    res["armed_over_unarmed"] = res["armed"]["median_ms"] / res["unarmed"]["median_ms"]
    res["covariance_info"], res["summary_info"] = armed.covariance_info(), armed.summary_info()
    # what the co-moment kernels read of the windows: K <= 8 is one tile (every selected value once per row); beyond, tiles of four -- a tile once, a pair of tiles 8 values
    tiles = -(-K // 4)
    reads_per_row = K if K <= 8 else 4 * tiles + 8 * tiles * (tiles - 1) // 2
    res["comoment_window_bytes"] = steps * reads_per_row * chains * 8
    res["fold_window_bytes"] = steps * PR * chains * 8
    if res["armed_minus_unarmed_ms"] > 0:
        res["comoment_GBps_from_the_difference"] = res["comoment_window_bytes"] / res["armed_minus_unarmed_ms"] / 1e6
    cov = armed.dataset_covariance()
    res["finite"] = bool((cov == cov).all())
    res["shape"] = {"model": model, "n_obs": n_obs, "chains": chains, "steps": steps, "thin": 1, "recorded_values": PR, "K": K}
    plain.close()
    armed.close()
    for k in ("unarmed", "armed"):
        show("a %s %s" % (name, k), res[k], "summarize, covariance of %d values %s" % (K, k))
    print("(a %s) armed - unarmed = %.3f ms (x %.4f); unarmed spread %.3f ms; fits: %s" % (name, res["armed_minus_unarmed_ms"], res["armed_over_unarmed"], res["unarmed"]["spread_ms"],
                                                                                      res["fits_in_unarmed_spread"]), flush=True)
    return res


def part_b(name):
    model, n_obs, G, chains, _, values = SHAPES[name]
    kept = STORED[name]
    s = A.Sampler(spec_of(model, n_obs, G), chains=chains, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)      # the draws stay in the library's device buffer: the kernels read them there
    s.sync()
    res = alternate({"K1": lambda: s.dataset_covariance([0]), "K": lambda: s.dataset_covariance(values)}, 7, clocked)
    K, PR = len(values), s.PR
    fold_bytes, co_bytes = kept * PR * chains * 8, kept * K * chains * 8
    res["fold_bytes"], res["comoment_bytes"] = fold_bytes, co_bytes
    res["fold_GBps"] = fold_bytes / res["K1"]["median_ms"] / 1e6      # (an under-estimate: K = 1 also zeroes the scratch and finishes)
    diff = res["K"]["median_ms"] - res["K1"]["median_ms"]
    res["comoment_ms"] = diff
    res["comoment_GBps"] = co_bytes / diff / 1e6 if diff > 0 else None
    res["comoment_over_fold_GBps"] = res["comoment_GBps"] / res["fold_GBps"] if diff > 0 else None
    res["shape"] = {"model": model, "n_obs": n_obs, "chains": chains, "kept_draws": kept, "recorded_values": PR, "K": K}
    s.close()
    show("b %s K=1" % name, res["K1"], "dataset_covariance of one value: the fold over %d bytes" % fold_bytes)
    show("b %s K=%d" % (name, K), res["K"], "dataset_covariance of %d values: the fold and the co-moment kernel" % K)
    print("(b %s) fold %.1f GB/s; co-moment kernel %.3f ms, %s GB/s" % (name, res["fold_GBps"], diff, "%.1f" % res["comoment_GBps"] if diff > 0 else "n/a"), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "covariance_cost.json"))
    args = ap.parse_args()
    version = A.lib().amwg_version().decode()
    res = {"library": version, "kernel_id": version.split("kernels ")[-1], "a_summarize": {k: part_a(k) for k in SHAPES}, "b_stored": {k: part_b(k) for k in STORED}}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
    print("kernel id %s; wrote %s" % (res["kernel_id"], args.json))


if __name__ == "__main__":
    main()
