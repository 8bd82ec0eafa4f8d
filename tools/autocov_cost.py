"""Development tool (GPU box; not part of the test suite): what the autocovariance along the chains costs (csrc/amwg_autocov.hip).
  (a) summarize with the autocovariance armed (set_autocovariance) against summarize without: the flagship's shape (Normal, 65 536 chains x 2 values, K = 2, 1 000
      kept draws) at max_lag 8, 32 and 128, and a cfg5-like one (Poisson GLM, 8 192 chains, K = 8: the coefficients) at max_lag 32.  Two samplers of the same seed,
      burnt in alike; one untimed warm-up call each, then the two alternate in this one process, five timings each.  The time is launch_info()'s kernel_ms: HIP
      events around everything the call enqueued, the folds and the lag-sum and carry kernels included.  The unarmed call is the path the library had before and
      is the baseline; the difference is reported against its own spread.
  (b) the stored path over 1 000 kept draws of the flagship shape (1.05 GB) at max_lag 8, 32 and 128: dataset_autocovariance, host clock around the call (which
      ends in a stream synchronise), one warm-up and seven timings each, alternating.  The whole array is one window there, so the ring is never read: the times
      are the zeroing of the state, the lag-sum kernel (one pass over the array per tile of 8 lags), the carry and the finish.  The slope between two max_lag is
      the cost of a tile's pass; the bytes a tile reads are known, so its bytes per second stand beside it.
Median [min - max] in milliseconds, and the kernel id of the library.
    python tools/autocov_cost.py [--json profiles/autocov_cost.json]"""
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
# name -> (model, n_obs, chains, steps of a summarising call, the values, the max_lag measured)
SHAPES = {
    "flagship_K2": ("normal", 10000, 65536, 1000, [0, 1], [8, 32, 128]),
    "cfg5_like_K8": ("pois_glm", 2000, 8192, 200, list(range(8)), [32]),
}
STORED = {"flagship_K2": 1000}      # kept draws of the stored path
TILE = 8


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


def part_a(name, lag):
    model, n_obs, chains, steps, values, _ = SHAPES[name]
    spec = model_spec.build_spec(model, model_spec.make_data(model, n_obs, 3000))
    plain = A.Sampler(spec, chains=chains, seed=SEED)
    armed = A.Sampler(spec, chains=chains, seed=SEED)
    for s in (plain, armed):
        s.burn(BURN)
    armed.set_autocovariance(values, lag)

    def run(s):
        s.summarize(steps)
        return s.launch_info()["kernel_ms"]

    res = alternate({"unarmed": lambda: run(plain), "armed": lambda: run(armed)}, 5, lambda call: call())
    K, PR, tiles = len(values), armed.PR, lag // TILE + 1
    res["armed_minus_unarmed_ms"] = res["armed"]["median_ms"] - res["unarmed"]["median_ms"]
    res["fits_in_unarmed_spread"] = res["armed_minus_unarmed_ms"] <= res["unarmed"]["spread_ms"]
    res["armed_over_unarmed"] = res["armed"]["median_ms"] / res["unarmed"]["median_ms"]
    res["autocovariance_info"], res["summary_info"] = armed.autocovariance_info(), armed.summary_info()
    # per kept row and chain a tile loads x_t and the x entering it (tile 0: x_t alone); the second is a row the first tile read shortly before
    res["lag_kernel_load_bytes"] = steps * K * chains * 8 * (2 * tiles - 1)
    res["window_bytes_selected"] = steps * K * chains * 8
    acov, mean, between = armed.dataset_autocovariance()
    res["finite"] = bool((acov == acov).all())
    res["tau_of_value_0"] = A.autocorrelation_ess(acov[0, 0], between[0, 0], steps, chains)["tau"]
    res["shape"] = {"model": model, "n_obs": n_obs, "chains": chains, "steps": steps, "thin": 1, "recorded_values": PR, "K": K, "max_lag": lag, "lag_tiles": tiles}
    plain.close()
    armed.close()
    for k in ("unarmed", "armed"):
        show("a %s L=%d %s" % (name, lag, k), res[k], "summarize, autocovariance of %d values %s" % (K, k))
    print("(a %s L=%d) armed - unarmed = %.3f ms (x %.4f); unarmed spread %.3f ms; fits: %s" % (name, lag, res["armed_minus_unarmed_ms"], res["armed_over_unarmed"],
                                                                                          res["unarmed"]["spread_ms"], res["fits_in_unarmed_spread"]), flush=True)
    return res


def part_b(name):
    model, n_obs, chains, _, values, lags = SHAPES[name]
    kept = STORED[name]
    s = A.Sampler(model_spec.build_spec(model, model_spec.make_data(model, n_obs, 3000)), chains=chains, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)      # the draws stay in the library's device buffer: the kernels read them there
    s.sync()
    res = alternate({"L%d" % lag: (lambda lag=lag: s.dataset_autocovariance(values, lag)) for lag in lags}, 7, clocked)
    K = len(values)
    res["draw_bytes"] = kept * s.PR * chains * 8
    for lo, hi in zip(lags, lags[1:]):
        d_ms, d_tiles = res["L%d" % hi]["median_ms"] - res["L%d" % lo]["median_ms"], hi // TILE - lo // TILE
        res["ms_per_tile_L%d_to_L%d" % (lo, hi)] = d_ms / d_tiles
        res["tile_GBps_L%d_to_L%d" % (lo, hi)] = 2 * kept * K * chains * 8 / (d_ms / d_tiles) / 1e6 if d_ms > 0 else None
    res["shape"] = {"model": model, "n_obs": n_obs, "chains": chains, "kept_draws": kept, "recorded_values": s.PR, "K": K, "max_lags": lags}
    s.close()
    for lag in lags:
        show("b %s L=%d" % (name, lag), res["L%d" % lag], "dataset_autocovariance of %d values over %d bytes of draws" % (K, res["draw_bytes"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "autocov_cost.json"))
    args = ap.parse_args()
    version = A.lib().amwg_version().decode()
    res = {"library": version, "kernel_id": version.split("kernels ")[-1],
           "a_summarize": {"%s_L%d" % (k, lag): part_a(k, lag) for k in SHAPES for lag in SHAPES[k][5]}, "b_stored": {k: part_b(k) for k in STORED}}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
    print("kernel id %s; wrote %s" % (res["kernel_id"], args.json))


if __name__ == "__main__":
    main()
