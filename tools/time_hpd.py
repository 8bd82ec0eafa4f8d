"""Development tool (GPU box; not part of the test suite): what the highest-density intervals cost on the device (csrc/amwg_hpd.hip) and beside what.
  (a) a dataset sampler of 256 datasets x 256 chains (the Normal family) holding 1 000 kept draws on the device (1.05 GB): dataset_hpd([0.95]) and
      dataset_hpd([0.5, 0.9, 0.95]).
  (b) the same sampler through dataset_quantiles at three probabilities (the radix select alone: what the thresholds of (a) are made of).
  (c) the route open without the call: fetch_draws() and, per dataset and value, a numpy sort and the rule on the host, at [0.95].  Its result is compared
      with (a)'s as bytes before anything is timed.
  (d) the flagship shape, one posterior over 65 536 chains x 1 000 kept draws (D = 1: one workgroup per value does the select, and the tails go through global passes),
      at [0.95].
Host clock around each call -- every one of them ends in a stream synchronise or on the host --, one untimed warm-up, then (a) and (b) alternate seven times,
(d) is timed five times, (c) twice (it takes seconds).  Median [min - max] in milliseconds, the ratios (c) / (a) and (a) / (b), and the kernel id of the library.
    python tools/time_hpd.py [--json profiles/hpd.json] [--small]"""
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
import hpd_reference as hr  # noqa: E402
import model_spec  # noqa: E402

SEED, BURN, N_OBS = 20261020, 300, 100


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms}


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def alternate(calls, timings):
    ms = {k: [] for k in calls}
    for k in calls:
        calls[k]()      # warm-up, untimed
    for _ in range(timings):
        for k in calls:
            ms[k].append(clocked(calls[k]))
    return {k: summary(v) for k, v in ms.items()}


def show(tag, r, what):
    print("(%s) %.3f ms [%.3f - %.3f]  %s" % (tag, r["median_ms"], r["min_ms"], r["max_ms"], what), flush=True)


def normal_spec(seed):
    data = model_spec.make_data("normal", N_OBS, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


def host_route(s, D, probs):
    return hr.of_array(s.fetch_draws(), D, probs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 8 datasets x 64 chains x 50 draws")
    a = ap.parse_args()
    D, cpd, kept, flag_chains = (8, 64, 50, 1024) if a.small else (256, 256, 1000, 65536)
    out = {"library": A.lib().amwg_version().decode(), "shape_a": {"datasets": D, "chains_per_dataset": cpd, "kept": kept, "values": 2}, "results": {}}
    R = out["results"]

    s = A.Sampler([normal_spec(500 + d) for d in range(D)], chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    one, three = [0.95], [0.5, 0.9, 0.95]
    got = s.dataset_hpd(one)
    want = host_route(s, D, one)
    assert hr.same_bytes(got, want), "the device and the host route differ"
    R.update(alternate({"a_hpd_1": lambda: s.dataset_hpd(one), "a_hpd_3": lambda: s.dataset_hpd(three), "b_quantiles_3": lambda: s.dataset_quantiles(three)}, 7))
    show("a", R["a_hpd_1"], "dataset_hpd([0.95]), %d datasets x %d chains x %d draws" % (D, cpd, kept))
    show("a", R["a_hpd_3"], "dataset_hpd([0.5, 0.9, 0.95])")
    show("b", R["b_quantiles_3"], "dataset_quantiles at three probabilities")
    R["c_host_1"] = summary([clocked(lambda: host_route(s, D, one)) for _ in range(2)])
    show("c", R["c_host_1"], "fetch_draws + numpy sort + the rule per dataset and value on the host, [0.95]")
    s.close()

    f = A.Sampler(normal_spec(500), chains=flag_chains, seed=SEED)
    f.burn(BURN)
    f.sample_async(kept)
    f.sync()
    f.dataset_hpd(one)      # warm-up
    R["d_flagship_1"] = summary([clocked(lambda: f.dataset_hpd(one)) for _ in range(5)])
    R["d_flagship_quantiles_2"] = summary([clocked(lambda: f.dataset_quantiles([0.025, 0.975])) for _ in range(5)])
    show("d", R["d_flagship_1"], "dataset_hpd([0.95]), one posterior over %d chains x %d draws" % (flag_chains, kept))
    show("d", R["d_flagship_quantiles_2"], "dataset_quantiles([0.025, 0.975]) there")
    f.close()

    out["ratios"] = {"host_route_over_device_c_over_a": R["c_host_1"]["median_ms"] / R["a_hpd_1"]["median_ms"],
                     "hpd_3_over_quantiles_3_a_over_b": R["a_hpd_3"]["median_ms"] / R["b_quantiles_3"]["median_ms"],
                     "hpd_3_over_hpd_1": R["a_hpd_3"]["median_ms"] / R["a_hpd_1"]["median_ms"]}
    print("the host route takes %.1f times the device call; three intervals take %.2f times three quantiles" %
          (out["ratios"]["host_route_over_device_c_over_a"], out["ratios"]["hpd_3_over_quantiles_3_a_over_b"]))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
