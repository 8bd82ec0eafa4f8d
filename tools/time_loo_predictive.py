"""Development tool (GPU box; not part of the test suite): what PSIS-LOO predictive calibration per dataset costs on the device (csrc/amwg_loo_predictive.hip),
beside dataset_loo() and the in-sample dataset_predictive() of the same run, and beside the host.
  (a) a dataset sampler of 256 datasets x 256 chains (the Normal family, n_obs = 1 000) holding 1 000 kept draws on the device: dataset_predictive(loo=True),
      dataset_loo() and dataset_predictive().  One further run of the same kernels over the fetched draws through the test library (amwg_loo_predictive_check) with
      the phase timing switched on (events around the phases: they add synchronisation, so this run is not among the timings): select, compaction, sort + fit + weight.
  (b) the route open without the call: fetch_draws() (timed whole), then per dataset the S x n terms, the weight rule of tests/loo_predictive_reference.py and the
      weighted means in numpy, timed on the first HOST_DATASETS datasets and scaled by datasets / HOST_DATASETS -- recorded as an EXTRAPOLATION.  Its values are
      compared with (a)'s before anything is reported.
Host clock around each call -- each ends in a stream synchronise --, one untimed warm-up, five timings.  Median [min - max] in milliseconds.
    python tools/time_loo_predictive.py [--json profiles/loo_predictive.json] [--small]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402,F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process; erfc of the host route)
import amwg_ctypes as A  # noqa: E402
import loo_predictive_reference as lpr  # noqa: E402
import loo_reference as lr  # noqa: E402
from time_loo import SEED, BURN, clocked, normal_spec, show, summary  # noqa: E402

HOST_DATASETS, HOST_OBS = 2, 50      # the host route's weights are timed on HOST_OBS observations of each of HOST_DATASETS datasets and scaled to all


def host_route(x, mu, sigma, obs):
    """pit, pred_mean, pred_sd of observations `obs` of one dataset in numpy: the terms, the reference's weights, the weighted means"""
    c, den = -0.5 * np.log(2 * np.pi) - np.log(sigma), 2 * sigma * sigma
    out = []
    for j in obs:
        w = np.asarray(lpr.weights(c - (x[j] - mu) ** 2 / den)[0], dtype=np.float64)
        F = 0.5 * torch.special.erfc(torch.from_numpy(-(x[j] - mu) / sigma * math.sqrt(0.5))).numpy()
        W, mean = w.sum(), (w * mu).sum() / w.sum()
        out.append([(w * F).sum() / W, mean, math.sqrt((w * (sigma * sigma + (mu - mean) ** 2)).sum() / W)])
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 8 datasets x 64 chains x 50 draws x 100 observations")
    a = ap.parse_args()
    D, cpd, kept, n_obs = (8, 64, 50, 100) if a.small else (256, 256, 1000, 1000)
    out = {"library": A.lib().amwg_version().decode(), "shape": {"datasets": D, "chains_per_dataset": cpd, "kept": kept, "n_obs": n_obs, "tail_length": lr.tail_len(cpd * kept)}, "results": {}}
    R = out["results"]
    specs = [normal_spec(n_obs, 500 + d) for d in range(D)]
    s = A.Sampler(specs, chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    calls = {"loo_predictive": lambda: s.dataset_predictive(loo=True), "loo": lambda: s.dataset_loo(), "predictive": lambda: s.dataset_predictive()}
    got = calls["loo_predictive"]()
    for tag, call in calls.items():
        call()      # warm-up
        R[tag] = summary([clocked(call) for _ in range(5)])
        show("a", R[tag], tag)
    out["ratios"] = {"loo_predictive_over_loo": R["loo_predictive"]["median_ms"] / R["loo"]["median_ms"],
                     "loo_predictive_over_loo_plus_predictive": R["loo_predictive"]["median_ms"] / (R["loo"]["median_ms"] + R["predictive"]["median_ms"])}
    R["high_k_observations"] = int(got["high"].sum())
    holder = {}
    R["fetch_draws"] = summary([clocked(lambda: holder.update(draws=s.fetch_draws()))])
    draws = holder["draws"]
    s.close()
    A.loo_stats(timing=True)
    A.loo_predictive_check(draws, specs, pointwise=False)
    passes, ms = A.loo_stats(timing=False)
    R["phases"] = {"select_passes_over_the_terms": passes, "select_ms": ms[1], "compaction_ms": ms[2], "sort_fit_weight_ms": ms[3]}
    print("(a) phases, timed apart: %s; ratios %s" % (R["phases"], out["ratios"]), flush=True)
    hd, obs = min(HOST_DATASETS, D), range(min(HOST_OBS, n_obs))
    t0 = time.perf_counter()
    host = [host_route(specs[d]["data"]["x"], draws[:, 0, d * cpd:(d + 1) * cpd].ravel(), draws[:, 1, d * cpd:(d + 1) * cpd].ravel(), obs) for d in range(hd)]
    numpy_ms = (time.perf_counter() - t0) * 1e3
    for d in range(hd):
        err = np.abs(host[d] - got["pointwise"][d][:len(obs), [0, 2, 3]]).max()
        assert err < 1e-6, "the device and the host route differ: %g" % err
    scaled = numpy_ms * (D / hd) * (n_obs / len(obs))
    R["numpy"] = {"datasets_timed": hd, "observations_timed_per_dataset": len(obs), "measured_ms": numpy_ms, "extrapolated_to_all_ms": scaled}
    out["ratios"]["host_route_extrapolated_over_device"] = (R["fetch_draws"]["median_ms"] + scaled) / R["loo_predictive"]["median_ms"]
    print("(b) fetch_draws %.1f ms; numpy on %d x %d observations %.1f ms, i.e. %.0f ms for all (EXTRAPOLATED): %.0f x the device"
          % (R["fetch_draws"]["median_ms"], hd, len(obs), numpy_ms, scaled, out["ratios"]["host_route_extrapolated_over_device"]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
