"""Development tool (GPU box; not part of the test suite): what PSIS-LOO per dataset costs on the device (csrc/amwg_loo.hip), beside WAIC and beside the host.
  (a) a dataset sampler of 256 datasets x 256 chains (the Normal family, n_obs = 1 000) holding 1 000 kept draws on the device (1.05 GB): dataset_loo(), and
      dataset_waic() in the same run.  One further run of the same kernels over the fetched draws through the test library (amwg_loo_check), with its phase timing switched on (events around the
      phases: they add synchronisation, so this run is not among the timings) says how many passes over the terms the select took and how the time divides: lppd (WAIC's kernels), select,
      compaction, sort + fit.
  (b) the route open without the call, in the same run: fetch_draws() (timed whole), then per dataset the S x n terms and the rule of tests/loo_reference.py in numpy
      fp64, timed on the first HOST_DATASETS datasets and scaled by datasets / HOST_DATASETS -- recorded as an EXTRAPOLATION beside what was measured.  Its values are
      compared with (a)'s before anything is reported.
  (c) one posterior over 4 096 chains x 1 000 kept draws at n_obs = 10 000 (4.1e10 evaluations a pass): dataset_loo() and dataset_waic().
Host clock around each call -- each ends in a stream synchronise --, one untimed warm-up, five timings of (a), three of (c), one of (b).  Median [min - max] in
milliseconds.
    python tools/time_loo.py [--json profiles/loo.json] [--small]"""
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
import loo_reference as lr  # noqa: E402
import model_spec  # noqa: E402

SEED, BURN = 20261021, 300
HOST_DATASETS = 2


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms}


def clocked(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def show(tag, r, what):
    print("(%s) %.3f ms [%.3f - %.3f]  %s" % (tag, r["median_ms"], r["min_ms"], r["max_ms"], what), flush=True)


def normal_spec(n_obs, seed):
    data = model_spec.make_data("normal", n_obs, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


def numpy_loo(x, mu, sigma):
    """elpd_loo_i, khat_i of one dataset from its draws in numpy fp64 (np.log for the terms: the route a user would write; the rule as tests/loo_reference.py states it)"""
    c = -0.5 * np.log(2 * np.pi) - np.log(sigma)
    den = 2 * sigma * sigma
    t = x[None, :] - mu[:, None]
    ll = c[:, None] - t * t / den[:, None]
    return lr.pointwise(ll, np.float64)


def phases(draws, specs):
    """the phase timing lives in the test library: the same kernels over the fetched draws (amwg_loo_check), with events around the phases"""
    A.loo_stats(timing=True)
    A.loo_check(draws, specs, pointwise=False)
    passes, ms = A.loo_stats(timing=False)
    return {"select_passes_over_the_terms": passes, "lppd_ms": ms[0], "select_ms": ms[1], "compaction_ms": ms[2], "sort_and_fit_ms": ms[3]}


def measure(s, R, tag, timings, what):
    s.dataset_loo()      # warm-up
    s.dataset_waic()
    R[tag + "_dataset_loo"] = summary([clocked(lambda: s.dataset_loo()) for _ in range(timings)])
    R[tag + "_dataset_waic"] = summary([clocked(lambda: s.dataset_waic()) for _ in range(timings)])
    R[tag + "_loo_over_waic"] = R[tag + "_dataset_loo"]["median_ms"] / R[tag + "_dataset_waic"]["median_ms"]
    show(tag, R[tag + "_dataset_loo"], "dataset_loo(), " + what)
    show(tag, R[tag + "_dataset_waic"], "dataset_waic(), the same draws: LOO costs %.2f WAIC calls" % R[tag + "_loo_over_waic"])


def show_phases(R, tag, draws, specs):
    p = R[tag + "_phases"] = phases(draws, specs)
    print("(%s) phases, timed apart: %d select passes over the terms; lppd %.1f ms, select %.1f ms, compaction %.1f ms, sort + fit %.1f ms"
          % (tag, p["select_passes_over_the_terms"], p["lppd_ms"], p["select_ms"], p["compaction_ms"], p["sort_and_fit_ms"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 8 datasets x 64 chains x 50 draws x 100 observations")
    a = ap.parse_args()
    D, cpd, kept, n_obs, flag_chains, flag_n = (8, 64, 50, 100, 256, 1000) if a.small else (256, 256, 1000, 1000, 4096, 10000)
    out = {"library": A.lib().amwg_version().decode(), "shape_a": {"datasets": D, "chains_per_dataset": cpd, "kept": kept, "n_obs": n_obs, "tail_length": lr.tail_len(cpd * kept)},
           "shape_c": {"chains": flag_chains, "kept": kept, "n_obs": flag_n, "tail_length": lr.tail_len(flag_chains * kept)}, "results": {}}
    R = out["results"]

    specs = [normal_spec(n_obs, 500 + d) for d in range(D)]
    s = A.Sampler(specs, chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    got = s.dataset_loo(pointwise=True)
    measure(s, R, "a", 5, "%d datasets x %d chains x %d draws x %d observations (a tail of %d + 1 terms per observation)" % (D, cpd, kept, n_obs, lr.tail_len(cpd * kept)))
    R["a_high_k_observations"] = int(got["high"].sum())
    holder = {}
    R["b_fetch_draws"] = summary([clocked(lambda: holder.update(draws=s.fetch_draws()))])
    draws = holder["draws"]
    show_phases(R, "a", draws, specs)
    hd = min(HOST_DATASETS, D)
    t0 = time.perf_counter()
    host = [numpy_loo(specs[d]["data"]["x"], draws[:, 0, d * cpd:(d + 1) * cpd].ravel(), draws[:, 1, d * cpd:(d + 1) * cpd].ravel()) for d in range(hd)]
    numpy_ms = (time.perf_counter() - t0) * 1e3
    for d in range(hd):
        fit = np.isfinite(host[d][1])
        err = np.abs(host[d][0] - got["pointwise"][d][:n_obs, 0]).max()
        errk = np.abs(host[d][1][fit] - got["pointwise"][d][:n_obs, 2][fit]).max() if fit.any() else 0.0
        assert err < 1e-6 and errk < 1e-6, "the device and the host route differ: elpd_loo_i %g, khat %g" % (err, errk)
    R["b_numpy"] = {"datasets_timed": hd, "measured_ms": numpy_ms, "extrapolated_to_all_datasets_ms": numpy_ms * D / hd}
    R["b_host_route_ms_extrapolated"] = R["b_fetch_draws"]["median_ms"] + R["b_numpy"]["extrapolated_to_all_datasets_ms"]
    print("(b) fetch_draws %.1f ms; numpy on %d of %d datasets %.1f ms, i.e. %.0f ms for all (EXTRAPOLATED): host route %.0f ms, %.0f x the device" %
          (R["b_fetch_draws"]["median_ms"], hd, D, numpy_ms, R["b_numpy"]["extrapolated_to_all_datasets_ms"], R["b_host_route_ms_extrapolated"],
           R["b_host_route_ms_extrapolated"] / R["a_dataset_loo"]["median_ms"]), flush=True)
    out["ratios"] = {"host_route_extrapolated_over_device": R["b_host_route_ms_extrapolated"] / R["a_dataset_loo"]["median_ms"]}
    s.close()
    del draws, holder

    flag_spec = normal_spec(flag_n, 500)
    f = A.Sampler(flag_spec, chains=flag_chains, seed=SEED)
    f.burn(BURN)
    f.sample_async(kept)
    f.sync()
    measure(f, R, "c", 3, "one posterior over %d chains x %d draws x %d observations (a tail of %d + 1 terms per observation)" % (flag_chains, kept, flag_n, lr.tail_len(flag_chains * kept)))
    show_phases(R, "c", f.fetch_draws(), [flag_spec])
    f.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
