"""Development tool (GPU box; not part of the test suite): what WAIC per dataset costs on the device (csrc/amwg_waic.hip) and beside what.
  (a) a dataset sampler of 256 datasets x 256 chains (the Normal family, n_obs = 1 000) holding 1 000 kept draws on the device (1.05 GB): dataset_waic().
  (b) the route open without the call, in the same run: fetch_draws() (timed whole), then per dataset S x n terms, exp and the two reductions in numpy.  At
      6.5e10 exponentials the numpy part takes minutes, so it is timed on the first HOST_DATASETS datasets and the figure for all of them is that time scaled by
      datasets / HOST_DATASETS -- recorded as an extrapolation, beside what was measured.  Its pairs are compared with (a)'s before anything is timed.
  (c) the flagship shape, one posterior over 65 536 chains x 1 000 kept draws at n_obs = 10 000 (6.6e11 evaluations): dataset_waic().  Fewer rows are used if the
      call exceeds a minute; the JSON says how many.  The host route is not run there.
Host clock around each call -- each ends in a stream synchronise --, one untimed warm-up, five timings of (a), three of (c), one of (b).  Median [min - max] in
milliseconds; evaluations per second; with the vector instructions per evaluation counted in the gfx950 disassembly of the draw loop (VALU_PER_EVAL below: `hipcc -S
--cuda-device-only` of amwg_waic.hip with the Makefile's flags, the instructions between the loop's label and its backward branch that start with v_), the fraction
of amwg_fp64_peak -- a ceiling in lane-operations per second -- those evaluations amount to.
    python tools/time_waic.py [--json profiles/waic.json] [--small]"""
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

SEED, BURN = 20261021, 300
HOST_DATASETS = 2
VALU_PER_EVAL = {"normal": 75}      # waic_partial_kernel<AMWG_MODEL_NORMAL>'s draw loop: 107 instructions, 75 vector (57 of them fp64), 4 LDS reads, no scratch access.  A STATIC
# count: the loop holds both forms of the quotient and exp's rare arguments behind exec-mask branches, so it is an upper bound on what issues per evaluation -- a
# fraction above 1 says exactly that


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


def numpy_pairs(x, mu, sigma, block=4096):
    """lppd_i, p_i of one dataset from its draws, in plain numpy (np.log / np.exp: the route a user would write), in blocks of draws to bound the memory"""
    S, n = mu.size, x.size
    c = -0.5 * np.log(2 * np.pi) - np.log(sigma)
    den = 2 * sigma * sigma
    m = np.full(n, -np.inf)
    total = np.zeros(n)
    for s0 in range(0, S, block):      # pass 1: the maximum and the sum of the terms
        t = x[None, :] - mu[s0:s0 + block, None]
        ll = c[s0:s0 + block, None] - t * t / den[s0:s0 + block, None]
        m = np.maximum(m, ll.max(axis=0))
        total += ll.sum(axis=0)
    mean = total / S
    se = np.zeros(n)
    ss = np.zeros(n)
    for s0 in range(0, S, block):      # pass 2: sum exp(l - m) and sum (l - mean)^2
        t = x[None, :] - mu[s0:s0 + block, None]
        ll = c[s0:s0 + block, None] - t * t / den[s0:s0 + block, None]
        se += np.exp(ll - m[None, :]).sum(axis=0)
        ss += ((ll - mean[None, :]) ** 2).sum(axis=0)
    return np.stack([m + np.log(se) - np.log(S), ss / (S - 1)], axis=1)


def rate(evals, r, peak):
    per_s = evals / (r["median_ms"] * 1e-3)
    return {"evaluations": evals, "evaluations_per_s": per_s, "valu_per_evaluation": VALU_PER_EVAL["normal"], "fp64_peak_lane_ops_per_s": peak,
            "fraction_of_fp64_peak": per_s * VALU_PER_EVAL["normal"] / peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 8 datasets x 64 chains x 50 draws x 100 observations")
    a = ap.parse_args()
    D, cpd, kept, n_obs, flag_chains, flag_n = (8, 64, 50, 100, 1024, 1000) if a.small else (256, 256, 1000, 1000, 65536, 10000)
    peak = A.fp64_peak()
    out = {"library": A.lib().amwg_version().decode(), "shape_a": {"datasets": D, "chains_per_dataset": cpd, "kept": kept, "n_obs": n_obs}, "results": {}}
    R = out["results"]

    specs = [normal_spec(n_obs, 500 + d) for d in range(D)]
    s = A.Sampler(specs, chains=D * cpd, seed=SEED)
    s.burn(BURN)
    s.sample_async(kept)
    s.sync()
    got = s.dataset_waic(pointwise=True)      # warm-up, and what the host route is compared with
    R["a_dataset_waic"] = summary([clocked(lambda: s.dataset_waic()) for _ in range(5)])
    R["a_dataset_waic"].update(rate(D * cpd * kept * n_obs, R["a_dataset_waic"], peak))
    show("a", R["a_dataset_waic"], "dataset_waic(), %d datasets x %d chains x %d draws x %d observations: %.3g evaluations/s, %.1f %% of the fp64 ceiling" %
         (D, cpd, kept, n_obs, R["a_dataset_waic"]["evaluations_per_s"], 100 * R["a_dataset_waic"]["fraction_of_fp64_peak"]))
    holder = {}
    R["b_fetch_draws"] = summary([clocked(lambda: holder.update(draws=s.fetch_draws()))])
    draws = holder["draws"]

    def host(d):
        return numpy_pairs(specs[d]["data"]["x"], draws[:, 0, d * cpd:(d + 1) * cpd].ravel(), draws[:, 1, d * cpd:(d + 1) * cpd].ravel())
    hd = min(HOST_DATASETS, D)
    t0 = time.perf_counter()
    pairs = [host(d) for d in range(hd)]
    numpy_ms = (time.perf_counter() - t0) * 1e3
    for d in range(hd):
        err = np.abs(pairs[d] - got["pointwise"][d][:n_obs]).max()
        assert err < 1e-8, "the device and the host route differ: %g" % err
    R["b_numpy"] = {"datasets_timed": hd, "measured_ms": numpy_ms, "extrapolated_to_all_datasets_ms": numpy_ms * D / hd}
    R["b_host_route_ms_extrapolated"] = R["b_fetch_draws"]["median_ms"] + R["b_numpy"]["extrapolated_to_all_datasets_ms"]
    print("(b) fetch_draws %.1f ms; numpy on %d of %d datasets %.1f ms, i.e. %.0f ms for all (extrapolated): host route %.0f ms" %
          (R["b_fetch_draws"]["median_ms"], hd, D, numpy_ms, R["b_numpy"]["extrapolated_to_all_datasets_ms"], R["b_host_route_ms_extrapolated"]), flush=True)
    out["ratios"] = {"host_route_extrapolated_over_device": R["b_host_route_ms_extrapolated"] / R["a_dataset_waic"]["median_ms"],
                     "fetch_draws_alone_over_device": R["b_fetch_draws"]["median_ms"] / R["a_dataset_waic"]["median_ms"]}
    s.close()
    del draws, holder

    f = A.Sampler(normal_spec(flag_n, 500), chains=flag_chains, seed=SEED)
    f.burn(BURN)
    rows = kept
    while True:
        f.sample_async(rows)
        f.sync()
        first = clocked(lambda: f.dataset_waic())      # warm-up
        if first < 60e3 or rows <= 10:
            break
        rows //= 4
    R["c_flagship"] = summary([clocked(lambda: f.dataset_waic()) for _ in range(3)])
    R["c_flagship"].update(rate(flag_chains * rows * flag_n, R["c_flagship"], peak))
    R["c_flagship"]["rows"] = rows
    show("c", R["c_flagship"], "dataset_waic(), one posterior over %d chains x %d draws x %d observations: %.3g evaluations/s, %.1f %% of the fp64 ceiling" %
         (flag_chains, rows, flag_n, R["c_flagship"]["evaluations_per_s"], 100 * R["c_flagship"]["fraction_of_fp64_peak"]))
    f.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
