"""Development tool (GPU box; not part of the test suite): what the certified Poisson / logistic tails buy a TRANSLATED closure on many datasets -- the logistic
closure (dst_logit) and the Poisson GLM closure (dst_pois_linear) of tests/js/dataset_tail_models.js at N = 1 000, 256 datasets x 256 chains, burn(1000), at the
geometry the planner gives each source (lanes_per_chain = 0, block_threads = 0).
  (a) translated by default: the one source carries the tail in its per-dataset form (kTailPerDataset), amwg_user_step_cert_ds where the planner takes 16 lanes;
  (b) translated with the caller's no_pois_tail / no_logit_tail: the expression in every update.  Its source is checked HERE, on the CPU, to be byte-identical to the
      translation of the same input under the options translate_datasets forced on every pass before it knew these tails (tests/js/translate_dataset_tails_cli.js,
      <tag>.forced.hip) -- so (b) is that earlier translate_datasets' workload, and (a) is never measured against itself;
  (a16) only when the planner did not give (a) 16 lanes per chain: (a)'s source at lanes_per_chain = 16, for the record.
The runs alternate in one process: one untimed warm-up each, then nine wall-clock timings each, median [min - max] in milliseconds, and updates/s from the median.
    python tools/time_user_dataset_tails.py [--json profiles/user_dataset_tails.json] [--workdir DIR]
    python tools/time_user_dataset_tails.py --rehearse          # tiny shapes"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, CPD, N_OBS, STEPS, REPS, SEED = 256, 256, 1000, 1000, 9, 20261018
CLOSURES = ("dst_logit", "dst_pois_linear")


def summary(ms, updates):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "timings": len(ms), "all_ms": ms, "updates_per_s": updates / (med * 1e-3)}


def fmt(r):
    return "%.1f ms [%.1f - %.1f]  %.3g updates/s" % (r["median_ms"], r["min_ms"], r["max_ms"], r["updates_per_s"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "user_dataset_tails.json"))
    ap.add_argument("--workdir", default="", help="keep / find the translations here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    n_datasets, cpd, n_obs, steps = (4, 64, 100, 20) if args.rehearse else (D, CPD, N_OBS, STEPS)
    sys.path[:0] = [os.path.join(ROOT, "bayes.js_amd"), os.path.join(ROOT, "tests")]
    try:
        import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
    except Exception:
        pass
    import amwg_ctypes as A
    import user_dataset_tails_lib as tl
    if args.workdir:
        tl.use_dir(args.workdir)
    res = {"shape": {"n_obs": n_obs, "datasets": n_datasets, "chains_per_dataset": cpd, "steps": steps, "timings": REPS},
           "command": "python tools/time_user_dataset_tails.py", "library": A.lib().amwg_version().decode(), "closures": {}}
    ok = True
    for name in CLOSURES:
        tag = tl.translate_sized(name, n_obs, n_datasets)
        src_a, meta_a, _ = tl.load(tag)
        src_b, meta_b, _ = tl.load(tag + ".notail")
        assert meta_a["tail_per_dataset"] and (meta_a["pois_tail_n"] or meta_a["logit_tail_n"]) == n_obs and "kTailPerDataset = true" in src_a, tag
        assert src_b == tl.forced_source(tag) and not meta_b["tail_per_dataset"] and "kTailPerDataset" not in src_b, tag + ": (b) is not the earlier translation"
        n_params = len(meta_a["init"])
        updates = float(n_datasets) * cpd * steps * n_params
        samplers = {"a_certified_tail": A.Sampler(tl.specs(tag), chains=n_datasets * cpd, seed=SEED),
                    "b_expression_every_update": A.Sampler(tl.specs(tag + ".notail"), chains=n_datasets * cpd, seed=SEED)}
        if samplers["a_certified_tail"].launch_info()["lanes_per_chain"] != 16:
            samplers["a16_certified_tail_at_16_lanes"] = A.Sampler(tl.specs(tag), chains=n_datasets * cpd, seed=SEED, lanes_per_chain=16)
        rec = {"launch": {k: s.launch_info() for k, s in samplers.items()}}
        times = {k: [] for k in samplers}
        for rep in range(REPS + 1):      # (the first round is the warm-up: log_post(init), first staging)
            for k, s in samplers.items():
                t = time.perf_counter()
                s.burn(steps)
                ms = (time.perf_counter() - t) * 1e3
                if rep:
                    times[k].append(ms)
        for k, s in samplers.items():
            rec[k] = summary(times[k], updates)
            li = rec["launch"][k]
            print("%-18s %-32s %-24s %3d lanes x %4d  %s" % (name, k, li["kernel"], li["lanes_per_chain"], li["block_threads"], fmt(rec[k])), flush=True)
            s.close()
        a, b = rec["a_certified_tail"], rec["b_expression_every_update"]
        rec["ratio_b_over_a"] = b["median_ms"] / a["median_ms"]
        rec["a_faster_and_ranges_apart"] = bool(a["median_ms"] < b["median_ms"] and a["max_ms"] < b["min_ms"])
        ok = ok and rec["a_faster_and_ranges_apart"]
        print("%-18s (b) / (a) = %.2f; (a) faster with the ranges apart: %s" % (name, rec["ratio_b_over_a"], rec["a_faster_and_ranges_apart"]), flush=True)
        res["closures"][name] = rec
    res["accepted"] = ok
    if not args.rehearse:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
