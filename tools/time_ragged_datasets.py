"""Development tool (GPU box; not part of the test suite): what datasets of unequal sizes in one sampler cost -- the Normal family, 256 datasets x 256
chains, one lane per chain, 256-thread workgroups.  Every row: one untimed warm-up launch, then nine launches of 100 steps, kernel_ms of amwg_launch_info
per launch, median [min - max] in milliseconds; the library's version string carries the kernel id.
  (a) no regression for equal sizes: the dataset sampler of DESIGN.md section 6 (b) (N = 10^4, through amwg_create_datasets) with THIS tree's library and
      with the parent commit's (--parent-tree: a checkout of the parent with its library built), each in a process of its own, alternating, two rounds.
      The bar: this tree's median inside the parent's own [min - max] of the same round.
  (b) what raggedness costs: sizes drawn once (fixed seed) log-uniformly from 10^2 to 10^4, in ascending, descending and shuffled order, beside an
      equal-size sampler at the mean size (the same sum of n); the three times and their ratio to the equal-size run.  No threshold.
  (b2) the same with 2048 datasets: more workgroups than the device holds at once, which is where the LDS of the largest dataset and the order show.
  (c) the job of (b) as 256 ordinary samplers x 256 chains launched side by side (burn_async on each, then sync), wall-clock around the joint launches.
    python tools/time_ragged_datasets.py --parent-tree ../parent [--json profiles/ragged_datasets.json]
    python tools/time_ragged_datasets.py --rehearse          # tiny shapes, host logic only as far as it goes without a device"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, CPD, STEPS, LAUNCHES, SEED = 256, 256, 100, 9, 20261018
N_EQUAL, N_LO, N_HI = 10000, 100, 10000


def load(tree):
    sys.path[:0] = [os.path.join(tree, "bayes.js_amd"), os.path.join(tree, "tests")]
    try:
        import torch  # noqa: F401  (before libamwg.so, as in tests/conftest.py: one HIP runtime per process)
    except Exception:
        pass
    import amwg_ctypes
    import model_spec
    return amwg_ctypes, model_spec


def ragged_sizes(n_datasets):
    import numpy as np
    rng = np.random.default_rng(SEED)
    return [int(round(v)) for v in np.exp(rng.uniform(np.log(N_LO), np.log(N_HI), n_datasets))]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms), "all_ms": ms}


def kernel_times(s):
    s.burn(STEPS)      # untimed: log_post(init), first staging, instruction cache
    out = []
    for _ in range(LAUNCHES):
        s.burn(STEPS)
        out.append(s.launch_info()["kernel_ms"])
    return out


def child_equal(tree, n_datasets, cpd, n_obs):
    """(a), one library: prints one JSON line"""
    A, model_spec = load(tree)
    specs = [model_spec.build_spec("normal", model_spec.make_data("normal", n_obs, 3000 + d)) for d in range(n_datasets)]
    s = A.Sampler(specs, chains=n_datasets * cpd, seed=SEED, lanes_per_chain=1, block_threads=256, steps_per_launch=STEPS)
    row = dict(summary(kernel_times(s)), kernel=s.launch_info()["kernel"], lds=s.launch_info().get("lds_bytes"), library=A.lib().amwg_version().decode())
    s.close()
    print("ROW " + json.dumps(row), flush=True)


def fmt(r):
    return "%.3f ms [%.3f - %.3f]" % (r["median_ms"], r["min_ms"], r["max_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ragged_datasets.json"))
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--child-equal", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--skip-c", action="store_true")
    args = ap.parse_args()
    n_datasets, cpd, n_equal = (4, 64, 300) if args.rehearse else (D, CPD, N_EQUAL)
    if args.child_equal:
        return child_equal(args.child_equal, n_datasets, cpd, n_equal)
    res = {"shape": {"model": "normal", "datasets": n_datasets, "chains_per_dataset": cpd, "steps_per_launch": STEPS, "launches": LAUNCHES, "lanes_per_chain": 1, "block_threads": 256},
           "command": "python tools/time_ragged_datasets.py --parent-tree <a checkout of the parent commit, its library built>"}

    # (a) alternating processes: parent, this tree, parent, this tree
    res["a_equal_sizes"] = []
    trees = ([("parent", os.path.abspath(args.parent_tree))] if args.parent_tree else []) + [("this", ROOT)]
    for rnd in range(2):
        for label, tree in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--child-equal", tree] + (["--rehearse"] if args.rehearse else [])
            env = dict(os.environ)
            env.pop("AMWG_LIB", None)
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
            if p.returncode != 0 or not rows:
                raise SystemExit("(a) %s failed (exit %d):\n%s\n%s" % (label, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            row = dict(json.loads(rows[0]), tree=label, round=rnd, n_obs=n_equal, what="dataset sampler, equal sizes, amwg_create_datasets, kernel_ms")
            res["a_equal_sizes"].append(row)
            print("(a) round %d %-6s %s  %s" % (rnd, label, fmt(row), row["library"]), flush=True)
    for rnd in range(2):
        rows = {r["tree"]: r for r in res["a_equal_sizes"] if r["round"] == rnd}
        if "parent" in rows:
            inside = rows["parent"]["min_ms"] <= rows["this"]["median_ms"] <= rows["parent"]["max_ms"]
            res.setdefault("a_verdict", []).append({"round": rnd, "this_median_inside_parents_min_max": inside})
            print("(a) round %d: this tree's median %s the parent's [min - max]" % (rnd, "inside" if inside else "OUTSIDE"), flush=True)

    # (b) the ragged sampler in three orders, beside an equal-size sampler at the mean size; (b2) the same with eight times the datasets, so that the launch has
    # more workgroups than the device holds at once -- at (b)'s shape every dataset is ONE workgroup and an MI355X has 256 CUs: all of them are resident from the
    # start, the launch lasts as long as the largest dataset's workgroup and the order cannot matter
    A, model_spec = load(ROOT)
    import numpy as np
    geometry = dict(lanes_per_chain=1, block_threads=256, steps_per_launch=STEPS)

    def ragged_rows(tag, sizes):
        mean_n = -(-sum(sizes) // len(sizes))
        res[tag + "_sizes"] = {"datasets": len(sizes), "sum": sum(sizes), "min": min(sizes), "max": max(sizes), "mean_rounded_up": mean_n, "all": sizes}
        specs = [model_spec.build_spec("normal", model_spec.make_data("normal", n, 5000 + d)) for d, n in enumerate(sizes)]
        by_size = sorted(range(len(sizes)), key=lambda d: (sizes[d], d))
        shuffled = [int(v) for v in np.random.default_rng(SEED + 1).permutation(len(sizes))]
        eq_specs = [model_spec.build_spec("normal", model_spec.make_data("normal", mean_n, 5000 + d)) for d in range(len(sizes))]
        s = A.Sampler(eq_specs, chains=len(sizes) * cpd, seed=SEED, **geometry)
        li = s.launch_info()
        res[tag + "_equal_at_mean"] = dict(summary(kernel_times(s)), kernel=li["kernel"], lds=li.get("lds_bytes"), grid=li.get("grid_blocks"), n_obs=mean_n, library=A.lib().amwg_version().decode())
        s.close()
        print("(%s) %d datasets, equal at mean size %d: %s" % (tag, len(sizes), mean_n, fmt(res[tag + "_equal_at_mean"])), flush=True)
        for name, order in (("ascending", by_size), ("descending", by_size[::-1]), ("shuffled", shuffled)):
            s = A.Sampler([specs[d] for d in order], chains=len(sizes) * cpd, seed=SEED, ragged=True, **geometry)
            li = s.launch_info()
            row = dict(summary(kernel_times(s)), kernel=li["kernel"], lds=li.get("lds_bytes"), grid=li.get("grid_blocks"))
            row["ratio_to_equal"] = row["median_ms"] / res[tag + "_equal_at_mean"]["median_ms"]
            res[tag + "_ragged_" + name] = row
            s.close()
            print("(%s) ragged %-10s %s  = %.3f x equal" % (tag, name, fmt(row), row["ratio_to_equal"]), flush=True)
        return specs

    sizes = ragged_sizes(n_datasets) if not args.rehearse else [5, 300, 64, 17]
    specs = ragged_rows("b", sizes)
    ragged_rows("b2", ragged_sizes(8 * n_datasets) if not args.rehearse else [5, 300, 64, 17, 9, 100, 33, 2])

    # (c) the same job as one ordinary sampler per dataset, launched side by side
    if not args.skip_c:
        many = [A.Sampler(specs[d], chains=cpd, seed=SEED, chain_offset=cpd * d, **geometry) for d in range(len(sizes))]      # (the datasets of (b))

        def joint():
            t0 = time.perf_counter()
            for q in many:
                q.burn_async(STEPS)
            for q in many:
                q.sync()
            return (time.perf_counter() - t0) * 1e3
        joint()
        res["c_one_sampler_per_dataset"] = dict(summary([joint() for _ in range(LAUNCHES)]), kernel=many[0].launch_info()["kernel"],
                                                what="%d ordinary samplers x %d chains launched side by side, wall-clock around the joint launches" % (len(sizes), cpd))
        for q in many:
            q.close()
        print("(c) %d samplers side by side: %s" % (len(sizes), fmt(res["c_one_sampler_per_dataset"])), flush=True)
    if not args.rehearse:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
