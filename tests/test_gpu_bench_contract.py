"""-m gpu: bench.py's one JSON line carries what the driver's contract asks for (a short run: 5 steps, small chain count)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra, detail=False):
    """-> the ONE stdout line (parsed; its size is part of the contract: the round-4 record was lost to a 19 KB line), or with detail=True
    (line, the whole record bench.py writes beside it)"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        side = os.path.join(tmp, "bench_detail.json")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--min-seconds", "0.05", *extra],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, AMWG_BENCH_DETAIL=side))
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout.count("\n") == 1 and p.stdout.startswith("{"), p.stdout[-2000:]      # ONE line, nothing else on stdout
        assert len(p.stdout) <= 4096 < 8192, "the bench line is %d bytes" % len(p.stdout)
        assert not any(ln.startswith("{") for ln in p.stderr.splitlines())                      # (nothing on stderr can be taken for it either)
        line = json.loads(p.stdout)
        full = json.load(open(side))
    return (line, full) if detail else line


def test_default_line_has_the_contract_fields_and_an_honest_roofline():
    d, full = _bench("--full", "--chains-per-gpu", "4096", "--lanes", "1", detail=True)     # (one lane per chain, as the full-size default picks: reference order)
    for key, want in (("unit", "param-updates/s"), ("n_gpus", 1), ("steps", 5), ("warmup", 2), ("higher_is_better", True), ("scaling", "weak"),
                      ("vs_baseline", None), ("dtype", "f64"), ("data", "synthetic")):
        assert d[key] == want and full[key] == want, key
    assert "param-updates" in d["metric"] and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["workload"].startswith("BASELINE.json configs[1]") and "model" not in d["config"]
    assert d["config"]["chains_per_gpu"] == 4096 and d["config"]["lanes_per_chain"] == 1 and "rccl_ranks_seen" in full["config"]
    assert abs(d["value"] - 4096 * 5 * 2 / (d["ms_per_step"] * 5e-3)) < 1e-5 * d["value"]          # value = chains x K x P / time of the K steps (7 digits on the line)
    assert abs(d["value"] - full["value"]) < 1e-6 * full["value"]
    r = d["roofline"]
    assert r["bound"] == "fp64_valu" and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6
    assert "traffic" in r and r["kernel"].startswith("amwg_step_kernel_cert<NormalModel,1") and "certified" in r["kernel"]
    # the default decides from the certified pass (2 operations per observation); the kernel that evaluates the reference's expression in every update is
    # measured beside it and is slower
    assert full["roofline"]["lane_ops_per_obs"] == 2 and 0 < d["full_evaluation"]["frac"] < 1 and d["full_evaluation"]["value"] < d["value"]
    c5 = full["other_configs"]["cfg5"]
    assert c5["lanes_per_chain"] == 16 and c5["roofline"]["lane_ops_per_obs"] == 27 and c5["full_evaluation_value"] < c5["value"]
    # the same configs as PLAIN closures through translate.js + hiprtc, reported beside the families' values (round 6: certified row plan / Poisson tail): the reference's
    # order, and within a factor of the hand-written kernels
    import shutil
    if shutil.which("node"):
        for name, kernel in (("cfg4", "amwg_user_sweep_cert"), ("cfg5", "amwg_user_step_cert")):
            tc = full["other_configs"][name]["translated_closure"]
            assert tc.get("kernel") == kernel and tc["summation_order"] == 1, tc
            assert 0.5 * full["other_configs"][name]["value"] < tc["value"] < 1.5 * full["other_configs"][name]["value"], tc
            assert d["other_configs"][name]["translated_closure_value"] == pytest.approx(tc["value"], rel=1e-3)
    assert r["effective_hbm"]["lds_resident"] is True and r["effective_hbm"]["unit"] == "GB/s"
    assert d["parity"]["draws_bit_identical"] and d["parity"]["accept_counts_identical"] and d["parity"]["final_state_bit_identical"]
    assert d["detail"].endswith("bench_detail.json")
    # the record beside the line
    assert full["timing"]["regions"] >= 3 and len(full["timing"]["region_ms"]) == min(64, full["timing"]["regions"])      # the first 64 regions are listed
    assert full["parity"]["from_timed_sampler"] is True and full["parity"]["chains_checked"] == [0, 65535]
    for name in ("cfg3", "cfg4", "cfg5", "cfg4_group_local"):          # the driver's record carries every north-star config
        o, q = full["other_configs"][name], d["other_configs"][name]
        assert "error" not in o, o
        assert o["value"] > 0 and o["parity"]["accept_counts_identical"] and o["parity"]["uniforms_consumed_identical"] and q["value"] > 0 and q["parity_ok"] is True
        if name == "cfg3":
            # value and frac describe the same kernel: the pass-free default against vector issue, priced with the committed PMC profile of THESE kernel sources
            # (frac is null, with the reason, while profiles/ holds none of this kernel id); the term-by-term pass beside it
            rr = o["roofline"]
            assert rr["bound"] == "valu_issue" and rr["kernel"].startswith("amwg_step_kernel<BetaBernModel,1,")
            assert (rr["frac"] is None and rr["profile_refused"]) or (0 < rr["frac"] < 1 and rr["valu_per_64_updates"] > 0)
            assert 0 < o["term_by_term_frac"] < 1 and q["term_by_term_value"] > 0
        else:
            assert 0 < o["roofline"]["frac"] < 1 and 0 < q["frac"] < 1
    assert full["other_configs"]["cfg3"]["parity"]["draws_bit_identical"] is True
    for name in ("cfg4", "cfg5"):      # round 5: the multi-lane defaults decide in the reference's own summation order -- the reference golden's chains, every bit
        pr = full["other_configs"][name]["parity"]
        assert pr["lanes_per_chain"] > 1 and pr["summation_order"] == 1 and pr["reference_order"] is True, pr
        assert pr["draws_bit_identical"] and pr["running_sums_bit_identical"] and pr["final_state_bit_identical"] and pr["log_post_bit_identical"], pr
    # cfg4: `value` and `frac` describe the SAME kernel (the sweep kernel against its one certified 2-operation pass per step); the price of strict reference order beside it
    c4 = full["other_configs"]["cfg4"]
    assert c4["roofline"]["kernel"].startswith("amwg_sweep_kernel_cert<") and c4["value_kernel"] == c4["roofline"]["kernel"]
    assert abs(c4["roofline"]["achieved"] - c4["value"] / 34 * 1 * 10000 * 2) < 1e-6 * c4["roofline"]["achieved"] and 0 < c4["full_evaluation_frac"] < 1
    assert d["other_configs"]["cfg4"]["kernel"].startswith("amwg_sweep_kernel")
    for name in ("cfg4", "cfg5"):
        ro = full["other_configs"][name]["reference_order"]
        assert "error" not in ro, ro
        assert ro["lanes_per_chain"] == 1 and 0 < ro["value"] and d["other_configs"][name]["reference_order_value"] > 0
    fr = full["parity"]["flip_rate"]
    assert ("refused" in fr) != ("flips_per_1e9" in fr)      # a campaign of other kernels is refused, not quoted
    # (cfg4's default is the sweep kernel since round 4 -- the reference's schedule; since it decides from certified sums (round 5: one 2-operation pass per step) the
    # opt-in group-local evaluation, two 8-operation passes per step, is BEHIND it: measured and reported, no longer a speed-up)
    assert 0.5 < full["other_configs"]["cfg4_group_local"]["speedup_over_cfg4"] < 1.0
    assert full["other_configs"]["cfg4"]["value"] > 2.5 * full["other_configs"]["cfg4"]["full_evaluation_value"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "param-updates/s" and c["sample"]
    assert c["kind"] == "reference" or c.get("reference_unavailable") is True


def test_plain_line_times_exactly_k_steps_once_and_dumps_the_same_outputs_every_run(tmp_path):
    """Without --full: one region of exactly --steps steps, the contract's fields and nothing measured beside them (no parity schedule, roofline, other
    configs or CPU baseline); --dump-outputs writes the last recorded draw of every chain, and two runs of the same arguments write the same bytes."""
    import numpy as np
    runs = []
    for i in range(2):
        out_dir = tmp_path / ("run%d" % i)
        d, full = _bench("--chains-per-gpu", "4096", "--dump-outputs", str(out_dir), detail=True)
        for key, want in (("unit", "param-updates/s"), ("n_gpus", 1), ("steps", 5), ("warmup", 2), ("higher_is_better", True), ("dtype", "f64")):
            assert d[key] == want, key
        assert "param-updates" in d["metric"] and d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] - 4096 * 5 * 2 / (d["ms_per_step"] * 5e-3)) < 1e-5 * d["value"]
        assert full["timing"]["regions"] == 1 and full["timing"]["steps_per_region"] == 5 and len(full["timing"]["region_ms"]) == 1
        assert abs(full["timing"]["region_ms"][0] - d["ms_per_step"] * 5) < 1e-5 * full["timing"]["region_ms"][0]
        for k in ("roofline", "parity", "other_configs", "cpu_baseline", "end_to_end_js", "sufficient_statistics", "posterior"):
            assert k not in full, k
        files = sorted(p.name for p in out_dir.iterdir())
        assert files == ["last_draws.npy"], files
        a = np.load(str(out_dir / "last_draws.npy"))
        assert a.dtype == np.float64 and a.shape == (2, 4096) and np.all(np.isfinite(a)) and np.all(a[1] > 0)      # (mu, sigma) of every chain; sigma > 0
        assert full["outputs"]["last_draws"]["shape"] == [2, 4096]
        runs.append(a)
    assert runs[0].tobytes() == runs[1].tobytes()


def test_gpus_n_without_a_launcher_never_leaves_without_a_line():
    """`python bench.py --gpus 2` with WORLD_SIZE unset (round-4 review: that was a SystemExit): the one-process multi-device path when two devices
    are visible, otherwise the "not measured" line -- rc 0 and one parseable line either way."""
    import torch
    env_keys = ("WORLD_SIZE", "RANK", "LOCAL_RANK")
    saved = {k: os.environ.pop(k) for k in env_keys if k in os.environ}
    try:
        d = _bench("--gpus", "2", "--chains-per-gpu", "2048", "--no-cpu-baseline")
    finally:
        os.environ.update(saved)
    assert d["n_gpus"] == 2 and d["inproc"] is True
    if torch.cuda.device_count() < 2:
        assert d["value"] is None and "not measured" in d["note"]
    else:
        assert d["value"] > 0 and d["config"]["rccl_ranks_seen"] == 2


@pytest.mark.parametrize("workload", ["cfg3", "cfg4"])
def test_other_workloads_report_a_roofline(workload):
    d = _bench("--full", "--workload", workload, "--no-cpu-baseline", "--chains-per-gpu", "2048")
    assert "cpu_baseline" not in d
    if workload == "cfg3":
        # value and roofline describe the same kernel: the pass-free default against vector issue (frac from the committed PMC profile of these kernel sources, or
        # null with the reason); the term-by-term pass beside it
        assert d["roofline"]["bound"] == "valu_issue" and d["roofline"]["kernel"].startswith("amwg_step_kernel<BetaBernModel,1,")
        assert (d["roofline"].get("frac") is None) or 0 < d["roofline"]["frac"] <= 1.0
        assert d["term_by_term"]["value"] > 0 and 0 < d["term_by_term"]["frac"] < 1
    else:
        assert d["roofline"]["bound"] == "fp64_valu" and d["roofline"]["frac"] > 0


def test_inproc_multi_device_path_runs_on_one_gpu_and_declines_more():
    """`--inproc`: the product's own multi-device path (one process, N samplers, amwg_group_moments) with the bench contract's fields; on a
    one-GPU box N = 1 is measured and N = 2 says so instead of inventing a number."""
    d, full = _bench("--inproc", "--workload", "cfg4", "--strong", "--chains-per-gpu", "512", detail=True)
    assert d["inproc"] is True and d["n_gpus"] == 1 and d["scaling"] == "strong" and d["value"] > 0 and d["config"]["chains_total"] == 16384
    assert d["config"]["rccl_ranks_seen"] == 1
    d = full
    assert len(d["posterior"]["mean"]) == 8 and all(abs(m) < 50 for m in d["posterior"]["mean"])
    import torch
    if torch.cuda.device_count() < 2:
        d2 = _bench("--inproc", "--gpus", "2")
        assert d2["value"] is None and "not measured" in d2["note"]


def test_two_ranks_under_the_launcher_on_one_visible_device_say_not_measured(tmp_path):
    """Round-5 review, item 7: `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2` -- the driver's scaling command -- on the one-GPU box: rc 0 on
    both ranks, ONE line from rank 0, value null, "not measured" (and with two devices visible: a measured line over the library's RCCL communicator)."""
    import torch
    from test_bench_host import run_bench_under_the_launcher
    line = run_bench_under_the_launcher(tmp_path, port=29641)
    assert line["n_gpus"] == 2
    if torch.cuda.device_count() < 2:
        assert line["value"] is None and "not measured" in line["note"]
    else:
        assert line["value"] > 0 and line["config"]["rccl_ranks_seen"] == 2


def test_two_real_processes_with_their_own_library_handles_share_the_one_gpu(tmp_path):
    """The N > 1 code path with REAL ranks (round-5 review: the gloo test on the CPU exercises shard offsets with the oracle standing in for the library): two processes
    started by torch.distributed.run, each with its own libamwg sampler on the one visible device (bench.py's development switches AMWG_BENCH_ONE_DEVICE = 1 +
    AMWG_BENCH_BACKEND = gloo: RCCL refuses two ranks on one device, so the gather of the recorded draws goes through torch.distributed), contiguous global chain ids,
    barrier + max-over-ranks timing, rank 0's line.  What it cannot show is xGMI traffic."""
    from test_bench_host import run_bench_under_the_launcher
    line = run_bench_under_the_launcher(tmp_path, port=29651, extra_env={"AMWG_BENCH_ONE_DEVICE": "1", "AMWG_BENCH_BACKEND": "gloo"},
                                        extra_args=["--chains-per-gpu", "2048", "--no-cpu-baseline", "--min-seconds", "0.05"])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["chains_total"] == 4096 and line["scaling"] == "weak"
    full = json.load(open(str(tmp_path / "d.json")))
    ranks = full["config"]["ranks"]
    assert len(ranks) == 2 and [r["chains"] for r in ranks] == [2048, 2048]
    assert abs(line["value"] - 4096 * 5 * 2 / (line["ms_per_step"] * 5e-3)) < 1e-5 * line["value"]
