"""-m gpu: the VALUES the certified kernels decide from, audited in every kernel class and form and per dataset (tests/README.value_audit.md).

The certified kernels decide exp(prop - curr) > u from a cheap value A of log_post and a hand-derived bound eps on |A - E|, E the reference's expression.  The byte
comparisons of tests/test_gpu_geometry.py, test_gpu_pass_edges.py and test_gpu_ragged_datasets.py cannot see a value that is slightly off or a bound that is too small
by a factor: |A - E| is 1e-2 .. 1e-1 of eps, and a wrong verdict needs a uniform inside a ~1e-12-wide window.  The audit build (csrc/libamwg_audit.so, -DAMWG_AUDIT:
tools/bound_audit.py run_case) evaluates E beside A in EVERY update and records max |A - E| / eps, max |dA - dE| / eta and the verdicts that contradict exp(dE) > u.

  group A   every class and form of the family kernels: the Normal pass in the 256-, 512- and 1024-thread classes with partial wavefronts, with and without the wave
            scratch, sufficient statistics, the replica fallback, the Poisson and the hierarchical family, a closure's tail in the 512 / 1024 classes
  group B   the families' DATASET kernels, per dataset, on datasets whose constants differ 2^10-fold, in both orders; every dataset's audit rows must also be the
            bytes an ordinary sampler on that dataset records: a bound formed from a neighbour's constants shows there whatever slack the derivation leaves
  group C   adversarial uniforms (AMWG_AUDIT_ADVERSARIAL=1: every certified decision's uniform 1.5 eta outside the sliver): no wrong verdict at the derived
            bounds, and wrong verdicts once the bounds are shrunk 2^-20 -- the detector behind `wrong_verdicts == 0` fires

Every non-adversarial case asserts the kernel and geometry it ran, wrong_verdicts == 0, no NaN ratio, both ratios <= 0.5 (the bars of tests/test_gpu_bound_audit.py:
the derivations leave a factor of two), and that it audited: the Normal family at one lane audits EVERY in-bounds proposal, every other case and every dataset some.
The audit library is a second libamwg, so every group runs in one fresh child process (as tests/test_gpu_pass_blocks.py does); the tests assert per case."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_NODE = shutil.which("node") is not None
needs_node = pytest.mark.skipif(not HAVE_NODE, reason="node is not installed")
SEED, OFFSET, SPL, STEPS = 8, 3, 13, 300
NORMAL = "amwg_step_kernel_cert<NormalModel,1,%d>"
NORMAL_DS = "amwg_step_kernel_cert_ds<NormalModel,1,%d>"
POIS = "amwg_step_kernel_cert<PoisGlmModel,16,256>"
POIS_DS = "amwg_step_kernel_cert_ds<PoisGlmModel,16,256>"
HIER = "amwg_sweep_kernel_cert<HierNormalModel,256>"
REPLICA_CHAINS, REPLICA_STEPS = 8205, 24      # (tests/test_gpu_geometry.py test_replica_fallback_with_a_certified_tail_has_a_scratch_line_per_wavefront)

# ---- the child: builds each case from its descriptor, runs it through tools/bound_audit.py run_case, prints one record per case

_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import bound_audit as B      # (points the binding at libamwg_audit.so before it is imported)
import numpy as np
import amwg_ctypes as A
import model_spec

SEED, OFFSET, SPL = 8, 3, 13
GLM_BETA = [0.2, -0.1, 0.05, 0.1, -0.2, 0.15, 0.3]
INF = float("inf")
QUICK = {}


def shared(specs):
    # (the list constructors pass ONE params / init / options array for the whole sampler: the first spec's)
    return [specs[0]] + [dict(q, params=specs[0]["params"], P=specs[0]["P"], init=specs[0]["init"], comp_opts=specs[0]["comp_opts"]) for q in specs[1:]]


def closure_spec(name, params, init):
    import user_host
    src, arrays, meta = user_host.translated(name)
    opt = dict(model_spec.DEFAULT_OPT)
    return {"user": user_host.user_spec_part(src, arrays, meta), "P": len(init), "init": list(init), "comp_opts": [dict(opt) for _ in init], "params": params}, arrays


def build(d):
    kind = d["kind"]
    c = dict(name=d["name"], seed=SEED, chain_offset=OFFSET, steps_per_launch=SPL, schedule="geometry", steps=d.get("steps", 300), state=None,
             block=d.get("block", 0), chains=d.get("chains", 0), lanes=1)
    if kind == "quick":      # a case of tools/bound_audit.py --quick as it stands there
        if not QUICK:
            QUICK.update({q["name"]: q for q in B.cases(True)})
        return dict(QUICK[d["case"]])
    if kind == "normal":
        c["spec"] = model_spec.build_spec("normal", model_spec.make_data("normal", d["n"], 31))
        c["suff"] = d.get("suff", 0)
    elif kind == "pois":
        import oracle_lib
        c["spec"] = model_spec.build_spec("pois_glm", model_spec.make_data("pois_glm", d["n"], 123, exp=oracle_lib.lib().orc_exp))
        c["lanes"] = 16
    elif kind == "hier":
        dd = model_spec.make_data("hier_normal", d["n"], 20260925 + d["n"], G=d["G"])
        c["spec"] = model_spec.build_spec("hier_normal", {"x": dd["x"], "g": dd["g"], "G": d["G"]}, G=d["G"])
        c["lanes"] = 64
    elif kind == "closure":      # the closure of tests/test_gpu_geometry.py's tail cases: the Normal family's parameters on its own observations
        import user_host
        fam = model_spec.build_spec("normal", {"x": user_host.translated(d["closure"])[1][0]})
        c["spec"], _ = closure_spec(d["closure"], fam["params"], fam["init"])
    elif kind == "replica":      # theta of dim [300]: 64 chains' LDS state does not fit a workgroup (tests/test_gpu_geometry.py REPLICA_PARAMS)
        params = [{"type": "real", "len": 300, "top": 300, "multidim": 1, "lower": -INF, "upper": INF}, {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": -INF, "upper": INF},
                  {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": 0.0, "upper": INF}]
        c["spec"], _ = closure_spec("bench_replica_tail", params, [0.0] * 300 + [0.5, 0.5])
    elif kind == "ds_normal":      # ragged Normal datasets; `data`: per dataset "synth" or (mean, sd) of numpy draws
        specs, starts = [], []
        for j, n in enumerate(d["sizes"]):
            how = d.get("data", ["synth"] * len(d["sizes"]))[j]
            x = model_spec.make_data("normal", n, 900 + 11 * j)["x"] if how == "synth" else how[0] + how[1] * np.random.default_rng(40 + j).standard_normal(n)
            specs.append(model_spec.build_spec("normal", {"x": np.asarray(x, dtype=np.float64)}))
            starts.append(d["starts"][j] if d.get("starts") else specs[0]["init"])
        order = list(range(len(specs)))[::-1] if d["reverse"] else list(range(len(specs)))
        c.update(spec=shared([specs[j] for j in order]), ragged=True, datasets=len(specs), chains=d["cpd"] * len(specs), suff=d.get("suff", 0))
        if d.get("starts"):
            c["state"] = np.concatenate([np.repeat(np.asarray(starts[j], dtype=np.float64)[:, None], d["cpd"], axis=1) for j in order], axis=1)
        c["sizes"] = [d["sizes"][j] for j in order]
    elif kind == "ds_pois":      # Poisson datasets from the tool's glm_data, one (design scale, intercept) each; every dataset's chains start at ITS generating coefficients
        specs, starts, facts = [], [], []
        for j, n in enumerate(d["sizes"]):
            X, y = B.glm_data(n, np.random.default_rng(70 + j), d["intercepts"][j], scale=d["scales"][j])
            specs.append(B.pois_case("", X, y, 0, 0)["spec"])
            starts.append([d["intercepts"][j]] + GLM_BETA + [float(int(0.4 * min(d["sizes"])))])      # (cp inside every dataset and inside the shared bound, the first spec's)
            facts.append({"n": n, "max_abs_x": float(np.abs(X[:, 1:]).max()), "sum_y": float(y.sum())})
        order = list(range(len(specs)))[::-1] if d["reverse"] else list(range(len(specs)))
        c.update(spec=shared([specs[j] for j in order]), ragged=True, datasets=len(specs), chains=d["cpd"] * len(specs), lanes=16)
        c["state"] = np.concatenate([np.repeat(np.asarray(starts[j], dtype=np.float64)[:, None], d["cpd"], axis=1) for j in order], axis=1)
        c["sizes"], c["facts"] = [d["sizes"][j] for j in order], [facts[j] for j in order]
    else:
        raise ValueError(kind)
    return c


out = []
for d in json.loads(sys.argv[2]):
    c = build(d)
    try:
        r = B.run_case(c, shift=d.get("shift", 0))
    except A.AmwgError as e:
        if not d.get("may_refuse"):
            raise
        out.append({"name": d["name"], "refused": str(e)})
        continue
    per = r["per"]
    twins = None
    if c.get("datasets") and d.get("twins"):
        # every dataset again as an ORDINARY sampler (amwg_create: its constants are its own by construction) at chain_offset + j cpd, the same geometry, start and
        # schedule: the chains are the same chains, so the four audit rows must be the same bytes -- a bound or a value formed from a neighbour's constants is not
        cpd, bump, twins = c["chains"] // c["datasets"], np.arange(1, c["chains"] - 1, 3), []
        for j in range(c["datasets"]):
            t = dict(c, spec=c["spec"][j], chains=cpd, chain_offset=OFFSET + j * cpd, ragged=False, datasets=0, state=None if c["state"] is None else c["state"][:, j * cpd:(j + 1) * cpd],
                     bump=bump[(bump >= j * cpd) & (bump < (j + 1) * cpd)] - j * cpd)
            tr = B.run_case(t, shift=d.get("shift", 0))
            mine = per[:, j * cpd:(j + 1) * cpd]
            twins.append({"dataset": j, "kernel": tr["kernel"], "equal": [bool(np.ascontiguousarray(mine[k]).tobytes() == np.ascontiguousarray(tr["per"][k]).tobytes()) for k in range(4)],
                          "max_value_ratio": float(np.max(tr["per"][0])), "max_difference_ratio": float(np.max(tr["per"][1])), "audited_decisions": int(tr["per"][2].sum())})
    e = {"name": d["name"], "launch": r["launch"], "twins": twins, "in_bounds_proposals": r["inbounds"], "audited_decisions": int(per[2].sum()), "wrong_verdicts": int(per[3].sum()),
         "nan": bool(np.isnan(per[0]).any() or np.isnan(per[1]).any()), "max_value_ratio": float(np.nanmax(per[0])), "max_difference_ratio": float(np.nanmax(per[1])),
         "seconds": round(r["wall"], 2), "datasets": r.get("datasets"), "sizes": c.get("sizes"), "facts": c.get("facts")}
    print("%-34s %-50s block %4d grid %5d  audited %9d of %9d  wrong %d  |A-E|/eps %.3g  |dA-dE|/eta %.3g  (%.2f s)" % (
        d["name"], r["kernel"], r["launch"]["block_threads"], r["launch"]["grid_blocks"], e["audited_decisions"], e["in_bounds_proposals"], e["wrong_verdicts"],
        e["max_value_ratio"], e["max_difference_ratio"], r["wall"]), flush=True)
    out.append(e)
print("RESULT " + json.dumps(out))
"""

_children = {}
_stopped = []      # set once a child ended by a signal, an abort or its time limit: nothing more is started on the device by this file


def _child(group, descriptors, env=None):
    """-> {name: record} of one child process over `descriptors`, run once per group and shared by its tests"""
    if group not in _children:
        assert not _stopped, "not started: the child of group %s ended abnormally (%s)" % tuple(_stopped[0])
        e = dict(os.environ)
        e.pop("AMWG_AUDIT_ADVERSARIAL", None)
        e.pop("AMWG_WAVE_SCRATCH", None)
        e.update(env or {})
        try:
            p = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tools"), json.dumps(descriptors)], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
        except subprocess.TimeoutExpired:
            _stopped.append((group, "time limit"))
            raise
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            _stopped.append((group, "exit status %d" % p.returncode))
        _children[group] = p
    p = _children[group]
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert [r["name"] for r in rec] == [d["name"] for d in descriptors]
    return {r["name"]: r for r in rec}


_largest = {}


def _note(family, r):
    """prints the case's line and keeps the largest two ratios per family (test_the_largest_ratios_seen prints them: the figures of tests/README.value_audit.md)"""
    print("%-34s %-50s block %4d grid %5d  audited %9d of %9d  wrong %d  |A-E|/eps %.3g  |dA-dE|/eta %.3g" % (
        r["name"], r["launch"]["kernel"], r["launch"]["block_threads"], r["launch"]["grid_blocks"], r["audited_decisions"], r["in_bounds_proposals"], r["wrong_verdicts"],
        r["max_value_ratio"], r["max_difference_ratio"]))
    for q in r.get("datasets") or []:
        print("    dataset %d (n_obs = %s): audited %d  wrong %d  |A-E|/eps %.3g  |dA-dE|/eta %.3g" % (
            q["dataset"], r["sizes"][q["dataset"]] if r.get("sizes") else "?", q["audited_decisions"], q["wrong_verdicts"], q["max_value_ratio"], q["max_difference_ratio"]))
    v, dd = _largest.get(family, (0.0, 0.0))
    _largest[family] = (max(v, r["max_value_ratio"]), max(dd, r["max_difference_ratio"]))


def _assert_geometry(r, kernel, block, grid):
    li = r["launch"]
    assert (li["kernel"], li["block_threads"], li["summation_order"]) == (kernel, block, 1), (r["name"], li)
    if grid is not None:
        assert li["grid_blocks"] == grid, (r["name"], li)


def _assert_bars(r, every_proposal, adversarial=False):
    """the bars of tests/test_gpu_bound_audit.py on one record, and per dataset where there are datasets"""
    assert r["wrong_verdicts"] == 0, r
    assert not r["nan"] and r["max_value_ratio"] == r["max_value_ratio"] and r["max_difference_ratio"] == r["max_difference_ratio"], r
    assert r["max_value_ratio"] <= 0.5 and r["max_difference_ratio"] <= 0.5, r
    if every_proposal and not adversarial:
        assert r["audited_decisions"] == r["in_bounds_proposals"] > 0, r
    else:
        assert r["audited_decisions"] > 0, r
    for q in r.get("datasets") or []:
        assert q["audited_decisions"] > 0 and q["wrong_verdicts"] == 0, (r["name"], q)
        assert q["max_value_ratio"] <= 0.5 and q["max_difference_ratio"] <= 0.5, (r["name"], q)      # (a NaN fails both)


def _grid(C, per_block):
    return -(-C // per_block)


# ---- group A: every class and form of the family kernels

def _rotate(blocks, sizes, chains):
    """(block, n_obs) in full, the chain count by rotation (as tests/test_gpu_geometry.py _normal_cases does), not the full product"""
    return [(b, chains[(bi + ni) % len(chains)], n) for bi, b in enumerate(blocks) for ni, n in enumerate(sizes)]


A_NORMAL = ([(256, b, c, n, 0) for b, c, n in _rotate((64, 128, 256), (65, 1040, 1855), (37, 2113))] +      # 1040: a block of 16 rows and a partly filled one; 1855: a block, 12 rows, 63 leftovers
            [(512, b, c, n, 0) for b, c, n in _rotate((512,), (7, 513, 1025, 1808, 12289), (2113, 37))] +   # 513: 8 rows and 1; 12289: global memory, not the LDS tile
            [(1024, b, c, n, 0) for b, c, n in _rotate((1024,), (7, 513, 1025, 12289), (2113, 1))] +        # the scalar-path pass
            [(512, 512, 2113, n, 1) for n in (513, 1025)])                                                    # sufficient statistics: no pass
A_NO_SCRATCH = [(max(b, 256), b, 2113, n, 0) for b in (256, 512) for n in (63, 65, 1040, 1855)]               # AMWG_WAVE_SCRATCH=0: the v_readlane form, leftovers added after the butterfly
A_POIS = [(64, 3, 61), (64, 1027, 449), (256, 1027, 61), (256, 3, 449)]                                       # the shapes of test_certified_poisson_kernel_with_a_partial_wavefront_*
A_HIER = [(64, 5, 640, 8), (64, 130, 65, 32), (256, 130, 640, 8), (256, 5, 65, 32)]
A_CLOSURE = [(512, 65), (1024, 65)]


def _normal_name(cls, block, chains, n, suff, tag=""):
    return "normal%s_b%d_c%d_n%d%s" % (tag, block, chains, n, "_suff" if suff else "")


def _normal_desc(cases, tag=""):
    return [dict(kind="normal", name=_normal_name(*k, tag=tag), block=k[1], chains=k[2], n=k[3], suff=k[4]) for k in cases]


def _a_descriptors():
    d = _normal_desc(A_NORMAL)
    d += [dict(kind="pois", name="pois_b%d_c%d_n%d" % k, block=k[0], chains=k[1], n=k[2]) for k in A_POIS]
    d += [dict(kind="hier", name="hier_b%d_c%d_n%d_g%d" % k, block=k[0], chains=k[1], n=k[2], G=k[3]) for k in A_HIER]
    if HAVE_NODE:
        d += [dict(kind="closure", name="closure_n65_b%d_c%d" % k, closure="bench_normal_n65", block=k[0], chains=k[1]) for k in A_CLOSURE]
        d += [dict(kind="replica", name="replica_tail", chains=REPLICA_CHAINS, steps=REPLICA_STEPS)]
    return d


def _group_a():
    return _child("A", _a_descriptors())


@pytest.mark.parametrize("cls,block,chains,n_obs,suff", A_NORMAL)
def test_normal_value_in_every_class(cls, block, chains, n_obs, suff):
    """amwg_step_kernel_cert<NormalModel,1,{256,512,1024}>: blocks of 16 and of 8 rows read a block ahead through LDS, the scalar-path pass, global memory beyond the
    tile's limit, partial wavefronts and workgroups, the pair (lpA, epsA) carried across launches of 13 steps: every in-bounds proposal audited."""
    r = _group_a()[_normal_name(cls, block, chains, n_obs, suff)]
    _note("normal", r)
    _assert_geometry(r, NORMAL % cls, block, _grid(chains, block))
    _assert_bars(r, every_proposal=True)


@pytest.mark.parametrize("cls,block,chains,n_obs,suff", A_NO_SCRATCH)
def test_normal_value_without_the_wave_scratch(cls, block, chains, n_obs, suff):
    """AMWG_WAVE_SCRATCH=0 (its own child): the means broadcast with v_readlane, the leftovers added after the butterfly; 63 / 65 either side of one row."""
    r = _child("A0", _normal_desc(A_NO_SCRATCH, "_noscratch"), env={"AMWG_WAVE_SCRATCH": "0"})[_normal_name(cls, block, chains, n_obs, suff, "_noscratch")]
    _note("normal, no wave scratch", r)
    _assert_geometry(r, NORMAL % cls, block, _grid(chains, block))
    _assert_bars(r, every_proposal=True)


@pytest.mark.parametrize("block,chains,n_obs", A_POIS)
def test_poisson_value_with_partial_wavefronts(block, chains, n_obs):
    r = _group_a()["pois_b%d_c%d_n%d" % (block, chains, n_obs)]
    _note("poisson", r)
    _assert_geometry(r, POIS, block, _grid(chains, block // 16))
    _assert_bars(r, every_proposal=False)


@pytest.mark.parametrize("block,chains,n_obs,G", A_HIER)
def test_hierarchical_sweep_value(block, chains, n_obs, G):
    r = _group_a()["hier_b%d_c%d_n%d_g%d" % (block, chains, n_obs, G)]
    _note("hierarchical", r)
    _assert_geometry(r, HIER, block, _grid(chains, block // 64))
    _assert_bars(r, every_proposal=False)


@needs_node
@pytest.mark.parametrize("block,chains", A_CLOSURE)
def test_closure_tail_value_in_the_large_classes(block, chains):
    """amwg_user_step_cert of bench_normal_n65 in 512- and 1024-thread workgroups: the uniform pass over tail_x_global (csrc/amwg_user.h)"""
    r = _group_a()["closure_n65_b%d_c%d" % (block, chains)]
    _note("closure tail", r)
    _assert_geometry(r, "amwg_user_step_cert", block, _grid(chains, block))
    _assert_bars(r, every_proposal=False)


@needs_node
def test_replica_fallback_value():
    """64-thread workgroups of fewer than 64 chains: a wavefront's line of the wave scratch per workgroup"""
    r = _group_a()["replica_tail"]
    _note("closure tail", r)
    _assert_geometry(r, "amwg_user_step_cert", 64, None)
    assert r["launch"]["grid_blocks"] > REPLICA_CHAINS // 64 + 64, r["launch"]
    _assert_bars(r, every_proposal=False)


# ---- group B: the families' dataset kernels, per dataset, smallest first and reversed

B_NORMAL = [(64, 64, (1, 65, 1025, 12289), 256), (256, 256, (1, 65, 1025, 12289), 256), (512, 512, (1, 513, 1025), 512)]      # (block, cpd, sizes, class): 2 n + 64 spans 66 .. 24 642 (.. 2 114)
SUFF_SIZES = (1, 65, 1025)
SUFF_DATA = [(0.0, 0.01), (1e8, 1.0), (3.0, 2.0)]      # the middle dataset is 1e8 + noise and its chains start next to it: suff_xbar_lo matters (suffstat_x1e8_start_near)
SUFF_STARTS = [[0.5, 0.5], [1e8, 1.0], [0.5, 0.5]]
# design scale and intercept per dataset.  max |X| over the design columns (column 0 is the constant 1) and sum y must each differ 2^10-fold between the first and the
# last dataset (asserted in test_poisson_dataset_value_per_dataset from plain numpy on the inputs): (0.02, 0.0), (0.5, 2.0), (1.5, 5.0) do not reach that; these do
POIS_SCALES, POIS_INTERCEPTS = (0.002, 0.5, 2.5), (-1.0, 2.0, 6.0)
B_POIS = [("equal", (300, 300, 300)), ("ragged", (17, 65, 500))]


def _b_descriptors(adversarial=False):
    d = []
    for rev in (False, True):
        tag = "_reversed" if rev else ""
        for block, cpd, sizes, _ in (B_NORMAL[:2] if adversarial else B_NORMAL):
            d.append(dict(kind="ds_normal", name="ds_normal_b%d%s" % (block, tag), block=block, cpd=cpd, sizes=list(sizes), reverse=rev, may_refuse=block == 512))
        if not adversarial:
            d.append(dict(kind="ds_normal", name="ds_suff%s" % tag, block=64, cpd=64, sizes=list(SUFF_SIZES), reverse=rev, suff=1, data=[list(q) for q in SUFF_DATA], starts=SUFF_STARTS))
        for what, sizes in (B_POIS[1:] if adversarial else B_POIS):
            d.append(dict(kind="ds_pois", name="ds_pois_%s%s" % (what, tag), block=256, cpd=16, sizes=list(sizes), reverse=rev, scales=list(POIS_SCALES), intercepts=list(POIS_INTERCEPTS)))
    return d


def _group_b():
    return _child("B", [dict(q, twins=True) for q in _b_descriptors()])


def _assert_twins(r):
    """dataset d's rows of the audit -- max |A - E| / eps, max |dA - dE| / eta, audited decisions, wrong verdicts, per chain -- are the bytes an ordinary sampler on
    dataset d records at chain_offset + d cpd.  The chains are the same (tests/test_gpu_ragged_datasets.py), so A and E are; what is left to differ is eps: a bound
    formed from another dataset's constants fails here whatever slack the derivation leaves, where the bar of 0.5 sees it only once the slack is used up."""
    assert len(r["twins"]) == len(r["datasets"]), r
    for t, q in zip(r["twins"], r["datasets"]):
        print("    twin of dataset %d: %s  audited %d  |A-E|/eps %.3g  |dA-dE|/eta %.3g  rows equal %s" % (t["dataset"], t["kernel"], t["audited_decisions"], t["max_value_ratio"], t["max_difference_ratio"], t["equal"]))
        assert t["kernel"] == r["launch"]["kernel"].replace("_ds<", "<"), (r["name"], t)
        assert all(t["equal"]), (r["name"], t, q)


def _sizes(sizes, rev):
    return list(sizes)[::-1] if rev else list(sizes)


@pytest.mark.parametrize("rev", [False, True], ids=["smallest_first", "reversed"])
@pytest.mark.parametrize("block,cpd,sizes,cls", B_NORMAL, ids=["b64", "b256", "b512"])
def test_normal_dataset_value_per_dataset(block, cpd, sizes, cls, rev):
    """amwg_step_kernel_cert_ds<NormalModel,1,{256,512}> on ragged datasets: n_obs enters eps ((2 n + 64) u ...), and dataset_view hands every workgroup its own"""
    r = _group_b()["ds_normal_b%d%s" % (block, "_reversed" if rev else "")]
    assert "refused" not in r, r      # (the planner accepts 512-thread workgroups of 512 chains per dataset)
    _note("normal datasets", r)
    _assert_geometry(r, NORMAL_DS % cls, block, len(sizes))
    assert r["sizes"] == _sizes(sizes, rev) and len(r["datasets"]) == len(sizes), r
    _assert_bars(r, every_proposal=True)
    _assert_twins(r)


@pytest.mark.parametrize("rev", [False, True], ids=["smallest_first", "reversed"])
def test_normal_dataset_value_with_sufficient_statistics(rev):
    """suff_xbar_hi / suff_xbar_lo / suff_ss per dataset: the middle dataset lies at 1e8 with its chains beside it, where a neighbour's xbar would be off by 1e8"""
    r = _group_b()["ds_suff%s" % ("_reversed" if rev else "")]
    _note("normal datasets, sufficient statistics", r)
    _assert_geometry(r, NORMAL_DS % 256, 64, 3)
    assert r["sizes"] == _sizes(SUFF_SIZES, rev), r
    _assert_bars(r, every_proposal=True)
    _assert_twins(r)


@pytest.mark.parametrize("rev", [False, True], ids=["smallest_first", "reversed"])
@pytest.mark.parametrize("what,sizes", B_POIS, ids=["equal", "ragged"])
def test_poisson_dataset_value_per_dataset(what, sizes, rev):
    """amwg_step_kernel_cert_ds<PoisGlmModel,16,256>, one 256-thread workgroup of 16 chains per dataset: glm_xmax, glm_sum_y, glm_sum_lf and n_obs per dataset"""
    r = _group_b()["ds_pois_%s%s" % (what, "_reversed" if rev else "")]
    _note("poisson datasets", r)
    _assert_geometry(r, POIS_DS, 256, 3)
    assert r["sizes"] == _sizes(sizes, rev), r
    first, last = (r["facts"][-1], r["facts"][0]) if rev else (r["facts"][0], r["facts"][-1])
    assert last["max_abs_x"] / first["max_abs_x"] >= 2.0 ** 10 and last["sum_y"] / first["sum_y"] >= 2.0 ** 10, r["facts"]
    _assert_bars(r, every_proposal=False)
    _assert_twins(r)


# ---- group C: adversarial uniforms

C_NORMAL = [A_NORMAL[4], A_NORMAL[10], A_NORMAL[15], A_NORMAL[18]]      # one case of each Normal row: (256) 128 threads n = 1040, (512) n = 513, (1024) n = 513, sufficient statistics
DETECTOR = ("normal_n1000", "hier_n640_g8", "pois_n500")
DETECTOR_SHIFT = -20      # profiles/r06_bound_audit.json: the first wrong verdicts at 2^-4 .. 2^-8; twelve binades past the latest


def _c_descriptors():
    d = _normal_desc(C_NORMAL, "_adv")
    d += [dict(kind="pois", name="pois_adv", block=A_POIS[1][0], chains=A_POIS[1][1], n=A_POIS[1][2])]
    d += [dict(kind="hier", name="hier_adv", block=A_HIER[2][0], chains=A_HIER[2][1], n=A_HIER[2][2], G=A_HIER[2][3])]
    if HAVE_NODE:
        d += [dict(kind="replica", name="replica_adv", chains=REPLICA_CHAINS, steps=REPLICA_STEPS)]
    d += [dict(q, name=q["name"] + "_adv", twins=True) for q in _b_descriptors(adversarial=True)]
    for name in DETECTOR:
        d += [dict(kind="quick", name="%s_shift%d" % (name, -k), case=name, shift=k) for k in (0, DETECTOR_SHIFT)]
    return d


def _group_c():
    return _child("C", _c_descriptors(), env={"AMWG_AUDIT_ADVERSARIAL": "1"})


def _assert_adversarial(r):
    _assert_bars(r, every_proposal=False, adversarial=True)


@pytest.mark.parametrize("cls,block,chains,n_obs,suff", C_NORMAL)
def test_adversarial_uniforms_normal(cls, block, chains, n_obs, suff):
    """every certified decision's uniform 1.5 eta outside the sliver: the derived bounds still give no wrong verdict, in every class"""
    r = _group_c()[_normal_name(cls, block, chains, n_obs, suff, "_adv")]
    _note("adversarial", r)
    _assert_geometry(r, NORMAL % cls, block, _grid(chains, block))
    _assert_adversarial(r)


def test_adversarial_uniforms_normal_without_the_wave_scratch():
    k = A_NO_SCRATCH[6]      # 512 threads, n = 1040
    r = _child("C0", _normal_desc([k], "_noscratch_adv"), env={"AMWG_AUDIT_ADVERSARIAL": "1", "AMWG_WAVE_SCRATCH": "0"})[_normal_name(*k, tag="_noscratch_adv")]
    _note("adversarial", r)
    _assert_geometry(r, NORMAL % k[0], k[1], _grid(k[2], k[1]))
    _assert_adversarial(r)


C_OTHER = {"pois_adv": POIS, "hier_adv": HIER, "replica_adv": "amwg_user_step_cert"}


@pytest.mark.parametrize("name", ["pois_adv", "hier_adv"] + (["replica_adv"] if HAVE_NODE else []))
def test_adversarial_uniforms_other_rows(name):
    r = _group_c()[name]
    _note("adversarial", r)
    assert r["launch"]["kernel"] == C_OTHER[name] and r["launch"]["summation_order"] == 1, r["launch"]
    _assert_adversarial(r)


@pytest.mark.parametrize("name", [q["name"] + "_adv" for q in _b_descriptors(adversarial=True)])
def test_adversarial_uniforms_per_dataset(name):
    """both orders of the ragged Normal and the ragged Poisson list: no wrong verdict in any dataset"""
    r = _group_c()[name]
    _note("adversarial", r)
    assert "_cert_ds<" in r["launch"]["kernel"] and len(r["datasets"]) == len(r["sizes"]), r
    _assert_adversarial(r)
    _assert_twins(r)      # (the twins run under the same adversarial uniforms)


@pytest.mark.parametrize("name", DETECTOR)
def test_the_detector_fires_once_the_bounds_are_too_small(name):
    """`wrong_verdicts == 0` means something: with the bounds shrunk 2^-20 the same adversarial uniforms MUST give wrong verdicts, and at the derived bounds none"""
    at0, shrunk = _group_c()["%s_shift0" % name], _group_c()["%s_shift%d" % (name, -DETECTOR_SHIFT)]
    print(name, "shift 0: audited %d wrong %d;  shift %d: audited %d wrong %d" % (at0["audited_decisions"], at0["wrong_verdicts"], DETECTOR_SHIFT, shrunk["audited_decisions"], shrunk["wrong_verdicts"]))
    assert "_cert" in at0["launch"]["kernel"] and at0["launch"] == shrunk["launch"]
    assert at0["audited_decisions"] > 0 and at0["wrong_verdicts"] == 0, at0
    assert shrunk["audited_decisions"] > 0 and shrunk["wrong_verdicts"] > 0, shrunk


def test_the_largest_ratios_seen():
    """prints the largest |A - E| / eps and |dA - dE| / eta per family over the cases that ran before it (recorded in tests/README.value_audit.md, asserted by each case)"""
    for family, (v, d) in sorted(_largest.items()):
        print("largest ratios, %-40s |A-E|/eps %.3g   |dA-dE|/eta %.3g" % (family, v, d))
        assert v <= 0.5 and d <= 0.5
