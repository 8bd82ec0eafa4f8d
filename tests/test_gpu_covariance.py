"""Posterior covariance on the device (csrc/amwg_covariance.hip), on the GPU.  tests/README.covariance.md says what each test pins.

(1) the kernels on synthetic arrays, through the test library (amwg_covariance_check): bit for bit the restated order (covariance_reference.kernel_order_cov),
    inside the cap of exact rational arithmetic, the same bytes however the rows are cut into windows, symmetric; K = 1, K = PR, K beyond a register tile;
    neighbours, permutations, scaling.
(2) a sampler that summarises with an armed covariance against its twin that stores; dataset samplers; a translated closure with a derived quantity; refusals.
(3) the JavaScript front end (tests/js/test_gpu_covariance.js)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import covariance_reference as cr
import model_spec
import summary_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
WINDOWS = [1, 3]      # and `rows`


def same_bytes(a, b):
    """equal as bytes; a NaN is held to a NaN (its sign and payload are not pinned)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a.view(np.uint64)[keep], b.view(np.uint64)[keep])


# ---- (1) the kernels on synthetic arrays

_worst = [0.0, ""]      # the largest |device - exact| / cap over this file's cases (printed; tests/README.covariance.md records it)


@pytest.mark.parametrize("pattern,kind", cr.CASES())
@pytest.mark.parametrize("rows,cpd", cr.SHAPES)
def test_the_matrix_on_patterns_and_shapes(rows, cpd, pattern, kind):
    a = cr.array(pattern, kind, rows, cpd)
    label = "%s/%s %dx%d" % (pattern, kind, rows, cpd)
    got = amwg_ctypes.covariance_check(a.draws, cr.D, cr.VALUES)
    assert got.shape == (cr.D, 3, 3)
    assert same_bytes(got, a.want), (label, got, a.want)                        # 1. bit for bit the restated order
    worst = [0.0, ""]
    cr.held_to_exact(got, a, cr.D, label, worst)                                # 2. inside the cap against exact
    for w in WINDOWS + [rows]:                                                  # 3. windows give the stored path's bytes
        assert same_bytes(amwg_ctypes.covariance_check(a.draws, cr.D, cr.VALUES, w), got), (label, "window_rows", w)
    assert same_bytes(got, np.transpose(got, (0, 2, 1)))                        # 4. symmetric as bytes
    pooled = amwg_ctypes.covariance_check(a.draws, 1, cr.VALUES)                 # 5. D = 1 over all chains
    cr.held_to_exact(pooled, a, 1, label + " pooled", worst)
    if worst[0] > _worst[0]:
        _worst[:] = worst
    print("device vs exact, %s: largest |error| / cap = %.4f (%s); largest so far %.4f (%s)" % (label, worst[0], worst[1], _worst[0], _worst[1]))


def wide_array(rows, cpd, pr):
    return cr.Array("healthy", "mixed", rows, cpd, n_datasets=2, values=tuple(range(pr)), pr=pr)


@pytest.mark.parametrize("pr,values", [(4, (1,)), (4, (0, 1, 2, 3)), (4, (3, 1)), (6, (5, 0, 2, 4, 1)), (8, tuple(range(8))), (11, (7, 3, 10, 0, 5, 9, 1, 8, 2, 6, 4)),
                                       (11, tuple(range(11))), (11, (10, 0, 9, 1, 8, 2, 7, 3, 6))])
def test_numbers_of_values_and_tile_seams(pr, values):
    """K = 1 (no pair), K = 2, K = PR, the tiles of 4 and 8 with repeats past K, and K = 9, 11 > 8: tiles of four and their crossings"""
    a = wide_array(9, 64, pr)
    want = cr.kernel_order_matrix(a.draws, 2, values)
    got = amwg_ctypes.covariance_check(a.draws, 2, values)
    assert got.shape == (2, len(values), len(values)) and same_bytes(got, want), (values, np.argwhere(got != want)[:5].tolist())
    for w in (1, 4, 9):
        assert same_bytes(amwg_ctypes.covariance_check(a.draws, 2, values, w), got), (values, w)
    assert same_bytes(got, np.transpose(got, (0, 2, 1)))


def test_neighbours_do_not_reach_a_matrix():
    a = cr.array("healthy", "mixed", 8, 257)
    base = amwg_ctypes.covariance_check(a.draws, cr.D, cr.VALUES)
    cpd = 257
    for d in range(cr.D):
        for fill in (np.nan, 1e300):
            other = np.full(a.draws.shape, fill)
            for p in cr.VALUES:
                other[:, p, d * cpd:(d + 1) * cpd] = a.draws[:, p, d * cpd:(d + 1) * cpd]
            for w in (0, 3):
                got = amwg_ctypes.covariance_check(other, cr.D, cr.VALUES, w)
                assert same_bytes(got[d], base[d]), (d, fill, w)
    for fill in (np.nan, 1e300, 0.0):      # the value that was not selected
        other = a.draws.copy()
        other[:, 1, :] = fill
        assert same_bytes(amwg_ctypes.covariance_check(other, cr.D, cr.VALUES), base), fill
    # a NaN among ONE selected value's draws in one dataset: that value's row and column there are NaN, every other entry keeps its bytes
    other = a.draws.copy()
    other[5, 0, cpd + 9] = np.nan      # value 0 = position 1 of VALUES, dataset 1
    got = amwg_ctypes.covariance_check(other, cr.D, cr.VALUES)
    hit = np.zeros(base.shape, dtype=bool)
    hit[1, 1, :] = hit[1, :, 1] = True
    assert np.all(np.isnan(got[hit])) and same_bytes(got[~hit], base[~hit])
    other[5, 0, cpd + 9] = np.inf
    got = amwg_ctypes.covariance_check(other, cr.D, cr.VALUES, 3)
    assert np.all(np.isnan(got[hit])) and same_bytes(got[~hit], base[~hit])


def test_permutations_of_values_and_datasets():
    a = cr.array("offset1e6", "mixed", 9, 64)
    base = amwg_ctypes.covariance_check(a.draws, cr.D, (0, 2, 3))
    for perm in ((2, 0, 3), (3, 2, 0), (0, 3, 2), (3, 0, 2), (2, 3, 0)):
        got = amwg_ctypes.covariance_check(a.draws, cr.D, perm, 4)
        idx = [(0, 2, 3).index(p) for p in perm]
        assert same_bytes(got, base[:, idx][:, :, idx]), perm
    order = [2, 0, 1]
    moved = np.concatenate([a.draws[:, :, d * 64:(d + 1) * 64] for d in order], axis=2)
    assert same_bytes(amwg_ctypes.covariance_check(moved, cr.D, (0, 2, 3)), base[order])


@pytest.mark.parametrize("k", [-200, 300])
def test_scaling_a_value_scales_its_row_and_column_exactly(k):
    a = cr.array("healthy", "mixed", 9, 64)
    base = amwg_ctypes.covariance_check(a.draws, cr.D, cr.VALUES)
    for pos, p in enumerate(cr.VALUES):
        scaled = a.draws.copy()
        scaled[:, p, :] = np.ldexp(scaled[:, p, :], k)
        got = amwg_ctypes.covariance_check(scaled, cr.D, cr.VALUES, 4)
        want = base.copy()
        want[:, pos, :] = np.ldexp(want[:, pos, :], k)
        want[:, :, pos] = np.ldexp(want[:, :, pos], k)      # (the diagonal entry twice: 2^2k, which neither overflows nor underflows here)
        assert np.all(np.isfinite(want)) and np.all(want[:, pos, pos] > 0)
        assert same_bytes(got, want), (k, p)


def test_a_doubled_column():
    """y = 2 x: cov_xy = 2 cov_xx as bytes, whichever of the two has the smaller index, and a correlation within 4 ulp of 1"""
    a = cr.array("healthy", "independent", 9, 64)
    for x, y in ((0, 3), (3, 0)):
        d = a.draws.copy()
        d[:, y, :] = 2.0 * d[:, x, :]
        got = amwg_ctypes.covariance_check(d, cr.D, (x, y), 4)
        assert same_bytes(got[:, 0, 1], 2.0 * got[:, 0, 0]) and same_bytes(got[:, 1, 1], 4.0 * got[:, 0, 0])
        cor = amwg_ctypes.correlation(got)
        assert np.all(np.abs(cor[:, 0, 1] - 1.0) <= 4 * 2.0 ** -52) and np.all(cor[:, 0, 0] == 1.0)


# ---- (2) samplers

def normal_spec(n_obs=50, seed=500):
    data = model_spec.make_data("normal", n_obs, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


BURN, CHAINS = 120, 128


def exact_matrix(draws, n_datasets, values):
    """draws [rows][PR][C] as fetched -> an Array-like holder for covariance_reference.held_to_exact"""
    class Holder:
        pass
    h = Holder()
    h.draws, h.values, h.rows = draws, tuple(values), draws.shape[0]
    h.columns = lambda n: cr.Array.columns(h, n)
    h.exact = lambda n: cr.Array.exact.__wrapped__(h, n)
    return h


_stored = {}


def stored_twin(n, thin):
    if (n, thin) not in _stored:
        a = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
        a.burn(BURN)
        a.sample_async(n, thin)
        a.sync()
        _stored[(n, thin)] = {"cov": a.dataset_covariance(), "draws": a.fetch_draws(), "conv": a.convergence(), "state": a.state(), "info": a.covariance_info()}
        a.sample_async(n, thin)      # a second batch, which continues the first: what a second summarising call of the twin must give, and nothing of the first batch
        a.sync()
        _stored[(n, thin)].update(cov2=a.dataset_covariance(), draws2=a.fetch_draws())
        a.close()
    return _stored[(n, thin)]


@pytest.mark.parametrize("window_rows", [1, 7, 0])
@pytest.mark.parametrize("n,thin", [(40, 3), (43, 3)])
def test_summarising_sampler_gives_its_storing_twins_matrix(n, thin, window_rows):
    A = stored_twin(n, thin)
    assert A["info"] == {"n_values": 0, "bytes": 0}
    plain = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)      # the same call without a covariance: what arming must not change
    plain.burn(BURN)
    plain.summarize(n, thin, window_rows)
    plain_conv, plain_state, plain_mom = plain.convergence(), plain.state(), plain.moments()
    si_plain, launches_plain = plain.summary_info(), plain.launch_info()["n_launches"]
    plain.close()
    b = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    b.burn(BURN)
    K = b.PR
    b.summarize(n, thin, window_rows, covariance=True)
    assert b.covariance_info() == {"n_values": K, "bytes": K * (K - 1) // 2 * CHAINS * 8 + K * 4}
    got = b.dataset_covariance()
    assert got.shape == (1, K, K) and same_bytes(got, A["cov"]), (n, thin, window_rows, got, A["cov"])
    worst = [0.0, ""]
    cr.held_to_exact(got, exact_matrix(A["draws"], 1, range(K)), 1, "sampler n=%d thin=%d window=%d" % (n, thin, window_rows), worst)
    print("summarised sampler vs exact on the twin's draws: largest |error| / cap = %.4f (%s)" % tuple(worst))
    mean, sd = b.moments()
    assert same_bytes(np.sqrt(np.diagonal(got[0])), sd) and same_bytes(sd, plain_mom[1]) and same_bytes(mean, plain_mom[0])
    conv = b.convergence()
    for i in range(2):
        assert conv[i].tobytes() == plain_conv[i].tobytes() == A["conv"][i].tobytes()
    assert b.state().tobytes() == plain_state.tobytes() == A["state"].tobytes()
    assert b.summary_info() == si_plain and b.launch_info()["n_launches"] == launches_plain
    # a second call starts afresh (in Python the covariance stays armed): its matrix is the twin's over the SECOND batch alone, every byte -- co-moments that
    # were not zeroed would add the first batch's to the off-diagonal entries
    b.summarize(n, thin, window_rows)
    again = b.dataset_covariance()
    assert same_bytes(again, A["cov2"]) and same_bytes(again, cr.kernel_order_matrix(A["draws2"], 1, range(K))), (n, thin, window_rows, again, A["cov2"])
    assert not same_bytes(again, got)
    cr.held_to_exact(again, exact_matrix(A["draws2"], 1, range(K)), 1, "second call n=%d thin=%d window=%d" % (n, thin, window_rows), worst)
    assert same_bytes(np.sqrt(np.diagonal(again[0])), b.moments()[1])
    cd = lambda a: a.ctypes.data_as(amwg_ctypes.C.POINTER(amwg_ctypes.C.c_double))
    for call in (lambda: b.dataset_covariance(range(K)), lambda: b.dataset_covariance([0]),
                 lambda: amwg_ctypes._check(amwg_ctypes.lib().amwg_last_sample_dataset_covariance(b.h, None, K - 1, cd(got)))):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_set_covariance" in str(ei.value), str(ei.value)
    b.set_covariance(None)
    assert b.covariance_info() == {"n_values": 0, "bytes": 0}
    b.close()


@pytest.mark.parametrize("sizes", [(50, 50, 50, 50), (20, 50, 35, 64)])
def test_a_dataset_sampler_gives_a_matrix_per_dataset(sizes):
    specs = [normal_spec(n_obs, 500 + 7 * d) for d, n_obs in enumerate(sizes)]
    ragged = len(set(sizes)) > 1
    a = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=ragged)
    a.burn(BURN)
    a.sample_async(40, 3)
    a.sync()
    draws = a.fetch_draws()
    values = list(range(a.PR))[::-1]
    stored = a.dataset_covariance(values)
    a.close()
    assert stored.shape == (4, len(values), len(values))
    holder = exact_matrix(draws, 4, values)
    worst = [0.0, ""]
    cr.held_to_exact(stored, holder, 4, "datasets %s stored" % (sizes,), worst)
    assert same_bytes(stored, cr.kernel_order_matrix(draws, 4, values))
    b = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=ragged)
    b.burn(BURN)
    b.set_covariance(values)
    b.summarize(40, 3, 4)
    got = b.dataset_covariance()
    b.close()
    assert same_bytes(got, stored)
    cr.held_to_exact(got, holder, 4, "datasets %s summarised" % (sizes,), worst)
    print("dataset sampler vs exact: largest |error| / cap = %.4f (%s)" % tuple(worst))


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_a_translated_closure_with_a_derived_quantity():
    import golden_io
    import user_host
    name = "norm_post_derived"
    rec = golden_io.load("user_" + name)["chains"][0]
    src, arrays, meta = user_host.translated(name)
    params, init, opts = [], [], []
    for p in rec["params_completed"]:
        params.append({"type": p["type"], "len": int(np.prod(p["dim"])), "top": p["dim"][0], "multidim": 0 if p["dim"] == [1] else 1, "lower": p["lower"], "upper": p["upper"]})
        init += p["init"]
    for o in rec["comp_opts"]:
        opts.append({"prop_log_scale": o.get("prop_log_scale", 0.0), "max_adaptation": o.get("max_adaptation", 0.33), "initial_adaptation": o.get("initial_adaptation", 1.0),
                     "target_accept_rate": o.get("target_accept_rate", 0.44), "batch_size": o.get("batch_size", 50), "is_adapting": o.get("is_adapting", True)})
    spec = {"user": user_host.user_spec_part(src, arrays, meta), "params": params, "P": len(init), "init": init, "comp_opts": opts}
    a = amwg_ctypes.Sampler(spec, chains=96, seed=7, lanes_per_chain=1)
    assert a.PR > a.P
    a.burn(BURN)
    draws = a.sample(30, 3)
    got = a.dataset_covariance()
    a.close()
    assert got.shape == (1, a.PR, a.PR)
    worst = [0.0, ""]
    cr.held_to_exact(got, exact_matrix(draws, 1, range(a.PR)), 1, "closure", worst)      # (the derived value's row among them; a draw that is not finite gives NaN there)
    assert same_bytes(got, cr.kernel_order_matrix(draws, 1, range(a.PR)))
    b = amwg_ctypes.Sampler(spec, chains=96, seed=7, lanes_per_chain=1)
    b.burn(BURN)
    b.summarize(30, 3, 4, covariance=True)
    assert same_bytes(b.dataset_covariance(), got)
    b.close()


def test_without_an_armed_covariance_and_without_a_sample():
    s = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_covariance([0, 1])
    assert "amwg_last_sample_dataset_covariance" in str(ei.value) and "no sample() call yet" in str(ei.value)
    s.burn(BURN)
    s.summarize(40, 3, 4)
    for call in (lambda: s.dataset_covariance(), lambda: s.dataset_covariance([0, 1])):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_set_covariance" in str(ei.value) and "amwg_last_sample_dataset_covariance" in str(ei.value), str(ei.value)
    s.set_covariance([1, 0])      # armed AFTER the call: there is still nothing folded for it
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.dataset_covariance()
    assert "amwg_set_covariance" in str(ei.value)
    for bad, why in (([0, 0], "listed twice"), ([0, s.PR], "outside the recorded values"), (list(range(s.PR + 1)), "values")):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            s.set_covariance(bad)
        assert "amwg_set_covariance" in str(ei.value) and why in str(ei.value), str(ei.value)
    draws = s.sample(8)
    got = s.dataset_covariance([1, 0])
    assert got.shape == (1, 2, 2) and same_bytes(got, cr.kernel_order_matrix(draws, 1, (1, 0)))
    s.close()


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_covariance_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_covariance.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu covariance ok" in p.stdout, p.stdout + "\n" + p.stderr
