"""Summaries without stored draws (amwg_sample_summarize; fold_window_kernel of csrc/amwg_diag.hip), on the GPU.  tests/README.summarize.md says what each test pins.

(1) kernel against kernel on arrays, through the test library (amwg_fold_check): the halves folded window by window equal chain_halves_kernel's on the whole array as
    BYTES; the moments formed from the whole-chain pairs agree with the exact moments of every dataset's slice within 4 N u S (below).
(2) a sampler that summarises against its twin that stores: split-R-hat and ESS as bytes, the chains' state / info / diag as bytes, the moments within the bound,
    what summary_info() and launch_info() report; the memory that does not grow with the run; dataset samplers; the refusals.
(3) the JavaScript front end (tests/js/test_gpu_summarize.js).

THE MOMENTS' BOUND.  A dataset's slice holds N = rows * cpd values of magnitude <= S.  The accumulated mean and sum of squares are the results of N sequential
updates whose partial results stay below S (resp. N S^2): to first order each rounding contributes at most u = 2^-53 relative to such a partial result, and an update
rounds a division and two products besides its additions -- hence 4 N u S for the mean and for the sd.  Derived, not tuned; it presumes squares that neither overflow
nor underflow (the 1e300 / 1e-300 array therefore checks its means only: its squares are not representable, in the stored path's kernel no more than here)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import amwg_ctypes
import model_spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261018
U = 2.0 ** -53
WINDOW_BYTES = 64 << 20      # kFoldWindowBytes of csrc/amwg_fold.h (window_rows = 0)


def bound(x):
    return 4.0 * x.size * U * float(np.max(np.abs(x)))


def exact_moments(x):
    """mean by exact summation, sd in long double, of all values of x"""
    flat = x.reshape(-1)
    n = flat.size
    xl = flat.astype(np.longdouble)
    m = xl.sum() / n
    sd = np.sqrt(((xl - m) ** 2).sum() / (n - 1)) if n > 1 else np.longdouble(0)
    return math.fsum(flat.tolist()) / n, float(sd)


def emulated_moments(x):
    """the recurrence and the formula of the library in numpy, fp64, in the kernel's order per chain (the tree over the chains is not reproduced: plain sums) -- x [rows][cpd]"""
    rows, cpd = x.shape
    m, m2 = np.zeros(cpd), np.zeros(cpd)
    for k in range(rows):
        dlt = x[k] - m
        m = m + dlt / np.float64(k + 1)
        m2 = m2 + dlt * (x[k] - m)
    mean = m.sum() / cpd
    ss = m2.sum() + np.float64(rows) * ((m - mean) ** 2).sum()
    n = rows * cpd
    return float(mean), float(np.sqrt(ss / (n - 1))) if n > 1 else 0.0


def check_moments(draws, D, mean, sd, what, sd_too=True):
    rows, PR, C = draws.shape
    cpd = C // D
    assert mean.shape == (D, PR) and sd.shape == (D, PR)
    for d in range(D):
        for p in range(PR):
            x = np.ascontiguousarray(draws[:, p, d * cpd:(d + 1) * cpd])
            em, es = exact_moments(x)
            b = bound(x)
            print("moments %s d=%d p=%d: mean err %.3e sd err %.3e bound %.3e" % (what, d, p, abs(mean[d, p] - em), abs(sd[d, p] - es), b))
            assert abs(mean[d, p] - em) <= b, (what, d, p, mean[d, p], em, b)
            if sd_too:
                assert abs(sd[d, p] - es) <= b, (what, d, p, sd[d, p], es, b)
                hm, hs = emulated_moments(x)      # the formula itself, on the CPU, stays inside the bound on this array
                assert abs(hm - em) <= b and abs(hs - es) <= b, (what, d, p, hm, hs, em, es, b)


def windows_of(rows):
    return sorted({1, 2, 3, max(1, rows // 2), rows + 5})


# ---- (1) kernel against kernel

def grid_array(rng, rows, PR, C):
    """every recorded value at its own location and scale, every chain with its own offset: a wrong stride or a wrong half shows"""
    x = rng.standard_normal((rows, PR, C))
    for p in range(PR):
        x[:, p, :] = (p + 1) * 2.5 + (0.5 + p) * x[:, p, :] + 0.25 * rng.standard_normal(C)[None, :]
    return x


@pytest.mark.parametrize("C,D", [(96, 1), (96, 3), (320, 1)])      # (neither a multiple of 256; 96 no multiple of 64; 3 does not divide 320)
@pytest.mark.parametrize("PR", [1, 3])
@pytest.mark.parametrize("rows", [4, 5, 9, 40])
def test_folded_halves_equal_the_stored_kernels_bytes(rows, PR, C, D):
    rng = np.random.default_rng([SEED, rows, PR, C, D])
    draws = grid_array(rng, rows, PR, C)
    first = None
    for w in windows_of(rows):
        hf, hd, mean, sd = amwg_ctypes.fold_check(draws, D, w)
        assert hf.tobytes() == hd.tobytes(), (rows, PR, C, D, w)
        if first is None:
            first = (hf.tobytes(), mean.tobytes(), sd.tobytes())
            check_moments(draws, D, mean, sd, "grid rows=%d PR=%d C=%d D=%d" % (rows, PR, C, D))
        assert (hf.tobytes(), mean.tobytes(), sd.tobytes()) == first, (rows, PR, C, D, w)      # the cut into windows changes no bit of anything
    # the halves are the halves: against numpy's two-pass values, to rounding (the bytes above compare two kernels that share the recurrence)
    half = rows // 2
    for h in range(2):
        seg = draws[h * half:(h + 1) * half]
        assert np.allclose(hf[h, 0], seg.mean(axis=0), rtol=1e-12, atol=0)
        if half > 1:
            assert np.allclose(hf[h, 1], seg.var(axis=0, ddof=1), rtol=1e-9, atol=0)
        else:
            assert np.all(hf[h, 1] == 0.0)


def test_a_constant_column_has_its_exact_mean_and_no_spread():
    rng = np.random.default_rng([SEED, 1])
    draws = grid_array(rng, 9, 3, 96)
    draws[:, 1, :] = 2.5
    for w in windows_of(9):
        hf, hd, mean, sd = amwg_ctypes.fold_check(draws, 3, w)
        assert hf.tobytes() == hd.tobytes()
        assert np.all(mean[:, 1] == 2.5) and np.all(sd[:, 1] == 0.0)
        assert np.all(hf[:, 0, 1, :] == 2.5) and np.all(hf[:, 1, 1, :] == 0.0)
    check_moments(draws, 3, mean, sd, "constant column")


def test_columns_at_the_ends_of_the_exponent_range():
    rng = np.random.default_rng([SEED, 2])
    draws = rng.standard_normal((9, 3, 96))
    draws[:, 0, :] *= 1e300
    draws[:, 1, :] *= 1e-300
    for w in windows_of(9):
        hf, hd, mean, sd = amwg_ctypes.fold_check(draws, 3, w)
        assert np.array_equal(hf, hd, equal_nan=True) and hf.tobytes() == hd.tobytes()
    check_moments(draws, 3, mean, sd, "1e300 / 1e-300", sd_too=False)      # (squares of these two columns are not representable: the module's docstring)
    x = np.ascontiguousarray(draws[:, 2, :32])
    assert abs(sd[0, 2] - exact_moments(x)[1]) <= bound(x)


def test_a_nan_and_an_infinity_travel_as_in_the_stored_kernel():
    rng = np.random.default_rng([SEED, 3])
    draws = grid_array(rng, 9, 3, 96)
    draws[2, 0, 5] = np.nan
    draws[6, 1, 70] = np.inf
    with np.errstate(invalid="ignore"):
        for w in windows_of(9):
            hf, hd, mean, sd = amwg_ctypes.fold_check(draws, 3, w)
            assert np.array_equal(hf, hd, equal_nan=True), w
    assert np.isnan(hf[0, 0, 0, 5]) and not np.isnan(hf[0, 0, 0, 6]) and not np.isnan(hf[1, 0, 0, 5])      # the NaN stays in its chain and its half
    assert np.isnan(mean[0, 0]) and np.isfinite(mean[1, 0]) and np.isfinite(mean[0, 2])                  # ... and in its dataset


# ---- (2) a summarising sampler against its storing twin

def normal_spec(n_obs=50, seed=500):
    data = model_spec.make_data("normal", n_obs, seed)
    data = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    return model_spec.build_spec("normal", data)


BURN, CHAINS = 120, 128


def after(s, dataset=False):
    out = {"conv": s.dataset_convergence() if dataset else s.convergence(), "mom": s.dataset_moments() if dataset else s.moments(),
           "state": s.state(), "info": s.info(), "diag": s.diag()}
    return out


def same_chains(a, b, what):
    assert a["state"].tobytes() == b["state"].tobytes(), what + ": state"
    for k in a["info"]:
        assert a["info"][k].tobytes() == b["info"][k].tobytes(), what + ": info " + k
    for k in ("uniforms", "named_order", "log_post"):
        assert a["diag"][k].tobytes() == b["diag"][k].tobytes(), what + ": diag " + k


_stored = {}


def stored_run(n, thin, spl):
    """sampler A: sample_async + sync, shared by the window sizes that compare against it"""
    k = (n, thin, spl)
    if k not in _stored:
        a = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED, steps_per_launch=spl)
        a.burn(BURN)
        a.sample_async(n, thin)
        a.sync()
        got = after(a)
        got["draws"] = a.fetch_draws()
        a.close()
        _stored[k] = got
    return _stored[k]


def expected_launches(n, thin, window, spl):
    """the cut of launch_steps: launches of at most spl (or 65535) steps, none recording past the end of the window"""
    chunk = spl if 0 < spl < 65535 else 65535
    done = row = launches = folds = 0
    while True:
        step0 = (thin - done % thin) % thin
        m = min(n - done, chunk, step0 + (window - row) * thin)
        row += (m - step0 + thin - 1) // thin if m > step0 else 0
        done += m
        launches += 1
        if row and (row == window or done >= n):
            folds += 1
            row = 0
        if done >= n:
            return launches, folds


@pytest.mark.parametrize("spl", [0, 5])
@pytest.mark.parametrize("window_rows", [1, 4, 7, 0])
@pytest.mark.parametrize("n,thin", [(40, 3), (43, 3), (16, 1)])      # kept 14, 15 (odd), 16
def test_summarising_sampler_equals_its_storing_twin(n, thin, window_rows, spl):
    A = stored_run(n, thin, spl)
    b = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED, steps_per_launch=spl)
    b.burn(BURN)
    kept = b.summarize(n, thin, window_rows)
    assert kept == -(-n // thin) == A["draws"].shape[0]
    li, si = b.launch_info(), b.summary_info()
    B = after(b)
    what = "n=%d thin=%d window=%d spl=%d" % (n, thin, window_rows, spl)
    for k in (0, 1):
        assert B["conv"][k].tobytes() == A["conv"][k].tobytes(), (what, "rhat" if k == 0 else "ess", B["conv"][k], A["conv"][k])
    same_chains(A, B, what)
    check_moments(A["draws"], 1, B["mom"][0][None, :], B["mom"][1][None, :], what)
    row_bytes = b.PR * CHAINS * 8
    w = window_rows if window_rows > 0 else min(kept, WINDOW_BYTES // row_bytes)
    launches, folds = expected_launches(n, thin, w, spl)
    assert si == {"rows": kept, "window_rows": w, "windows": -(-kept // w), "window_bytes": w * row_bytes, "accumulator_bytes": 6 * row_bytes}, (what, si)
    assert folds == si["windows"] and li["n_launches"] == launches, (what, li, launches)
    if spl == 5 and thin == 3 and window_rows in (4, 7):
        assert launches > si["windows"] > 1      # several launches share a window, and a launch starts between recorded steps
    b.close()


def test_the_window_does_not_grow_with_the_run():
    n, w = 3000, 7
    A = stored_run(n, 1, 0)
    short = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    short.burn(BURN)
    short.summarize(40, 1, w)
    small = short.summary_info()
    short.close()
    b = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    b.burn(BURN)
    b.summarize(n, 1, w)
    si, li = b.summary_info(), b.launch_info()
    assert si["window_bytes"] == small["window_bytes"] == w * b.PR * CHAINS * 8 and si["accumulator_bytes"] == small["accumulator_bytes"]
    assert si["rows"] == n and si["windows"] == -(-n // w) and li["n_launches"] == -(-n // w) and li["kernel_ms"] > 0      # every launch of the call, not the last window's
    B = after(b)
    assert B["conv"][0].tobytes() == A["conv"][0].tobytes() and B["conv"][1].tobytes() == A["conv"][1].tobytes()
    same_chains(A, B, "n=3000")
    check_moments(A["draws"], 1, B["mom"][0][None, :], B["mom"][1][None, :], "n=3000")
    # a burn leaves the summary alone, as it leaves draws alone
    b.burn(5)
    again = b.convergence()
    assert again[0].tobytes() == B["conv"][0].tobytes() and again[1].tobytes() == B["conv"][1].tobytes() and b.summary_info() == si
    b.close()


@pytest.mark.parametrize("sizes", [(50, 50, 50, 50), (20, 50, 35, 64)])
def test_dataset_samplers_summarise_per_dataset(sizes):
    specs = [normal_spec(n_obs, 500 + 7 * d) for d, n_obs in enumerate(sizes)]
    ragged = len(set(sizes)) > 1
    runs = []
    for summarise in (False, True):
        s = amwg_ctypes.Sampler(specs, chains=4 * 32, seed=SEED, ragged=ragged)
        s.burn(BURN)
        if summarise:
            s.summarize(40, 3, 4)
        else:
            s.sample_async(40, 3)
            s.sync()
        got = after(s, dataset=True)
        for pooled in (s.moments, s.convergence):      # the pooled calls stay refused
            with pytest.raises(amwg_ctypes.AmwgError) as ei:
                pooled()
            assert "pooled summaries are refused" in str(ei.value)
        if not summarise:
            got["draws"] = s.fetch_draws()
        s.close()
        runs.append(got)
    A, B = runs
    assert B["conv"][0].shape == (4, 2)
    assert B["conv"][0].tobytes() == A["conv"][0].tobytes() and B["conv"][1].tobytes() == A["conv"][1].tobytes()
    same_chains(A, B, str(sizes))
    check_moments(A["draws"], 4, B["mom"][0], B["mom"][1], "datasets " + str(sizes))


def test_calls_that_need_the_draws_are_refused_until_the_next_sample():
    s = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    s.burn(BURN)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.summary_info()
    assert "amwg_summary_info" in str(ei.value)
    s.summarize(40, 3, 4)
    for call in (lambda: s.quantiles([0.5]), lambda: s.dataset_quantiles([0.5]), s.fetch_draws, lambda: s.fetch_draws_slices([(0, 1)]),
                 lambda: amwg_ctypes.group_moments([s]), lambda: amwg_ctypes.group_convergence([s]), lambda: amwg_ctypes.group_quantiles([s], [0.5])):
        with pytest.raises(amwg_ctypes.AmwgError) as ei:
            call()
        assert "amwg error -1" in str(ei.value) and "amwg_sample_summarize" in str(ei.value) and "not kept" in str(ei.value), str(ei.value)
    assert s.sample(8).shape == (8, s.PR, CHAINS)
    assert s.quantiles([0.5]).shape == (s.PR, 1) and s.dataset_quantiles([0.5]).shape == (1, s.PR, 1)
    s.sample_async(8)
    assert s.fetch_draws().shape == (8, s.PR, CHAINS)
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.summary_info()
    assert "amwg_summary_info" in str(ei.value)
    s.close()


def test_summarising_nothing_leaves_nothing_to_summarise():
    s = amwg_ctypes.Sampler(normal_spec(), chains=CHAINS, seed=SEED)
    s.burn(BURN)
    assert s.summarize(0) == 0
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.moments()
    assert "no sample() call yet" in str(ei.value)
    with pytest.raises(amwg_ctypes.AmwgError):
        s.summary_info()
    # too few kept draws for the diagnostics: the stored path's refusal
    s.summarize(3)
    assert np.all(np.isfinite(s.moments()[0]))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        s.convergence()
    assert ">= 4 kept draws" in str(ei.value)
    s.close()


# ---- (3) the JavaScript front end

@pytest.mark.node
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_front_end_summarize_on_gpu():
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "test_gpu_summarize.js")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gpu summarize ok" in p.stdout, p.stdout + "\n" + p.stderr
