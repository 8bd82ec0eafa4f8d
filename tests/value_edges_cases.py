"""The inputs of tests/test_gpu_value_edges.py and tests/test_value_edges_host.py (README.edges.md): samplers whose log_post is not finite, or whose values leave
the range the fast arithmetic needs.  No tolerance anywhere: what is compared is compared as bits.

A case: {"name", "family", "spec", "kind", "components", "reaches"}.
  kind        "alive": on the oracle's two chains every adapting component has 0 < accepts < inbounds
              "alive_any": some chain of the sampler accepts (the oracle's two chains taken together have 0 < sum accepts < sum inbounds)
              "stuck": accepts == 0 on every chain
              "frozen": every proposal inside the bounds equals the current value and is accepted (accepts == inbounds), the state never changes
  components  for "alive": the components the condition is asked of (None: all)
  reaches     a function of the spec that ASSERTS, on the inputs, that the case reaches the branch it is aimed at (mid_range / wide_range restated on high words)
"""
import numpy as np

import model_spec

SEED = 23
CHAINS = 100
BURN, N1, THIN, N2 = 50, 70, 3, 5      # burn 50, sample(70, thin 3), diag, sample(5), diag: adaptation batches of 50 close inside the first sample call
STEPS = BURN + N1 + N2
INF = float("inf")
NAN = float("nan")


# ---- csrc/amwg_div.h restated on the high words
def hi_word(v):
    return (np.atleast_1d(np.asarray(v, dtype=np.float64)).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def mid_range(v):
    """2^-200 <= v <= 2^200 (positive, normal): high word in [0x33700000, 0x4C700000], as an unsigned 32-bit difference"""
    return (hi_word(v) - np.uint32(0x33700000)) <= np.uint32(0x4C700000 - 0x33700000)


def wide_range(v):
    """2^-600 <= |v| <= 2^600; exactly zero is not included"""
    return ((hi_word(v) & np.uint32(0x7FFFFFFF)) - np.uint32(0x1A700000)) <= np.uint32(0x65700000 - 0x1A700000)


def data_mid_range(x):
    """csrc/amwg_create.hip upload_normal_data: every observation is 0 or has |x| inside mid_range"""
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all((x == 0.0) | mid_range(np.abs(x))))


# ---- spec builders
def _opts(scales):
    return [dict(model_spec.DEFAULT_OPT, prop_log_scale=float(s)) for s in scales]


def normal_spec(x, init=(0.5, 0.5), hyper=None, scales=(0.0, 0.0), mu_type="real", sigma_lower=0.0):
    params = [{"type": mu_type, "len": 1, "top": 1, "multidim": 0, "lower": -INF, "upper": INF, "init": [float(init[0])]},
              {"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": float(sigma_lower), "upper": INF, "init": [float(init[1])]}]
    return model_spec.build_spec("normal", {"x": np.array(x, dtype=np.float64)}, params=params, comp_opts=_opts(scales), hyper=hyper)


def normal_x(n_obs=200):
    return np.array(model_spec.make_data("normal", n_obs, 31)["x"], dtype=np.float64)


def _with(x, i, v):
    x = np.array(x, dtype=np.float64)
    x[i] = v
    return x


WIDE_HYPER = [0.0, 1e80, 0.0, 1e80]


def _den(sigma):
    return 2.0 * sigma * sigma


def _r_one_out(spec):
    x = spec["data"]["x"]
    assert not data_mid_range(x) and int((~mid_range(np.abs(x))).sum()) == 1      # data_mid_range == 0 for one observation
    assert np.isfinite(x * x).all() and wide_range((x[5] - spec["init"][0]) ** 2).all()      # finite squares, inside the prior's wide_range
    assert not mid_range(_den(spec["init"][1])).all() and not mid_range(abs(spec["init"][0])).all() and not mid_range(_den(spec["hyper"][1])).all()      # den, mu and the prior's den0 are outside as well
    assert np.isfinite(_den(spec["init"][1])) and np.isfinite(_den(spec["hyper"][1]))


def _r_tiny(spec):
    assert data_mid_range(spec["data"]["x"])      # the data stay in range ...
    assert not mid_range(_den(spec["init"][1])).all() and _den(spec["init"][1]) > 0.0      # ... den = 2 sigma^2 is below 2^-200: den_ok is false
    assert spec["init"][0] == 0.0      # (mu == 0: its own term of the condition)


def _r_subnormal_den(spec):
    den = _den(spec["init"][1])
    assert 0.0 < den < np.finfo(np.float64).tiny and not mid_range(den).all()      # den = 2e-310 is subnormal: den_ok is false ...
    with np.errstate(over="ignore"):
        assert np.isinf(np.float64(1.0) / np.float64(den))      # ... and the reciprocal the fast quotient multiplies by would be +inf
    assert not data_mid_range(spec["data"]["x"])      # (the data are below 2^-200 as well)


def _r_huge(spec):
    assert data_mid_range(spec["data"]["x"]) and mid_range(abs(spec["init"][0])).all()
    assert not mid_range(_den(spec["init"][1])).all() and np.isfinite(_den(spec["init"][1]))      # den = 2e80 is above 2^200
    h = spec["hyper"]
    assert not mid_range(_den(h[1])).all()      # the prior's den0_ok is false as well (2e90)


def _r_offset(spec):
    x = spec["data"]["x"]
    assert data_mid_range(x) and mid_range(abs(spec["init"][0])).all() and mid_range(_den(spec["init"][1])).all()      # INSIDE: the fast pass runs, on differences that cancel
    assert np.spacing(1e15) == 0.125 and np.all(np.abs(x - 1e15) < 32.0)


def _r_outside_support(spec):
    h = spec["hyper"]
    assert not (h[2] <= spec["init"][1] <= h[3])      # ld.unif is -inf at the start
    assert data_mid_range(spec["data"]["x"])


def _r_unbounded_sigma(spec):
    assert spec["params"][1]["lower"] == -INF and spec["init"][1] > 0.0


def _r_int_mu_zero(spec):
    x = spec["data"]["x"]
    assert spec["params"][0]["type"] == "int" and spec["init"][0] == 0.0 and data_mid_range(x)      # mu == 0 exactly: the special case of ps.fast
    assert abs(float(x.mean())) < 0.5      # centred: the rounded proposals stay at 0 and +-1


def _r_constant(spec):
    x = spec["data"]["x"]
    assert spec["params"][0]["type"] == "int" and np.all(x == spec["init"][0])      # S2 == 0 exactly at the start


def _r_non_finite(spec):
    x = spec["data"]["x"]
    with np.errstate(over="ignore", invalid="ignore"):
        bad = ~np.isfinite(x * x)
    assert int(bad.sum()) == 1 and not data_mid_range(x)      # NaN, inf, or a square that overflows: one term is not finite


def normal_cases():
    x = normal_x()
    c = []
    add = lambda name, spec, kind, reaches, components=None: c.append({"name": name, "family": "normal", "spec": spec, "kind": kind, "reaches": reaches, "components": components})
    add("a_one_out_of_mid_range", normal_spec(_with(x, 5, 1e70), (1e68, 1e69), WIDE_HYPER, (156, 158)), "alive", _r_one_out)
    add("b_scale_1e-40", normal_spec(x * 1e-40, (0.0, 1e-40), None, (-94, -94)), "alive", _r_tiny)
    add("b_scale_1e-155", normal_spec(x * 1e-155, (0.0, 1e-155), None, (-357, -357)), "alive", _r_subnormal_den)
    add("c_scale_1e40", normal_spec(x * 1e40, (1e40, 1e40), [0.0, 1e45, 0.0, 1e45], (90, 90)), "alive", _r_huge)
    add("d_offset_1e15", normal_spec(x + 1e15, (1e15, 2.0), [0.0, 1e17, 0.0, 100.0], (-2, -2)), "alive", _r_offset)
    add("e_scale_1e-40_default_scale", normal_spec(x * 1e-40, (0.0, 1e-40)), "stuck", _r_tiny)
    add("e_scale_1e40_default_scale", normal_spec(x * 1e40, (1e40, 1e40), [0.0, 1e45, 0.0, 1e45]), "frozen", _r_huge)
    add("e_offset_1e15_default_scale", normal_spec(x + 1e15, (1e15, 2.0), [0.0, 1e17, 0.0, 100.0]), "alive", _r_offset)
    add("f_outside_support", normal_spec(x, (0.5, 0.5), [0.0, 100.0, 1.0, 2.0]), "alive", _r_outside_support)
    add("g_sigma_unbounded", normal_spec(x, (0.5, 0.5), None, (0, 0), sigma_lower=-INF), "alive", _r_unbounded_sigma)
    add("h_int_mu_zero", normal_spec(x - x.mean(), (0.0, 0.5), None, (0, 0), mu_type="int"), "alive", _r_int_mu_zero)
    add("h_int_mu_constant_data", normal_spec(np.full(200, 3.0), (3.0, 0.5), None, (0, 0), mu_type="int"), "alive", _r_constant)
    add("i_nan", normal_spec(_with(x, 7, NAN)), "stuck", _r_non_finite)
    add("i_inf", normal_spec(_with(x, 7, INF)), "stuck", _r_non_finite)
    add("i_1e250", normal_spec(_with(x, 5, 1e250)), "stuck", _r_non_finite)
    add("a_2049_observations", normal_spec(_with(normal_x(2049), 5, 1e70), (1e68, 1e69), WIDE_HYPER, (156, 158)), "alive", _r_one_out)
    return c


DAGGER = ["a_one_out_of_mid_range", "d_offset_1e15", "f_outside_support"]      # also: block_threads 512 and 1024, sufficient_statistics, 64 lanes


def dataset_specs(middle):
    """three datasets of 200 observations for amwg_step_kernel_cert_ds: the MIDDLE one is case a or case f.  Parameters, start and stepper options are the
    sampler's (those of the first spec) and the hyper-parameters are shared (amwg_create_datasets insists); the data -- and with them data_mid_range -- are
    each dataset's own: the neighbours are ordinary data under the middle case's start, proposal scales and priors."""
    mid = case("normal", middle)["spec"]
    out = []
    for d in range(3):
        x = np.array(model_spec.make_data("normal", 200, 500 + 7 * d)["x"], dtype=np.float64)
        s = normal_spec(x, mid["init"], mid["hyper"], [o["prop_log_scale"] for o in mid["comp_opts"]])
        out.append(s)
    out[1] = mid
    return out


# ---- Beta-Bernoulli, n = 300
def bern_spec(x, init=0.5, hyper=None, lower=0.0, upper=1.0):
    params = [{"type": "real", "len": 1, "top": 1, "multidim": 0, "lower": float(lower), "upper": float(upper), "init": [float(init)]}]
    return model_spec.build_spec("beta_bern", {"x": np.array(x, dtype=np.float64)}, params=params, hyper=hyper)


def _r_theta_at(v):
    def r(spec):
        assert spec["init"][0] == v      # log_v8(0) in one of the two terms: lp = -inf at the start
    return r


def _r_all(v, hyper=None):
    def r(spec):
        assert np.all(spec["data"]["x"] == v) and (hyper is None or spec["hyper"] == hyper)
    return r


def _r_hyper(spec):
    assert spec["hyper"] == [0.5, 0.5]


def _r_theta_unbounded(spec):
    assert spec["params"][0]["lower"] == -INF and spec["params"][0]["upper"] == INF


def _r_invalid(spec):
    x = spec["data"]["x"]
    assert int(((x != 0.0) & (x != 1.0)).sum()) == 1      # has_invalid


def bern_cases():
    x = np.array(model_spec.make_data("beta_bern", 300, 31)["x"], dtype=np.float64)
    assert 0 < x.sum() < 300
    c = []
    add = lambda name, spec, kind, reaches: c.append({"name": name, "family": "beta_bern", "spec": spec, "kind": kind, "reaches": reaches, "components": None})
    add("theta_init_0", bern_spec(x, 0.0), "alive", _r_theta_at(0.0))
    add("theta_init_1", bern_spec(x, 1.0), "alive", _r_theta_at(1.0))
    add("all_ones", bern_spec(np.ones(300)), "alive", _r_all(1.0))
    add("all_zeros_flat_prior", bern_spec(np.zeros(300), hyper=[1.0, 1.0]), "alive", _r_all(0.0, [1.0, 1.0]))
    add("hyper_half_half", bern_spec(x, hyper=[0.5, 0.5]), "alive", _r_hyper)
    add("theta_unbounded", bern_spec(x, lower=-INF, upper=INF), "alive", _r_theta_unbounded)
    add("invalid_2.0", bern_spec(_with(x, 17, 2.0)), "stuck", _r_invalid)
    add("invalid_0.5", bern_spec(_with(x, 17, 0.5)), "stuck", _r_invalid)
    return c


# ---- Poisson GLM with a change point, n = 300, data seed 123
def pois_data():
    import oracle_lib
    d = model_spec.make_data("pois_glm", 300, 123, exp=oracle_lib.lib().orc_exp)
    return {"x": np.array(d["x"], dtype=np.float64), "y": np.array(d["y"], dtype=np.float64), "K": d["K"]}


def _r_eta_large(spec):
    X = spec["data"]["x"].reshape(300, -1)
    assert np.abs(X[:, 1:]).max() > 100.0      # |eta| passes 690 and 709 for betas of a few units: proposals at the default scale reach them


def _r_zero_rows(spec):
    X, y = spec["data"]["x"].reshape(300, -1), spec["data"]["y"]
    assert int((y == 0).sum()) > 20 and np.all(X[y == 0, 1:] >= 0.0) and X[y == 0, 1:].max() > 745.0 and np.abs(X[y != 0, 1:]).max() < 5.0
    # a beta of -1 puts an eta of a zero-count row below -745.2: exp_v8 gives 0, and the expression 0 * log(0) = NaN, where e^eta y - e^eta is an ordinary 0


def _r_y3(v):
    def r(spec):
        y = spec["data"]["y"]
        assert (y[3] == v) and np.all(np.delete(y, 3) >= 0) and np.all(np.delete(y, 3) == np.round(np.delete(y, 3)))
    return r


def _r_all_zero(spec):
    assert np.all(spec["data"]["y"] == 0.0)


def pois_cases():
    d = pois_data()
    mk = lambda **kw: model_spec.build_spec("pois_glm", dict(d, **kw))
    c = []
    add = lambda name, spec, kind, reaches, components=None: c.append({"name": name, "family": "pois_glm", "spec": spec, "kind": kind, "reaches": reaches, "components": components})
    add("X_times_150", mk(x=d["x"] * 150.0), "alive_any", _r_eta_large)
    # (every eta of a row with a positive count stays small; only rows whose count is 0 can leave the range, and only downwards for negative betas: no e^eta
    # overflows there, so nothing but the H > 690 guard makes eps non-finite)
    Z = d["x"].reshape(300, -1).copy()
    Z[d["y"] == 0, 1:] = np.abs(Z[d["y"] == 0, 1:]) * 600.0
    add("zero_count_rows_times_600", mk(x=Z.reshape(-1)), "alive", _r_zero_rows)
    add("negative_count", mk(y=_with(d["y"], 3, -1.0)), "stuck", _r_y3(-1.0))
    add("non_integer_count", mk(y=_with(d["y"], 3, 2.5)), "alive", _r_y3(2.5))
    add("count_1e6", mk(y=_with(d["y"], 3, 1e6)), "alive", _r_y3(1e6))
    # (all counts zero: the betas run to -20, every e^eta to 0, and log_post no longer depends on the change point -- the oracle accepts EVERY proposal of it,
    # 299 of 299 in 300 steps on both chains; the condition is asked of the eight betas)
    add("all_counts_zero", mk(y=np.zeros(300)), "alive", _r_all_zero, components=list(range(8)))
    return c


# ---- hierarchical Normal, n = 640, G = 8
def hier_spec(y, g, G, theta, mu, sigma, hyper, scales):
    P_ = lambda ln, lower, init: {"type": "real", "len": ln, "top": ln, "multidim": int(ln != 1), "lower": lower, "upper": INF, "init": [float(init)] * ln}
    params = [P_(G, -INF, theta), P_(1, -INF, mu), P_(1, 0.0, sigma)]
    return model_spec.build_spec("hier_normal", {"x": np.array(y, dtype=np.float64), "g": g, "G": G}, params=params, comp_opts=_opts(scales), G=G, hyper=hyper)


def _r_hier_one_out(spec):
    x = spec["data"]["x"]
    assert not data_mid_range(x) and int((~mid_range(np.abs(x))).sum()) == 1 and np.isfinite(x * x).all()


def _r_hier_outside(spec):
    h = spec["hyper"]
    assert not (h[2] <= spec["init"][-1] <= h[3]) and data_mid_range(spec["data"]["x"])


def hier_cases():
    d = model_spec.make_data("hier_normal", 640, 77, G=8)
    y, g = np.array(d["x"], dtype=np.float64), d["g"]
    c = []
    add = lambda name, spec, kind, reaches: c.append({"name": name, "family": "hier_normal", "spec": spec, "kind": kind, "reaches": reaches, "components": None})
    add("one_out_of_mid_range", hier_spec(_with(y, 5, 1e70), g, 8, 1e68, 1e68, 1e69, [0.0, 1e80, 0.0, 1e80, 1e69], [156] * 8 + [159, 158]), "alive", _r_hier_one_out)
    add("outside_support", hier_spec(y, g, 8, 0.5, 0.5, 1.0, [0.0, 100.0, 1.5, 3.0, 10.0], [0] * 10), "alive", _r_hier_outside)
    return c


FAMILIES = {"normal": normal_cases, "beta_bern": bern_cases, "pois_glm": pois_cases, "hier_normal": hier_cases}
EXPECTED = {
    "normal": ["a_one_out_of_mid_range", "b_scale_1e-40", "b_scale_1e-155", "c_scale_1e40", "d_offset_1e15", "e_scale_1e-40_default_scale", "e_scale_1e40_default_scale",
               "e_offset_1e15_default_scale", "f_outside_support", "g_sigma_unbounded", "h_int_mu_zero", "h_int_mu_constant_data", "i_nan", "i_inf", "i_1e250",
               "a_2049_observations"],
    "beta_bern": ["theta_init_0", "theta_init_1", "all_ones", "all_zeros_flat_prior", "hyper_half_half", "theta_unbounded", "invalid_2.0", "invalid_0.5"],
    "pois_glm": ["X_times_150", "zero_count_rows_times_600", "negative_count", "non_integer_count", "count_1e6", "all_counts_zero"],
    "hier_normal": ["one_out_of_mid_range", "outside_support"],
}
_cache = {}


def cases(family):
    if family not in _cache:
        _cache[family] = FAMILIES[family]()
    return _cache[family]


def case(family, name):
    return {c["name"]: c for c in cases(family)}[name]


# ---- the schedule, on the oracle and on a sampler, and the comparison
DOUBLES = ("draws1", "draws2", "state", "prop_log_scale")      # compared as bytes (-0.0 is not +0.0)
MAYBE_NAN = ("log_post0", "log_post1", "log_post2")      # both NaN, or the same bits


def oracle_record(spec, chain, lanes=1, group_local=False):
    import oracle_lib
    o = oracle_lib.OracleChain(spec, SEED, chain, lanes=lanes, group_local=group_local)
    lp0 = o.log_post()
    o.burn(BURN)
    d1 = o.sample(N1, THIN)
    lp1, or1, un1 = o.log_post(), o.named_order().copy(), o.uniforms()
    d2 = o.sample(N2, 1)
    out = {"draws1": d1, "draws2": d2, "state": o.state(), "log_post0": lp0, "log_post1": lp1, "log_post2": o.log_post(), "order1": or1, "order2": o.named_order().copy(),
           "uniforms1": un1, "uniforms2": o.uniforms()}
    out.update(o.info())
    return out


def sampler_record(s):
    g0 = s.diag()      # straight after construction: log_post after zero steps
    s.burn(BURN)
    d1 = s.sample(N1, THIN)
    g1 = s.diag()
    d2 = s.sample(N2, 1)
    g2 = s.diag()
    out = {"draws1": d1, "draws2": d2, "state": s.state(), "log_post0": g0["log_post"], "log_post1": g1["log_post"], "log_post2": g2["log_post"], "order1": g1["named_order"],
           "order2": g2["named_order"], "uniforms1": g1["uniforms"], "uniforms2": g2["uniforms"]}
    out.update(s.info())
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def same(key, a, b):
    """a, b: the same entry of two records.  Doubles as bits -- for log_post: both NaN, or the same bits --, everything else as integers."""
    if key in DOUBLES or key in MAYBE_NAN:
        x, y = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
        if x.shape != y.shape:
            return False
        eq = x.view(np.uint64) == y.view(np.uint64)
        if key in MAYBE_NAN:
            eq = eq | (np.isnan(x) & np.isnan(y))
        return bool(eq.all())
    x, y = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return x.shape == y.shape and bool((x == y).all())


def chain_of(rec, key, local):
    """what a sampler's record holds for its chain `local`, in the oracle's shapes"""
    v = rec[key]
    if key.startswith("draws"):
        return v[:, :, local]
    if key.startswith("order"):
        return v[local]
    return v[:, local] if v.ndim == 2 else v[local]


def differences(got, want):
    """two samplers' records over all chains -> the entries that differ"""
    return [k for k in want if not same(k, got[k], want[k])]


def differences_from_oracle(got, want, local):
    return ["oracle chain %d: %s" % (local, k) for k, w in want.items() if not same(k, chain_of(got, k, local), w)]


def adapting(spec):
    return [i for i, o in enumerate(spec["comp_opts"]) if o["is_adapting"]]


def kind_holds(kind, records, spec, components=None):
    """records: a list of per-chain info (oracle records, or chain_of slices) -> None, or what is wrong"""
    comps = adapting(spec) if components is None else components
    acc = np.array([[int(np.asarray(r["accepts"])[i]) for i in comps] for r in records])
    inb = np.array([[int(np.asarray(r["inbounds"])[i]) for i in comps] for r in records])
    if kind == "alive":
        ok = (acc > 0).all() and (acc < inb).all()
    elif kind == "alive_any":
        ok = acc.sum() > 0 and acc.sum() < inb.sum()
    elif kind == "stuck":
        ok = (acc == 0).all() and (inb > 0).any()
    elif kind == "frozen":
        ok = (acc == inb).all() and (inb > 0).all()
    else:
        raise ValueError(kind)
    return None if ok else "%s does not hold: accepts %s inbounds %s" % (kind, acc.tolist(), inb.tolist())
