"""TEST INFRASTRUCTURE (numpy only): one set of cases for the K-valued exact fast-forward of csrc/amwg_kval.h (k_valued_sum<K>), used by its host twin
(tests/test_kval_host.py, the header compiled with g++) and on the device (tests/test_gpu_kval.py, amwg_k_valued_sum_check).  README.kval.md has the tables.

Three things live here, none of which reads the code under test:
  * tables():    the data-only tables, restated from the header's comment;
  * plain_sum(): the sequential sum acc = acc + c[idx[i]], observation after observation, vectorised over the lanes (NOT np.sum: that is pairwise) -- the reference;
  * census():    which branches of the header a lane's plain sum would ask for, by the definitions of the header's comment (ulp of the binade, d_k, ties), so that
                 the tests cannot pass by never arriving."""
import numpy as np

SHAPES = [(0, 2), (1, 1), (31, 2), (32, 3), (33, 2), (64, 3), (777, 3), (777, 5), (4099, 13), (5000, 8), (20000, 16)]
INSTANTIATED = (1, 2, 3, 5, 8, 13, 16)      # the K of amwg_k_valued_sum_check (13: what pois_const_rate compiles)
KINDS = ("iid_skewed", "runs", "one_value", "absent_value", "block_edges")
M = 2048
COPIES_SHAPE, COPY_OF = (4099, 13), 203      # lanes 0 .. 63 of this shape are 64 copies of lane COPY_OF: a wavefront in uniform control flow
STALL = slice(64, 128)                       # acc0 = -2^(40 .. 84)
FALLBACK_ADDENDS = (-np.inf, np.nan, 0.25, 0.0, -5e-324, -1e-310)      # lanes 128 .. 133: summed term by term by the header
FALLBACK0, POWERS_LANE, ACC0_FIXED0 = 128, 134, 136
ACC0_FIXED = (0.0, -0.0, 1e300, -1e300)      # lanes 136 .. 139
LANDING = slice(140, 172)                    # sums that land EXACTLY on a power of two, at or beside a block boundary (see lanes())
LANDING_AT = (32, 64, 33, 31, 1, 96, 1000, 10 ** 9, -1, 2048, 160, 7, 4096, 640, 63, 65)      # after how many observations (clipped to n; -1: n - 1)
ORDINARY0 = 172                              # from here on every lane is a random one
RUN_LENGTHS = (1, 3, 7, 31, 33, 45, 63, 65, 97, 130)      # none a multiple of 32

U64 = np.uint64
MANT, HIDDEN = U64(0x000FFFFFFFFFFFFF), U64(0x0010000000000000)


def words(n):
    return n // 32 + 2


def tables(idx, K):
    """The header's recipe: W = n // 32 + 2 blocks; block w holds pre[K] (how often every value occurs among the observations [0, 32 w)) and then mask[K]
    (bit j of mask[k]: observation 32 w + j has value k) -> uint32 [2 K W]"""
    idx = np.asarray(idx, dtype=np.uint8)
    n, W = idx.size, words(idx.size)
    t = np.zeros((W, 2 * K), dtype=np.uint64)
    i = np.arange(n)
    np.add.at(t, (i >> 5, K + idx.astype(np.int64)), U64(1) << (i & 31).astype(np.uint64))      # (every bit is set once: the sum is the OR)
    counts = np.zeros((W, K), dtype=np.uint64)
    np.add.at(counts, (i >> 5, idx.astype(np.int64)), U64(1))
    t[1:, :K] = np.cumsum(counts, axis=0)[:-1]
    return t.astype(np.uint32).reshape(-1)


def _qualifying_exponent(acc, emax):
    """the biased exponent of acc where the header may fast-forward (acc < 0, finite, exponent >= the largest addend's + 1), else 0; emax = 0x7ff marks a lane
    whose addends send it term by term"""
    b = (-acc).view(np.uint64)
    e = (b >> U64(52)).astype(np.int64)      # includes the sign bit of -acc: > 0x7ff when acc > 0
    return np.where((e >= emax + 1) & (e < 0x7FF), e, 0).astype(np.uint16)


def addend_parts(c):
    """c [m][K] -> (ok [m]: every addend negative, finite and normal; ek [m][K] biased exponents; mk [m][K] significands with the hidden bit)"""
    b = (-c).view(np.uint64)
    ek = (b >> U64(52)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = ((c < 0) & (ek > 0) & (ek < 0x7FF)).all(axis=1)
    return ok, ek, (b & MANT) | HIDDEN


def plain_sum(idx, acc0, c, record=False):
    """acc[j] = (...((acc0[j] + c[j][idx[0]]) + c[j][idx[1]]) ...), one IEEE addition per observation -> acc [m]; with record also E [n][m] uint16: the
    qualifying exponent (see above) of the sum each observation is added to"""
    c = np.ascontiguousarray(c, dtype=np.float64)
    ct = np.ascontiguousarray(c.T)
    acc = np.array(acc0, dtype=np.float64)
    E = None
    if record:
        ok, ek, _ = addend_parts(c)
        emax = np.where(ok, ek.max(axis=1), 0x7FF)
        E = np.zeros((len(idx), acc.size), dtype=np.uint16)
    with np.errstate(all="ignore"):
        for i, v in enumerate(np.asarray(idx).tolist()):
            if record:
                E[i] = _qualifying_exponent(acc, emax)
            acc = acc + ct[v]
    return (acc, E) if record else acc


LANE_FLAGS = ("one_tie_ge64", "one_tie_32_63", "one_tie_lt32", "several_ties", "tie_free", "stalled", "partial_zero", "starts_nonneg", "fallback")


def census(idx, acc0, c):
    """-> (final sums [m], dict of bool arrays [m] named in LANE_FLAGS, set of the kinds of fallback addends met).
    A visit is a maximal run of observations added to a sum of one qualifying exponent e.  In it the ulp is 2^(e - 1075) and addend k of exponent ek, significand mk
    moves the significand by d_k = mk >> s rounded to nearest, s = e - ek (0 from s = 54 on); it TIES when its remainder mk mod 2^s is exactly 2^(s - 1).
    Classes of a visit: no tie and some d_k != 0 (fast-forwarded by bisection); exactly one tying addend (walked by blocks), by its length in observations; two or
    more (term by term); no tie and every d_k = 0 (stalled).  partial_zero: a visit with some but not all d_k = 0, whatever its class."""
    c = np.ascontiguousarray(c, dtype=np.float64)
    acc0 = np.asarray(acc0, dtype=np.float64)
    m, K = c.shape
    n = len(idx)
    acc, E = plain_sum(idx, acc0, c, record=True)
    ok, ek, mk = addend_parts(c)
    flags = {k: np.zeros(m, dtype=bool) for k in LANE_FLAGS}
    with np.errstate(invalid="ignore"):
        flags["starts_nonneg"] = ~np.signbit(acc0) & ~np.isnan(acc0)
    flags["fallback"] = ~ok
    kinds = set()
    bad = c[~ok]
    with np.errstate(invalid="ignore"):
        for name, hit in (("-inf", bad == -np.inf), ("nan", np.isnan(bad)), ("positive", bad > 0), ("zero", bad == 0), ("subnormal", (bad < 0) & (bad > -2.2250738585072014e-308))):
            if hit.any():
                kinds.add(name)
    if n == 0:
        return acc, flags, kinds
    Et = np.ascontiguousarray(E.T)
    start = np.ones((m, n), dtype=bool)
    start[:, 1:] = Et[:, 1:] != Et[:, :-1]
    lane, pos = np.nonzero(start)
    flat = lane * n + pos
    length = np.append(flat[1:], m * n) - flat      # (every lane starts a run at observation 0: the next start, in this lane or the next, ends this one)
    e = Et[lane, pos].astype(np.int64)
    keep = e != 0
    lane, length, e = lane[keep], length[keep], e[keep]
    s = e[:, None] - ek[lane]                        # >= 1
    far = s >= 54
    sc = np.minimum(s, 53).astype(np.uint64)
    mkv = mk[lane]
    r = mkv & ((U64(1) << sc) - U64(1))
    h = U64(1) << (sc - U64(1))
    tie = ~far & (r == h)
    d = np.where(far, U64(0), (mkv >> sc) + (r > h).astype(np.uint64))
    n_tie, zero = tie.sum(axis=1), (d == 0)
    all_zero, some_zero = zero.all(axis=1), zero.any(axis=1)
    mark = lambda name, sel: flags[name].__setitem__(lane[sel], True)
    mark("one_tie_ge64", (n_tie == 1) & (length >= 64))
    mark("one_tie_32_63", (n_tie == 1) & (length >= 32) & (length < 64))
    mark("one_tie_lt32", (n_tie == 1) & (length < 32))
    mark("several_ties", n_tie >= 2)
    mark("tie_free", (n_tie == 0) & ~all_zero)
    mark("stalled", (n_tie == 0) & all_zero)
    mark("partial_zero", some_zero & ~all_zero)
    return acc, flags, kinds


def _trail(x, z, setbit):
    """clears the z lowest significand bits of x and, where setbit, sets bit z: such an addend ties in the binade whose ulp is 2^(z + 1) of its own"""
    u = x.view(np.uint64).copy()
    zz = z.astype(np.uint64)
    u = ((u >> zz) << zz) | ((U64(1) << zz) * setbit.astype(np.uint64))
    return u.view(np.float64).copy()


def sequence(n, K, kind, rng):
    """-> idx [n] uint8, every entry < K"""
    p = 0.6 ** np.arange(K)
    p /= p.sum()
    iid = lambda vals, size: rng.choice(np.asarray(vals), size=size, p=p[: len(vals)] / p[: len(vals)].sum())
    if kind == "iid_skewed":
        x = iid(np.arange(K), n)
    elif kind == "runs":
        x = np.empty(0, dtype=np.int64)
        while x.size < n:
            x = np.append(x, np.full(rng.choice(RUN_LENGTHS), rng.integers(0, K)))
        x = x[:n]
    elif kind == "one_value":
        x = np.full(n, K - 1)
    elif kind == "absent_value":      # value 0 never occurs (K >= 2)
        x = iid(np.arange(1, K), n)
    elif kind == "block_edges":       # value 0 at the first and the last observation of a block only (K >= 2), in two blocks of three
        x = iid(np.arange(1, K), n)
        i = np.arange(n)
        x[((i & 31) == 0) | ((i & 31) == 31)] = 0
        x[(i >> 5) % 3 == 2] = np.where(x[(i >> 5) % 3 == 2] == 0, 1, x[(i >> 5) % 3 == 2])
    else:
        raise ValueError(kind)
    return x.astype(np.uint8)


def _landing_lanes(idx, K, acc0, c):
    """Lanes whose sum reaches a power of two EXACTLY after p observations: the binade [2^53, 2^54) has ulp 2, the addends are -2, -4, -6 (d = 1, 2, 3 by value index)
    and the start is -(2^54 - 2 G), G = the growth of the significand over the first p observations.  Even lanes: no tie, the bisection must stop one short of p
    (growth == limit is not < limit).  Odd lanes (K >= 2): the last value's addend is -1, half an ulp, a tie that rounds up iff the significand is odd -- the
    block walk must leave a block whose end would be 2^54.  G is followed in integers for either starting parity; the start must have the parity it was followed
    with (if neither has, the lane keeps the tie-free addends)."""
    n = len(idx)
    d = np.arange(K) % 3 + 1
    seq = np.asarray(idx).tolist()
    free = np.concatenate([[0], np.cumsum(d[np.asarray(idx, dtype=np.int64)])]) if n else np.zeros(1, dtype=np.int64)
    tied = []
    for parity in (0, 1):
        a, g, out = parity, 0, [0]
        for v in seq:
            inc = (a & 1) if v == K - 1 else int(d[v])
            g += inc
            a = (a + inc) & 1
            out.append(g)
        tied.append(out)
    for q, lane in enumerate(range(LANDING.start, LANDING.stop)):
        at = LANDING_AT[(q // 2) % len(LANDING_AT)]
        p = max(0, min(n, n - 1 if at < 0 else at))
        c[lane] = -2.0 * d
        G = int(free[p])
        if q % 2 == 1 and K >= 2:
            ok = [par for par in (0, 1) if tied[par][p] % 2 == par]
            if ok:
                c[lane, K - 1], G = -1.0, tied[ok[0]][p]
        acc0[lane] = -(2.0 ** 54 - 2.0 * G) if G else -2.0 ** 53


def lanes(idx, K, kind, rng, m=M):
    """-> (acc0 [m], c [m][K]) as the module docstring of tests/test_gpu_kval.py lists them"""
    n = len(idx)
    j = np.arange(m)
    c = -np.exp(rng.uniform(-12, 3, (m, K)))
    wide = j % 8 == 2
    c[wide] = -np.exp(rng.uniform(-80, 3, (int(wide.sum()), K)))      # some d_k are 0 in a binade where others are not
    setbit = rng.integers(0, 2, (m, K)).astype(bool)
    if kind == "block_edges":
        setbit[:, 0] = True                                           # value 0 is the would-be tying one
    # z < 40 trailing zero bits, small z more often (z = 40 u^2): the binades right above an addend are short, and it is there that a one-tie visit of less than a
    # block happens (uniform z left the n = 777, K = 3 shape at 9.9 % of such lanes where the census asks for 10 %)
    c = _trail(c, np.floor(40 * rng.uniform(size=(m, K)) ** 2).astype(np.int64), setbit)
    mult = j % 8 == 1
    c[mult] = c[mult, :1] * np.arange(1, K + 1)                       # c, 2c, 3c, ...: a log-linear family, exact multiples tie together
    if kind == "one_value":                                           # the one value that occurs carries the lane's largest addend: the sum climbs above every addend
        big = np.abs(c).argmax(axis=1)
        c[j, big], c[:, K - 1] = c[:, K - 1].copy(), c[j, big].copy()
    acc0 = np.where(rng.uniform(size=m) < 0.5, rng.normal(0, 3, m), -np.exp(rng.uniform(-5, 25, m)))
    acc0[STALL] = -np.ldexp(1.0, 40 + (j[STALL] - STALL.start) % 45)
    for q, v in enumerate(FALLBACK_ADDENDS):
        c[FALLBACK0 + q, (FALLBACK0 + q) % K] = v
    c[POWERS_LANE, 0], c[POWERS_LANE, K - 1] = -1.0, (-0.5 if K > 1 else -1.0)
    acc0[ACC0_FIXED0:ACC0_FIXED0 + 4] = ACC0_FIXED
    _landing_lanes(idx, K, acc0, c)
    if (n, K) == COPIES_SHAPE:
        c[:64], acc0[:64] = c[COPY_OF], acc0[COPY_OF]
    return acc0, c


def case_list():
    return [(n, K, kind) for n, K in SHAPES for kind in KINDS if K > 1 or kind in KINDS[:3]]


_built = {}


def case(n, K, kind):
    """-> dict(n, K, kind, idx, tab, acc0, c, want: the plain sums, flags, kinds); computed once and shared (nobody may write to the arrays)"""
    key = (n, K, kind)
    if key not in _built:
        rng = np.random.default_rng([11, n, K, KINDS.index(kind)])
        idx = sequence(n, K, kind, rng)
        acc0, c = lanes(idx, K, kind, rng)
        want, flags, kinds = census(idx, acc0, c)
        d = dict(n=n, K=K, kind=kind, idx=idx, tab=tables(idx, K), acc0=acc0, c=c, want=want, flags=flags, kinds=kinds)
        for a in (idx, d["tab"], acc0, c, want) + tuple(flags.values()):
            a.setflags(write=False)
        _built[key] = d
    return _built[key]


def same_bits(a, b):
    """the same bits, or both NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def shape_share(n, K, flag):
    """the share of the lanes of every case of a shape (all its sequences together) with a flag"""
    f = np.concatenate([case(n, K, kind)["flags"][flag] for (nn, KK, kind) in case_list() if (nn, KK) == (n, K)])
    return float(f.mean())


def suite_count(flag):
    return int(sum(case(*k)["flags"][flag].sum() for k in case_list()))


# the census conditions (conditions on the INPUTS; if one fails, the inputs change, not the condition)
SHARE_MIN = {"one_tie_ge64": 0.10, "one_tie_lt32": 0.10, "several_ties": 0.01, "tie_free": 0.80}      # over every shape with n >= 777
SUITE_MIN = {"stalled": 100, "partial_zero": 100, "starts_nonneg": 100}
FALLBACK_KINDS = {"-inf", "nan", "positive", "zero", "subnormal"}


def census_table():
    rows = ["| n | K | " + " | ".join(LANE_FLAGS) + " |", "|---|---|" + "---|" * len(LANE_FLAGS)]
    for n, K in SHAPES:
        rows.append("| %d | %d | " % (n, K) + " | ".join("%.1f %%" % (100 * shape_share(n, K, f)) for f in LANE_FLAGS) + " |")
    rows.append("| suite (lanes) | | " + " | ".join(str(suite_count(f)) for f in LANE_FLAGS) + " |")
    return "\n".join(rows)


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(census_table())
    print("fallback addends met:", sorted(set().union(*[case(*k)["kinds"] for k in case_list()])))
    print("%d cases, %.1f s" % (len(case_list()), time.time() - t0))
