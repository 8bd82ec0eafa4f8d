"""TEST INFRASTRUCTURE (numpy only): one set of cases for the two-valued exact fast-forward of csrc/amwg_twoval.h (two_valued_sum), used by its host twin
(tests/test_twoval_host.py, the header compiled with g++), on the device (tests/test_gpu_twoval.py, amwg_two_valued_sum_check) and by tools/twoval_mutations.py.
README.twoval.md has the tables.

Four things live here, none of which reads the code under test:
  * tables():    the six data-only tables, restated from the header's comment;
  * plain_sum(): the sequential sum acc = acc + (x[i] ? l1 : l0), observation after observation, vectorised over the lanes (NOT np.sum: that is pairwise) -- the
                 reference;
  * the cases:   per shape and sequence 2 048 lanes, most of them CONSTRUCTED for a class of binade visit (lanes());
  * census():    which branches of the header a lane's plain sum would ask for, by the definitions of the header's comment (ulp of the binade, q, d, ties, the
                 parity of the other increment, the odd-run marks), so that the tests cannot pass by never arriving."""
import numpy as np

SHAPES = [0, 1, 31, 32, 33, 63, 64, 65, 777, 4099, 8192, 20000]
KINDS = ("iid_50", "iid_02", "iid_97", "runs", "runs_32k", "alternating", "period3_one", "period3_zero", "period4_one", "period4_zero", "period5_one", "period5_zero",
         "period6_one", "period6_zero", "all_ones", "all_zeros", "sparse_ones", "sparse_zeros")
SPARSE_AT = (0, 31, 32, -1)                  # sparse_ones: zeros except at these observations (-1: n - 1); sparse_zeros: the complement
M = 2048
# the lanes of every case, by range (lanes() and the docstring of tests/test_gpu_twoval.py)
STALL = slice(64, 128)                       # acc0 = -2^(40 .. 84)
FALLBACK_ADDENDS = (-np.inf, np.nan, 0.25, 0.0, -0.0, -5e-324, -1e-310)      # summed term by term by the header: lanes 128 .. 134 as l1, 135 .. 141 as l0
FALLBACK0 = 128
EQUAL = slice(142, 148)                      # l0 = l1
RATIO = slice(148, 154)                      # l0 = l1 * 2^(+-1 .. 3)
POWERS = slice(154, 160)                     # both addends powers of two
ACC0_FIXED0, ACC0_FIXED = 160, (0.0, -0.0, 1e300, -1e300)      # lanes 160 .. 163
BELOW_POW2 = slice(164, 196)                 # starts 1 .. 4 ulps below a power of two
LANDING = slice(196, 260)                    # sums that land EXACTLY on a power of two (see _landing_lanes)
LANDING_AT = (32, 64, 33, 31, 1, 96, 1000, 10 ** 9, -1, 2048, 160, 7, 4096, 640, 63, 65)      # after how many observations (clipped to n; -1: n - 1)
SATURATION = slice(260, 268)                 # n * d wraps 2^64 (see _saturation_lanes)
HALF_ULP = slice(268, 292)                   # an addend of exactly half an ulp (q = 0) on a sum that otherwise stalls
CONSTRUCTED = slice(292, 1316)               # built for mode 1, 2 or 3 with a visit of >= 64 observations (see _constructed_lanes)
RUN_MAX = 130

U64 = np.uint64
MANT, HIDDEN, SIGN = U64(0x000FFFFFFFFFFFFF), U64(0x0010000000000000), U64(0x8000000000000000)


def words(n):
    return n // 32 + 2


# ---- the tables, restated from the header's comment

def odd_marks(x, sym):
    """bool [n]: observation i has the value sym and the run of the OTHER value right in front of it (back to the previous sym, or to the start) has odd length"""
    x = np.asarray(x, dtype=np.uint8)
    at = np.flatnonzero(x == sym)
    out = np.zeros(x.size, dtype=bool)
    if at.size:
        run = at - np.concatenate([[-1], at[:-1]]) - 1
        out[at[run % 2 == 1]] = True
    return out


def _pack(bits, W):
    """bool [n] -> (uint32 [W]: observation i = bit (i & 31) of word i >> 5; uint32 [W]: how many are set in the words before)"""
    b = np.zeros(W * 32, dtype=np.uint8)
    b[:bits.size] = bits
    b = b.reshape(W, 32)
    w = (b.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    before = np.concatenate([[0], np.cumsum(b.sum(axis=1))[:-1]])
    return w.astype(np.uint32), before.astype(np.uint32)


def tables(x):
    """-> (w, pre, om1, po1, om0, po0), each uint32 [n // 32 + 2]: the observations as bits, the ones before every word, and for each value the marks of its
    occurrences after an odd run of the other value with their counts before every word"""
    x = np.asarray(x, dtype=np.uint8)
    W = words(x.size)
    w, pre = _pack(x == 1, W)
    om1, po1 = _pack(odd_marks(x, 1), W)
    om0, po0 = _pack(odd_marks(x, 0), W)
    return w, pre, om1, po1, om0, po0


def tables_flat(x):
    """the six back to back, as the library, the translator and the host build take them"""
    return np.concatenate(tables(x))


# ---- the plain sum

def plain_sum(x, acc0, l1, l0, snaps=()):
    """acc[j] = (...((acc0[j] + t_0) + t_1) ...), t_i = l1[j] where x[i] = 1 and l0[j] where it is 0, one IEEE addition per observation -> acc [m]; with snaps
    (numbers of observations) -> (acc, {p: the sums after the first p observations})"""
    lt = np.ascontiguousarray(np.stack([np.asarray(l0, dtype=np.float64), np.asarray(l1, dtype=np.float64)]))
    acc = np.array(acc0, dtype=np.float64)
    want, got = set(snaps), {}
    with np.errstate(all="ignore"):
        for i, v in enumerate(np.asarray(x).tolist()):
            if i in want:
                got[i] = acc.copy()
            acc = acc + lt[v]
    if len(x) in want:
        got[len(x)] = acc.copy()
    return (acc, got) if snaps else acc


def follow(x, acc0, l1, l0):
    """plain_sum that also says where the sign-and-exponent field of the sum changed -> (acc [m], lane [v], pos [v], bits [v]): observation pos of lane is added
    to a sum (whose bits are given) of another sign or exponent than the observation before it was; every lane has pos = 0.  Sorted by lane, then pos."""
    lt = np.ascontiguousarray(np.stack([np.asarray(l0, dtype=np.float64), np.asarray(l1, dtype=np.float64)]))
    acc = np.array(acc0, dtype=np.float64)
    bits = acc.view(np.uint64)
    m = acc.size
    top, prev, ch = np.empty(m, dtype=np.uint64), np.full(m, 0xFFFF, dtype=np.uint64), np.empty(m, dtype=bool)
    lanes_, pos_, bits_ = [], [], []
    with np.errstate(all="ignore"):
        for i, v in enumerate(np.asarray(x).tolist()):
            np.right_shift(bits, U64(52), out=top)
            np.not_equal(top, prev, out=ch)
            if ch.any():
                k = np.flatnonzero(ch)
                lanes_.append(k)
                pos_.append(np.full(k.size, i, dtype=np.int64))
                bits_.append(bits[k])
            prev, top = top, prev
            np.add(acc, lt[v], out=acc)
    if not lanes_:
        return acc, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64)
    lane, pos, b = np.concatenate(lanes_), np.concatenate(pos_), np.concatenate(bits_)
    o = np.argsort(lane, kind="stable")
    return acc, lane[o], pos[o], b[o]


# ---- the census

MODE_FLAGS = tuple("mode%d_%s" % (k, ln) for k in range(4) for ln in ("lt32", "32_63", "ge64"))
LANE_FLAGS = MODE_FLAGS + ("mode3_absent", "mode3_first_at_start", "mode3_odd_and_even", "mode3_two_boundaries", "mode2_no_tying_symbol", "tie_free", "stalled",
                           "half_ulp_tie_odd", "half_ulp_tie_even", "one_increment_zero", "landing", "starts_nonneg", "fallback")


def addend_parts(c):
    """c [m] -> (ok: negative, finite and normal; biased exponent; significand with the hidden bit)"""
    b = (-np.asarray(c, dtype=np.float64)).view(np.uint64)
    e = (b >> U64(52)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = (c < 0) & (e > 0) & (e < 0x7FF)
    return ok, e, (b & MANT) | HIDDEN


def _rounding(e, ec, mc):
    """in the binade of biased exponent e (ulp 2^(e - 1075)) the addend of exponent ec, significand mc is (q + r / 2^s) ulps, s = e - ec >= 1: -> (q, d = q rounded
    up where r is above half, tie: r exactly half); all 0 / False from s = 54 on"""
    s = e - ec
    far = s >= 54
    sc = np.clip(s, 1, 53).astype(np.uint64)
    r = mc & ((U64(1) << sc) - U64(1))
    h = U64(1) << (sc - U64(1))
    q = np.where(far, U64(0), mc >> sc)
    return q, np.where(far, U64(0), q + (r > h).astype(np.uint64)), ~far & (r == h)


def census(x, acc0, l1, l0):
    """-> (final sums [m], dict of bool arrays [m] named in LANE_FLAGS, set of the kinds of fallback addends met).
    A visit is a maximal run of observations [i, end) added to a sum of one sign and exponent e; it counts where the header may fast-forward: acc < 0, finite,
    e >= the larger addend's + 1.  In it addend c moves the significand A by d_c (see _rounding) unless it TIES.  Mode 0: no tie; 1: both tie; one ties (value t,
    the other value's d_n): 2 where d_n is even, 3 where it is odd.  Every mode by the visit's length in observations, and
      mode3_absent            no t among the observations from i to the END OF THE DATA           mode3_first_at_start    x[i] = t
      mode3_odd_and_even      behind the first t of [i, end) the visit holds a t after an odd run of the other value and one after an even run (the marks)
      mode3_two_boundaries    the visit crosses two 32-observation word boundaries or more         mode2_no_tying_symbol   no t in [i, end)
      tie_free                mode 0 and some d != 0 (fast-forwarded by the plain bisection)      stalled                 mode 0 and both d = 0
      half_ulp_tie_odd/_even  a tying addend with q = 0 (exactly half an ulp), by the parity of A at the start of the visit
      one_increment_zero      one d is 0 and the other is not (a tying addend's d is its q)
      landing                 a sum reached by an addition is exactly a negative power of two"""
    x = np.asarray(x, dtype=np.uint8)
    acc0, l1, l0 = (np.ascontiguousarray(v, dtype=np.float64) for v in (acc0, l1, l0))
    m, n = acc0.size, x.size
    acc, lane, pos, b = follow(x, acc0, l1, l0)
    ok1, e1, m1 = addend_parts(l1)
    ok0, e0, m0 = addend_parts(l0)
    ok = ok1 & ok0
    flags = {k: np.zeros(m, dtype=bool) for k in LANE_FLAGS}
    with np.errstate(invalid="ignore"):
        flags["starts_nonneg"] = ~np.signbit(acc0) & ~np.isnan(acc0)
    flags["fallback"] = ~ok
    kinds = set()
    bad = np.concatenate([l1[~ok1], l0[~ok0]])
    with np.errstate(invalid="ignore"):
        for name, hit in (("-inf", bad == -np.inf), ("nan", np.isnan(bad)), ("positive", bad > 0), ("zero", bad == 0), ("subnormal", (bad < 0) & (bad > -2.2250738585072014e-308))):
            if hit.any():
                kinds.add(name)
    if n == 0:
        return acc, flags, kinds
    end = np.where(np.append(lane[1:], -1) == lane, np.append(pos[1:], n), n)
    ab = b ^ SIGN                                   # the bits of -acc
    e = (ab >> U64(52)).astype(np.int64)            # includes the sign bit of -acc: > 0x7ff when acc > 0
    emax = np.maximum(e1, e0)
    mark = lambda name, sel, ln: flags[name].__setitem__(ln[sel], True)
    # landing: a visit that begins, behind an addition, with the significand 1.0 -- or the final sum
    neg_normal = (e > 0) & (e < 0x7FF) & ok[lane]
    mark("landing", neg_normal & (pos > 0) & ((ab & MANT) == 0), lane)
    fb = (-acc).view(np.uint64)
    fe = (fb >> U64(52)).astype(np.int64)
    flags["landing"] |= ok & (fe > 0) & (fe < 0x7FF) & ((fb & MANT) == 0) & (fb != (-acc0).view(np.uint64))
    keep = ok[lane] & (e >= emax[lane] + 1) & (e < 0x7FF)
    lane, pos, end, e, ab = lane[keep], pos[keep], end[keep], e[keep], ab[keep]
    A = (ab & MANT) | HIDDEN
    q1, d1, tie1 = _rounding(e, e1[lane], m1[lane])
    q0, d0, tie0 = _rounding(e, e0[lane], m0[lane])
    length = end - pos
    one = tie1 != tie0
    dn = np.where(tie1, d0, d1)
    mode = np.where(tie1 & tie0, 1, np.where(one, np.where(dn % U64(2) == 0, 2, 3), 0))
    for k in range(4):
        mark("mode%d_lt32" % k, (mode == k) & (length < 32), lane)
        mark("mode%d_32_63" % k, (mode == k) & (length >= 32) & (length < 64), lane)
        mark("mode%d_ge64" % k, (mode == k) & (length >= 64), lane)
    both_zero = (d1 == 0) & (d0 == 0)
    mark("tie_free", (mode == 0) & ~both_zero, lane)
    mark("stalled", (mode == 0) & both_zero, lane)
    mark("one_increment_zero", (d1 == 0) != (d0 == 0), lane)
    half = (tie1 & (q1 == 0)) | (tie0 & (q0 == 0))
    mark("half_ulp_tie_odd", half & (A % U64(2) == 1), lane)
    mark("half_ulp_tie_even", half & (A % U64(2) == 0), lane)
    # the data's side of modes 2 and 3, from plain prefix counts (not from the tables)
    i_all = np.arange(n)
    t = np.where(tie1, 1, 0)
    count = np.stack([np.concatenate([[0], np.cumsum(x == s)]) for s in (0, 1)])                     # [2][n + 1]
    odd = np.stack([np.concatenate([[0], np.cumsum(odd_marks(x, s))]) for s in (0, 1)])
    nxt = np.stack([np.append(np.minimum.accumulate(np.where(x == s, i_all, n)[::-1])[::-1], n) for s in (0, 1)])
    jt = nxt[t, pos]
    behind = np.minimum(jt + 1, end)
    n_t, n_odd = count[t, end] - count[t, behind], odd[t, end] - odd[t, behind]
    mark("mode3_absent", (mode == 3) & (jt == n), lane)
    mark("mode3_first_at_start", (mode == 3) & (jt == pos), lane)
    mark("mode3_odd_and_even", (mode == 3) & (n_odd > 0) & (n_t - n_odd > 0), lane)
    mark("mode3_two_boundaries", (mode == 3) & (((end - 1) >> 5) - (pos >> 5) >= 2), lane)
    mark("mode2_no_tying_symbol", (mode == 2) & (count[t, end] - count[t, pos] == 0), lane)
    return acc, flags, kinds


# ---- the cases

def sequence(n, kind, rng):
    """-> x [n] uint8 of 0 / 1"""
    i = np.arange(n)
    if kind.startswith("iid_"):
        x = rng.uniform(size=n) < int(kind[4:]) / 100.0
    elif kind in ("runs", "runs_32k"):
        if kind == "runs":                      # runs of 1 .. 130 observations, none a multiple of 32
            ln = rng.integers(1, RUN_MAX + 1, n + 2)
            ln = ln[ln % 32 != 0]
        else:                                   # runs of 32 k - 1, 32 k, 32 k + 1 that end one observation before, on and one behind a word boundary
            # the offset of a run's end from the boundary: -1, 0 or 1, moving by at most one from run to run (a cycle: a few runs already meet all three)
            off = np.array([-1, 0, 1, 1, 0, -1, 0])[(np.arange(n // 31 + 2) + rng.integers(0, 7)) % 7]
            ln = 32 * rng.integers(1, 4, off.size) + np.diff(np.concatenate([[0], off]))
        x = np.repeat((np.arange(ln.size) + rng.integers(0, 2)) % 2, ln)[:n]
        assert x.size == n
    elif kind == "alternating":
        x = (i + rng.integers(0, 2)) % 2
    elif kind.startswith("period"):
        p = int(kind[6])
        x = (i % p == rng.integers(0, p)) == kind.endswith("_one")
    elif kind in ("all_ones", "all_zeros"):
        x = np.full(n, kind == "all_ones")
    elif kind in ("sparse_ones", "sparse_zeros"):
        x = np.zeros(n, dtype=bool)
        for a in SPARSE_AT:
            if -n <= a < n:
                x[a] = True
        x = x == (kind == "sparse_ones")
    else:
        raise ValueError(kind)
    return np.asarray(x).astype(np.uint8)


def _trail(x, z, setbit):
    """clears the z lowest significand bits of x and, where setbit, sets bit z: such an addend ties in the binade whose ulp is 2^(z + 1) of its own"""
    u = x.view(np.uint64).copy()
    zz = z.astype(np.uint64)
    u = ((u >> zz) << zz) | ((U64(1) << zz) * setbit.astype(np.uint64))
    return u.view(np.float64).copy()


def _negative(e, sig):
    """-(sig * 2^(e - 1075)) for biased exponents e and significands sig in [2^52, 2^53)"""
    return ((e.astype(np.uint64) << U64(52)) | (sig.astype(np.uint64) & MANT) | SIGN).view(np.float64).copy()


def _constructed_lanes(x, rng, count):
    """Lanes BUILT for a class.  The tying addend c_t has z trailing zero bits under a set bit z: it ties exactly where the ulp is 2^(z + 1) of its own, in the
    binade of exponent E = e_t + z + 1, and with |c| < 2^(E - z) per observation the sum stays there for at least 2^z >= 64 observations.  The other addend
    (exponent e_n = e_t + k, s_n = E - e_n) is built to the class: mode 1 -- it ties there too (s_n - 1 trailing zeros under a set bit); mode 2 -- its increment
    there is even (q even and r below half, or q odd and r above; or no increment at all, 54 binades down); mode 3 -- odd.  The start is a few observations'
    worth below 2^E (so that the visit begins inside the data, wherever the sum happens to cross) or, one lane in four, inside the binade.
    -> (acc0, l1, l0), lane q: class q % 4 (0: mode 1, 1: mode 2, 2 and 3: mode 3), tying value (q // 4) % 2"""
    n = x.size
    q = np.arange(count)
    cls, tsym, sub = q % 4, (q // 4) % 2, (q // 8) % 4
    k = rng.integers(-3, 3, count)
    z = rng.integers(6, 13, count) + np.maximum(k, 0)
    e_t = 1023 + rng.integers(-12, 4, count)
    rand = lambda: rng.integers(0, 1 << 52, count).astype(np.uint64)
    zz = z.astype(np.uint64)
    m_t = HIDDEN | ((rand() >> zz) << zz) | (U64(1) << zz)
    E = e_t + z + 1
    e_n = e_t + k
    s_n = (E - e_n).astype(np.uint64)
    zn = s_n - U64(1)
    tied = HIDDEN | ((rand() >> zn) << zn) | (U64(1) << zn)
    below = rng.integers(0, 2, count).astype(bool)
    parity = np.where(cls == 1, 0, 1) ^ np.where(below, 0, 1)       # q's parity: the increment's, or the other where the remainder rounds it up
    qn = (((HIDDEN | rand()) >> s_n) & ~U64(1)) | parity.astype(np.uint64)
    h = U64(1) << (s_n - U64(1))
    r = np.where(below, rand() % h, h + U64(1) + rand() % (h - U64(1)))
    m_n = np.where(cls == 0, tied, (qn << s_n) | r)
    far = (cls == 1) & (sub == 2)                                   # mode 2 with no increment at all: the other addend 54 .. 58 binades under the sum
    e_n = np.where(far, E - 54 - rng.integers(0, 5, count), e_n)
    m_n = np.where(far, HIDDEN | rand(), m_n)
    l_t, l_n = _negative(e_t, m_t), _negative(e_n, m_n)
    l1, l0 = np.where(tsym == 1, l_t, l_n), np.where(tsym == 1, l_n, l_t)
    p1 = float(x.mean()) if n else 0.5
    avg = p1 * np.abs(l1) + (1 - p1) * np.abs(l0)
    top = np.ldexp(1.0, E - 1023)
    lead = np.minimum(rng.integers(1, 90, count), np.floor(0.4 * top / avg))
    inside = rng.uniform(size=count) < 0.25
    acc0 = np.where(inside, -top * (1 + rng.uniform(0, 0.5, count)), -(top - lead * avg))
    return acc0, l1, l0


LANDING_PAIRS = (((-2, -4), (-4, -2), (-2, -6), (-6, -2), (-4, -6), (-6, -4), (-2, -2), (-4, -4)),      # no tie (ulp 2: d = 1, 2, 3)
                 ((-1, -2), (-3, -2), (-1, -6), (-5, -2)),                                            # the ones tie (half an ulp, 1.5, 2.5), d0 odd: mode 3
                 ((-4, -1), (-4, -3), (-2, -1), (-6, -3)),                                            # the zeros tie, d1 even (mode 2) or odd (mode 3)
                 ((-1, -3), (-3, -1), (-1, -1), (-3, -5)))                                            # both tie: mode 1


def _landing_lanes(x, acc0, l1, l0):
    """Lanes whose sum reaches a power of two EXACTLY after p observations: the binade [2^53, 2^54) has ulp 2, the addends are small even integers (no tie) or
    odd ones (ties), and the start is -(2^54 - 2 G), G = the growth of the significand over the first p observations.  G is followed by plain_sum itself from
    -(2^53 + 2 parity) -- inside a binade the roundings depend on the parity of the significand alone -- for either parity; the start must have the parity it was
    followed with (if neither has, the lane keeps tie-free addends).  p: LANDING_AT, at and beside word boundaries and the end of the data."""
    n = x.size
    lanes_ = np.arange(LANDING.start, LANDING.stop)
    qs = lanes_ - LANDING.start
    at = np.array([LANDING_AT[(q // 4) % len(LANDING_AT)] for q in qs])
    p = np.clip(np.where(at < 0, n - 1, at), 0, n)
    pair = np.array([LANDING_PAIRS[q % 4][(q // 4) % len(LANDING_PAIRS[q % 4])] for q in qs], dtype=np.float64)
    free = np.array([LANDING_PAIRS[0][(q // 4) % 8] for q in qs], dtype=np.float64)
    G = np.full((2, qs.size), -1, dtype=np.int64)
    for par in (0, 1):
        start = np.full(qs.size, -(2.0 ** 53 + 2.0 * par))
        _, snap = plain_sum(x[:int(p.max())], start, pair[:, 0], pair[:, 1], snaps=set(p.tolist()))
        for j, pj in enumerate(p.tolist()):
            G[par, j] = int((start[j] - snap[pj][j]) / 2.0)
    for j, lane in enumerate(lanes_.tolist()):
        ok = [par for par in (0, 1) if G[par, j] % 2 == par]
        if ok:
            g, (l1[lane], l0[lane]) = int(G[ok[0], j]), pair[j]
        else:
            l1[lane], l0[lane] = free[j]
            g = int(np.where(x[:p[j]] == 1, -free[j, 0], -free[j, 1]).sum() / 2)
        acc0[lane] = -(2.0 ** 54 - 2.0 * g) if g else -2.0 ** 53


def _saturation_lanes(x, acc0, l1, l0):
    """Lanes on which the product n * d of the bisection's first probe is a multiple of 2^64 plus a little: the sum sits one binade above the addend (s = 1, d =
    half its significand, in [2^51, 2^52)), and with N >= 4 097 occurrences d = ceil(k 2^64 / N) + 2 j gives N d = k 2^64 + (less than N (1 + 2 j)).  Computed
    exactly (32 x 32 bit products, saturating) it is far beyond the limit; wrapped to 64 bits it is small and the whole data would be jumped at once.  Only where
    the data has that many of a value (lane parity: which value); elsewhere the lanes stay ordinary."""
    n1 = int(x.sum())
    for v, lane in enumerate(range(SATURATION.start, SATURATION.stop)):
        side = v & 1
        N = n1 if side else x.size - n1
        k_min, k_max = -(-N // 8192), -(-N // 4096) - 1
        if N < 4097 or k_max < k_min:
            continue
        k = k_min + (v // 2) % (k_max - k_min + 1)
        d = -(-(k << 64) // N) + 2 * (v // 2)
        a = 3 * (v // 2)
        if not ((1 << 51) <= d < (1 << 52) and (N * d) % (1 << 64) < (1 << 52) - a):
            continue
        ec = 1022 + v
        c = -float(np.ldexp(float(2 * d), ec - 1075))
        acc0[lane] = -float(np.ldexp(float((1 << 52) + a), ec + 1 - 1075))
        (l1 if side else l0)[lane] = c
        (l0 if side else l1)[lane] = c * 2.0 ** -30


def _half_ulp_lanes(acc0, l1, l0):
    """Lanes whose tying addend is EXACTLY half an ulp (a power of two 53 binades under the sum: q = 0) while the other moves nothing either: 2^-2 of it (a
    quarter of an ulp), 2^-70 of it, or the same again (both tie: mode 1).  A odd: the first tying observation must round to even, one ulp up, and everything
    after it finds A even; A even: nothing moves at all.  By lane: which value ties, A's parity, the other addend, the scale."""
    for v, lane in enumerate(range(HALF_ULP.start, HALF_ULP.stop)):
        side, odd, other, scale = v & 1, (v >> 1) & 1 == 0, (v // 4) % 3, 2.0 ** (0, 5, -9, 30)[(v // 6) % 4]
        a = 2 * (v // 4) + 1 if odd else 2 * (v // 4)
        acc0[lane] = -(2.0 ** 53 + 2.0 * a) * scale
        t, o = -1.0 * scale, (-0.25, -2.0 ** -70, -1.0)[other] * scale
        l1[lane], l0[lane] = (t, o) if side else (o, t)


def lanes(x, rng, m=M):
    """-> (acc0 [m], l1 [m], l0 [m]) as the module docstring of tests/test_gpu_twoval.py lists them"""
    j = np.arange(m)
    l = -np.exp(rng.uniform(-12, 3, (2, m)))
    wide = j % 8 == 2
    l[:, wide] = -np.exp(rng.uniform(-80, 3, (2, int(wide.sum()))))      # one increment is 0 in a binade where the other is not
    z = np.minimum(np.floor(52 * rng.uniform(size=(2, m)) ** 2), 51).astype(np.int64)
    l1, l0 = _trail(l[0], z[0], rng.integers(0, 2, m).astype(bool)), _trail(l[1], z[1], rng.integers(0, 2, m).astype(bool))
    acc0 = np.where(rng.uniform(size=m) < 0.5, rng.normal(0, 3, m), -np.exp(rng.uniform(-5, 25, m)))
    acc0[STALL] = -np.ldexp(1.0, 40 + (j[STALL] - STALL.start) % 45)
    nf = len(FALLBACK_ADDENDS)
    l1[FALLBACK0:FALLBACK0 + nf] = FALLBACK_ADDENDS
    l0[FALLBACK0 + nf:FALLBACK0 + 2 * nf] = FALLBACK_ADDENDS
    l0[EQUAL] = l1[EQUAL]
    l0[RATIO] = l1[RATIO] * np.array([2.0, 0.5, 4.0, 0.25, 8.0, 0.125])
    l1[POWERS], l0[POWERS] = [-1.0, -0.5, -1.0, -2.0 ** -7, -8.0, -2.0 ** -20], [-0.5, -1.0, -1.0, -2.0, -2.0 ** -9, -2.0 ** -3]
    acc0[ACC0_FIXED0:ACC0_FIXED0 + 4] = ACC0_FIXED
    # starts 1 .. 4 ulps below a power of two, 1 .. 12 binades above the larger addend
    q = j[BELOW_POW2] - BELOW_POW2.start
    emax = np.maximum(addend_parts(l1[BELOW_POW2])[1], addend_parts(l0[BELOW_POW2])[1])
    acc0[BELOW_POW2] = ((((emax + 1 + q % 12).astype(np.uint64)) << U64(52)) - (1 + q % 4).astype(np.uint64) | SIGN).view(np.float64)
    _landing_lanes(x, acc0, l1, l0)
    _saturation_lanes(x, acc0, l1, l0)
    _half_ulp_lanes(acc0, l1, l0)
    acc0[CONSTRUCTED], l1[CONSTRUCTED], l0[CONSTRUCTED] = _constructed_lanes(x, rng, CONSTRUCTED.stop - CONSTRUCTED.start)
    return acc0, l1, l0


def case_list():
    return [(n, kind) for n in SHAPES for kind in KINDS]


_built = {}


def case(n, kind):
    """-> dict(n, kind, x, tab: the six tables back to back, acc0, l1, l0, want: the plain sums, flags, kinds); computed once and shared (nobody may write to the
    arrays)"""
    key = (n, kind)
    if key not in _built:
        rng = np.random.default_rng([13, n, KINDS.index(kind)])
        x = sequence(n, kind, rng)
        acc0, l1, l0 = lanes(x, rng)
        want, flags, kinds = census(x, acc0, l1, l0)
        d = dict(n=n, kind=kind, x=x, tab=tables_flat(x), acc0=acc0, l1=l1, l0=l0, want=want, flags=flags, kinds=kinds)
        for a in (x, d["tab"], acc0, l1, l0, want) + tuple(flags.values()):
            a.setflags(write=False)
        _built[key] = d
    return _built[key]


def same_bits(a, b):
    """the same bits, or both NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def shape_share(n, flag):
    """the share of the lanes of every case of a shape (all its sequences together) with a flag"""
    return float(np.concatenate([case(n, kind)["flags"][flag] for kind in KINDS]).mean())


def suite_count(flag):
    return int(sum(case(*k)["flags"][flag].sum() for k in case_list()))


# the census conditions (conditions on the INPUTS; if one fails, the inputs change, not the condition)
SUITE_MIN = {"mode1_ge64": 500, "mode2_ge64": 500, "mode3_ge64": 500, "mode3_absent": 100, "mode3_first_at_start": 100, "mode3_odd_and_even": 100,
             "mode3_two_boundaries": 100, "mode2_no_tying_symbol": 100, "stalled": 100, "half_ulp_tie_odd": 100, "half_ulp_tie_even": 100, "one_increment_zero": 100,
             "landing": 100}
SHARE_MIN = {"tie_free": 0.80, "mode3_ge64": 0.05}      # over every shape with n >= 777
FALLBACK_KINDS = {"-inf", "nan", "positive", "zero", "subnormal"}


def check_census_conditions():
    """asserted by both test files"""
    for flag, least in SUITE_MIN.items():
        assert suite_count(flag) >= least, (flag, suite_count(flag))
    for n in SHAPES:
        if n >= 777:
            for flag, least in SHARE_MIN.items():
                assert shape_share(n, flag) >= least, (n, flag, shape_share(n, flag))
    assert set().union(*[case(*k)["kinds"] for k in case_list()]) == FALLBACK_KINDS


def census_table():
    cols = ("mode0_ge64", "mode1_lt32", "mode1_32_63", "mode1_ge64", "mode2_lt32", "mode2_32_63", "mode2_ge64", "mode3_lt32", "mode3_32_63", "mode3_ge64") + LANE_FLAGS[len(MODE_FLAGS):]
    rows = ["| n | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for n in SHAPES:
        rows.append("| %d | " % n + " | ".join("%.1f %%" % (100 * shape_share(n, f)) for f in cols) + " |")
    rows.append("| suite (lanes) | " + " | ".join(str(suite_count(f)) for f in cols) + " |")
    return "\n".join(rows)


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(census_table())
    print("fallback addends met:", sorted(set().union(*[case(*k)["kinds"] for k in case_list()])))
    print("%d cases, %.1f s" % (len(case_list()), time.time() - t0))
    check_census_conditions()
