"""What the stream tests compare against (tests/test_gpu_stream_words.py, tests/README.stream.md): the uniform stream from any position, and the flag words of
the window stream (csrc/amwg_window.h), restated in numpy.

The values come from synth.uniforms (numpy, every word of the Philox counter and key kept as 64-bit integers, pinned by the Random123 known answers).  The flag
predicate is the reference's rnorm loop condition (mcmc.js:44-53) in float64, one rounding per operation, with the oracle's logarithm."""
import numpy as np

import oracle_lib
import synth

KEY = 0x9E3779B97F4A7C15      # k1 != 0 and the top bit set: a detour through int64 or a double shows
OFFSET = 2 ** 32 - 3          # local chains 3 and up carry into c3
SEEDS = [2 ** 32 - 1, 2 ** 32, KEY, 2 ** 64 - 1]
CHAIN0S = [OFFSET, 2 ** 63 + 5]
# positions (uniforms consumed): around the refills of every lane count, and around the carry of the block number into its high word -- block 2^32 - k at parity p:
#   k = 1, 2, 5, 33: b0 + lane crosses 2^32 inside one fill of a chain on 2, 4, 8, 64 lanes;  k = 64: the second fill (the window's half B) starts at 2^32;
#   k = 65: the carry inside half B;  k = 130: inside the half B computed after one shift()
CARRY_K = [1, 2, 5, 33, 64, 65, 130]
_LOW = [0, 1, 2, 127, 128, 129, 255, 256]
_CARRY = [2 * (2 ** 32 - k) + p for k in CARRY_K for p in (0, 1)]
# (a low position, then the two parities of a carry position, and so on: chains that are neighbours in a wavefront are of both parities, and some pass the carry
# while others are far from it)
POSITIONS = [p for j in range(7) for p in (_LOW[j], _CARRY[2 * j], _CARRY[2 * j + 1])] + [_LOW[7], 2 ** 62 - 3]

_cache = {}


def uniforms(seed, chain, start, n):
    """uniforms number start .. start + n - 1 of stream (seed, chain); start of either parity"""
    key = (seed, chain, start, n)
    if key not in _cache:
        even = start & ~1
        _cache[key] = np.ascontiguousarray(synth.uniforms(seed, chain, n + (start - even), even)[start - even:])
    return _cache[key]


def pair_ok(u, v_raw):
    """does rnorm accept the pair (u, v_raw)?  the negation of the loop condition of mcmc.js:51, the logarithm evaluated only where `&&` and `||` reach it"""
    u, v_raw = np.asarray(u, dtype=np.float64), np.asarray(v_raw, dtype=np.float64)
    v = 1.7156 * (v_raw - 0.5)
    x = u - 0.449871
    y = np.abs(v) + 0.386595
    q = x * x + y * (0.19600 * y - 0.25472 * x)
    again = q > 0.27846
    log = oracle_lib.lib().orc_log
    for i in np.nonzero((q > 0.27597) & ~again)[0]:
        ui, vi = float(u[i]), float(v[i])
        again[i] = vi * vi > -4 * log(ui) * ui * ui
    return ~((q > 0.27597) & again)


def _word(bits):
    return sum(1 << j for j, b in enumerate(bits) if b)


def half_flags(half, first_of_next=None):
    """(E, O) of one half of the window: 128 uniforms.  Bit j of E: the pair at the even position 2j; bit j of O: the pair at the odd position 2j + 1, whose second
    uniform for j = 63 is the first of the next half (None: the bit is clear)."""
    E = _word(pair_ok(half[0::2], half[1::2]))
    if first_of_next is None:
        O = _word(pair_ok(half[1:127:2], half[2:128:2]))
    else:
        O = _word(pair_ok(half[1::2], np.append(half[2::2], first_of_next)))
    return E, O


def window_after(seed, chain, consumed0, n_draws):
    """WindowStream after n_draws next() calls from consumed0 and a position(): -> (first block of half A, position in the window)"""
    total = (consumed0 & 1) + n_draws
    return (consumed0 >> 1) + 64 * (total // 128), total % 128
