"""gm_udiv64 and pcg_uniform64 (csrc/gaps_math.h) against exact integers: the inputs and the checks, shared by
tests/test_sequential_oracle.py (the shared source compiled for the host) and tests/test_sequential_oracle_gpu.py (the device).

gm_udiv64 stands in for the compiler's 64-bit division in the integer draws; at run time only the sequential sampler reaches it with
divisors of every size (a birth over the whole domain, a move between two neighbours).  Its own comments reason about four places, and
the edge inputs below sit on them: the subtraction loop for divisors from 2^62 (quotients up to 3), the divisor 1, the clamp of the first
quotient estimate at the largest double below 2^64, and the fix-ups that follow the second estimate -- one step down (a quotient
estimated one too high: the dividends just below a multiple) and one step up (one too low: exact multiples, multiple_pairs())."""
import numpy as np
import pytest

M64 = (1 << 64) - 1


# ---- gm_udiv64 ----------------------------------------------------------------------------------------------------------------------
def edge_divisors():
    b = {1, 2, 3, (1 << 62) - 1, 1 << 62, 1 << 63, M64}
    for k in range(1, 64):
        b.update(((1 << k) - 1, 1 << k, (1 << k) + 1))
    return sorted(x for x in b if 1 <= x <= M64)


def edge_pairs():
    """every edge divisor with the dividends around its multiples: 0, b - 1, b, b + 1, m b - 1, m b, m b + 1 for m around 2^20, 2^32 and
    the largest quotient floor((2^64 - 1) / b), and the dividends around 2^53 (where doubles stop holding every integer), 2^63 and 2^64"""
    a_out, b_out = [], []
    for b in edge_divisors():
        top = M64 // b
        ms = {m + d for m in (1 << 20, 1 << 32, top) for d in (-1, 0, 1)}
        a = {0, b - 1, b, b + 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - 1, M64}
        for m in ms:
            a.update((m * b - 1, m * b, m * b + 1))
        for x in sorted(a):
            if 0 <= x <= M64:
                a_out.append(x), b_out.append(b)
    return np.array(a_out, dtype=np.uint64), np.array(b_out, dtype=np.uint64)


def multiple_pairs():
    """exact multiples a = m b, where a quotient estimate that falls short by the last bit leaves a whole divisor as remainder: every
    divisor up to 300 and every edge divisor, with m = the powers of 3 that fit and the three largest quotients"""
    a_out, b_out = [], []
    for b in sorted(set(range(1, 301)) | set(edge_divisors())):
        top = M64 // b
        ms, m = {top, max(top - 1, 0), max(top - 2, 0)}, 1
        while m <= top:
            ms.add(m)
            m *= 3
        for m in sorted(ms):
            a_out.append(m * b), b_out.append(b)
    return np.array(a_out, dtype=np.uint64), np.array(b_out, dtype=np.uint64)


def random_pairs(n=1 << 20, seed=64):
    """n pairs whose bit lengths are uniform over 1 .. 64, independently for dividend and divisor"""
    g = np.random.Generator(np.random.MT19937(seed))

    def draw():
        bits = g.integers(1, 65, n).astype(np.uint64)
        x = g.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False) >> (np.uint64(64) - bits)
        return x | (np.uint64(1) << (bits - np.uint64(1)))      # the top bit of the drawn length is set
    return draw(), draw()


def check_udiv64(fn, a, b):
    """fn(a, b) against Python's integers, pair by pair"""
    q = fn(a, b)
    want = np.array([x // y for x, y in zip(a.tolist(), b.tolist())], dtype=np.uint64)
    bad = np.nonzero(q != want)[0]
    assert bad.size == 0, "%d of %d quotients differ, first: %d // %d = %d, got %d" % (
        bad.size, a.size, int(a[bad[0]]), int(b[bad[0]]), int(want[bad[0]]), int(q[bad[0]]))


# ---- pcg_uniform64 ------------------------------------------------------------------------------------------------------------------
def pcg_u32(s):
    """GapsRng::uniform32() (Random.cpp:40-56): advance, then output"""
    s = (s * 6364136223846793005 + 55) & M64
    x = (((s >> 18) ^ s) >> 27) & 0xFFFFFFFF
    rot = s >> 59
    return s, ((x >> rot) | (x << ((-rot) & 31))) & 0xFFFFFFFF


def pcg_u64(s):
    """GapsRng::uniform64() (Random.cpp:98-103): the high word first"""
    s, hi = pcg_u32(s)
    s, lo = pcg_u32(s)
    return s, (hi << 32) | lo


def uniform64(s, a, b):
    """GapsRng::uniform64(a, b) (Random.cpp:105-123) in Python's integers, with the 64-bit wrap of `range` written out.  For the whole
    64-bit range, b + 1 - a wraps to 0 and the reference divides by it: ZeroDivisionError here, an integer division by zero there."""
    if b == a:
        return s, a
    rng = (b + 1 - a) & M64
    s, x = pcg_u64(s)
    i_part = M64 // rng
    while x >= rng * i_part:
        s, x = pcg_u64(s)
    return s, x // i_part + a


def uniform64_inputs(seed=65, states_per_range=24):
    """ranges of 1, 2, 3, 2^62 - 1, 2^62 + 1, 2^63 and 2^64 - 1 values, each at the bottom, near the bottom and at the top of the 64-bit
    numbers; the sampler's own ranges (1 .. domain length for a few bin counts) and random ones; several generator states each"""
    g = np.random.Generator(np.random.MT19937(seed))
    ranges = []
    for size in (1, 2, 3, (1 << 62) - 1, (1 << 62) + 1, 1 << 63, M64):
        for lo in (0, 1, 987654321, M64 - (size - 1)):
            if lo + size - 1 <= M64:
                ranges.append((lo, lo + size - 1))
    for bins in (2, 10, 27, 4089, 24000, 210003):
        ranges.append((1, (M64 // bins) * bins))
    for _ in range(40):
        lo, hi = sorted(int(x) >> int(sh) for x, sh in zip(g.integers(0, 1 << 64, 2, dtype=np.uint64), g.integers(0, 64, 2)))
        ranges.append((lo, hi))
    ranges = sorted(set(ranges))
    states = g.integers(0, 1 << 64, (len(ranges), states_per_range), dtype=np.uint64)
    s = states.reshape(-1)
    lo = np.repeat(np.array([r[0] for r in ranges], dtype=np.uint64), states_per_range)
    hi = np.repeat(np.array([r[1] for r in ranges], dtype=np.uint64), states_per_range)
    return s, lo, hi


def check_uniform64(fn):
    """fn(states, lo, hi) -> (values, states after): the restatement's, draw by draw -- the value and how far the generator went"""
    s, lo, hi = uniform64_inputs()
    v, after = fn(s, lo, hi)
    redrawn = 0
    for i, (si, a, b) in enumerate(zip(s.tolist(), lo.tolist(), hi.tolist())):
        ws, wv = uniform64(si, a, b)
        assert a <= wv <= b
        assert (int(v[i]), int(after[i])) == (wv, ws), "uniform64(%d, %d) from state %d: value %d, state %d; expected %d, %d" % (a, b, si, int(v[i]), int(after[i]), wv, ws)
        redrawn += a != b and ws != pcg_u64(si)[0]
    assert redrawn > 0      # (the rejection loop ran: a range of 2^63 values rejects every other draw)


def check_refusals(lib, on_device):
    """what neither function is defined for is refused before anything runs: a divisor 0; a range with hi < lo; and the whole 64-bit range,
    whose number of values wraps to 0 -- the reference divides by that zero (the restatement above shows it), and pcg_uniform64 would
    never leave its rejection loop.  No caller asks for it: the sampler's lower bounds start at 1."""
    from cogaps_amd import _capi
    with pytest.raises(ZeroDivisionError):
        uniform64(12345, 0, M64)
    one = np.array([1], dtype=np.uint64)
    with pytest.raises(_capi.CogapsError, match="divisor"):
        _capi.debug_udiv64(one, one * np.uint64(0), on_device=on_device, lib=lib)
    with pytest.raises(_capi.CogapsError, match="fewer than 2\\^64 values"):
        _capi.debug_uniform64(one, one * np.uint64(0), one * np.uint64(M64), on_device=on_device, lib=lib)
    with pytest.raises(_capi.CogapsError, match="lo <= hi"):
        _capi.debug_uniform64(one, one * np.uint64(5), one * np.uint64(4), on_device=on_device, lib=lib)
