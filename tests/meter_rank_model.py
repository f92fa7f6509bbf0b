"""The model, the data and the cases of the meter ranks (fxb_meter_rank, fxb_meter_rank_match, fxb_meter_rank_level), shared by
tests/test_meter_rank_model.py (their coverage, no GPU), tests/test_meter_rank_stub.py (the CPU stand-in) and
tests/test_gpu_meter_rank.py (the kernels).  No test lives here.

The model is numpy over the arrays fxb_meter_read / _read_match / _read_level return, as include/fx8010_amd.h "Meter ranks" defines
the call: V per family (the models of the selects: meter_list_model.value, meter_target_model.V, meter_level_model.V), the
candidates of the range by `>=` or `<` against the threshold as a float64, then np.lexsort((n, V)) - V descending with LARGEST, ties
to the smaller instance number.  The bar is equality: the list word for word, the values as integer words, the return value, and
every word of the caller's two buffers behind min(M, k) still holding the mark it was given.

The kernels find the k-th key by a radix select over 64-bit keys, DIGIT_BITS bits at a time (csrc/fx_meter_rank.hpp
kMeterRankDigitBits, mirrored here and compared by the model test).  keys() is the transform the header describes; the model
itself never uses it - only the coverage functions do: digit_ks() finds, for a V, the k at which the k-th and (k + 1)-th keys of
the order first differ in each digit, and the scenes below are built so that every digit, a tie at the k-th key across a wavefront
and across a chunk boundary, M < k, M == k, M == 0, k == 0, every V equal and LARGEST with ties all occur."""
import ctypes as C

import numpy as np

import meter_level_model as L
import meter_list_model as M
import meter_target_model as T

DIGIT_BITS = 8                    # kMeterRankDigitBits
PASSES = 64 // DIGIT_BITS
CHUNK, WAVE = 256, 64             # kMeterSelectChunk, a wavefront
BELOW, LARGEST = 1, 2             # FXB_METER_BELOW, FXB_METER_LARGEST
FAMILIES = ("meter", "match", "level")
STATS = {"meter": (0, 1, 2, 3), "match": (0, 1), "level": (0, 1)}
CALL = {"meter": "fxb_meter_rank", "match": "fxb_meter_rank_match", "level": "fxb_meter_rank_level"}
COUNTER = {"meter": "meter_ranks", "match": "meter_match_ranks", "level": "meter_level_ranks"}
INFO = {"meter": 71, "match": 72, "level": 73}   # FXB_INFO_METER_RANKS / _MATCH_RANKS / _LEVEL_RANKS
MARK = M.MARK                                     # what a list buffer holds where nothing may be written
VMARK = np.uint64(0x7FF8BADC0FFEE123)             # ... and a value buffer, as a word (a NaN no V can be)
PAD = 7


def value(family, rows, stat):
    """V(n) of the select of the same family, as float64"""
    return M.value(rows, stat) if family == "meter" else T.V(rows, stat) if family == "match" else L.V(rows, stat)


def rank(V, k, threshold=-np.inf, below=False, largest=False, first=0, n_range=None):
    """(M, list, values): the candidates of first .. first + n_range - 1 in the order (V, n), the first min(M, k) of them"""
    n_range = V.size - first if n_range is None else n_range
    part = V[first:first + n_range]
    t = np.float64(threshold)
    n = first + np.nonzero(part < t if below else part >= t)[0].astype(np.int64)
    v = V[n]
    order = np.lexsort((n, -v if largest else v))   # the last key is the primary one; compares of real numbers: -0.0 == +0.0
    take = order[:max(min(int(k), n.size), 0)]
    return int(n.size), n[take], v[take]


def k_values(m):
    return sorted(k for k in {0, 1, 2, 63, 64, 65, 257, m - 1, m, m + 1} if k >= 0)


def keys(V, largest=False):
    """the 64-bit keys, monotone in the real order: V + 0.0, the sign-flip transform, complemented for LARGEST"""
    u = (np.asarray(V, dtype=np.float64) + 0.0).view(np.uint64)
    key = np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
    return ~key if largest else key


def first_digit(a, b):
    """the most significant digit in which two keys differ (0 is the top one), None for equal keys"""
    x = int(a) ^ int(b)
    return None if x == 0 else (64 - x.bit_length()) // DIGIT_BITS


def digit_ks(V, largest=False):
    """{digit: k}: a k (1 <= k < N) at which the k-th and (k + 1)-th keys of the whole order first differ in that digit"""
    ordered = np.sort(keys(V, largest))
    out = {}
    for k in range(1, ordered.size):
        d = first_digit(ordered[k - 1], ordered[k])
        if d is not None:
            out.setdefault(d, k)
    return out


def tie(V, k, largest=False):
    """the tie at the k-th key of the whole order: (the instances whose key equals it, how many of them win)"""
    key = keys(V, largest)
    kth = np.sort(key)[k - 1]
    return np.nonzero(key == kth)[0], k - int((key < kth).sum())


# ---- the scenes: inputs for a program whose output is its input ------------------------------------------------------------------

LADDER_N = 300
LADDER_HALF = (10, 70, 200, 257, 290)                      # energy 0.25
LADDER_AT = (275, 271, 277, 273, 272, 276, 274)            # energy 1 + 2^-2j, j in LADDER_J: not in instance order
LADDER_J = (26, 22, 18, 14, 10, 6, 2)


def ladder_voices(S=33):
    """x [S, 1, LADDER_N]: every voice has one sample of 1.0 - energy 1.0 exactly, 288 of them: the run of equals - but five with
    0.5 (energy 0.25) and seven two-sample voices (1.0, 2^-j): energy 1 + 2^-2j, both products and the sum exact in fp64, the
    mantissa bit 52 - 2j set - one in every digit below the top one.  Nothing is non-finite and nothing reaches the rail twice:
    `nonfinite` is 0 for every voice (every V equal), `peak` is 1.0 or 0.5 (LARGEST with ties)."""
    x = np.zeros((S, 1, LADDER_N), dtype=np.float32)
    x[0, 0, :] = 1.0
    x[0, 0, list(LADDER_HALF)] = 0.5
    for n, j in zip(LADDER_AT, LADDER_J):
        x[1, 0, n] = np.float32(2.0 ** -j)
    return x


def target_for(x):
    """a target [S, channels, N] for voices() inputs, one column per instance (group = 1): half a unit with the sample's sign, negated
    for every third instance - their cross product is negative, the others' positive, a silent voice's 0"""
    S, channels, N = x.shape
    sign = np.where(np.arange(S) % 2 == 0, 0.5, -0.5)[:, None, None] * np.where(np.arange(N) % 3 == 0, -1.0, 1.0)[None, None, :]
    return np.ascontiguousarray(np.broadcast_to(sign, (S, channels, N)), dtype=np.float32)


LEVEL_RELEASE, LEVEL_FLOOR = np.float32(0.9), np.float32(0.05)


def thresholds(V):
    """-Inf (the whole range), a value of V itself near the middle (`>=` takes it, BELOW leaves it), +Inf"""
    return [-np.inf, float(np.sort(V)[V.size // 2]), np.inf]


# ---- the calls against the model ---------------------------------------------------------------------------------------------

def raw_rank(lib, b, family, stat, k, t, flags, first, n_range, null_list=False, null_value=False):
    """(the list buffer and the value buffer of k + PAD words, filled with their marks before the call, and the return value)"""
    room = max(int(k), 0) + PAD
    lst, val = np.full(room, MARK, dtype=np.int64), np.full(room, VMARK, dtype=np.uint64)
    fn = getattr(lib, CALL[family])
    m = fn(b._h, int(stat), int(k), C.c_double(t), int(first), int(n_range), None if null_list else C.c_void_p(lst.ctypes.data),
           None if null_value else C.c_void_p(val.ctypes.data), int(flags))
    return lst, val, int(m)


def check_one(lib, b, family, V, stat, k, t=-np.inf, below=False, largest=False, first=0, n_range=None, what=""):
    n_range = V.size - first if n_range is None else n_range
    m, want, values = rank(V, k, t, below, largest, first, n_range)
    lst, val, got = raw_rank(lib, b, family, stat, k, t, (BELOW if below else 0) | (LARGEST if largest else 0), first, n_range)
    tag = (what, family, stat, k, t, "below" if below else "at or above", "largest" if largest else "smallest", first, n_range, got, m)
    r = want.size
    assert got == m, tag
    assert np.array_equal(lst[:r], want), tag + (lst[:8], want[:8])
    assert np.array_equal(val[:r], values.view(np.uint64)), tag
    assert (lst[r:] == MARK).all() and (val[r:] == VMARK).all(), ("words behind min(M, k) were written",) + tag
    return m


def check_ranks(lib, b, family, rows, what="", ks=None, starts=(0, 1, 63, 64, 65)):
    """every stat of the family, the four flag combinations, thresholds(): the whole range with k_values(M) (or `ks`); on the
    middle threshold also the sub-ranges first in `starts` x n_range in {0, 1, 64, N - first} with k = 3 and k = n_range.  Returns
    the number of calls made."""
    calls = 0
    for stat in STATS[family]:
        V = value(family, rows, stat)
        N = V.size
        for below in (False, True):
            for largest in (False, True):
                for t in thresholds(V):
                    m = rank(V, 0, t, below, largest)[0]
                    for k in (k_values(m) if ks is None else ks):
                        check_one(lib, b, family, V, stat, k, t, below, largest, 0, N, what)
                        calls += 1
                t = thresholds(V)[1]
                for first in starts:
                    if first > N:
                        continue
                    for n_range in sorted({0, min(1, N - first), min(64, N - first), N - first}):
                        for k in (3, n_range):
                            check_one(lib, b, family, V, stat, k, t, below, largest, first, n_range, what)
                            calls += 1
    return calls


def check_digits(lib, b, family, V, stat, what=""):
    """the k of digit_ks, k + 1 beside each, both directions: the k-th and (k + 1)-th keys first differ in every digit there is"""
    seen = set()
    for largest in (False, True):
        for d, k in digit_ks(V, largest).items():
            for kk in (k, k + 1):
                check_one(lib, b, family, V, stat, kk, largest=largest, what=what + " digit %d" % d)
            seen.add(d)
    return seen
