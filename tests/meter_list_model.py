"""The model and the cases of the meter queries by list (fxb_meter_select, fxb_meter_read_list, fxb_meter_reset_list), shared by
tests/test_meter_list_stub.py (the CPU stand-in) and tests/test_gpu_meter_list.py (the kernels).  No test lives here.

The model is numpy over the arrays fxb_meter_read returns, as include/fx8010_amd.h "Meter queries by list" defines the select:
every accumulator converted to float64 - exact for a float32 and for a uint32 - the maximum over the channels, `>=` or `<` against
the threshold as a float64, np.nonzero restricted to the range.  The bar is equality: the list word for word, the count, and every
word of the caller's buffer behind min(M, cap) still holding the mark it was given."""
import ctypes as C

import numpy as np

FIELDS = ("energy", "peak", "full_scale", "nonfinite")   # stat 0..3
BELOW = 1
MARK = -0x0123456789ABCDEF   # what a list buffer holds where nothing may be written
PAD = 7                      # words of the buffer behind `cap`


def voices(N, channels, S, seed=0):
    """x [S, channels, N] float32 for a program whose output is its input: per instance one level on channel n % channels and half
    of it on the others, so the maximum sits on a different channel from instance to instance; the sign alternates by sample.
    Levels: 0.99 for instance 0 alone (the largest), 0.9 for every 64th, 0.8 for one in a hundred, 0.6 for every second of the
    rest by a coin, 0.3 for the others, 0.1 for instance N - 1 alone (the smallest that sounds).  On top, by residues of n: silence
    on every channel; a +-1.0 word (the rail); the float just below 1; a denormal; a NaN; a -Inf and a +Inf - each in one sample
    of the instance's loud channel; instances 0 and N - 1 are left as they are."""
    rng = np.random.default_rng(1000 + seed)
    n = np.arange(N)
    level = np.where(rng.random(N) < 0.5, 0.6, 0.3)
    level[rng.random(N) < 0.01] = 0.8
    level[n % 64 == 0] = 0.9
    level[n % 9 == 4] = 0.0
    if N > 1:
        level[N - 1] = 0.1
    level[0] = 0.99
    loud = n % channels
    amp = np.where(np.arange(channels)[:, None] == loud[None, :], level[None, :], 0.5 * level[None, :]).astype(np.float32)
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x = np.ascontiguousarray(sign[:, None, None] * amp[None, :, :], dtype=np.float32)
    special = ((7, 3, 1 % S, 1.0), (7, 5, 1 % S, -1.0), (17, 8, 5 % S, np.nextafter(np.float32(1.0), np.float32(0.0))), (5, 2, 0, np.float32(1e-42)),
               (11, 5, 2 % S, np.nan), (13, 6, 3 % S, -np.inf), (13, 6, 4 % S, np.inf), (13, 7, 3 % S, np.inf))
    for mod, res, s, v in special:
        hit = n[(n % mod == res) & (n % 9 != 4) & (n != 0) & (n != N - 1)]
        x[s, loud[hit], hit] = v
    return x


def pattern_voices(N, channels, S, loud):
    """x [S, channels, N] float32 of plain levels, no special words: the instances of `loud` at 0.9, every other instance at 0.3, on
    EVERY channel alike - whichever input word a program's output channel hears (the reference's input-refresh rule lets a later
    channel hear an earlier one's), a voice's meters are those of its level - the sign alternating by sample.  A peak threshold of
    0.5 and an energy threshold of 0.25 S separate the two kinds (0.3 and 0.09 S against 0.9 and 0.81 S).  The loud channel that
    moves from instance to instance is voices()'s business."""
    level = np.full(N, 0.3)
    level[np.asarray(loud, dtype=np.int64)] = 0.9
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return np.ascontiguousarray(sign[:, None, None] * np.broadcast_to(level.astype(np.float32), (channels, N))[None, :, :], dtype=np.float32)


def check_patterns(lib, b, N, channels, S=8):
    """The match patterns by name, each the answer of ONE select over the whole batch, the list and M asserted against the list
    written out here (not against the model): none; all; only instance 0; only instance N - 1 - the single match in the last chunk,
    every chunk count in front of it zero; the same two as the only voice BELOW the threshold; every 64th.  Each pattern is a full
    reset and one block of pattern_voices through a program whose output is its input; peak and energy, the list taken with
    cap = N into a marked buffer, and as a count query with a null list."""
    every = np.arange(0, N, 64)
    cases = (("none", [], False, []), ("all", n_all(N), False, n_all(N)), ("only instance 0", [0], False, [0]), ("only N - 1", [N - 1], False, [N - 1]),
             ("only instance 0 below", np.arange(1, N), True, [0]), ("only N - 1 below", np.arange(N - 1), True, [N - 1]), ("every 64th", every, False, every))
    for name, loud, below, want in cases:
        b.meter_read(reset=True)
        b.process_block(pattern_voices(N, channels, S, loud))
        want = np.asarray(want, dtype=np.int64)
        for stat, t in ((1, 0.5), (0, 0.25 * S)):
            got, m = b.meter_select(stat, t, below=below)
            assert m == want.size and np.array_equal(got, want), (name, N, FIELDS[stat], m, got[:8])
            buf, m = raw_select(lib, b, stat, t, below, 0, N, N)
            assert m == want.size and np.array_equal(buf[:m], want) and (buf[m:] == MARK).all(), (name, N, FIELDS[stat], m)
            assert raw_select(lib, b, stat, t, below, 0, N, 0, null=True)[1] == want.size, (name, N, FIELDS[stat])
    return len(cases)


def n_all(N):
    return np.arange(N, dtype=np.int64)


def value(rows, stat):
    """V(n): the maximum over the channels of accumulator `stat`, as float64 (exact)"""
    return rows[FIELDS[stat]].astype(np.float64).max(axis=0)


def model(rows, stat, threshold, below, first=0, n_range=None):
    V = value(rows, stat)
    n_range = V.size - first if n_range is None else n_range
    part = V[first:first + n_range]
    t = np.float64(threshold)
    return (first + np.nonzero(part < t if below else part >= t)[0]).astype(np.int64)


def thresholds(rows, stat):
    """-Inf, a negative value, 0, +Inf; every distinct value of V itself (one instance's value exactly: `>=` includes it, BELOW
    excludes it) and a double strictly between every two adjacent ones - for the peak that is a double between two floats, which
    no float32 compare could honour.  At most the 12 lowest and 12 highest distinct values are taken."""
    u = np.unique(value(rows, stat))
    if u.size > 24:
        u = np.concatenate([u[:12], u[-12:]])
    mid = [float(a + (b - a) / 2) for a, b in zip(u[:-1], u[1:]) if a < a + (b - a) / 2 < b]
    out = [-np.inf, -1.0, 0.0, np.inf] + [float(v) for v in u] + mid
    if stat == 1:
        p = rows["peak"].max()
        up = np.nextafter(np.float32(p), np.float32(np.inf))
        out.append((float(p) + float(up)) / 2)   # strictly between the largest peak and the next float above it
    return out


def raw_select(lib, b, stat, threshold, below, first, n_range, cap, null=False):
    """(the buffer of cap + PAD words, filled with MARK before the call, and the return value)"""
    buf = np.full(max(cap, 0) + PAD, MARK, dtype=np.int64)
    m = lib.fxb_meter_select(b._h, int(stat), C.c_double(threshold), int(first), int(n_range), None if null else C.c_void_p(buf.ctypes.data), int(cap), BELOW if below else 0)
    return buf, int(m)


def check_one(lib, b, rows, stat, t, below, first, n_range, cap, what=""):
    want = model(rows, stat, t, below, first, n_range)
    buf, m = raw_select(lib, b, stat, t, below, first, n_range, cap)
    take = min(want.size, cap)
    tag = (what, FIELDS[stat], t, "below" if below else "at or above", first, n_range, cap, m, want.size)
    assert m == want.size, tag
    assert np.array_equal(buf[:take], want[:take]), tag
    assert (buf[take:] == MARK).all(), ("words behind min(M, cap) were written",) + tag
    return want


def check_selects(lib, b, rows, N, what=""):
    """every stat, both directions, thresholds(): whole range with cap = N; then the caps 0, 1, M - 1, M, M + 1, N + 5 and the ranges
    first in {0, 1, 63, 64, 65} x n_range in {0, 1, 64, N - first} on thresholds that split the batch.  Returns the number of
    distinct match counts seen (a test can ask that the cases were no empty exercise)."""
    seen = set()
    for stat in range(4):
        ts = thresholds(rows, stat)
        for below in (False, True):
            for t in ts:
                seen.add(check_one(lib, b, rows, stat, t, below, 0, N, N, what).size)
        # the thresholds whose answer is neither nothing nor everything, where there are such: caps and ranges
        split = [t for t in ts if 0 < model(rows, stat, t, False).size < N][:3] or [0.0]
        for t in split:
            for below in (False, True):
                M = model(rows, stat, t, below).size
                for cap in sorted({0, 1, max(M - 1, 0), M, M + 1, N + 5}):
                    check_one(lib, b, rows, stat, t, below, 0, N, cap, what)
                for first in (0, 1, 63, 64, 65):
                    if first > N:
                        continue
                    for n_range in sorted({0, min(1, N - first), min(64, N - first), N - first}):
                        want = check_one(lib, b, rows, stat, t, below, first, n_range, n_range, what)
                        check_one(lib, b, rows, stat, t, below, first, n_range, max(want.size - 1, 0), what)
    return len(seen)


def same_rows(got, want):
    """bit for bit: fp64 and fp32 words are compared as integers"""
    views = {"energy": np.uint64, "peak": np.uint32, "full_scale": np.uint32, "nonfinite": np.uint32}
    return all(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(np.ascontiguousarray(got[k]).view(views[k]), np.ascontiguousarray(want[k]).view(views[k])) for k in FIELDS)


def columns(rows, L):
    return {k: np.ascontiguousarray(rows[k][:, L]) for k in FIELDS}


def zeroed(rows, L):
    out = {k: v.copy() for k, v in rows.items()}
    for k in FIELDS:
        out[k][:, L] = 0
    return out


def lists_of(rng, N):
    """one entry; the two ends; 63, 64, 65 and 257 entries in a shuffled order (as many as N has); all of N"""
    out = [[N // 2], [0, N - 1]]
    for k in (63, 64, 65, 257):
        out.append(rng.permutation(N)[:min(k, N)])
    out.append(rng.permutation(N))
    return [np.asarray(L, dtype=np.int64) for L in out]
