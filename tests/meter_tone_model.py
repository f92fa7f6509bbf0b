"""The model of the tone meters (fxb_meter_set_tones, fxb_meter_read_tones, fxb_meter_read_tones_list, fxb_meter_select_tone,
fxb_meter_rank_tone), shared by tests/test_meter_tone_model.py (the definition itself), tests/test_meter_tone_stub.py (the CPU
stand-in) and tests/test_gpu_meter_tone.py (the kernels).  No test lives here.

tone_model is the definition of include/fx8010_amd.h "Tone meters" in numpy float64, one operation per line: numpy rounds every
product, sum and difference once and fuses nothing.  power is P; V, select, rank (numpy.lexsort, as meter_rank_model.rank) and
zeroed are the models of the queries over the arrays fxb_meter_read_tones returns.  The bar is equality of words: fp64 is
compared as uint64 everywhere.  Input words come from meter_level_model.words."""
import ctypes as C

import numpy as np

import meter_level_model as L
import meter_rank_model as R

MAX_TONES = 8                     # FXB_METER_MAX_TONES
BELOW, LARGEST = 1, 2             # FXB_METER_BELOW, FXB_METER_LARGEST
MARK, VMARK, PAD = R.MARK, R.VMARK, R.PAD
words = L.words


def coeff(k, n):
    """c = 2 cos(2 pi k / n) as the caller computes it: the library takes the double as given"""
    return float(2.0 * np.cos(2.0 * np.pi * k / n))


def tone_zero(tones, channels, N):
    return {"s1": np.zeros((tones, channels, N), dtype=np.float64), "s2": np.zeros((tones, channels, N), dtype=np.float64)}


def tone_model(y, coeffs, acc=None):
    """y [S, channels, N] float32 is taken sample by sample; coeffs as the call was given them.  Returns {"s1", "s2"}, [K, C, N]."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    S, channels, N = y.shape
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1) + 0.0   # (-0.0 is taken as +0.0)
    acc = tone_zero(c.size, channels, N) if acc is None else {k: v.copy() for k, v in acc.items()}
    s1 = acc["s1"]
    s2 = acc["s2"]
    ck = c[:, None, None]
    with np.errstate(all="ignore"):
        for s in range(S):
            fin = np.abs(y[s]) < np.float32(np.inf)
            x = np.where(fin, y[s].astype(np.float64), np.float64(0.0))
            p = ck * s1
            q = x[None] + p
            s0 = q - s2
            s2 = s1
            s1 = s0
    assert s1.dtype == np.float64 and s2.dtype == np.float64
    return {"s1": s1, "s2": s2}


def power(acc, coeffs):
    """P = (s1*s1 + s2*s2) - (c*s1)*s2: five operations, in this order"""
    c = (np.asarray(coeffs, dtype=np.float64).reshape(-1) + 0.0)[:, None, None]
    s1, s2 = acc["s1"], acc["s2"]
    with np.errstate(all="ignore"):
        a = s1 * s1
        b = s2 * s2
        total = a + b
        p = c * s1
        m = p * s2
        return total - m


def rows_of(acc, coeffs):
    """what fxb_meter_read_tones returns for these accumulators"""
    return {"s1": acc["s1"], "s2": acc["s2"], "power": power(acc, coeffs)}


def same_tones(got, want, keys=("s1", "s2", "power")):
    return all(got[k].shape == want[k].shape and got[k].dtype == np.float64
               and np.array_equal(np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64)) for k in keys)


def differing(got, want):
    return {k: np.argwhere(np.ascontiguousarray(got[k]).view(np.uint64) != np.ascontiguousarray(want[k]).view(np.uint64))[:4].tolist() for k in ("s1", "s2", "power")}


def zeroed(acc, lst):
    out = {k: v.copy() for k, v in acc.items()}
    for k in out:
        out[k][:, :, lst] = 0.0
    return out


def V(rows, tone):
    """the maximum over the channels of P(tone, c, n)"""
    return rows["power"][tone].max(axis=0)


def select(rows, tone, threshold, below, first=0, n_range=None):
    value = V(rows, tone)
    n_range = value.size - first if n_range is None else n_range
    part = value[first:first + n_range]
    t = np.float64(threshold)
    return (first + np.nonzero(part < t if below else part >= t)[0]).astype(np.int64)


def rank(rows, tone, k, threshold=-np.inf, below=False, largest=False, first=0, n_range=None):
    """(M, list, values) through numpy.lexsort, as meter_rank_model.rank does it"""
    return R.rank(V(rows, tone), k, threshold, below, largest, first, n_range)


def thresholds(rows, tone):
    """-Inf, 0, +Inf; the 8 lowest and 8 highest distinct values of V and a double between adjacent ones"""
    u = np.unique(V(rows, tone))
    if u.size > 16:
        u = np.concatenate([u[:8], u[-8:]])
    mid = [float(a + (b - a) / 2) for a, b in zip(u[:-1], u[1:]) if np.isfinite(b - a) and a < a + (b - a) / 2 < b]
    return [-np.inf, 0.0, np.inf] + [float(v) for v in u] + mid


def check_select(lib, b, rows, tone, t, below, first, n_range, cap, what=""):
    """one fxb_meter_select_tone call against select(): the count, the list, and the words behind min(M, cap) untouched"""
    want = select(rows, tone, t, below, first, n_range)
    buf = np.full(max(cap, 0) + PAD, MARK, dtype=np.int64)
    m = int(lib.fxb_meter_select_tone(b._h, int(tone), C.c_double(t), int(first), int(n_range), C.c_void_p(buf.ctypes.data), int(cap), BELOW if below else 0))
    take = min(want.size, cap)
    tag = (what, tone, t, below, first, n_range, cap, m, want.size)
    assert m == want.size, tag
    assert np.array_equal(buf[:take], want[:take]), tag
    assert (buf[take:] == MARK).all(), ("words behind min(M, cap) were written",) + tag
    return want


def check_selects(lib, b, rows, N, tones, what="", starts=(0, 1, 63, 64, 65, 77)):
    """every tone, both directions, thresholds(): the whole range with cap = N; then caps and sub-ranges on a threshold that splits
    the batch.  Returns the number of distinct match counts seen."""
    seen = set()
    for tone in range(tones):
        ts = thresholds(rows, tone)
        for below in (False, True):
            for t in ts:
                seen.add(check_select(lib, b, rows, tone, t, below, 0, N, N, what).size)
        split = [t for t in ts if 0 < select(rows, tone, t, False).size < N][:1] or [0.0]
        for t in split:
            for below in (False, True):
                M = select(rows, tone, t, below).size
                for cap in sorted({0, 1, max(M - 1, 0), M, M + 7}):
                    check_select(lib, b, rows, tone, t, below, 0, N, cap, what)
                for first in starts:
                    if first > N:
                        continue
                    for n_range in sorted({0, min(1, N - first), min(64, N - first), N - first}):
                        want = check_select(lib, b, rows, tone, t, below, first, n_range, n_range, what)
                        check_select(lib, b, rows, tone, t, below, first, n_range, max(want.size - 1, 0), what)
    return len(seen)


def check_rank(lib, b, rows, tone, k, t=-np.inf, below=False, largest=False, first=0, n_range=None, what=""):
    """one fxb_meter_rank_tone call against rank(): M, the list word for word, the values as words, the marks behind min(M, k)"""
    N = rows["power"].shape[2]
    n_range = N - first if n_range is None else n_range
    m, want, values = rank(rows, tone, k, t, below, largest, first, n_range)
    room = max(int(k), 0) + PAD
    lst, val = np.full(room, MARK, dtype=np.int64), np.full(room, VMARK, dtype=np.uint64)
    got = int(lib.fxb_meter_rank_tone(b._h, int(tone), int(k), C.c_double(t), int(first), int(n_range), C.c_void_p(lst.ctypes.data), C.c_void_p(val.ctypes.data),
                                      (BELOW if below else 0) | (LARGEST if largest else 0)))
    tag = (what, tone, k, t, below, largest, first, n_range, got, m)
    r = want.size
    assert got == m, tag
    assert np.array_equal(lst[:r], want), tag + (lst[:8], want[:8])
    assert np.array_equal(val[:r], np.ascontiguousarray(values).view(np.uint64)), tag
    assert (lst[r:] == MARK).all() and (val[r:] == VMARK).all(), ("words behind min(M, k) were written",) + tag
    return m


def check_ranks(lib, b, rows, tones, what="", starts=(0, 65)):
    """every tone, the four flag combinations: the whole range on -Inf, a middle value of V and +Inf with meter_rank_model.k_values;
    sub-ranges on the middle threshold.  Returns the number of calls."""
    calls = 0
    N = rows["power"].shape[2]
    for tone in range(tones):
        value = V(rows, tone)
        for below in (False, True):
            for largest in (False, True):
                for t in R.thresholds(value):
                    m = rank(rows, tone, 0, t, below, largest)[0]
                    for k in R.k_values(m):
                        check_rank(lib, b, rows, tone, k, t, below, largest, 0, N, what)
                        calls += 1
                t = R.thresholds(value)[1]
                for first in starts:
                    if first > N:
                        continue
                    for n_range in sorted({0, min(64, N - first), N - first}):
                        for k in (3, n_range):
                            check_rank(lib, b, rows, tone, k, t, below, largest, first, n_range, what)
                            calls += 1
    return calls


def sines(S, bins, amplitude, N, channels=1, phase=0.3):
    """x [S, channels, N] float32: voice n carries amplitude * sin(2 pi bins[n % len(bins)] t / S + phase) on every channel"""
    t = np.arange(S, dtype=np.float64)[:, None]
    k = np.asarray(bins, dtype=np.float64)[np.arange(N) % len(bins)][None, :]
    x = (amplitude * np.sin(2.0 * np.pi * k * t / S + phase)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(x[:, None, :], (S, channels, N)))
