"""The model of the level meters (fxb_meter_set_level, fxb_meter_read_level, fxb_meter_read_level_list, fxb_meter_select_level),
shared by tests/test_meter_level_stub.py (the CPU stand-in) and tests/test_gpu_meter_level.py (the kernels).  No test lives here.

level_model is the definition of include/fx8010_amd.h "Level meters" in numpy float32 / uint32 / uint64, one operation per line:
numpy float32 keeps denormals and rounds `level * release` once.  V, select and zeroed are the models of the queries over the
arrays fxb_meter_read_level returns.  The bar is equality of words: fp32 is compared as uint32."""
import ctypes as C

import numpy as np

ENVELOPE, QUIET = 0, 1   # FXB_LEVEL_ENVELOPE, FXB_LEVEL_QUIET
C_DOUBLE = C.c_double
SATURATED = np.uint32(0xFFFFFFFF)


def level_zero(channels, N):
    return {"level": np.zeros((channels, N), dtype=np.float32), "quiet": np.zeros((channels, N), dtype=np.uint32)}


def level_model(y, release, floor, acc=None):
    """y [S, channels, N] float32 is taken sample by sample; release, floor as the call was given them.  Returns the accumulators."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    S, channels, N = y.shape
    release = np.float32(release)
    floor = np.float32(floor)
    acc = level_zero(channels, N) if acc is None else {k: v.copy() for k, v in acc.items()}
    level = acc["level"]
    quiet = acc["quiet"]
    inf = np.float32(np.inf)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for s in range(S):
            mag = np.abs(y[s])
            fin = mag < inf
            w = np.where(fin, mag, zero)
            d = level * release
            level = np.where(w.view(np.uint32) > d.view(np.uint32), w, d)
            loud = ~fin | (w >= floor)
            more = quiet.astype(np.uint64) + np.uint64(1)
            more = np.minimum(more, np.uint64(SATURATED)).astype(np.uint32)
            quiet = np.where(loud, np.uint32(0), more)
    assert level.dtype == np.float32 and quiet.dtype == np.uint32
    return {"level": level, "quiet": quiet}


def same_level(got, want):
    return (got["level"].shape == want["level"].shape and got["level"].dtype == np.float32 and got["quiet"].dtype == np.uint32
            and np.array_equal(np.ascontiguousarray(got["level"]).view(np.uint32), np.ascontiguousarray(want["level"]).view(np.uint32))
            and np.array_equal(got["quiet"], want["quiet"]))


def zeroed(rows, L):
    out = {k: v.copy() for k, v in rows.items()}
    for k in out:
        out[k][:, L] = 0
    return out


def V(rows, stat):
    """the maximum over the channels of (double)level; the MINIMUM over the channels of (double)quiet"""
    if stat == ENVELOPE:
        return rows["level"].astype(np.float64).max(axis=0)
    return rows["quiet"].astype(np.float64).min(axis=0)


def select(rows, stat, threshold, below, first=0, n_range=None):
    value = V(rows, stat)
    n_range = value.size - first if n_range is None else n_range
    part = value[first:first + n_range]
    t = np.float64(threshold)
    return (first + np.nonzero(part < t if below else part >= t)[0]).astype(np.int64)


def thresholds(rows, stat):
    """-Inf, a negative value, 0, +Inf; the 12 lowest and 12 highest distinct values of V and a double between adjacent ones"""
    u = np.unique(V(rows, stat))
    if u.size > 24:
        u = np.concatenate([u[:12], u[-12:]])
    mid = [float(a + (b - a) / 2) for a, b in zip(u[:-1], u[1:]) if a < a + (b - a) / 2 < b]
    return [-np.inf, -1.0, 0.0, np.inf] + [float(v) for v in u] + mid


MARK = -0x0123456789ABCDEF
PAD = 7


def check_one(lib, b, rows, stat, t, below, first, n_range, cap, what=""):
    """one fxb_meter_select_level call against select(): the count, the list, and the words behind min(M, cap) untouched"""
    want = select(rows, stat, t, below, first, n_range)
    buf = np.full(max(cap, 0) + PAD, MARK, dtype=np.int64)
    m = int(lib.fxb_meter_select_level(b._h, int(stat), C.c_double(t), int(first), int(n_range), C.c_void_p(buf.ctypes.data), int(cap), 1 if below else 0))
    take = min(want.size, cap)
    tag = (what, stat, t, below, first, n_range, cap, m, want.size)
    assert m == want.size, tag
    assert np.array_equal(buf[:take], want[:take]), tag
    assert (buf[take:] == MARK).all(), ("words behind min(M, cap) were written",) + tag
    return want


def check_selects(lib, b, rows, N, what="", starts=(0, 1, 63, 64, 65, 77)):
    """both stats, both directions, thresholds() - at, between and beyond the distinct values of V, +-Inf included: the whole range
    with cap = N; then the caps 0, 1, M - 1, M, M + 7 and sub-ranges (77 starts in mid-wavefront) on thresholds that split the
    batch.  Returns the number of distinct match counts seen."""
    seen = set()
    for stat in (ENVELOPE, QUIET):
        ts = thresholds(rows, stat)
        for below in (False, True):
            for t in ts:
                seen.add(check_one(lib, b, rows, stat, t, below, 0, N, N, what).size)
        split = [t for t in ts if 0 < select(rows, stat, t, False).size < N][:3] or [0.0]
        for t in split:
            for below in (False, True):
                M = select(rows, stat, t, below).size
                for cap in sorted({0, 1, max(M - 1, 0), M, M + 7}):
                    check_one(lib, b, rows, stat, t, below, 0, N, cap, what)
                for first in starts:
                    if first > N:
                        continue
                    for n_range in sorted({0, min(1, N - first), min(64, N - first), N - first}):
                        want = check_one(lib, b, rows, stat, t, below, first, n_range, n_range, what)
                        check_one(lib, b, rows, stat, t, below, first, n_range, max(want.size - 1, 0), what)
    return len(seen)


def words(rng, shape, scale=1.0):
    """float32 words for y: levels over many decades with runs of silence, and, in places of their own, NaN, +-Inf, +-0,
    denormals, +-1.0"""
    x = (rng.standard_normal(shape) * scale * 10.0 ** rng.integers(-6, 1, shape)).astype(np.float32)
    x[rng.random(shape) < 0.4] = 0.0
    flat = x.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, -1e-44, 1.0, -1.0):
        flat[rng.integers(0, flat.size, max(flat.size // 60, 1))] = np.float32(v)
    return x
