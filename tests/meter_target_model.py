"""The model of the target meters (fxb_meter_set_target, fxb_meter_read_match, fxb_meter_select_match, fxb_meter_best), shared by
tests/test_meter_target_stub.py (the CPU stand-in) and tests/test_gpu_meter_target.py (the kernels).  No test lives here.

match_model is the definition of include/fx8010_amd.h "Target meters" in numpy float64, one operation per line: every line is
one IEEE operation with one rounding, numpy never fuses.  V, select and best are the models of the queries over the arrays
fxb_meter_read_match returns.  The bar is equality: fp64 words are compared as integers."""
import ctypes as C

import numpy as np

ERROR, CROSS = 0, 1   # FXB_MATCH_ERROR, FXB_MATCH_CROSS
C_DOUBLE = C.c_double


def match_zero(channels, N):
    return {"err": np.zeros((channels, N), dtype=np.float64), "cross": np.zeros((channels, N), dtype=np.float64)}


def match_model(y, target, group, pos, loop, acc=None):
    """y [S, channels, N] float32 is taken sample by sample against target [T, channels, G] float32 (G = ceil(N / group),
    instance n against column n // group), the first sample at target position `pos`.  Returns (acc, the position afterwards)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    target = np.ascontiguousarray(target, dtype=np.float32)
    S, channels, N = y.shape
    T = target.shape[0]
    group = min(int(group), N)
    assert target.shape[1:] == (channels, -(-N // group)), (target.shape, channels, N, group)
    col = np.arange(N) // group
    acc = match_zero(channels, N) if acc is None else {k: v.copy() for k, v in acc.items()}
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        for s in range(S):
            q = pos + s
            if loop:
                q = q % T
            if q >= T:
                continue
            t = target[q][:, col]
            ok = (np.abs(y[s]) < inf) & (np.abs(t) < inf)
            yd = y[s].astype(np.float64)
            td = t.astype(np.float64)
            d = yd - td
            e = d * d
            err = acc["err"] + e
            yt = yd * td
            cross = acc["cross"] + yt
            acc["err"] = np.where(ok, err, acc["err"])
            acc["cross"] = np.where(ok, cross, acc["cross"])
    after = pos + S
    if loop:
        after = after % T
    return acc, after


def same_match(got, want):
    return all(got[k].shape == want[k].shape and got[k].dtype == np.float64 and np.array_equal(np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64))
               for k in ("err", "cross"))


def zeroed(rows, L):
    out = {k: v.copy() for k, v in rows.items()}
    for k in out:
        out[k][:, L] = 0
    return out


def V(rows, stat):
    """((v0 + v1) + v2) + v3 over the channels, in channel order, starting from v0"""
    v = rows[("err", "cross")[stat]]
    out = v[0].copy()
    for c in range(1, v.shape[0]):
        out = out + v[c]
    return out


def select(rows, stat, threshold, below, first=0, n_range=None):
    value = V(rows, stat)
    n_range = value.size - first if n_range is None else n_range
    part = value[first:first + n_range]
    t = np.float64(threshold)
    return (first + np.nonzero(part < t if below else part >= t)[0]).astype(np.int64)


def best(rows, stat, group, largest=False):
    """(winner, value) per group: the smallest (largest) V, ties to the smallest instance number"""
    value = V(rows, stat)
    N = value.size
    group = min(int(group), N)
    G = -(-N // group)
    winner, out = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.float64)
    for g in range(G):
        part = value[g * group:(g + 1) * group]
        k = int(np.argmax(part) if largest else np.argmin(part))   # (the first of equal ones)
        winner[g], out[g] = g * group + k, part[k]
    return winner, out


def same_best(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


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
    want = select(rows, stat, t, below, first, n_range)
    buf = np.full(max(cap, 0) + PAD, MARK, dtype=np.int64)
    m = int(lib.fxb_meter_select_match(b._h, int(stat), C.c_double(t), int(first), int(n_range), C.c_void_p(buf.ctypes.data), int(cap), 1 if below else 0))
    take = min(want.size, cap)
    tag = (what, stat, t, below, first, n_range, cap, m, want.size)
    assert m == want.size, tag
    assert np.array_equal(buf[:take], want[:take]), tag
    assert (buf[take:] == MARK).all(), ("words behind min(M, cap) were written",) + tag
    return want


def check_selects(lib, b, rows, N, what=""):
    """both stats, both directions, thresholds(): the whole range with cap = N; then the caps 0, 1, M - 1, M, M + 1, N + 5 and the
    ranges first in {0, 1, 63, 64, 65} x n_range in {0, 1, 64, N - first} on thresholds that split the batch (the cases of
    meter_list_model.check_selects, on V).  Returns the number of distinct match counts seen."""
    seen = set()
    for stat in (0, 1):
        ts = thresholds(rows, stat)
        for below in (False, True):
            for t in ts:
                seen.add(check_one(lib, b, rows, stat, t, below, 0, N, N, what).size)
        split = [t for t in ts if 0 < select(rows, stat, t, False).size < N][:3] or [0.0]
        for t in split:
            for below in (False, True):
                M = select(rows, stat, t, below).size
                for cap in sorted({0, 1, max(M - 1, 0), M, M + 1, N + 5}):
                    check_one(lib, b, rows, stat, t, below, 0, N, cap, what)
                for first in (0, 1, 63, 64, 65):
                    if first > N:
                        continue
                    for n_range in sorted({0, min(1, N - first), min(64, N - first), N - first}):
                        want = check_one(lib, b, rows, stat, t, below, first, n_range, n_range, what)
                        check_one(lib, b, rows, stat, t, below, first, n_range, max(want.size - 1, 0), what)
    return len(seen)


def words(rng, shape, scale=1.0):
    """float32 words for y or t: levels over many decades and, in places of their own, NaN, +-Inf, +-0, denormals, +-1.0"""
    x = (rng.standard_normal(shape) * scale * 10.0 ** rng.integers(-6, 1, shape)).astype(np.float32)
    flat = x.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, -1e-44, 1.0, -1.0):
        flat[rng.integers(0, flat.size, max(flat.size // 60, 1))] = np.float32(v)
    return x
