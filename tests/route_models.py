"""The numpy models the route tests hold the device to, in one place: the definitions of include/fx8010_amd.h restated - the group
mix in its fixed fp32 order, bus gains with their ramp, sends, feeds, the four output meters.  Moved here unchanged from the
test files they grew up in (test_bus_stub.py, test_bus_gain_stub.py, test_bus_send_stub.py, test_bus_feed_stub.py,
test_meter_stub.py), which import them back and still test them against the sums written out one add at a time; the meter
queries, target and level meters have meter_list_model.py, meter_target_model.py and meter_level_model.py."""
import numpy as np


def mix_model(y, K):
    """[..., N] -> [..., G]: every group's sum in the order include/fx8010_amd.h fixes, in fp32 (numpy adds float32 arrays in
    float32, round to nearest, one rounding per add): 64 partial sums start at +0.0; member m = j * 64 + l of a group, where it
    exists, is added to p[l] for j ascending; then p[l] = p[l] + p[l + step] for l < step, step = 32 ... 1; the sum is p[0].
    Only the lanes below W = min(64, K) are held: no member is ever added to a lane at or above K, so those lanes are +0.0 when
    the tree starts, a tree step can only give them +0.0 + +0.0, and where a step reads one of them it adds that +0.0."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    N = y.shape[-1]
    K = min(int(K), N)
    G, J, W = -(-N // K), -(-K // 64), min(64, K)
    lead = y.shape[:-1]
    members = np.zeros(lead + (G * K,), dtype=np.float32)
    members[..., :N] = y
    exists = np.arange(G * K) < N
    members, exists = members.reshape(lead + (G, K)), exists.reshape(G, K)
    p = np.zeros(lead + (G, W), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(J):
            w = min(64, K - j * 64)
            p[..., :w] = np.where(exists[:, j * 64:j * 64 + w], p[..., :w] + members[..., j * 64:j * 64 + w], p[..., :w])
        for step in (32, 16, 8, 4, 2, 1):
            held = min(step, W)                      # lanes l < step that are held
            paired = max(0, min(W - step, step))     # ... whose partner l + step is held as well
            other = np.zeros(lead + (G, held), dtype=np.float32)
            other[..., :paired] = p[..., step:step + paired]
            p[..., :held] = p[..., :held] + other
    return np.ascontiguousarray(p[..., 0])


def expand(x, K, N):
    """[..., G] -> [..., N]: instance n hears column n // K"""
    return np.ascontiguousarray(x[..., np.arange(N) // min(int(K), N)])


def same_words(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and (np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


DENORMAL, TINY, HUGE = np.float32(1e-41), np.float32(2.0 ** -126), np.float32(1e30)


def gain_weights(a, b, ramp, S):
    """[S, C, N] float32: the weight of every member at every sample of a call of S samples (numpy works on float32 arrays in
    float32, round to nearest, one rounding per operation, denormals kept)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if not ramp:
        return np.ascontiguousarray(np.broadcast_to(b, (S,) + b.shape))
    r = np.float32(1.0) / np.float32(S)
    t = np.arange(1, S + 1).astype(np.float32) * r          # (float)(s + 1) * r
    with np.errstate(all="ignore"):
        d = b - a
        w = a[None] + d[None] * t[:, None, None]
    w[S - 1] = b
    return np.ascontiguousarray(w, dtype=np.float32)


def gain_mix_model(y, a, b, ramp, S, K):
    """y: [S, C, N], a / b: [C, N] -> [S, C, G]: the definition of include/fx8010_amd.h "Bus gains" feeding mix_model"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert y.shape[0] == S and y.ndim == 3
    w = gain_weights(a, b, ramp, S)
    with np.errstate(all="ignore"):
        term = np.where(w == 0.0, np.float32(0.0), w * y).astype(np.float32)
    return mix_model(term, K)


def gains_for(rng, C_, N, special=True):
    g = (rng.standard_normal((C_, N)) * 10.0 ** rng.integers(-3, 2, (C_, N))).astype(np.float32)
    if special:
        for i, v in enumerate((np.float32(0.0), np.float32(-0.0), np.float32(-1.5), DENORMAL, TINY, HUGE, -HUGE)):
            g[(i // N) % C_, (i * 3) % N] = v   # (for N = 1 the last one stays)
    return g


CHUNK = 1024


def tree(seq):
    """T of include/fx8010_amd.h "Bus sends" over the last axis, [..., L] -> [...]: 64 partial sums start at +0.0; v[j*64+l],
    where it exists, is added to p[l] for j ascending; then p[l] = p[l] + p[l+step] for l < step, step = 32 .. 1; T is p[0]
    (numpy adds float32 arrays in float32, round to nearest, one rounding per add, denormals kept)"""
    seq = np.ascontiguousarray(seq, dtype=np.float32)
    L = seq.shape[-1]
    p = np.zeros(seq.shape[:-1] + (64,), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(-(-L // 64)):
            w = min(64, L - j * 64)
            p[..., :w] = p[..., :w] + seq[..., j * 64:j * 64 + w]
        for step in (32, 16, 8, 4, 2, 1):
            p[..., :step] = p[..., :step] + p[..., step:2 * step]
    return np.ascontiguousarray(p[..., 0])


def send_model(y, offsets, members, a, b, ramp, S):
    """y: [S, C, N], a / b: [C, E] -> [S, C, A]: the definition of include/fx8010_amd.h "Bus sends".  The weights are those of
    "Bus gains" by entry; the positions of a bus are cut into chunks of 1 024, a bus of one chunk is that chunk's T, a larger one
    T over its chunk sums, an empty one +0.0"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    offsets, members = np.asarray(offsets, dtype=np.int64), np.asarray(members, dtype=np.int64)
    assert y.ndim == 3 and y.shape[0] == S
    A = offsets.size - 1
    w = gain_weights(a, b, ramp, S)   # [S, C, E]
    with np.errstate(all="ignore"):
        term = np.where(w == 0.0, np.float32(0.0), w * y[:, :, members[:offsets[-1]]]).astype(np.float32)
    out = np.zeros(y.shape[:2] + (A,), dtype=np.float32)
    for bus in range(A):
        lo, hi = int(offsets[bus]), int(offsets[bus + 1])
        if hi - lo <= CHUNK:
            out[:, :, bus] = tree(term[:, :, lo:hi])
        else:
            out[:, :, bus] = tree(np.stack([tree(term[:, :, q:min(q + CHUNK, hi)]) for q in range(lo, hi, CHUNK)], axis=-1))
    return out


def feed_model(src, offsets, sources, a, b, ramp, S):
    """src: [S, C, M], a / b: [C, E] (b None: unweighted) -> [S, C, N]: the definition of include/fx8010_amd.h "Bus feeds".
    Instance n owns the entries offsets[n] .. offsets[n+1] - 1; entry e has x = src[s, c, sources[e]] and the term x (unweighted)
    or (w == 0 ? +0.0 : w * x) with the weights of "Bus gains" by entry; the word is +0.0 for no entry, term_0 for one (a select:
    the pattern moves), else ((term_0 + term_1) + term_2) + ... (numpy adds float32 arrays in float32, round to nearest, one
    rounding per add, denormals kept)"""
    src = np.ascontiguousarray(src, dtype=np.float32)
    offsets, sources = np.asarray(offsets, dtype=np.int64), np.asarray(sources, dtype=np.int64)
    assert src.ndim == 3 and src.shape[0] == S
    N = offsets.size - 1
    count = np.diff(offsets)
    out = np.zeros(src.shape[:2] + (N,), dtype=np.float32)
    w = None if b is None else gain_weights(b if a is None else a, b, ramp, S)   # [S, C, E]
    with np.errstate(all="ignore"):
        for k in range(int(count.max()) if N else 0):
            has = k < count
            e = np.where(has, offsets[:-1] + k, 0)
            x = src[:, :, sources[e]]
            term = x if w is None else np.where(w[:, :, e] == 0.0, np.float32(0.0), w[:, :, e] * x).astype(np.float32)
            out = np.where(has, term if k == 0 else out + term, out)
    return np.ascontiguousarray(out, dtype=np.float32)


FIELDS = ("energy", "peak", "full_scale", "nonfinite")


def meter_zero(channels, N):
    return {"energy": np.zeros((channels, N), dtype=np.float64), "peak": np.zeros((channels, N), dtype=np.float32),
            "full_scale": np.zeros((channels, N), dtype=np.uint32), "nonfinite": np.zeros((channels, N), dtype=np.uint32)}


def meter_model(y, acc=None):
    """The definition of include/fx8010_amd.h, restated: y [S, channels, N] float32 is taken sample by sample into the four
    accumulators `acc` (a new set when None).  One fp64 add of an exact product per sample; max; two saturating counts."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    S, channels, N = y.shape
    acc = meter_zero(channels, N) if acc is None else {k: v.copy() for k, v in acc.items()}
    with np.errstate(all="ignore"):
        mag = np.abs(y)
        fin = mag < np.float32(np.inf)                        # false for NaN and +-Inf
        w = np.where(fin, mag, np.float32(0.0)).astype(np.float32)
        for s in range(S):
            wd = w[s].astype(np.float64)
            acc["energy"] = acc["energy"] + wd * wd           # the product is exact: one rounding, in the add
        if S:
            acc["peak"] = np.maximum(acc["peak"], w.max(axis=0))
        for key, hit in (("full_scale", fin & (mag >= np.float32(1.0))), ("nonfinite", ~fin)):
            acc[key] = np.minimum(acc[key].astype(np.uint64) + hit.sum(axis=0, dtype=np.uint64), 0xFFFFFFFF).astype(np.uint32)
    return acc


def same_meters(got, want):
    """bit for bit: fp64 and fp32 words are compared as integers"""
    views = {"energy": np.uint64, "peak": np.uint32, "full_scale": np.uint32, "nonfinite": np.uint32}
    for k in FIELDS:
        if got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or not np.array_equal(got[k].view(views[k]), want[k].view(views[k])):
            return False
    return True
