"""Meter queries by list without a GPU: fxb_meter_select / fxb_meter_read_list / fxb_meter_reset_list on the library's host sources
linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like
tests/test_tram_list_stub.py (this file is also that child).  The stand-ins of the kernels (tests/hipstub/fx_meter_list_stub.cpp)
work in stream order with a formulation of their own - one loop over the range, long double compares.

The stand-in's emulation launch copies input to output, so the meters are a function of the input the test builds
(meter_list_model.voices).  The model is numpy over the arrays fxb_meter_read returns (meter_list_model.model); the bar is
equality everywhere, and the words of a list buffer behind min(M, cap) must still hold their mark.  This checks the host layers:
argument checks, staging, the copy back in two parts, ranges and lists by shard, ordering, the counters.  The kernels themselves:
tests/test_gpu_meter_list.py.  The Python-driven cases do not run under a sanitizer: that is tests/hipstub/meter_list_checks.cpp,
a program of its own (tests/test_meter_list_checks.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_list_model as M  # noqa: E402
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, PROGRAM, ROOT, STEREO, Pinned  # noqa: E402
from test_meter_stub import meter_model, meter_zero  # noqa: E402

N = 200
QUAD = STEREO.replace("output out1 1", "input in2 2\ninput in3 3\noutput out1 1\noutput out2 2\noutput out3 3").replace("\nend", "\nmacs out2, in2, a, 0.5\nmacs out3, in3, a, 0.5\nend")
TEXT = {1: PROGRAM, 2: STEREO, 4: QUAD}


def run_child(which, marker, devices=1):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("channels", (1, 2, 4))
def test_select_equals_the_numpy_model_on_the_hip_stand_in(channels):
    """N = 200; all four stats, both directions; thresholds, match patterns, caps and ranges of meter_list_model"""
    run_child("select-%d" % channels, "meter list select ok")


def test_read_list_and_its_reset_on_the_hip_stand_in():
    run_child("read", "meter list read ok")


def test_reset_list_between_blocks_on_other_streams_on_the_hip_stand_in():
    run_child("streams", "meter list streams ok")


def test_meter_list_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "meter list refusals ok")


def test_meter_list_calls_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "meter list shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def list_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_meter_selects", "fxstub_meter_gathers", "fxstub_meter_zeros", "fxstub_meter_list_strays", "fxstub_live_allocations", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_meter_launches"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def handle(A, n, channels, devices=None):
    b = A.Batch(n, channels, 0) if devices is None else A.Batch(n, channels, devices=devices)
    assert b.load_text(TEXT[channels]), b.errors()
    assert b.meter_enable() == 0
    return b


def clean(lib):
    assert lib.fxstub_meter_list_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0


def child_select(channels):
    A, lib = list_library()
    b = handle(A, N, channels)
    x = M.voices(N, channels, 33, seed=channels)
    b.process_block(x[:16])
    b.process_block(x[16:])
    rows = b.meter_read()
    assert M.same_rows(rows, meter_model(x)), "the stand-in's emulation launch copies its input"
    loud = rows["peak"].argmax(axis=0)
    assert channels == 1 or len(set(loud[rows["peak"].max(axis=0) > 0].tolist())) == channels, "the maximum sits on every channel somewhere"
    before = (b.info("meter_selects"), lib.fxstub_meter_selects())
    kinds = M.check_selects(lib, b, rows, N)
    assert kinds >= 6, kinds
    assert b.info("meter_selects") - before[0] == lib.fxstub_meter_selects() - before[1] > 100
    # on these mixed levels: none and all by the thresholds at the ends; the quiet voices; about a half (the match patterns by name,
    # each the whole answer of one select over the batch, follow below: check_patterns)
    V = M.value(rows, 1)
    for t, below, want in ((np.inf, False, []), (-np.inf, False, list(range(N))), (np.inf, True, list(range(N))), (0.0, True, []), (-1.0, True, [])):
        got, m = b.meter_select(A.METER_PEAK, t, below=below)
        assert got.tolist() == want and m == len(want), (t, below)
    # (V is quiet where a voice is silent: BELOW 0.05 finds those; instance N - 1 alone lies in 0.05 .. 0.2)
    quiet, m = b.meter_select(A.METER_PEAK, 0.2, below=True)
    silent, _ = b.meter_select(A.METER_PEAK, 0.05, below=True)
    assert np.setdiff1d(quiet, silent).tolist() == [N - 1] and m == quiet.size
    rail = np.nonzero(V >= 0.999)[0]
    got, m = b.meter_select(A.METER_PEAK, 0.95, first=0, n_range=3)
    assert got.tolist() == [0] and m == 1, "in its neighbourhood only instance 0 is that loud"
    got, _ = b.meter_select(A.METER_PEAK, 0.85)
    assert np.array_equal(np.setdiff1d(got, rail), np.setdiff1d(np.array([0, 64, 128, 192]), rail)), "every 64th (and the voices at the rail)"
    half, _ = b.meter_select(A.METER_PEAK, 0.5)
    assert N // 4 < half.size < 3 * N // 4
    # one instance's value exactly: `>=` includes it, BELOW excludes it; a double between two adjacent float peaks
    k = 77
    at, _ = b.meter_select(A.METER_ENERGY, M.value(rows, 0)[k])
    under, _ = b.meter_select(A.METER_ENERGY, M.value(rows, 0)[k], below=True)
    assert k in at and k not in under and at.size + under.size == N
    p = np.float32(0.6)
    up = np.nextafter(p, np.float32(1.0))
    between = (float(p) + float(up)) / 2
    assert float(p) < between < float(up) and np.float32(between) in (p, up)
    got, _ = b.meter_select(A.METER_PEAK, between)
    assert np.array_equal(got, np.nonzero(V > float(p))[0]) and (V == float(p)).any(), "a float32 compare would have taken the voices at 0.6 along, or dropped those just above"
    # a count query
    assert lib.fxb_meter_select(b._h, 1, C.c_double(0.5), 0, N, None, 0, 0) == half.size
    assert M.same_rows(b.meter_read(), rows) and b.meter_samples() == 33
    # the match patterns by name: none, all, only instance 0, only N - 1, every 64th - each ONE select over the whole batch
    assert M.check_patterns(lib, b, N, channels) == 7
    b.close()
    clean(lib)
    print("meter list select ok")


def child_read():
    A, lib = list_library()
    rng = np.random.default_rng(3)
    channels = 2
    b = handle(A, N, channels)
    x = M.voices(N, channels, 33, seed=9)
    b.process_block(x)
    rows = b.meter_read()
    lists = M.lists_of(rng, N) + [np.array([5, 5, N - 1, 0, 5], dtype=np.int64), np.concatenate([rng.permutation(N), rng.permutation(N)[:50]]).astype(np.int64)]
    for L in lists:
        assert M.same_rows(b.meter_read_list(L), M.columns(rows, L)), L[:8]
    assert b.info("meter_list_reads") == len(lists) == lib.fxstub_meter_gathers()
    # null arrays, one at a time and all four
    L = np.array([N - 1, 0, 130], dtype=np.int64)
    for k, field in enumerate(M.FIELDS):
        out = [None] * 4
        out[k] = np.full((channels, 3), 0x55, dtype=rows[field].dtype)
        assert lib.fxb_meter_read_list(b._h, ptr(L), 3, *[ptr(o) for o in out], 0) == 0
        assert out[k].tobytes() == rows[field][:, L].tobytes(), field
    assert lib.fxb_meter_read_list(b._h, ptr(L), 3, None, None, None, None, 0) == 0
    assert lib.fxb_meter_read_list(b._h, None, 0, None, None, None, None, 1) == 0 and b.meter_read_list([])["peak"].shape == (channels, 0)
    # reset = 1 zeroes exactly the listed columns: the whole fxb_meter_read before and after
    for L in M.lists_of(rng, N):
        before = b.meter_read()
        assert M.same_rows(b.meter_read_list(L, reset=True), M.columns(before, L))
        assert M.same_rows(b.meter_read(), M.zeroed(before, L))
        b.process_block(M.voices(N, channels, 8, seed=int(L[0])))
    # reset_list: repeats allowed, the sample count stays
    b.process_block(x)
    before, samples, resets = b.meter_read(), b.meter_samples(), b.info("meter_list_resets")
    L = np.array([3, 3, 0, N - 1, 64, 3], dtype=np.int64)
    assert b.meter_reset_list(L) == 0 and b.sync() == 0
    assert M.same_rows(b.meter_read(), M.zeroed(before, L)) and b.meter_samples() == samples and b.info("meter_list_resets") == resets + 1 == lib.fxstub_meter_zeros()
    assert b.meter_reset_list([]) == 0 and b.info("meter_list_resets") == resets + 1
    # a full reset still zeroes everything and the count
    b.meter_read(reset=True)
    assert M.same_rows(b.meter_read(), meter_zero(channels, N)) and b.meter_samples() == 0
    assert b.info("meter_selects") == 0 and [b.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")] == [b._lib.fxb_info(b._h, w) for w in (57, 58, 59)]
    b.close()
    clean(lib)
    print("meter list read ok")


def child_streams():
    """a list reset behind a slow block on stream A returns while that block is still running and has not run yet; a block on
    stream B is ordered behind it; the result is block 1 zeroed on L, plus block 2"""
    A, lib = list_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(5)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    n, S = 1000, 8
    b = handle(A, n, 1)
    b.process_block(M.voices(n, 1, S, seed=1))
    b.meter_reset_list([1, 2])   # (the staging exists before anything is timed)
    b.meter_read(reset=True)

    def fresh(seed):
        p, o = pinned((S, 1, n)), pinned((S, 1, n))
        p[...] = M.voices(n, 1, S, seed=seed)
        o[...] = -7.0
        return p, o

    def dev(bufs, stream):
        return lib.fxb_process_block_dev(b._h, ptr(bufs[0]), ptr(bufs[1]), S, stream)

    first, second, third = fresh(11), fresh(12), fresh(13)
    L = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:63]]).astype(np.int64)
    zeros = lib.fxstub_meter_zeros()
    lib.fxstub_set_kernel_micros(150000)   # the emulation launch takes 150 ms
    assert dev(first, streams[0]) == 0
    assert b.meter_reset_list(L) == 0
    L_given = L.copy()
    L[:] = 7   # the caller's list is free on return
    assert (first[1][S - 1] == -7.0).all(), "the list reset returned while the block in front of it was still running"
    assert lib.fxstub_meter_zeros() == zeros, "... and it is queued behind that block: it has not run"
    lib.fxstub_set_kernel_micros(150)
    assert dev(second, streams[1]) == 0
    got, m = b.meter_select(A.METER_ENERGY, 0.0)   # waits for everything queued
    assert lib.fxstub_meter_zeros() == zeros + 1 and not (first[1][S - 1] == -7.0).any() and m == n
    want = meter_model(second[0], M.zeroed(meter_model(first[0]), L_given))
    rows = b.meter_read()
    assert M.same_rows(rows, want) and not M.same_rows(rows, meter_model(second[0], meter_model(first[0])))
    assert b.meter_samples() == 2 * S, "the handle-wide count since the last full reset"
    # a second reset right behind the first waits for it on the host only; a block on the default stream; the list read covers it
    L2 = L_given[::-1][:20].copy()
    assert b.meter_reset_list(L_given[:5]) == 0 and b.meter_reset_list(L2) == 0
    assert dev(third, None) == 0
    want = meter_model(third[0], M.zeroed(want, np.concatenate([L_given[:5], L2])))
    assert M.same_rows(b.meter_read_list(np.arange(n)), want)
    # every call that reads the meters observes a reset that is still queued behind a slow block
    for name, call in (("select", lambda: b.meter_select(A.METER_PEAK, 0.5)), ("read_list", lambda: b.meter_read_list([0, 1])), ("read", lambda: b.meter_read()), ("sync", lambda: b.sync())):
        zeros = lib.fxstub_meter_zeros()
        lib.fxstub_set_kernel_micros(30000)
        assert dev(first, streams[0]) == 0
        assert b.meter_reset_list(L_given) == 0 and lib.fxstub_meter_zeros() == zeros
        lib.fxstub_set_kernel_micros(150)
        call()
        assert lib.fxstub_meter_zeros() == zeros + 1, name
        want = M.zeroed(meter_model(first[0], want), L_given)
        assert M.same_rows(b.meter_read(), want), name
    pinned.free()
    b.close()
    clean(lib)
    print("meter list streams ok")


def child_refusals():
    A, lib = list_library()
    channels = 2
    b = handle(A, N, channels)
    b.process_block(M.voices(N, channels, 16, seed=2))
    rows = b.meter_read()
    counters = lambda: ([b.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")], lib.fxstub_meter_selects(), lib.fxstub_meter_gathers(), lib.fxstub_meter_zeros())  # noqa: E731
    seen = counters()
    buf = np.full(N + 8, M.MARK, dtype=np.int64)
    selects = (("stat = 4", "stat", 4, 0.0, 0, N, buf, N, 0), ("stat = -1", "stat", -1, 0.0, 0, N, buf, N, 0), ("a NaN threshold", "NaN", 1, np.nan, 0, N, buf, N, 0),
               ("an unknown flag bit", "flags", 1, 0.0, 0, N, buf, N, 2), ("an unknown high flag bit", "flags", 1, 0.0, 0, N, buf, N, 1 << 31), ("first < 0", "first", 1, 0.0, -1, 4, buf, 4, 0),
               ("n_range < 0", "n_range", 1, 0.0, 0, -1, buf, 4, 0), ("first + n_range = N + 1", "n_range", 1, 0.0, 1, N, buf, N, 0), ("first = N + 1", "first", 1, 0.0, N + 1, 0, buf, N, 0),
               ("n_range = 2^62", "n_range", 1, 0.0, 5, 1 << 62, buf, N, 0), ("cap < 0", "cap", 1, 0.0, 0, N, buf, -1, 0), ("a null list with cap > 0", "null list", 1, 0.0, 0, N, None, 1, 0))
    for what, word, stat, t, first, n_range, L, cap, flags in selects:
        got = lib.fxb_meter_select(b._h, stat, C.c_double(t), first, n_range, ptr(L), cap, flags)
        assert got == FX_E_ARG and word in b.last_error(), (what, got, b.last_error())
        assert counters() == seen and (buf == M.MARK).all(), what
    out = [np.full((channels, 3), 0x55, dtype=rows[k].dtype) for k in M.FIELDS]
    held = [o.copy() for o in out]
    lists = (("an instance of N", "entry 1", np.array([0, N, 1], dtype=np.int64), 3, 0), ("an instance of -1", "entry 2", np.array([0, 1, -1], dtype=np.int64), 3, 0),
             ("count < 0", "count", np.array([0, 1, 2], dtype=np.int64), -1, 0), ("count = 2^31", "count", np.zeros(1, dtype=np.int64), 1 << 31, 0), ("a null list", "list", None, 3, 0))
    for what, word, L, count, reset in lists:
        for rc in (lib.fxb_meter_read_list(b._h, ptr(L), count, *[ptr(o) for o in out], reset), lib.fxb_meter_reset_list(b._h, ptr(L), count)):
            assert rc == FX_E_ARG and word in b.last_error(), (what, rc, b.last_error())
        assert counters() == seen and all(o.tobytes() == h.tobytes() for o, h in zip(out, held)), what
    twice = np.array([5, 9, 5], dtype=np.int64)
    assert lib.fxb_meter_read_list(b._h, ptr(twice), 3, *[ptr(o) for o in out], 1) == FX_E_ARG and "more than once" in b.last_error()
    assert counters() == seen and M.same_rows(b.meter_read(), rows)
    assert lib.fxb_meter_read_list(b._h, ptr(twice), 3, *[ptr(o) for o in out], 0) == 0, "repeats are a refusal of the reset only"
    for f, args in ((lib.fxb_meter_select, (1, C.c_double(0.0), 0, N, ptr(buf), N, 0)), (lib.fxb_meter_read_list, (ptr(twice), 3, None, None, None, None, 0)), (lib.fxb_meter_reset_list, (ptr(twice), 3))):
        assert f(None, *args) == FX_E_ARG
    # metering off: every call, also those with nothing to do
    off = A.Batch(N, channels, 0)
    assert off.load_text(STEREO)
    for rc in (lib.fxb_meter_select(off._h, 1, C.c_double(0.0), 0, N, ptr(buf), N, 0), lib.fxb_meter_select(off._h, 1, C.c_double(0.0), 0, 0, None, 0, 0),
               lib.fxb_meter_read_list(off._h, ptr(twice), 3, *[ptr(o) for o in out], 0), lib.fxb_meter_reset_list(off._h, ptr(twice), 3)):
        assert rc == FX_E_ARG and "metering is off" in off.last_error()
    assert (buf == M.MARK).all() and [off.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")] == [0, 0, 0]
    off.close()
    b.close()
    # an allocation that fails, at each allocation of the call (the device staging, the pinned staging): FX_E_MEMORY, nothing
    # changed, then the same call succeeds
    L = np.array([3, 0, N - 1], dtype=np.int64)
    calls = (("select", lambda h: lib.fxb_meter_select(h._h, 1, C.c_double(0.5), 0, N, ptr(buf), N, 0)), ("read_list", lambda h: lib.fxb_meter_read_list(h._h, ptr(L), 3, *[ptr(o) for o in out], 1)),
             ("reset_list", lambda h: lib.fxb_meter_reset_list(h._h, ptr(L), 3)))
    for name, call in calls:
        for nth in (0, 1):
            h = handle(A, N, channels)
            h.process_block(M.voices(N, channels, 16, seed=2))
            assert h.prepare(16, True) == 0   # (the builder thread is idle: no allocation of its own meets the injected failure)
            live = lib.fxstub_live_allocations()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = call(h)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and h.last_error(), (name, nth, rc)
            assert [h.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")] == [0, 0, 0] and lib.fxstub_live_allocations() <= live + 1
            assert M.same_rows(h.meter_read(), rows) and (buf == M.MARK).all(), (name, nth)
            rc = call(h)
            assert rc == (M.model(rows, 1, 0.5, False).size if name == "select" else 0) and h.sync() == 0, (name, nth, rc)
            assert M.same_rows(h.meter_read(), rows if name == "select" else M.zeroed(rows, L))
            buf[:] = M.MARK
            h.close()
    clean(lib)
    print("meter list refusals ok")


def child_shards():
    """three shards: ranges that cross both borders, caps that end inside the second shard, shards with no entry, lists on every
    shard and inside one, refusals in front of every shard, allocation failures on whichever shard"""
    A, lib = list_library()
    rng = np.random.default_rng(7)
    n, channels = 3 * 256 + 40, 2
    b, one = handle(A, n, channels, devices=[0, 1, 2]), handle(A, n, channels)
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    x = M.voices(n, channels, 33, seed=4)
    for h in (b, one):
        h.process_block(x[:16])
        h.process_block(x[16:])
    rows = one.meter_read()
    assert M.same_rows(b.meter_read(), rows)
    M.check_selects(lib, b, rows, n, "three shards")
    for first, n_range in ((300, 300), (319, 2), (319, 258), (320, 256), (0, n), (575, 2), (330, 100), (600, 50)):
        for stat, t, below in ((1, 0.5, False), (1, 0.5, True), (0, 0.0, False), (3, 1.0, False), (2, 1.0, False)):
            want = M.check_one(lib, b, rows, stat, t, below, first, n_range, n_range)
            in0, in1 = int((want < 320).sum()), int((want < 576).sum())
            for cap in {0, 1, in0, in0 + 1, (in0 + in1) // 2, max(in1 - 1, 0), in1, in1 + 1, max(want.size - 1, 0), want.size + 3}:
                M.check_one(lib, b, rows, stat, t, below, first, n_range, cap)
    for (first, n_range), launches in (((330, 100), 1), ((319, 2), 2), ((0, n), 3), ((600, 50), 1), ((100, 0), 0)):
        before = (b.info("meter_selects"), lib.fxstub_meter_selects())
        b.meter_select(1, 0.5, first=first, n_range=n_range)
        assert (b.info("meter_selects") - before[0], lib.fxstub_meter_selects() - before[1]) == (launches, launches), "a shard whose part is empty launches nothing"
    inside = rng.permutation(np.arange(330, 400)).astype(np.int64)
    everywhere = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:128]]).astype(np.int64)
    for L, launches in ((inside, 1), (everywhere, 3), (np.concatenate([everywhere[:40], inside[:10], everywhere[:40]]), 3), (np.array([319, 320, 575, 576, 319], dtype=np.int64), 3)):
        before = b.info("meter_list_reads")
        assert M.same_rows(b.meter_read_list(L), M.columns(rows, L)) and b.info("meter_list_reads") == before + launches
    for L, launches in ((inside, 1), (everywhere, 3)):
        before = b.info("meter_list_reads")
        assert M.same_rows(b.meter_read_list(L, reset=True), M.columns(rows, L)) and b.info("meter_list_reads") == before + launches
        rows = M.zeroed(rows, L)
        assert M.same_rows(b.meter_read(), rows)
    b.process_block(x)
    one.meter_read_list(np.unique(np.concatenate([inside, everywhere])), reset=True)
    one.process_block(x)
    rows = one.meter_read()
    assert M.same_rows(b.meter_read(), rows)
    for L, launches in ((np.array([700, 701, 700], dtype=np.int64), 1), (np.array([319, 320], dtype=np.int64), 2), (everywhere, 3)):
        before = b.info("meter_list_resets")
        assert b.meter_reset_list(L) == 0 and b.info("meter_list_resets") == before + launches, "a shard without an entry launches nothing"
        rows = M.zeroed(rows, L)
        assert M.same_rows(b.meter_read(), rows) and b.meter_samples() == 66
    # refused for the whole handle, in front of every shard
    seen = ([b.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")], lib.fxstub_meter_zeros(), lib.fxstub_meter_gathers())
    buf = np.full(n + 8, M.MARK, dtype=np.int64)
    assert lib.fxb_meter_reset_list(b._h, ptr(np.array([0, 700, n], dtype=np.int64)), 3) == FX_E_ARG and "entry 2" in b.last_error()
    assert lib.fxb_meter_read_list(b._h, ptr(np.array([0, n - 1, 0], dtype=np.int64)), 3, None, None, None, None, 1) == FX_E_ARG
    assert lib.fxb_meter_select(b._h, 1, C.c_double(0.0), 600, n - 599, ptr(buf), n, 0) == FX_E_ARG
    assert seen == ([b.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")], lib.fxstub_meter_zeros(), lib.fxstub_meter_gathers()) and M.same_rows(b.meter_read(), rows)
    for h in (b, one):
        h.close()
    # an allocation that fails on whichever shard - two per shard, each shard has entries: FX_E_MEMORY, and no shard has changed
    out = [np.zeros((channels, everywhere.size), dtype=d) for d in (np.float64, np.float32, np.uint32, np.uint32)]
    calls = (("select", lambda h: lib.fxb_meter_select(h._h, 1, C.c_double(0.5), 0, n, ptr(buf), n, 0)), ("read_list", lambda h: lib.fxb_meter_read_list(h._h, ptr(everywhere), everywhere.size, *[ptr(o) for o in out], 1)),
             ("reset_list", lambda h: lib.fxb_meter_reset_list(h._h, ptr(everywhere), everywhere.size)))
    for name, call in calls:
        for nth in range(6):
            c = handle(A, n, channels, devices=[0, 1, 2])
            c.process_block(x)
            rows = c.meter_read()
            assert c.prepare(33, True) == 0   # (the builder threads are idle: no allocation of their own meets the injected failure)
            lib.fxstub_fail_mallocs(nth, 1)
            rc = call(c)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and c.last_error(), (name, nth, rc)
            assert [c.info(k) for k in ("meter_selects", "meter_list_reads", "meter_list_resets")] == [0, 0, 0] and (buf == M.MARK).all()
            assert M.same_rows(c.meter_read(), rows), (name, nth, "no shard has changed")
            rc = call(c)
            assert rc == (M.model(rows, 1, 0.5, False).size if name == "select" else 0) and c.sync() == 0
            assert M.same_rows(c.meter_read(), rows if name == "select" else M.zeroed(rows, everywhere))
            buf[:] = M.MARK
            c.close()
    clean(lib)
    print("meter list shards ok")


if __name__ == "__main__":
    which = sys.argv[1]
    if which.startswith("select-"):
        child_select(int(which[7:]))
    else:
        {"read": child_read, "streams": child_streams, "refusals": child_refusals, "shards": child_shards}[which]()
