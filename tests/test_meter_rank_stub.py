"""Meter ranks without a GPU: fxb_meter_rank / fxb_meter_rank_match / fxb_meter_rank_level on the library's host sources linked
against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like
tests/test_meter_list_stub.py (this file is also that child).  The stand-in of the kernels (tests/hipstub/fx_meter_rank_stub.cpp)
works in stream order with a formulation of its own - one stable sort of the range, long double compares, no radix select.

The stand-in's emulation launch copies input to output, so the meters are a function of the input the test builds
(meter_list_model.voices, meter_rank_model.ladder_voices / target_for).  The model is numpy over the arrays the read calls return
(meter_rank_model.rank); the bar is equality everywhere, and the words of both buffers behind min(M, k) must still hold their
marks.  This checks the host layers: argument checks, staging, the one copy back, the sort into rank order, ranges by shard and
their merge, the counters.  The kernels themselves: tests/test_gpu_meter_rank.py.  The Python-driven cases do not run under a
sanitizer: that is tests/hipstub/meter_rank_checks.cpp, a program of its own (tests/test_meter_rank_checks.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_level_model as L  # noqa: E402
import meter_list_model as M  # noqa: E402
import meter_rank_model as R  # noqa: E402
import meter_target_model as T  # noqa: E402
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, PROGRAM, ROOT, STEREO  # noqa: E402
from test_meter_list_stub import QUAD  # noqa: E402
from test_meter_stub import meter_model  # noqa: E402

N = 200
TEXT = {1: PROGRAM, 2: STEREO, 4: QUAD}


def run_child(which, marker, devices=1):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("channels", (1, 2, 4))
def test_ranks_equal_the_numpy_model_on_the_hip_stand_in(channels):
    """N = 200; the three families, every stat, the four flag combinations; thresholds, k values and ranges of meter_rank_model"""
    run_child("ranks-%d" % channels, "meter rank ranks ok")


def test_the_directed_ladder_on_the_hip_stand_in():
    run_child("ladder", "meter rank ladder ok")


def test_meter_rank_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "meter rank refusals ok")


def test_meter_ranks_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "meter rank shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def rank_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_meter_ranks", "fxstub_meter_rank_pairs", "fxstub_live_allocations", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return A, lib


def handle(A, n, channels, x=None, devices=None, target=True, level=True, meters=True):
    """a handle with everything the three families need, and the blocks of 16 + 17 samples of x through it"""
    b = A.Batch(n, channels, 0) if devices is None else A.Batch(n, channels, devices=devices)
    assert b.load_text(TEXT[channels]), b.errors()
    if meters:
        assert b.meter_enable() == 0
    if target and x is not None:
        assert b.meter_set_target(R.target_for(x), group=1) == 0
    if level:
        assert b.meter_set_level(R.LEVEL_RELEASE, R.LEVEL_FLOOR) == 0
    if x is not None:
        b.process_block(x[:16])
        b.process_block(x[16:])
    return b


def rows_of(b):
    return {"meter": b.meter_read(), "match": b.meter_read_match(), "level": b.meter_read_level()}


def same_all(got, want):
    return M.same_rows(got["meter"], want["meter"]) and T.same_match(got["match"], want["match"]) and L.same_level(got["level"], want["level"])


def model_rows(x):
    return {"meter": meter_model(x), "match": T.match_model(x, R.target_for(x), 1, 0, False)[0], "level": L.level_model(x, R.LEVEL_RELEASE, R.LEVEL_FLOOR)}


def counters(b, lib):
    return [b.info(R.COUNTER[f]) for f in R.FAMILIES], lib.fxstub_meter_ranks(), lib.fxstub_meter_rank_pairs()


def clean(lib):
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0


def child_ranks(channels):
    A, lib = rank_library()
    x = M.voices(N, channels, 33, seed=channels)
    b = handle(A, N, channels, x)
    rows = rows_of(b)
    assert same_all(rows, model_rows(x)), "the stand-in's emulation launch copies its input"
    cross = R.value("match", rows["match"], T.CROSS)
    assert (cross < 0).any() and (cross > 0).any()
    for family in R.FAMILIES:
        before = (b.info(R.COUNTER[family]), lib.fxstub_meter_ranks())
        calls = R.check_ranks(lib, b, family, rows[family], "channels=%d" % channels)
        launched = b.info(R.COUNTER[family]) - before[0]
        assert launched == lib.fxstub_meter_ranks() - before[1] and 0 < launched < calls, "a call over an empty range launches nothing, every other one once"
        assert b.info(R.COUNTER[family]) == b._lib.fxb_info(b._h, R.INFO[family])
    assert R.check_digits(lib, b, "match", cross, T.CROSS) >= {0}, "a negative against a positive cross: the top digit"
    # the Python surface: (M, list, values), the defaults take the whole range
    m, lst, val = b.meter_rank_level(A.LEVEL_ENVELOPE, 5)
    want = R.rank(R.value("level", rows["level"], 0), 5)
    assert (m, lst.tolist()) == (want[0], want[1].tolist()) and np.array_equal(val.view(np.uint64), want[2].view(np.uint64)) and lst.dtype == np.int64 and val.dtype == np.float64
    m, lst, val = b.meter_rank(A.METER_PEAK, 7, threshold=0.5, below=True, largest=True, first=3, n_range=150)
    want = R.rank(R.value("meter", rows["meter"], 1), 7, 0.5, True, True, 3, 150)
    assert (m, lst.tolist(), val.tolist()) == (want[0], want[1].tolist(), want[2].tolist())
    m, lst, val = b.meter_rank_match(A.MATCH_ERROR, 0)
    assert m == N and lst.size == 0 and val.size == 0, "k == 0 is a count query"
    # a null value array; a count query with both null
    V = R.value("meter", rows["meter"], 0)
    lst, val, m = R.raw_rank(lib, b, "meter", 0, 9, -np.inf, 0, 0, N, null_value=True)
    assert m == N and np.array_equal(lst[:9], R.rank(V, 9)[1]) and (lst[9:] == R.MARK).all() and (val == R.VMARK).all()
    assert R.raw_rank(lib, b, "meter", 0, 0, 0.5, 0, 0, N, null_list=True, null_value=True)[2] == R.rank(V, 0, 0.5)[0]
    assert same_all(rows_of(b), rows) and b.meter_samples() == 33, "a rank changes nothing"
    b.close()
    clean(lib)
    print("meter rank ranks ok")


def child_ladder():
    """the directed scene of the model: every digit below the top one, ties at the k-th key across instance 63 | 64 and 255 | 256,
    M < k, M == k, M == 0, every V equal, LARGEST with ties"""
    A, lib = rank_library()
    x = R.ladder_voices()
    b = handle(A, R.LADDER_N, 1, x, target=False)
    rows = b.meter_read()
    assert M.same_rows(rows, meter_model(x))
    energy, peak, nonfinite = (R.value("meter", rows, s) for s in (0, 1, 3))
    assert R.check_digits(lib, b, "meter", energy, 0) >= set(range(1, R.PASSES))
    for k in (99, 100, 101, 269, 270, 271, 288 + 5, 288 + 6):
        for largest in (False, True):
            R.check_one(lib, b, "meter", energy, 0, k, largest=largest, what="ladder tie")
            R.check_one(lib, b, "meter", peak, 1, k, largest=largest, what="ladder peak tie")
    t = 1.0 + 2.0 ** -30
    for k in R.k_values(4):
        assert R.check_one(lib, b, "meter", energy, 0, k, t, what="inside the ladder") == 4
        assert R.check_one(lib, b, "meter", energy, 0, k, np.inf) == 0
        R.check_one(lib, b, "meter", nonfinite, 3, k, largest=bool(k & 1), what="every V equal")
    R.check_ranks(lib, b, "meter", rows, "ladder", starts=(0, 63, 255, 257))
    b.close()
    clean(lib)
    print("meter rank ladder ok")


def child_refusals():
    A, lib = rank_library()
    channels = 2
    x = M.voices(N, channels, 33, seed=2)
    b = handle(A, N, channels, x)
    rows = rows_of(b)
    seen = counters(b, lib)
    lst, val = np.full(N + 8, R.MARK, dtype=np.int64), np.full(N + 8, R.VMARK, dtype=np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data if a is not None else 0)  # noqa: E731

    def refused(h, family, stat, k, t, first, n_range, L_, flags, word, what):
        got = getattr(lib, R.CALL[family])(h._h, stat, k, C.c_double(t), first, n_range, ptr(L_), ptr(val), flags)
        assert got == FX_E_ARG and word in h.last_error(), (what, family, got, h.last_error())
        assert (lst == R.MARK).all() and (val == R.VMARK).all(), (what, family)

    for family in R.FAMILIES:
        top = R.STATS[family][-1]
        for what, word, stat, k, t, first, n_range, L_, flags in (
                ("stat above the family's", "stat", top + 1, 3, 0.0, 0, N, lst, 0), ("stat = -1", "stat", -1, 3, 0.0, 0, N, lst, 0), ("a NaN threshold", "NaN", 0, 3, np.nan, 0, N, lst, 0),
                ("an unknown flag bit", "flags", 0, 3, 0.0, 0, N, lst, 4), ("an unknown high flag bit", "flags", 0, 3, 0.0, 0, N, lst, 1 << 31), ("first < 0", "first", 0, 3, 0.0, -1, 4, lst, 0),
                ("n_range < 0", "n_range", 0, 3, 0.0, 0, -1, lst, 0), ("first + n_range = N + 1", "n_range", 0, 3, 0.0, 1, N, lst, 0), ("first = N + 1", "first", 0, 3, 0.0, N + 1, 0, lst, 0),
                ("n_range = 2^62", "n_range", 0, 3, 0.0, 5, 1 << 62, lst, 0), ("k < 0", "k < 0", 0, -1, 0.0, 0, N, lst, 0), ("a null list with k > 0", "null list", 0, 1, 0.0, 0, N, None, 0)):
            refused(b, family, stat, k, t, first, n_range, L_, flags, word, what)
            assert counters(b, lib) == seen, (what, family)
        assert getattr(lib, R.CALL[family])(None, 0, 3, C.c_double(0.0), 0, N, ptr(lst), ptr(val), 0) == FX_E_ARG
        assert getattr(lib, R.CALL[family])(b._h, 0, 3, C.c_double(0.0), 5, 0, ptr(lst), ptr(val), 3) == 0, "n_range == 0 returns 0 without a launch"
        assert counters(b, lib) == seen
    assert same_all(rows_of(b), rows)
    b.close()
    # the mode off: every call of the family, also those with nothing to do; the other families keep answering
    for family, kwargs, word in (("meter", dict(meters=False, target=False, level=False), "metering is off"), ("match", dict(target=False), "no target is set"), ("level", dict(level=False), "the mode is off")):
        off = handle(A, N, channels, x, **kwargs)
        for k, n_range in ((3, N), (0, N), (0, 0)):
            refused(off, family, 0, k, 0.0, 0, n_range, lst, 0, word, "the mode off")
        assert [off.info(R.COUNTER[f]) for f in R.FAMILIES] == [0, 0, 0]
        if family != "meter":
            assert R.check_one(lib, off, "meter", R.value("meter", rows["meter"], 1), 1, 5) == N
        off.close()
    # an allocation that fails, at each staging allocation of the call (the device block, the pinned block): FX_E_MEMORY, nothing
    # changed, then the same call succeeds
    V = R.value("level", rows["level"], 0)
    for family, stat in (("meter", 1), ("match", 0), ("level", 0)):
        for nth in (0, 1):
            h = handle(A, N, channels, x)
            assert h.prepare(16, True) == 0   # (the builder thread is idle: no allocation of its own meets the injected failure)
            live, ranks = lib.fxstub_live_allocations(), lib.fxstub_meter_ranks()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = getattr(lib, R.CALL[family])(h._h, stat, 9, C.c_double(-np.inf), 0, N, ptr(lst), ptr(val), 0)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and h.last_error(), (family, nth, rc)
            assert [h.info(R.COUNTER[f]) for f in R.FAMILIES] == [0, 0, 0] and lib.fxstub_meter_ranks() == ranks and lib.fxstub_live_allocations() <= live + 1
            assert same_all(rows_of(h), rows) and (lst == R.MARK).all() and (val == R.VMARK).all(), (family, nth)
            assert R.check_one(lib, h, family, R.value(family, rows[family], stat), stat, 9) == N and h.info(R.COUNTER[family]) == 1
            h.close()
    assert R.rank(V, 3)[0] == N
    clean(lib)
    print("meter rank refusals ok")


def child_shards():
    """three shards against the single handle: ranges that cross both borders, k inside and beyond every part, ties across the
    borders, shards with no part, refusals in front of every shard, allocation failures on whichever shard"""
    A, lib = rank_library()
    n, channels = 3 * 256 + 40, 2
    x = M.voices(n, channels, 33, seed=4)
    b, one = handle(A, n, channels, x, devices=[0, 1, 2]), handle(A, n, channels, x)
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    rows = rows_of(one)
    assert same_all(rows_of(b), rows)
    for family in R.FAMILIES:
        R.check_ranks(lib, b, family, rows[family], "three shards", ks=(0, 1, 64, 257, 321, n, n + 1), starts=(0, 319, 320, 575, 600))
        for stat in R.STATS[family]:
            V = R.value(family, rows[family], stat)
            for first, n_range in ((300, 300), (319, 2), (319, 258), (320, 256), (0, n), (575, 2), (330, 100), (600, 50)):
                for flags in range(4):
                    for k in (1, 5, n_range - 1, n_range, n_range + 3):
                        args = (stat, k, float(np.median(V)), flags, first, n_range)
                        got, want = R.raw_rank(lib, b, family, *args), R.raw_rank(lib, one, family, *args)
                        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the single handle's words"
                        R.check_one(lib, b, family, V, stat, k, args[2], bool(flags & 1), bool(flags & 2), first, n_range, "three shards")
    for (first, n_range), launches in (((330, 100), 1), ((319, 2), 2), ((0, n), 3), ((600, 50), 1), ((100, 0), 0)):
        before = (b.info("meter_level_ranks"), lib.fxstub_meter_ranks())
        b.meter_rank_level(0, 4, first=first, n_range=n_range)
        assert (b.info("meter_level_ranks") - before[0], lib.fxstub_meter_ranks() - before[1]) == (launches, launches), "a shard whose part is empty launches nothing"
    # refused for the whole handle, in front of every shard
    seen = counters(b, lib)
    lst, val = np.full(n + 8, R.MARK, dtype=np.int64), np.full(n + 8, R.VMARK, dtype=np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.fxb_meter_rank(b._h, 1, 3, C.c_double(0.0), 600, n - 599, ptr(lst), ptr(val), 0) == FX_E_ARG
    assert lib.fxb_meter_rank_level(b._h, 2, 3, C.c_double(0.0), 0, n, ptr(lst), ptr(val), 0) == FX_E_ARG
    assert counters(b, lib) == seen and (lst == R.MARK).all() and same_all(rows_of(b), rows)
    for h in (b, one):
        h.close()
    # an allocation that fails on whichever shard - two per shard: FX_E_MEMORY, nothing written, then the call succeeds
    for nth in range(6):
        c = handle(A, n, channels, x, devices=[0, 1, 2])
        assert c.prepare(33, True) == 0   # (the builder threads are idle: no allocation of their own meets the injected failure)
        lib.fxstub_fail_mallocs(nth, 1)
        rc = lib.fxb_meter_rank(c._h, 1, 400, C.c_double(-np.inf), 0, n, ptr(lst), ptr(val), 0)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.last_error(), (nth, rc)
        assert [c.info(R.COUNTER[f]) for f in R.FAMILIES] == [0, 0, 0] and (lst == R.MARK).all() and (val == R.VMARK).all()
        assert same_all(rows_of(c), rows), (nth, "no shard has changed")
        assert R.check_one(lib, c, "meter", R.value("meter", rows["meter"], 1), 1, 400) == n and c.info("meter_ranks") == 3
        c.close()
    clean(lib)
    print("meter rank shards ok")


if __name__ == "__main__":
    which = sys.argv[1]
    if which.startswith("ranks-"):
        child_ranks(int(which[6:]))
    else:
        {"ladder": child_ladder, "refusals": child_refusals, "shards": child_shards}[which]()
