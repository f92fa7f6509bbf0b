"""Level meters without a GPU: fxb_meter_set_level / _clear_level / _get_level / _read_level / _read_level_list / _select_level on
the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C
ABI in a child process like tests/test_meter_stub.py (this file is also that child).  The stand-in's emulation launch copies input
to output, so the figures are a function of the input the test builds; the stand-ins of the kernels
(tests/hipstub/fx_meter_level_stub.cpp) work in stream order with a formulation of their own - floats where the kernels compare
bit patterns.  The model is meter_level_model.level_model; the bar is equality of words, fp32 as uint32.

This checks the host layers: every route a block can take with the mode on, beside a twin without it whose four (with a target:
six) accumulators must be equal; 16 + 17 samples against 33, pieces, the segments of an armed control track, shards on unaligned
starts; a second set_level; every reset rule; the list reset behind a slow block; refusals and allocation failures; the counters.
The saturation of `quiet` at 0xFFFFFFFF is checked on the model alone (2^32 samples).  The kernels: tests/test_gpu_meter_level.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_level_model as L  # noqa: E402
import meter_target_model as T  # noqa: E402
from test_meter_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MORE, PROGRAM, ROOT, STEREO, Pinned, expand, same_meters  # noqa: E402

COUNTERS = ("meter_level_launches", "meter_level_selects", "meter_level_list_reads")
PARAMS = ((0.5, 0.25), (1.0, 0.0), (0.0, 1.0), (0.999, 1e-4))


def run_child(which, marker, devices=1):
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_level_model_splits_denormals_saturation_and_the_written_out_loop():
    """the restatement itself: 16 + 17 samples give the words of 33; one column written out sample by sample; the fall through the
    denormals; a denormal at rest; release = 1 is the peak, release = 0 the last magnitude, floor = 0 no count; the saturation of
    `quiet`, which no device test can reach"""
    rng = np.random.default_rng(3)
    y = L.words(rng, (33, 2, 70))
    for release, floor in PARAMS:
        whole = L.level_model(y, release, floor)
        part = L.level_model(y[16:], release, floor, L.level_model(y[:16], release, floor))
        assert L.same_level(part, whole), (release, floor)
        for c, n in ((0, 0), (1, 5), (0, 69)):
            lv, q = np.float32(0.0), 0
            for s in range(33):
                a = y[s, c, n]
                fin = bool(np.isfinite(a))
                w = np.float32(abs(a)) if fin else np.float32(0.0)
                d = np.float32(lv * np.float32(release))
                lv = w if w > d else d
                q = 0 if (not fin or w >= np.float32(floor)) else min(q + 1, 0xFFFFFFFF)
            assert (lv.view(np.uint32), q) == (whole["level"][c, n].view(np.uint32), whole["quiet"][c, n]), (release, floor, c, n)
        assert np.isfinite(whole["level"]).all() and not np.signbit(whole["level"]).any()
    peak = np.where(np.isfinite(y), np.abs(y), np.float32(0)).max(axis=0)
    assert np.array_equal(L.level_model(y, 1.0, 0.0)["level"].view(np.uint32), peak.view(np.uint32)) and not L.level_model(y, 1.0, 0.0)["quiet"].any()
    last = np.where(np.isfinite(y[-1]), np.abs(y[-1]), np.float32(0))
    assert np.array_equal(L.level_model(y, 0.0, 1.0)["level"].view(np.uint32), last.view(np.uint32))
    # an impulse of 1.0 and zeros, release 0.5: the pattern 1 after 150 samples, 0 after 151
    imp = np.zeros((151, 1, 1), dtype=np.float32)
    imp[0] = 1.0
    a = L.level_model(imp[:150], 0.5, 0.25)
    assert a["level"].view(np.uint32).tolist() == [[1]] and a["quiet"].tolist() == [[149]]
    a = L.level_model(imp[150:], 0.5, 0.25, a)
    assert a["level"].view(np.uint32).tolist() == [[0]] and a["quiet"].tolist() == [[150]]
    # a denormal comes to rest: k units times the release rounds back to k once k * (1 - release) is at most half a unit (a tie
    # goes to the even k) - at the pattern 500 for release 0.999, at 7 for 0.93 (7 * 0.07 = 0.49, 8 * 0.07 = 0.56)
    for release, pattern in ((0.999, 500), (0.93, 7)):
        rest = L.level_model(np.zeros((100000, 1, 1), dtype=np.float32), release, 0.0, {"level": np.array([[1e-30]], dtype=np.float32), "quiet": np.zeros((1, 1), dtype=np.uint32)})
        assert rest["level"].view(np.uint32).tolist() == [[pattern]], (release, rest["level"].view(np.uint32))
    # the counter saturates
    acc = {"level": np.zeros((1, 3), dtype=np.float32), "quiet": np.array([[0xFFFFFFFD, 0xFFFFFFFF, 5]], dtype=np.uint32)}
    acc = L.level_model(np.array([[[0.0, 0.0, 0.0]]] * 4, dtype=np.float32), 0.5, 0.25, acc)
    assert acc["quiet"].tolist() == [[0xFFFFFFFF, 0xFFFFFFFF, 9]]
    assert L.level_model(np.array([[[0.0, 0.5, np.nan]]], dtype=np.float32), 0.5, 0.25, acc)["quiet"].tolist() == [[0xFFFFFFFF, 0, 0]]
    rows = {"level": np.array([[0.5, 0.0, 1.0], [0.25, 2.0, 0.0]], dtype=np.float32), "quiet": np.array([[3, 9, 0], [7, 2, 5]], dtype=np.uint32)}
    assert L.V(rows, 0).tolist() == [0.5, 2.0, 1.0] and L.V(rows, 1).tolist() == [3.0, 2.0, 0.0]
    assert L.select(rows, 1, 2.0, False).tolist() == [0, 1] and L.select(rows, 0, 1.0, True).tolist() == [0]


def test_level_meters_on_every_route_on_the_hip_stand_in():
    run_child("routes", "level routes ok")


def test_level_meters_through_pieces_and_track_segments_on_the_hip_stand_in():
    run_child("pieces", "level pieces ok")


def test_level_refusals_resets_and_allocation_failures_on_the_hip_stand_in():
    run_child("refusals", "level refusals ok")


def test_level_reset_list_behind_a_slow_block_on_the_hip_stand_in():
    run_child("streams", "level streams ok")


def test_level_queries_on_the_hip_stand_in():
    run_child("queries", "level queries ok")


def test_level_meters_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "level shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_live_allocations", "fxstub_meter_level_launches", "fxstub_meter_target_level_launches",
              "fxstub_level_selects", "fxstub_level_gathers", "fxstub_level_zeros", "fxstub_level_strays", "fxstub_meter_zeros", "fxstub_match_zeros"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def clean(lib):
    assert lib.fxstub_level_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0


class Pair:
    """a handle with level meters on, its twin with meters on and the mode off, and the model of the two rows"""

    def __init__(self, A, lib, N, ch, release, floor, devices=None, target=None):
        text = {1: PROGRAM, 2: STEREO}[ch]
        self.lib, self.N, self.ch = lib, N, ch
        self.b = A.Batch(N, ch, 0) if devices is None else A.Batch(N, ch, devices=devices)
        self.twin = A.Batch(N, ch, 0)
        for h in (self.b, self.twin):
            assert h.load_text(text), h.errors()
            assert h.meter_enable() == 0
            if target is not None:
                assert h.meter_set_target(*target) == 0
        self.targeted = target is not None
        self.shards = 1 if devices is None else len(devices)
        self.launches = 0
        self.set(release, floor)
        self.acc = L.level_zero(ch, N)

    def set(self, release, floor):
        assert self.b.meter_set_level(release, floor) == 0
        self.release, self.floor = np.float32(release), np.float32(floor)
        got = self.b.meter_get_level()
        assert (np.float32(got[0]), np.float32(got[1])) == (self.release, self.floor), got

    def both(self, call):
        for h in (self.b, self.twin):
            call(h)

    def took(self, what, y, launches=1):
        """both handles were given the same call, which returned the per-instance block y in `launches` launches per shard"""
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, self.ch, self.N)
        self.acc = L.level_model(y, self.release, self.floor, self.acc)
        self.launches += launches * self.shards
        got = self.b.meter_read_level()
        assert L.same_level(got, self.acc), (what, np.argwhere(got["level"].view(np.uint32) != self.acc["level"].view(np.uint32))[:4].tolist(), np.argwhere(got["quiet"] != self.acc["quiet"])[:4].tolist())
        assert same_meters(self.b.meter_read(), self.twin.meter_read()), (what, "the four with the mode on are those of a twin without it")
        if self.targeted:
            assert T.same_match(self.b.meter_read_match(), self.twin.meter_read_match()) and self.b.meter_target_pos() == self.twin.meter_target_pos(), (what, "the six")
        assert self.b.meter_samples() == self.twin.meter_samples(), what
        assert self.b.info("meter_level_launches") == self.launches, (what, self.b.info("meter_level_launches"), self.launches)
        counted = "meter_target_launches" if self.targeted else "meter_launches"
        other = "meter_launches" if self.targeted else "meter_target_launches"
        assert self.b.info(counted) == self.twin.info(counted) * self.shards == self.launches and self.b.info(other) == 0, (what, "the same blocks are counted")

    def close(self):
        self.b.close()
        self.twin.close()


def child_routes():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(161)
    S = 33
    cases = ((5, 1, PARAMS[0], False), (197, 1, PARAMS[3], False), (256, 2, PARAMS[1], False), (257, 2, PARAMS[2], False), (130, 2, PARAMS[0], True), (197, 1, PARAMS[3], True))
    for N, ch, (release, floor), targeted in cases:
        target = (T.words(rng, (40, ch, -(-N // 3))), 3, True) if targeted else None
        p = Pair(A, lib, N, ch, release, floor, target=target)
        seen = (lib.fxstub_meter_level_launches(), lib.fxstub_meter_target_level_launches())
        # 16 + 17 samples; then 33 at once
        x = L.words(rng, (S, ch, N))
        p.both(lambda h: h.process_block(x[:16]))
        p.took("pageable, 16 samples", x[:16])
        p.both(lambda h: h.process_block(x[16:]))
        p.took("pageable, 17 more", x[16:])
        assert L.same_level(p.acc, L.level_model(x, release, floor)), "16 + 17 against 33"
        x = L.words(rng, (S, ch, N))
        p.both(lambda h: h.process_block(x))
        p.took("pageable, 33 at once", x)
        # pinned in place; the device entry; a pitch
        pin, pout = pinned((S, ch, N)), pinned((S, ch, N))
        pin[...] = L.words(rng, (S, ch, N))
        for h in (p.b, p.twin):
            assert h.process_block(pin, out=pout) is pout
        p.took("pinned in place", pout)
        for h in (p.b, p.twin):
            assert h.process_block_dev(int(pin.ctypes.data), int(pout.ctypes.data), S) == 0
        p.took("device entry", pout)
        P = N + 59
        win = pinned((S, ch, P))
        win[...] = L.words(rng, (S, ch, P))
        for h in (p.b, p.twin):
            assert h.process_block_dev_pitched(int(win.ctypes.data), int(win.ctypes.data), S, P) == 0
        p.took("device entry, pitch N + 59", win[:, :, :N])
        # bus blocks: the scratch block between the emulation and the mix
        for K in (3, 64):
            g = p.b.bus_groups(K)
            xg, xn = L.words(rng, (S, ch, g)), L.words(rng, (S, ch, N))
            p.both(lambda h: h.process_block_bus(xg, K, True, False))
            p.took("bus %d shared in" % K, expand(xg, K, N))
            p.both(lambda h: h.process_block_bus(xn, K, False, True))
            p.took("bus %d mix out" % K, xn)
            p.both(lambda h: h.process_block_bus(xg, K, True, True))
            p.took("bus %d both" % K, expand(xg, K, N))
            pg, po = pinned((S, ch, g)), pinned((S, ch, g))
            pg[...] = xg
            for h in (p.b, p.twin):
                assert h.process_block_bus_dev(int(pg.ctypes.data), int(po.ctypes.data), S, K) == 0
            p.took("bus %d device entry" % K, expand(xg, K, N))
        # instance-major
        xi = np.ascontiguousarray(L.words(rng, (N, S, ch)))
        p.both(lambda h: h.process_block_imajor(xi))
        p.took("instance-major", np.ascontiguousarray(xi.transpose(1, 2, 0)))
        ran = (lib.fxstub_meter_level_launches() - seen[0], lib.fxstub_meter_target_level_launches() - seen[1])
        assert ran == ((0, p.launches) if targeted else (p.launches, 0)), (ran, p.launches)
        # a second set_level keeps the accumulators and changes later blocks only
        p.set(0.25, 0.5)
        assert L.same_level(p.b.meter_read_level(), p.acc), "a second set keeps the accumulators"
        x = L.words(rng, (S, ch, N))
        p.both(lambda h: h.process_block(x))
        p.took("after a second set", x)
        # the mode cleared: the plain kernels again, the others go on
        assert p.b.meter_clear_level() == 0 and lib.fxb_meter_get_level(p.b._h, None, None) == FX_E_ARG
        p.both(lambda h: h.process_block(x))
        assert p.b.info("meter_level_launches") == p.launches and same_meters(p.b.meter_read(), p.twin.meter_read())
        pinned.free()
        p.close()
    clean(lib)
    print("level routes ok")


def child_pieces():
    A, lib = stub_library()
    rng = np.random.default_rng(167)
    # 96 samples of 262 144 instances on a bus: two pieces of 48 samples; a pageable block of 32 MiB: eight pieces
    N, S, K = 262144, 96, 64
    p = Pair(A, lib, N, 1, 0.999, 1e-4)
    xg = L.words(rng, (S, 1, p.b.bus_groups(K)))
    p.both(lambda h: h.process_block_bus(xg, K))
    p.took("bus, two pieces", expand(xg, K, N), launches=2)
    x = L.words(rng, (32, 1, N))
    p.both(lambda h: h.process_block(x))
    p.took("pipelined host block", x, launches=8)
    p.close()
    # an armed control track: the interpreter tier cuts the block at the change points - five segments, five level launches; the
    # translated tier reads the schedule by itself - one
    for tier, segments in (("asm", 5), (None, 1)):
        if tier:
            os.environ["FX_KERNEL"] = tier
        p = Pair(A, lib, 197, 1, 0.5, 0.25)
        os.environ.pop("FX_KERNEL", None)
        assert (p.b.info("kernel") >= 9) == (tier is None), p.b.info("kernel")
        for route in ("pageable", "bus"):
            for h in (p.b, p.twin):
                assert h.set_register_track("vol", [0.1, 0.2, 0.3, 0.4, 0.5], 8) == 0
            if route == "pageable":
                x = L.words(rng, (33, 1, 197))
                p.both(lambda h: h.process_block(x))
                p.took("armed, " + route, x, launches=segments)
            else:
                xg = L.words(rng, (33, 1, p.b.bus_groups(64)))
                p.both(lambda h: h.process_block_bus(xg, 64))
                p.took("armed, " + route, expand(xg, 64, 197), launches=segments)
        p.close()
    clean(lib)
    print("level pieces ok")


def child_refusals():
    os.environ["FX_BUILDER"] = "0"   # (allocations are counted below: none may come from the handle's builder thread meanwhile)
    A, lib = stub_library()
    rng = np.random.default_rng(171)
    N, S, ch = 197, 33, 2
    b = A.Batch(N, ch, 0)
    assert b.load_text(STEREO), b.errors()
    x = L.words(rng, (S, ch, N))
    level, quiet = np.full((ch, N), 9.0, dtype=np.float32), np.full((ch, N), 9, dtype=np.uint32)
    buf = np.full(N + 8, L.MARK, dtype=np.int64)
    two = np.array([3, 5], dtype=np.int64)
    rel, flo = C.c_float(9.0), C.c_float(9.0)

    def queries(h):
        return (lib.fxb_meter_read_level(h, ptr(level), ptr(quiet), 0), lib.fxb_meter_read_level_list(h, ptr(two), 2, ptr(level), ptr(quiet), 0),
                lib.fxb_meter_select_level(h, 0, C.c_double(0.0), 0, N, ptr(buf), N, 0), lib.fxb_meter_select_level(h, 1, C.c_double(0.0), 0, 0, None, 0, 0),
                lib.fxb_meter_get_level(h, C.byref(rel), C.byref(flo)))

    def untouched():
        return (level == 9.0).all() and (quiet == 9).all() and (buf == L.MARK).all() and rel.value == 9.0 and flo.value == 9.0

    # metering off: the set is refused; so is every query; clear has nothing to drop
    live = lib.fxstub_live_allocations()
    assert lib.fxb_meter_set_level(b._h, 0.5, 0.25, 0) == FX_E_ARG and "metering is off" in b.last_error()
    assert set(queries(b._h)) == {FX_E_ARG} and untouched() and lib.fxb_meter_clear_level(b._h) == 0 and lib.fxstub_live_allocations() == live
    assert b.meter_enable() == 0
    # metering on, the mode off: every query is refused, nothing launched, nothing written
    assert set(queries(b._h)) == {FX_E_ARG} and "mode is off" in b.last_error() and untouched()
    live = lib.fxstub_live_allocations()
    # the refusals of the set: nothing changes
    for what, word, release, floor, flags in (("a NaN release", "release", np.nan, 0.25, 0), ("an infinite release", "release", np.inf, 0.25, 0), ("release > 1", "release", np.nextafter(np.float32(1), np.float32(2)), 0.25, 0),
                                              ("release < 0", "release", -1e-45, 0.25, 0), ("a NaN floor", "floor", 0.5, np.nan, 0), ("an infinite floor", "floor", 0.5, np.inf, 0),
                                              ("floor < 0", "floor", 0.5, -1e-45, 0), ("a flag", "flags", 0.5, 0.25, 1), ("a high flag", "flags", 0.5, 0.25, 1 << 31)):
        assert lib.fxb_meter_set_level(b._h, float(release), float(floor), flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
        assert lib.fxstub_live_allocations() == live and set(queries(b._h)) == {FX_E_ARG} and untouched(), what
    assert all(f(None, *a) == FX_E_ARG for f, a in ((lib.fxb_meter_set_level, (0.5, 0.25, 0)), (lib.fxb_meter_clear_level, ()), (lib.fxb_meter_get_level, (None, None)), (lib.fxb_meter_read_level, (None, None, 0)),
                                                    (lib.fxb_meter_read_level_list, (None, 0, None, None, 0)), (lib.fxb_meter_select_level, (0, C.c_double(0.0), 0, 0, None, 0, 0))))
    b.process_block(x)
    assert b.info("meter_launches") == 1 and [b.info(k) for k in COUNTERS] == [0, 0, 0]
    live = lib.fxstub_live_allocations()   # (the block's own buffers exist now)
    # an allocation that fails at the one allocation of the set: FX_E_MEMORY, the mode off, the handle usable
    lib.fxstub_fail_mallocs(0, 1)
    assert lib.fxb_meter_set_level(b._h, 0.5, 0.25, 0) == FX_E_MEMORY and b.last_error()
    lib.fxstub_fail_mallocs(-1, 0)
    assert lib.fxstub_live_allocations() == live and set(queries(b._h)) == {FX_E_ARG} and untouched()
    b.process_block(x)
    assert b.info("meter_level_launches") == 0 and b.info("meter_launches") == 2
    # set: all device allocation of the feature happens here - none inside a block; -0.0 is taken as 0
    assert b.meter_set_level(-0.0, -0.0) == 0 and lib.fxstub_live_allocations() == live + 1
    got = b.meter_get_level()
    assert not np.signbit(np.float32(got[0])) and not np.signbit(np.float32(got[1])) and got == (0.0, 0.0)
    b.process_block(x)
    assert L.same_level(b.meter_read_level(), L.level_model(x, 0.0, 0.0)) and lib.fxstub_live_allocations() == live + 1
    assert b.meter_set_level(0.5, 0.25) == 0 and lib.fxstub_live_allocations() == live + 1, "a second set allocates nothing"
    b.meter_read_level(reset=True)
    b.process_block(x)
    want = L.level_model(x, 0.5, 0.25)
    assert L.same_level(b.meter_read_level(), want) and lib.fxstub_live_allocations() == live + 1 and b.info("meter_level_launches") == 2 and b.info("meter_launches") == 4
    # a refused set with the mode on changes neither parameter nor a word
    assert lib.fxb_meter_set_level(b._h, 2.0, 0.25, 0) == FX_E_ARG and b.meter_get_level() == (0.5, 0.25) and L.same_level(b.meter_read_level(), want)
    # the refusals of the queries with the mode on: nothing launched, nothing written
    assert b.meter_select_level(0, 0.0)[1] == N and b.meter_read_level_list([1])["level"].shape == (ch, 1)   # (their staging exists from here)
    seen = ([b.info(k) for k in COUNTERS], lib.fxstub_level_selects(), lib.fxstub_level_gathers())
    for what, word, stat, thr, first, n_range, lst, cap, flags in (("stat = 2", "stat", 2, 0.0, 0, N, buf, N, 0), ("stat = -1", "stat", -1, 0.0, 0, N, buf, N, 0), ("a NaN threshold", "NaN", 0, np.nan, 0, N, buf, N, 0),
                                                                   ("an unknown flag", "flags", 0, 0.0, 0, N, buf, N, 2), ("first < 0", "first", 0, 0.0, -1, 4, buf, 4, 0), ("first + n_range = N + 1", "n_range", 0, 0.0, 1, N, buf, N, 0),
                                                                   ("cap < 0", "cap", 0, 0.0, 0, N, buf, -1, 0), ("a null list with cap > 0", "null list", 0, 0.0, 0, N, None, 1, 0)):
        assert lib.fxb_meter_select_level(b._h, stat, C.c_double(thr), first, n_range, ptr(lst), cap, flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
    for what, lst, count, reset in (("count < 0", two, -1, 0), ("a null list", None, 2, 0), ("an entry = N", np.array([3, N], dtype=np.int64), 2, 0), ("an entry < 0", np.array([-1, 3], dtype=np.int64), 2, 0),
                                    ("a repeat under reset", np.array([3, 5, 3], dtype=np.int64), 3, 1)):
        assert lib.fxb_meter_read_level_list(b._h, ptr(lst), count, ptr(level), ptr(quiet), reset) == FX_E_ARG and b.last_error(), what
    assert lib.fxb_meter_select(b._h, 4, C.c_double(0.0), 0, N, ptr(buf), N, 0) == FX_E_ARG, "fxb_meter_select keeps refusing stat = 4"
    assert seen == ([b.info(k) for k in COUNTERS], lib.fxstub_level_selects(), lib.fxstub_level_gathers()) and (buf == L.MARK).all() and (level == 9.0).all() and (quiet == 9).all()
    assert L.same_level(b.meter_read_level(), want)
    # either pointer may be NULL; a repeat without reset is fine
    assert lib.fxb_meter_read_level(b._h, ptr(level), None, 0) == 0 and (quiet == 9).all() and np.array_equal(level.view(np.uint32), want["level"].view(np.uint32))
    assert lib.fxb_meter_read_level(b._h, None, ptr(quiet), 0) == 0 and np.array_equal(quiet, want["quiet"])
    got = b.meter_read_level_list([5, 3, 5, N - 1])
    assert L.same_level(got, {k: v[:, [5, 3, 5, N - 1]] for k, v in want.items()}) and b.info("meter_level_list_reads") == 2
    # read_level with reset zeroes only the two new rows; fxb_meter_read(reset) zeroes them as well
    four = b.meter_read()
    assert L.same_level(b.meter_read_level(reset=True), want) and L.same_level(b.meter_read_level(), L.level_zero(ch, N))
    assert same_meters(b.meter_read(), four) and b.meter_samples() == 4 * S
    b.process_block(x)
    assert L.same_level(b.meter_read_level(), want)
    b.meter_read(reset=True)
    assert L.same_level(b.meter_read_level(), L.level_zero(ch, N)) and b.meter_samples() == 0 and not b.meter_read()["energy"].any() and b.meter_get_level() == (0.5, 0.25)
    # read_level_list with reset zeroes the listed columns of the two rows alone; reset_list those of every row
    b.process_block(x)
    four = b.meter_read()
    got = b.meter_read_level_list([7, 0], reset=True)
    assert L.same_level(got, {k: v[:, [7, 0]] for k, v in want.items()})
    want = L.zeroed(want, [7, 0])
    assert L.same_level(b.meter_read_level(), want) and same_meters(b.meter_read(), four)
    zeros = (lib.fxstub_meter_zeros(), lib.fxstub_level_zeros())
    assert b.meter_reset_list([9, 196]) == 0
    want = L.zeroed(want, [9, 196])
    for k in four:
        four[k][:, [9, 196]] = 0
    assert L.same_level(b.meter_read_level(), want) and same_meters(b.meter_read(), four) and (lib.fxstub_meter_zeros(), lib.fxstub_level_zeros()) == (zeros[0] + 1, zeros[1] + 1)
    # instance copy and reset leave the level rows alone, as they leave every meter alone
    assert b.copy_instances([1], [2]) == 0 and b.reset_instances([2, 3]) == 0 and b.sync() == 0
    assert L.same_level(b.meter_read_level(), want) and same_meters(b.meter_read(), four)
    # a program load zeroes the rows and keeps the mode and its parameters
    live = lib.fxstub_live_allocations()
    assert b.load_text(MORE), b.errors()
    assert b.meter_get_level() == (0.5, 0.25) and L.same_level(b.meter_read_level(), L.level_zero(ch, N)) and b.meter_samples() == 0
    launches = b.info("meter_level_launches")
    b.process_block(x)
    assert b.info("meter_level_launches") == launches + 1 and L.same_level(b.meter_read_level(), L.level_model(x, 0.5, 0.25))
    # clear_level and meter_enable(0) free the rows
    live = lib.fxstub_live_allocations()
    assert b.meter_clear_level() == 0 and lib.fxstub_live_allocations() == live - 1 and set(queries(b._h)) == {FX_E_ARG}
    assert b.meter_set_level(1.0) == 0 and lib.fxstub_live_allocations() == live
    assert b.meter_enable(False) == 0 and lib.fxstub_live_allocations() == live - 2
    assert b.meter_enable() == 0 and set(queries(b._h)) == {FX_E_ARG}
    b.close()
    clean(lib)
    print("level refusals ok")


def child_streams():
    """a list reset behind a slow block returns while that block is still running; when everything has run, the level columns of
    the listed voices - and only those - are zero behind block 1, and block 2 has been taken by all"""
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(173)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    n, S = 1000, 8
    b = A.Batch(n, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    assert b.meter_enable() == 0 and b.meter_set_level(0.999, 1e-4) == 0
    b.process_block(L.words(rng, (S, 1, n)))
    b.meter_reset_list([1, 2])   # (the staging exists before anything is timed)
    b.meter_read(reset=True)

    def fresh():
        p, o = pinned((S, 1, n)), pinned((S, 1, n))
        p[...] = L.words(rng, (S, 1, n))
        o[...] = -7.0
        return p, o

    first, second = fresh(), fresh()
    lst = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:63]]).astype(np.int64)
    zeros = (lib.fxstub_meter_zeros(), lib.fxstub_level_zeros())
    lib.fxstub_set_kernel_micros(150000)
    assert lib.fxb_process_block_dev(b._h, ptr(first[0]), ptr(first[1]), S, streams[0]) == 0
    assert b.meter_reset_list(lst) == 0
    given = lst.copy()
    lst[:] = 7
    assert (first[1][S - 1] == -7.0).all(), "the list reset returned while the block in front of it was still running"
    assert (lib.fxstub_meter_zeros(), lib.fxstub_level_zeros()) == zeros, "... and both zeroing launches are queued behind that block"
    lib.fxstub_set_kernel_micros(150)
    # (a second set while blocks are queued: for the blocks queued after it only)
    assert b.meter_set_level(0.5, 0.25) == 0
    assert lib.fxb_process_block_dev(b._h, ptr(second[0]), ptr(second[1]), S, streams[1]) == 0
    got = b.meter_read_level()
    assert (lib.fxstub_meter_zeros(), lib.fxstub_level_zeros()) == (zeros[0] + 1, zeros[1] + 1)
    one = L.level_model(first[0], 0.999, 1e-4)
    want = L.level_model(second[0], 0.5, 0.25, L.zeroed(one, given))
    assert L.same_level(got, want) and not L.same_level(got, L.level_model(second[0], 0.5, 0.25, one))
    # with the mode off the list reset launches fx_meter_zero alone
    assert b.meter_clear_level() == 0 and b.meter_reset_list(given) == 0 and b.sync() == 0
    assert (lib.fxstub_meter_zeros(), lib.fxstub_level_zeros()) == (zeros[0] + 2, zeros[1] + 1)
    pinned.free()
    b.close()
    clean(lib)
    print("level streams ok")


def quiet_voices(rng, S, ch, N):
    """voices that fall silent at many different samples, so that V has many distinct values for both stats"""
    x = L.words(rng, (S, ch, N))
    x[x == 0] = 0.5
    for n in range(N):
        x[S - (n * 5) % (S + 1):, :, n] = 0.0
    x[:, 0, 7] = 0.5   # one channel goes on sounding: the voice is not quiet
    return x


def child_queries():
    A, lib = stub_library()
    rng = np.random.default_rng(179)
    for ch, N in ((1, 200), (2, 257)):
        p = Pair(A, lib, N, ch, 0.5, 0.25)
        x = quiet_voices(rng, 33, ch, N)
        p.both(lambda h: h.process_block(x))
        p.took("one block", x)
        rows = p.b.meter_read_level()
        if ch == 2:
            assert rows["quiet"][0, 7] == 0 and rows["quiet"][1, 7] > 0 and L.V(rows, 1)[7] == 0, "the minimum over the channels"
        before = (p.b.info("meter_level_selects"), lib.fxstub_level_selects())
        assert L.check_selects(lib, p.b, rows, N) >= 6
        assert p.b.info("meter_level_selects") - before[0] == lib.fxstub_level_selects() - before[1] > 50 and p.b.info("meter_selects") == 0
        got, m = p.b.meter_select_level(A.LEVEL_ENVELOPE, np.inf, below=True)
        assert m == N and np.array_equal(got, np.arange(N))
        assert lib.fxb_meter_select_level(p.b._h, 1, C.c_double(8.0), 0, N, None, 0, 0) == L.select(rows, 1, 8.0, False).size > 0, "a count query"
        assert L.same_level(p.b.meter_read_level(), rows), "the queries change nothing"
        p.close()
    clean(lib)
    print("level queries ok")


def child_shards():
    """three shards starting at 320 and 576"""
    os.environ["FX_BUILDER"] = "0"
    A, lib = stub_library()
    rng = np.random.default_rng(183)
    N, S, ch = 3 * 256 + 40, 33, 2
    for targeted in (False, True):
        target = (T.words(rng, (40, ch, -(-N // 3))), 3, True) if targeted else None
        p = Pair(A, lib, N, ch, 0.5, 0.25, devices=[0, 1, 2], target=target)
        assert [(d, f) for d, f, _ in p.b.shards()] == [(0, 0), (1, 320), (2, 576)], p.b.shards()
        x = quiet_voices(rng, S, ch, N)
        p.both(lambda h: h.process_block(x[:16]))
        p.took("pageable, 16 samples", x[:16])
        p.both(lambda h: h.process_block(x[16:]))
        p.took("pageable, 17 more", x[16:])
        xg = L.words(rng, (S, ch, p.b.bus_groups(64)))
        p.both(lambda h: h.process_block_bus(xg, 64))
        p.took("bus 64", expand(xg, 64, N))
        p.both(lambda h: h.process_block(x))
        p.took("the voices fall silent again", x)
        rows = p.b.meter_read_level()
        L.check_selects(lib, p.b, rows, N, "three shards", starts=(0, 65, 319, 575))
        for first, n_range in ((300, 300), (319, 2), (319, 258), (575, 2), (600, 50)):
            for stat, t in ((0, float(np.median(L.V(rows, 0)))), (1, 8.0)):
                want = L.check_one(lib, p.b, rows, stat, t, False, first, n_range, n_range)
                for cap in {0, 1, want.size // 2, max(want.size - 1, 0), want.size + 3}:
                    L.check_one(lib, p.b, rows, stat, t, True, first, n_range, cap)
        # list read, list reset and read with reset on every shard
        lst = np.array([N - 1, 0, 319, 320, 575, 576, 320], dtype=np.int64)
        assert L.same_level(p.b.meter_read_level_list(lst), {k: v[:, lst] for k, v in rows.items()})
        lst = lst[:6]
        p.both(lambda h: h.meter_reset_list(lst))
        p.acc = L.zeroed(p.acc, lst)
        p.took("a list reset", np.zeros((0, ch, N), dtype=np.float32), launches=0)
        got = p.b.meter_read_level_list([1, 321, 577], reset=True)
        assert L.same_level(got, {k: v[:, [1, 321, 577]] for k, v in p.acc.items()})
        p.acc = L.zeroed(p.acc, [1, 321, 577])
        p.set(0.999, 1e-4)
        p.both(lambda h: h.process_block(x))
        p.took("after a second set", x)
        p.close()
    # an allocation that fails on whichever shard (one per shard): FX_E_MEMORY, the mode off on every shard, then the same call works
    x = L.words(rng, (S, ch, N))
    for nth in range(3):
        c = A.Batch(N, ch, devices=[0, 1, 2])
        assert c.load_text(STEREO) and c.meter_enable() == 0
        c.process_block(x)   # (the block's own buffers exist before allocations are counted)
        live = lib.fxstub_live_allocations()
        lib.fxstub_fail_mallocs(nth, 1)
        rc = lib.fxb_meter_set_level(c._h, 0.5, 0.25, 0)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.last_error() and lib.fxstub_live_allocations() == live, nth
        assert lib.fxb_meter_get_level(c._h, None, None) == FX_E_ARG and lib.fxb_meter_read_level(c._h, None, None, 0) == FX_E_ARG
        c.process_block(x)
        assert c.info("meter_level_launches") == 0 and c.info("meter_launches") == 6, "no shard takes level rows"
        assert c.meter_set_level(0.5, 0.25) == 0 and lib.fxstub_live_allocations() == live + 3
        c.process_block(x)
        assert L.same_level(c.meter_read_level(), L.level_model(x, 0.5, 0.25)) and c.info("meter_level_launches") == 3
        assert c.load_text(MORE) and c.meter_get_level() == (0.5, 0.25) and not c.meter_read_level()["level"].any()
        c.close()
    clean(lib)
    print("level shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "pieces": child_pieces, "refusals": child_refusals, "streams": child_streams, "queries": child_queries, "shards": child_shards}[sys.argv[1]]()
