"""Tone meters without a GPU: fxb_meter_set_tones / _get_tones / _clear_tones / _read_tones / _read_tones_list / _select_tone /
_rank_tone on the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven
through the C ABI in a child process like tests/test_meter_level_stub.py (this file is also that child).  The stand-in's emulation
launch copies input to output, so the figures are a function of the input the test builds; the stand-ins of the kernels
(tests/hipstub/fx_meter_tone_stub.cpp) work in stream order with a formulation of their own.  The model is
meter_tone_model.tone_model; the bar is equality of words, fp64 as uint64.

This checks the host layers: every route a block can take with the mode on, beside a twin without it whose four (with a target
and level meters: eight) accumulators must be equal; 16 + 17 samples against 33, pieces, the segments of an armed control track,
shards on unaligned starts; a second set_tones, which zeroes; every reset rule; the list reset behind a slow block; refusals with
nothing changed and an allocation failure at each allocation; select and rank against the model; the counters.  The kernels:
tests/test_gpu_meter_tone.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_level_model as L  # noqa: E402
import meter_target_model as TG  # noqa: E402
import meter_tone_model as T  # noqa: E402
from test_meter_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MORE, PROGRAM, ROOT, STEREO, Pinned, expand, same_meters  # noqa: E402

COUNTERS = ("meter_tone_launches", "meter_tone_selects", "meter_tone_list_reads", "meter_tone_ranks")
COEFFS = ([T.coeff(5, 64)], [2.0, -2.0, 0.0], [T.coeff(k, 64) for k in range(1, 9)], [1.25, T.coeff(16, 64)])


def run_child(which, marker, devices=1):
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_tone_meters_on_every_route_on_the_hip_stand_in():
    run_child("routes", "tone routes ok")


def test_tone_meters_through_pieces_and_track_segments_on_the_hip_stand_in():
    run_child("pieces", "tone pieces ok")


def test_tone_refusals_resets_and_allocation_failures_on_the_hip_stand_in():
    run_child("refusals", "tone refusals ok")


def test_tone_reset_list_behind_a_slow_block_on_the_hip_stand_in():
    run_child("streams", "tone streams ok")


def test_tone_select_and_rank_on_the_hip_stand_in():
    run_child("queries", "tone queries ok")


def test_tone_meters_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "tone shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_live_allocations", "fxstub_meter_tone_launches", "fxstub_tone_selects", "fxstub_tone_gathers",
              "fxstub_tone_zeros", "fxstub_tone_ranks", "fxstub_tone_strays", "fxstub_meter_zeros", "fxstub_level_zeros", "fxstub_match_zeros"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def clean(lib):
    assert lib.fxstub_tone_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0


class Pair:
    """a handle with tone meters on, its twin with meters on and the mode off, and the model of the rows.  With `full` both also
    carry a target and level meters: the eight accumulators"""

    def __init__(self, A, lib, N, ch, coeffs, devices=None, full=None):
        text = {1: PROGRAM, 2: STEREO}[ch]
        self.lib, self.N, self.ch = lib, N, ch
        self.b = A.Batch(N, ch, 0) if devices is None else A.Batch(N, ch, devices=devices)
        self.twin = A.Batch(N, ch, 0)
        for h in (self.b, self.twin):
            assert h.load_text(text), h.errors()
            assert h.meter_enable() == 0
            if full is not None:
                assert h.meter_set_target(*full) == 0 and h.meter_set_level(0.5, 0.25) == 0
        self.full = full is not None
        self.shards = 1 if devices is None else len(devices)
        self.launches = 0
        self.set(coeffs)

    def set(self, coeffs):
        """every set takes the rows into force zeroed"""
        assert self.b.meter_set_tones(coeffs) == 0
        self.coeffs = [float(c) + 0.0 for c in coeffs]
        got = self.b.meter_get_tones()
        assert np.array_equal(got.view(np.uint64), np.array(self.coeffs).view(np.uint64)), got
        self.acc = T.tone_zero(len(coeffs), self.ch, self.N)

    def both(self, call):
        for h in (self.b, self.twin):
            call(h)

    def took(self, what, y, launches=1):
        """both handles were given the same call, which returned the per-instance block y in `launches` launches per shard"""
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, self.ch, self.N)
        self.acc = T.tone_model(y, self.coeffs, self.acc)
        self.launches += launches * self.shards
        got = self.b.meter_read_tones()
        want = T.rows_of(self.acc, self.coeffs)
        assert T.same_tones(got, want), (what, T.differing(got, want))
        assert same_meters(self.b.meter_read(), self.twin.meter_read()), (what, "the four with the mode on are those of a twin without it")
        if self.full:
            assert TG.same_match(self.b.meter_read_match(), self.twin.meter_read_match()) and self.b.meter_target_pos() == self.twin.meter_target_pos(), (what, "the six")
            assert L.same_level(self.b.meter_read_level(), self.twin.meter_read_level()), (what, "the eight")
        assert self.b.meter_samples() == self.twin.meter_samples(), what
        assert self.b.info("meter_tone_launches") == self.launches, (what, self.b.info("meter_tone_launches"), self.launches)
        for counted in ("meter_launches", "meter_target_launches", "meter_level_launches"):
            assert self.b.info(counted) == self.twin.info(counted) * self.shards, (what, counted, "the same blocks are counted")

    def close(self):
        self.b.close()
        self.twin.close()


def child_routes():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(261)
    S = 33
    cases = ((5, 1, COEFFS[0], False), (197, 1, COEFFS[2], False), (256, 2, COEFFS[1], False), (257, 2, COEFFS[3], False), (130, 2, COEFFS[1], True), (197, 1, COEFFS[2], True))
    for N, ch, coeffs, full in cases:
        target = (TG.words(rng, (40, ch, -(-N // 3))), 3, True) if full else None
        p = Pair(A, lib, N, ch, coeffs, full=target)
        seen = lib.fxstub_meter_tone_launches()
        # 16 + 17 samples; then 33 at once
        x = L.words(rng, (S, ch, N))
        p.both(lambda h: h.process_block(x[:16]))
        p.took("pageable, 16 samples", x[:16])
        p.both(lambda h: h.process_block(x[16:]))
        p.took("pageable, 17 more", x[16:])
        assert T.same_tones(p.acc, T.tone_model(x, coeffs), ("s1", "s2")), "16 + 17 against 33"
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
            pg, po = pinned((S, ch, g)), pinned((S, ch, g))
            pg[...] = xg
            for h in (p.b, p.twin):
                assert h.process_block_bus_dev(int(pg.ctypes.data), int(po.ctypes.data), S, K) == 0
            p.took("bus %d device entry" % K, expand(xg, K, N))
        # instance-major
        xi = np.ascontiguousarray(L.words(rng, (N, S, ch)))
        p.both(lambda h: h.process_block_imajor(xi))
        p.took("instance-major", np.ascontiguousarray(xi.transpose(1, 2, 0)))
        assert lib.fxstub_meter_tone_launches() - seen == p.launches
        # a second set_tones zeroes: other coefficients, another count
        p.set([1.5] if len(coeffs) > 1 else [0.25, -0.25])
        assert T.same_tones(p.b.meter_read_tones(), T.rows_of(p.acc, p.coeffs)) and not p.b.meter_read_tones()["s1"].any(), "a second set zeroes"
        x = L.words(rng, (S, ch, N))
        p.both(lambda h: h.process_block(x))
        p.took("after a second set", x)
        # the mode cleared: no tone launch, the others go on
        assert p.b.meter_clear_tones() == 0 and lib.fxb_meter_get_tones(p.b._h, None, None) == FX_E_ARG
        p.both(lambda h: h.process_block(x))
        assert p.b.info("meter_tone_launches") == p.launches and same_meters(p.b.meter_read(), p.twin.meter_read())
        pinned.free()
        p.close()
    clean(lib)
    print("tone routes ok")


def child_pieces():
    A, lib = stub_library()
    rng = np.random.default_rng(267)
    # 96 samples of 262 144 instances on a bus: two pieces of 48 samples; a pageable block of 32 MiB: eight pieces
    N, S, K = 262144, 96, 64
    p = Pair(A, lib, N, 1, [T.coeff(3, 32)])
    xg = L.words(rng, (S, 1, p.b.bus_groups(K)))
    p.both(lambda h: h.process_block_bus(xg, K))
    p.took("bus, two pieces", expand(xg, K, N), launches=2)
    x = L.words(rng, (32, 1, N))
    p.both(lambda h: h.process_block(x))
    p.took("pipelined host block", x, launches=8)
    p.close()
    # an armed control track: the interpreter tier cuts the block at the change points - five segments, five tone launches; the
    # translated tier reads the schedule by itself - one
    for tier, segments in (("asm", 5), (None, 1)):
        if tier:
            os.environ["FX_KERNEL"] = tier
        p = Pair(A, lib, 197, 1, COEFFS[1])
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
    print("tone pieces ok")


def child_refusals():
    os.environ["FX_BUILDER"] = "0"   # (allocations are counted below: none may come from the handle's builder thread meanwhile)
    A, lib = stub_library()
    rng = np.random.default_rng(271)
    N, S, ch = 197, 33, 2
    b = A.Batch(N, ch, 0)
    assert b.load_text(STEREO), b.errors()
    x = L.words(rng, (S, ch, N))
    rows = [np.full((8, ch, N), 9.0, dtype=np.float64) for _ in range(3)]
    buf = np.full(N + 8, T.MARK, dtype=np.int64)
    val = np.full(N + 8, 9.0, dtype=np.float64)
    two = np.array([3, 5], dtype=np.int64)
    cnt, got8 = C.c_int(9), np.full(8, 9.0, dtype=np.float64)
    good = np.array([1.0, -1.0], dtype=np.float64)

    def queries(h):
        return (lib.fxb_meter_read_tones(h, ptr(rows[0]), ptr(rows[1]), ptr(rows[2]), 0), lib.fxb_meter_read_tones_list(h, ptr(two), 2, ptr(rows[0]), ptr(rows[1]), ptr(rows[2]), 0),
                lib.fxb_meter_select_tone(h, 0, C.c_double(0.0), 0, N, ptr(buf), N, 0), lib.fxb_meter_select_tone(h, 0, C.c_double(0.0), 0, 0, None, 0, 0),
                lib.fxb_meter_rank_tone(h, 0, 4, C.c_double(0.0), 0, N, ptr(buf), ptr(val), 0), lib.fxb_meter_get_tones(h, C.byref(cnt), ptr(got8)))

    def untouched():
        return all((r == 9.0).all() for r in rows) and (buf == T.MARK).all() and (val == 9.0).all() and cnt.value == 9 and (got8 == 9.0).all()

    # metering off: the set is refused; so is every query; clear has nothing to drop
    live = lib.fxstub_live_allocations()
    assert lib.fxb_meter_set_tones(b._h, 2, ptr(good), 0) == FX_E_ARG and "metering is off" in b.last_error()
    assert set(queries(b._h)) == {FX_E_ARG} and untouched() and lib.fxb_meter_clear_tones(b._h) == 0 and lib.fxstub_live_allocations() == live
    assert b.meter_enable() == 0
    # metering on, the mode off: every query is refused, nothing launched, nothing written
    assert set(queries(b._h)) == {FX_E_ARG} and "mode is off" in b.last_error() and untouched()
    live = lib.fxstub_live_allocations()

    def refused_sets(state, held=0):
        for what, word, n, coeff, flags in (("no tone", "n_tones", 0, good, 0), ("nine tones", "n_tones", 9, np.zeros(9), 0), ("a negative count", "n_tones", -1, good, 0), ("a null coeff", "null", 2, None, 0),
                                            ("a NaN", "coeff[1]", 2, np.array([1.0, np.nan]), 0), ("an infinity", "coeff[0]", 2, np.array([np.inf, 1.0]), 0),
                                            ("beyond 2", "coeff[1]", 2, np.array([2.0, np.nextafter(2.0, 3.0)]), 0), ("below -2", "coeff[0]", 1, np.array([np.nextafter(-2.0, -3.0)]), 0),
                                            ("a flag", "flags", 2, good, 1), ("a high flag", "flags", 2, good, 1 << 31)):
            assert lib.fxb_meter_set_tones(b._h, n, ptr(coeff), flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
            assert lib.fxstub_live_allocations() == live + held and state(), what

    refused_sets(lambda: set(queries(b._h)) == {FX_E_ARG} and untouched())
    assert all(f(None, *a) == FX_E_ARG for f, a in ((lib.fxb_meter_set_tones, (2, ptr(good), 0)), (lib.fxb_meter_clear_tones, ()), (lib.fxb_meter_get_tones, (None, None)), (lib.fxb_meter_read_tones, (None, None, None, 0)),
                                                    (lib.fxb_meter_read_tones_list, (None, 0, None, None, None, 0)), (lib.fxb_meter_select_tone, (0, C.c_double(0.0), 0, 0, None, 0, 0)),
                                                    (lib.fxb_meter_rank_tone, (0, 0, C.c_double(0.0), 0, 0, None, None, 0))))
    b.process_block(x)
    assert b.info("meter_launches") == 1 and [b.info(k) for k in COUNTERS] == [0, 0, 0, 0]
    live = lib.fxstub_live_allocations()   # (the block's own buffers exist now)
    # an allocation that fails at the one allocation of the set: FX_E_MEMORY, the mode off, the handle usable
    lib.fxstub_fail_mallocs(0, 1)
    assert lib.fxb_meter_set_tones(b._h, 2, ptr(good), 0) == FX_E_MEMORY and b.last_error()
    lib.fxstub_fail_mallocs(-1, 0)
    assert lib.fxstub_live_allocations() == live and set(queries(b._h)) == {FX_E_ARG} and untouched()
    b.process_block(x)
    assert b.info("meter_tone_launches") == 0 and b.info("meter_launches") == 2
    # set: all device allocation of the feature happens here - none inside a block; -0.0 is taken as +0.0
    assert b.meter_set_tones([-0.0, 2.0, -2.0]) == 0 and lib.fxstub_live_allocations() == live + 1
    got = b.meter_get_tones()
    assert got.tolist() == [0.0, 2.0, -2.0] and not np.signbit(got[0])
    b.process_block(x)
    want = T.rows_of(T.tone_model(x, [0.0, 2.0, -2.0]), [0.0, 2.0, -2.0])
    assert T.same_tones(b.meter_read_tones(), want) and lib.fxstub_live_allocations() == live + 1
    # with the mode on: a failing allocation and every refused set leave the mode, the coefficients and every word as they were
    lib.fxstub_fail_mallocs(0, 1)
    assert lib.fxb_meter_set_tones(b._h, 2, ptr(good), 0) == FX_E_MEMORY
    lib.fxstub_fail_mallocs(-1, 0)
    refused_sets(lambda: b.meter_get_tones().tolist() == [0.0, 2.0, -2.0] and T.same_tones(b.meter_read_tones(), want), held=1)
    assert lib.fxstub_live_allocations() == live + 1 and b.meter_get_tones().tolist() == [0.0, 2.0, -2.0] and T.same_tones(b.meter_read_tones(), want)
    # a second set zeroes and replaces the block: one allocation in force before and after
    assert b.meter_set_tones(good) == 0 and lib.fxstub_live_allocations() == live + 1 and not b.meter_read_tones()["s1"].any()
    b.process_block(x)
    coeffs = good.tolist()
    want = T.rows_of(T.tone_model(x, coeffs), coeffs)
    assert T.same_tones(b.meter_read_tones(), want) and b.info("meter_tone_launches") == 2 and b.info("meter_launches") == 4
    # the refusals of the queries with the mode on: nothing launched, nothing written
    assert b.meter_select_tone(0, -np.inf)[1] == N and b.meter_read_tones_list([1])["s1"].shape == (2, ch, 1) and b.meter_rank_tone(1, 3)[0] == N   # (their staging exists from here)
    seen = ([b.info(k) for k in COUNTERS], lib.fxstub_tone_selects(), lib.fxstub_tone_gathers(), lib.fxstub_tone_ranks())
    for what, word, tone, thr, first, n_range, lst, cap, flags in (("tone = K", "tone", 2, 0.0, 0, N, buf, N, 0), ("tone = 8", "tone", 8, 0.0, 0, N, buf, N, 0), ("tone = -1", "tone", -1, 0.0, 0, N, buf, N, 0),
                                                                   ("a NaN threshold", "NaN", 0, np.nan, 0, N, buf, N, 0), ("an unknown flag", "flags", 0, 0.0, 0, N, buf, N, 2), ("first < 0", "first", 0, 0.0, -1, 4, buf, 4, 0),
                                                                   ("first + n_range = N + 1", "n_range", 0, 0.0, 1, N, buf, N, 0), ("cap < 0", "cap", 0, 0.0, 0, N, buf, -1, 0), ("a null list with cap > 0", "null list", 0, 0.0, 0, N, None, 1, 0)):
        assert lib.fxb_meter_select_tone(b._h, tone, C.c_double(thr), first, n_range, ptr(lst), cap, flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
    for what, word, tone, k, thr, first, n_range, lst, flags in (("tone = K", "tone", 2, 3, 0.0, 0, N, buf, 0), ("tone = -1", "tone", -1, 3, 0.0, 0, N, buf, 0), ("a NaN threshold", "NaN", 0, 3, np.nan, 0, N, buf, 0),
                                                                 ("an unknown flag", "flags", 0, 3, 0.0, 0, N, buf, 4), ("k < 0", "k < 0", 0, -1, 0.0, 0, N, buf, 0), ("a null list", "null list", 0, 3, 0.0, 0, N, None, 0),
                                                                 ("a range beyond N", "n_range", 0, 3, 0.0, 1, N, buf, 0)):
        assert lib.fxb_meter_rank_tone(b._h, tone, k, C.c_double(thr), first, n_range, ptr(lst), ptr(val), flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
    for what, lst, count, reset in (("count < 0", two, -1, 0), ("a null list", None, 2, 0), ("an entry = N", np.array([3, N], dtype=np.int64), 2, 0), ("an entry < 0", np.array([-1, 3], dtype=np.int64), 2, 0),
                                    ("a repeat under reset", np.array([3, 5, 3], dtype=np.int64), 3, 1)):
        assert lib.fxb_meter_read_tones_list(b._h, ptr(lst), count, ptr(rows[0]), ptr(rows[1]), ptr(rows[2]), reset) == FX_E_ARG and b.last_error(), what
    assert lib.fxb_meter_select(b._h, 4, C.c_double(0.0), 0, N, ptr(buf), N, 0) == FX_E_ARG, "fxb_meter_select keeps refusing stat = 4"
    assert lib.fxb_meter_rank_level(b._h, 0, 3, C.c_double(0.0), 0, N, ptr(buf), ptr(val), 0) == FX_E_ARG, "fxb_meter_rank_level keeps asking for its mode"
    assert seen == ([b.info(k) for k in COUNTERS], lib.fxstub_tone_selects(), lib.fxstub_tone_gathers(), lib.fxstub_tone_ranks()) and untouched()
    assert T.same_tones(b.meter_read_tones(), want)
    # any of the three pointers may be NULL; a repeat without reset is fine
    for keep in range(3):
        out = [np.full((2, ch, N), 9.0) for _ in range(3)]
        assert lib.fxb_meter_read_tones(b._h, *[ptr(out[i]) if i == keep else None for i in range(3)], 0) == 0
        assert np.array_equal(out[keep].view(np.uint64), want[("s1", "s2", "power")[keep]].view(np.uint64)) and all((out[i] == 9.0).all() for i in range(3) if i != keep)
        out = [np.full((2, ch, 2), 9.0) for _ in range(3)]
        assert lib.fxb_meter_read_tones_list(b._h, ptr(two), 2, *[ptr(out[i]) if i == keep else None for i in range(3)], 0) == 0
        assert np.array_equal(out[keep].view(np.uint64), np.ascontiguousarray(want[("s1", "s2", "power")[keep]][:, :, two]).view(np.uint64)) and all((out[i] == 9.0).all() for i in range(3) if i != keep)
    lst = [5, 3, 5, N - 1]
    reads = b.info("meter_tone_list_reads")
    assert T.same_tones(b.meter_read_tones_list(lst), {k: v[:, :, lst] for k, v in want.items()}) and b.info("meter_tone_list_reads") == reads + 1
    # read_tones with reset zeroes only the tone rows; fxb_meter_read(reset) zeroes them as well and keeps the mode
    four = b.meter_read()
    zero = T.rows_of(T.tone_zero(2, ch, N), coeffs)
    assert T.same_tones(b.meter_read_tones(reset=True), want) and T.same_tones(b.meter_read_tones(), zero)
    assert same_meters(b.meter_read(), four) and b.meter_samples() == 4 * S
    b.process_block(x)
    assert T.same_tones(b.meter_read_tones(), want)
    b.meter_read(reset=True)
    assert T.same_tones(b.meter_read_tones(), zero) and b.meter_samples() == 0 and not b.meter_read()["energy"].any() and b.meter_get_tones().tolist() == coeffs
    # read_tones_list with reset zeroes the listed columns of the tone rows alone; reset_list those of every row
    b.process_block(x)
    four = b.meter_read()
    acc = T.tone_model(x, coeffs)
    got = b.meter_read_tones_list([7, 0], reset=True)
    assert T.same_tones(got, {k: v[:, :, [7, 0]] for k, v in want.items()})
    acc = T.zeroed(acc, [7, 0])
    assert T.same_tones(b.meter_read_tones(), T.rows_of(acc, coeffs)) and same_meters(b.meter_read(), four)
    zeros = (lib.fxstub_meter_zeros(), lib.fxstub_tone_zeros())
    assert b.meter_reset_list([9, 196]) == 0
    acc = T.zeroed(acc, [9, 196])
    for k in four:
        four[k][:, [9, 196]] = 0
    assert T.same_tones(b.meter_read_tones(), T.rows_of(acc, coeffs)) and same_meters(b.meter_read(), four) and (lib.fxstub_meter_zeros(), lib.fxstub_tone_zeros()) == (zeros[0] + 1, zeros[1] + 1)
    # instance copy and reset leave the tone rows alone, as they leave every meter alone
    assert b.copy_instances([1], [2]) == 0 and b.reset_instances([2, 3]) == 0 and b.sync() == 0
    assert T.same_tones(b.meter_read_tones(), T.rows_of(acc, coeffs)) and same_meters(b.meter_read(), four)
    # a program load zeroes the rows and keeps the mode and its coefficients
    assert b.load_text(MORE), b.errors()
    assert b.meter_get_tones().tolist() == coeffs and T.same_tones(b.meter_read_tones(), zero) and b.meter_samples() == 0
    launches = b.info("meter_tone_launches")
    b.process_block(x)
    assert b.info("meter_tone_launches") == launches + 1 and T.same_tones(b.meter_read_tones(), want)
    # clear_tones and meter_enable(0) free the rows
    live = lib.fxstub_live_allocations()
    assert b.meter_clear_tones() == 0 and lib.fxstub_live_allocations() == live - 1 and set(queries(b._h)) == {FX_E_ARG}
    assert b.meter_set_tones([1.0]) == 0 and lib.fxstub_live_allocations() == live
    assert b.meter_enable(False) == 0 and lib.fxstub_live_allocations() == live - 2
    assert b.meter_enable() == 0 and set(queries(b._h)) == {FX_E_ARG}
    b.close()
    clean(lib)
    print("tone refusals ok")


def child_streams():
    """a list reset behind a slow block returns while that block is still running; when everything has run, the tone columns of the
    listed voices - and only those - are zero behind block 1, and block 2 has been taken by all"""
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(273)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    n, S = 1000, 8
    coeffs = [T.coeff(1, 8), 2.0]
    b = A.Batch(n, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    assert b.meter_enable() == 0 and b.meter_set_tones(coeffs) == 0
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
    zeros = (lib.fxstub_meter_zeros(), lib.fxstub_tone_zeros())
    lib.fxstub_set_kernel_micros(150000)
    assert lib.fxb_process_block_dev(b._h, ptr(first[0]), ptr(first[1]), S, streams[0]) == 0
    assert b.meter_reset_list(lst) == 0
    given = lst.copy()
    lst[:] = 7
    assert (first[1][S - 1] == -7.0).all(), "the list reset returned while the block in front of it was still running"
    assert (lib.fxstub_meter_zeros(), lib.fxstub_tone_zeros()) == zeros, "... and both zeroing launches are queued behind that block"
    lib.fxstub_set_kernel_micros(150)
    assert lib.fxb_process_block_dev(b._h, ptr(second[0]), ptr(second[1]), S, streams[1]) == 0
    got = b.meter_read_tones()
    assert (lib.fxstub_meter_zeros(), lib.fxstub_tone_zeros()) == (zeros[0] + 1, zeros[1] + 1)
    one = T.tone_model(first[0], coeffs)
    want = T.tone_model(second[0], coeffs, T.zeroed(one, given))
    assert T.same_tones(got, T.rows_of(want, coeffs)) and not T.same_tones(got, T.rows_of(T.tone_model(second[0], coeffs, one), coeffs))
    # with the mode off the list reset launches fx_meter_zero alone
    assert b.meter_clear_tones() == 0 and b.meter_reset_list(given) == 0 and b.sync() == 0
    assert (lib.fxstub_meter_zeros(), lib.fxstub_tone_zeros()) == (zeros[0] + 2, zeros[1] + 1)
    pinned.free()
    b.close()
    clean(lib)
    print("tone streams ok")


def tied_voices(rng, S, ch, N, group=7):
    """groups of `group` neighbouring voices get identical input, so that P ties bit for bit and the instance number decides;
    one channel of voice 7 carries a louder signal of its own: the maximum over the channels"""
    g = -(-N // group)
    x = np.repeat(L.words(rng, (S, ch, g)), group, axis=2)[:, :, :N].copy()
    if ch > 1:
        x[:, 1, 7] = 1.0
    return x


def child_queries():
    A, lib = stub_library()
    rng = np.random.default_rng(279)
    for ch, N, coeffs in ((1, 200, COEFFS[1]), (2, 257, COEFFS[3])):
        p = Pair(A, lib, N, ch, coeffs)
        x = tied_voices(rng, 33, ch, N)
        p.both(lambda h: h.process_block(x))
        p.took("one block", x)
        rows = p.b.meter_read_tones()
        if ch == 2:
            assert T.V(rows, 0)[7] == rows["power"][0, 1, 7] > rows["power"][0, 0, 7], "the maximum over the channels"
        before = (p.b.info("meter_tone_selects"), lib.fxstub_tone_selects(), p.b.info("meter_tone_ranks"), lib.fxstub_tone_ranks())
        assert T.check_selects(lib, p.b, rows, N, len(coeffs)) >= 6
        calls = T.check_ranks(lib, p.b, rows, len(coeffs))
        assert p.b.info("meter_tone_selects") - before[0] == lib.fxstub_tone_selects() - before[1] > 50 and p.b.info("meter_selects") == 0
        assert p.b.info("meter_tone_ranks") - before[2] == lib.fxstub_tone_ranks() - before[3] > 50 and calls > 50 and p.b.info("meter_ranks") == 0
        got, m = p.b.meter_select_tone(0, np.inf, below=True)
        assert m == N and np.array_equal(got, np.arange(N))
        m, lst, val = p.b.meter_rank_tone(0, 5, largest=True)
        want = T.rank(rows, 0, 5, largest=True)
        assert m == N and np.array_equal(lst, want[1]) and np.array_equal(val.view(np.uint64), want[2].view(np.uint64))
        assert T.same_tones(p.b.meter_read_tones(), rows), "the queries change nothing"
        p.close()
    clean(lib)
    print("tone queries ok")


def child_shards():
    """three shards starting at 320 and 576"""
    os.environ["FX_BUILDER"] = "0"
    A, lib = stub_library()
    rng = np.random.default_rng(283)
    N, S, ch = 3 * 256 + 40, 33, 2
    for full in (False, True):
        target = (TG.words(rng, (40, ch, -(-N // 3))), 3, True) if full else None
        p = Pair(A, lib, N, ch, COEFFS[1], devices=[0, 1, 2], full=target)
        assert [(d, f) for d, f, _ in p.b.shards()] == [(0, 0), (1, 320), (2, 576)], p.b.shards()
        x = tied_voices(rng, S, ch, N)
        p.both(lambda h: h.process_block(x[:16]))
        p.took("pageable, 16 samples", x[:16])
        p.both(lambda h: h.process_block(x[16:]))
        p.took("pageable, 17 more", x[16:])
        xg = L.words(rng, (S, ch, p.b.bus_groups(64)))
        p.both(lambda h: h.process_block_bus(xg, 64))
        p.took("bus 64", expand(xg, 64, N))
        rows = p.b.meter_read_tones()
        T.check_selects(lib, p.b, rows, N, 3, "three shards", starts=(0, 65, 319, 575))
        T.check_ranks(lib, p.b, rows, 3, "three shards", starts=(0, 319, 575))
        for first, n_range in ((300, 300), (319, 2), (319, 258), (575, 2), (600, 50)):
            t = float(np.median(T.V(rows, 1)))
            want = T.check_select(lib, p.b, rows, 1, t, False, first, n_range, n_range)
            for cap in {0, 1, want.size // 2, max(want.size - 1, 0), want.size + 3}:
                T.check_select(lib, p.b, rows, 1, t, True, first, n_range, cap)
            for k in (0, 1, 5, n_range):
                T.check_rank(lib, p.b, rows, 1, k, t, False, True, first, n_range, "a range across shards")
        # list read, list reset and read with reset on every shard
        lst = np.array([N - 1, 0, 319, 320, 575, 576, 320], dtype=np.int64)
        assert T.same_tones(p.b.meter_read_tones_list(lst), {k: v[:, :, lst] for k, v in rows.items()})
        lst = lst[:6]
        p.both(lambda h: h.meter_reset_list(lst))
        p.acc = T.zeroed(p.acc, lst)
        p.took("a list reset", np.zeros((0, ch, N), dtype=np.float32), launches=0)
        got = p.b.meter_read_tones_list([1, 321, 577], reset=True)
        assert T.same_tones(got, {k: v[:, :, [1, 321, 577]] for k, v in T.rows_of(p.acc, p.coeffs).items()})
        p.acc = T.zeroed(p.acc, [1, 321, 577])
        p.both(lambda h: h.process_block(x))
        p.took("a block behind the list resets", x)
        p.set(COEFFS[3])
        p.both(lambda h: h.process_block(x))
        p.took("after a second set", x)
        p.close()
    # an allocation that fails on whichever shard (one per shard): FX_E_MEMORY, the mode as it was on every shard, then the same call works
    x = L.words(rng, (S, ch, N))
    for was_on in (False, True):
        for nth in range(3):
            c = A.Batch(N, ch, devices=[0, 1, 2])
            assert c.load_text(STEREO) and c.meter_enable() == 0
            if was_on:
                assert c.meter_set_tones([0.5]) == 0
            c.process_block(x)   # (the block's own buffers exist before allocations are counted)
            before = T.rows_of(T.tone_model(x, [0.5]), [0.5])
            live = lib.fxstub_live_allocations()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = lib.fxb_meter_set_tones(c._h, 2, ptr(np.array([1.0, -1.0])), 0)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and c.last_error() and lib.fxstub_live_allocations() == live, nth
            if was_on:
                assert c.meter_get_tones().tolist() == [0.5] and T.same_tones(c.meter_read_tones(), before), "the mode as it was"
            else:
                assert lib.fxb_meter_get_tones(c._h, None, None) == FX_E_ARG and lib.fxb_meter_read_tones(c._h, None, None, None, 0) == FX_E_ARG
            c.process_block(x)
            assert c.info("meter_tone_launches") == (6 if was_on else 0) and c.info("meter_launches") == 6
            assert c.meter_set_tones([1.0, -1.0]) == 0 and lib.fxstub_live_allocations() == live + (0 if was_on else 3)
            c.process_block(x)
            assert T.same_tones(c.meter_read_tones(), T.rows_of(T.tone_model(x, [1.0, -1.0]), [1.0, -1.0]))
            assert c.load_text(MORE) and c.meter_get_tones().tolist() == [1.0, -1.0] and not c.meter_read_tones()["s1"].any()
            c.close()
    clean(lib)
    print("tone shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "pieces": child_pieces, "refusals": child_refusals, "streams": child_streams, "queries": child_queries, "shards": child_shards}[sys.argv[1]]()
