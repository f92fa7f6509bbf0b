"""Target meters without a GPU: fxb_meter_set_target / _clear_target / _target_seek / _target_pos / _read_match / _select_match /
fxb_meter_best on the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`),
driven through the C ABI in a child process like tests/test_meter_stub.py (this file is also that child).  The stand-in's
emulation launch copies input to output, so the figures are a function of the input the test builds; the stand-ins of the kernels
(tests/hipstub/fx_meter_target_stub.cpp) work in stream order with a formulation of their own.  The model is
meter_target_model.match_model; the bar is equality, fp64 words as integers.

This checks the host layers: every route a block can take with a target set, the position carried from launch to launch (16 + 17
samples against 33, pieces, the segments of an armed control track, shards on unaligned starts), the four existing accumulators
against a twin without a target, resets, refusals, allocation failures, the counters.  The kernels: tests/test_gpu_meter_target.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_target_model as T  # noqa: E402
from test_meter_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MORE, PROGRAM, ROOT, STEREO, Pinned, expand, same_meters  # noqa: E402

COUNTERS = ("meter_target_launches", "meter_match_selects", "meter_match_bests")


def run_child(which, marker, devices=1):
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_match_model_splits_and_the_written_out_loop():
    """the restatement itself: 16 + 17 samples give the bits of 33, with the position carried; one column written out in Python
    floats; a sample past the end without LOOP and a non-finite word change nothing"""
    rng = np.random.default_rng(3)
    y, t = T.words(rng, (33, 2, 70)), T.words(rng, (20, 2, 24))
    for loop in (False, True):
        whole, after = T.match_model(y, t, 3, 7, loop)
        part, pos = T.match_model(y[:16], t, 3, 7, loop)
        part, pos = T.match_model(y[16:], t, 3, pos, loop, part)
        assert T.same_match(part, whole) and pos == after == ((7 + 33) % 20 if loop else 40)
        for c, n in ((0, 0), (1, 5), (0, 69)):
            e = x = 0.0
            for s in range(33):
                q = (7 + s) % 20 if loop else 7 + s
                if q >= 20:
                    continue
                a, b = float(y[s, c, n]), float(t[q, c, n // 3])
                if not (abs(a) < np.inf and abs(b) < np.inf):
                    continue
                d = a - b
                e = e + d * d
                x = x + a * b
            assert (e, x) == (whole["err"][c, n], whole["cross"][c, n]), (loop, c, n)
        assert np.isfinite(whole["err"]).all() and np.isfinite(whole["cross"]).all()
    rows = {"err": np.array([[1.0, 0.5, 0.5, 2.0, 0.25]]), "cross": np.array([[-1.0, 3.0, 3.0, 0.0, -2.0]])}
    assert T.best(rows, 0, 2)[0].tolist() == [1, 2, 4] and T.best(rows, 0, 9)[0].tolist() == [4] and T.best(rows, 1, 5, largest=True)[0].tolist() == [1]
    assert T.select(rows, 1, 0.0, True).tolist() == [0, 4] and T.select(rows, 0, 0.5, False, 1, 3).tolist() == [1, 2, 3]


def test_target_meters_on_every_route_on_the_hip_stand_in():
    run_child("routes", "target routes ok")


def test_target_position_through_pieces_and_track_segments_on_the_hip_stand_in():
    run_child("pieces", "target pieces ok")


def test_target_refusals_resets_and_allocation_failures_on_the_hip_stand_in():
    run_child("refusals", "target refusals ok")


def test_target_reset_list_behind_a_slow_block_on_the_hip_stand_in():
    run_child("streams", "target streams ok")


def test_target_queries_on_the_hip_stand_in():
    run_child("queries", "target queries ok")


def test_target_meters_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "target shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_kernels_run", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_meter_launches", "fxstub_live_allocations", "fxstub_meter_target_launches",
              "fxstub_match_selects", "fxstub_match_bests", "fxstub_match_zeros", "fxstub_match_strays", "fxstub_meter_zeros"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def clean(lib):
    assert lib.fxstub_match_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0


class Pair:
    """a handle with a target, its twin without one, and the model of the match rows and the position"""

    def __init__(self, A, lib, N, ch, devices=None):
        text = {1: PROGRAM, 2: STEREO}[ch]
        self.lib, self.N, self.ch = lib, N, ch
        self.b = A.Batch(N, ch, 0) if devices is None else A.Batch(N, ch, devices=devices)
        self.twin = A.Batch(N, ch, 0)
        for h in (self.b, self.twin):
            assert h.load_text(text), h.errors()
            assert h.meter_enable() == 0
        self.shards = 1 if devices is None else len(devices)
        self.launches = 0

    def target(self, t, group, loop):
        assert self.b.meter_set_target(t, group, loop) == 0
        self.t, self.group, self.loop, self.pos, self.acc = t, group, loop, 0, T.match_zero(self.ch, self.N)
        assert self.b.meter_target_pos() == 0

    def took(self, what, y, launches=1):
        """both handles were given the same call, which returned the per-instance block y in `launches` launches per shard"""
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, self.ch, self.N)
        self.acc, self.pos = T.match_model(y, self.t, self.group, self.pos, self.loop, self.acc)
        self.launches += launches * self.shards
        assert T.same_match(self.b.meter_read_match(), self.acc), what
        assert self.b.meter_target_pos() == self.pos, (what, self.b.meter_target_pos(), self.pos)
        assert same_meters(self.b.meter_read(), self.twin.meter_read()), (what, "the four with a target set are those of a twin without one")
        assert self.b.meter_samples() == self.twin.meter_samples(), what
        assert self.b.info("meter_target_launches") == self.launches, (what, self.b.info("meter_target_launches"), self.launches)

    def close(self):
        self.b.close()
        self.twin.close()


def child_routes():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(61)
    S = 33
    for ch in (1, 2):
        for N, group, tlen, loop in ((5, 1, 5, True), (197, 3, 40, True), (256, 64, 20, False), (257, 65, 33, False), (130, 1000, 7, True)):
            p = Pair(A, lib, N, ch)
            G = -(-N // min(group, N))
            before = (lib.fxstub_meter_launches(), p.b.info("meter_launches"))
            p.target(T.words(rng, (tlen, ch, G)), group, loop)
            # 16 + 17 samples; then 33 at once: the model carries the position through both
            x = T.words(rng, (S, ch, N))
            for h in (p.b, p.twin):
                h.process_block(x[:16])
            p.took("pageable, 16 samples", x[:16])
            for h in (p.b, p.twin):
                h.process_block(x[16:])
            p.took("pageable, 17 more", x[16:])
            if not loop:
                assert p.b.meter_target_seek(0) == 0
                p.pos = 0
            x = T.words(rng, (S, ch, N))
            for h in (p.b, p.twin):
                h.process_block(x)
            p.took("pageable, 33 at once", x)
            # pinned in place; the device entry; a pitch
            pin, pout = pinned((S, ch, N)), pinned((S, ch, N))
            pin[...] = T.words(rng, (S, ch, N))
            if not loop:
                assert p.b.meter_target_seek(11) == 0
                p.pos = 11
            for h in (p.b, p.twin):
                assert h.process_block(pin, out=pout) is pout
            p.took("pinned in place", pout)
            for h in (p.b, p.twin):
                assert h.process_block_dev(int(pin.ctypes.data), int(pout.ctypes.data), S) == 0
            p.took("device entry", pout)
            P = N + 59
            win = pinned((S, ch, P))
            win[...] = T.words(rng, (S, ch, P))
            for h in (p.b, p.twin):
                assert h.process_block_dev_pitched(int(win.ctypes.data), int(win.ctypes.data), S, P) == 0
            p.took("device entry, pitch N + 59", win[:, :, :N])
            # bus blocks: the scratch block between the emulation and the mix
            if not loop:
                assert p.b.meter_target_seek(0) == 0
                p.pos = 0
            for K in (3, 64):
                g = p.b.bus_groups(K)
                xg, xn = T.words(rng, (S, ch, g)), T.words(rng, (S, ch, N))
                for h in (p.b, p.twin):
                    h.process_block_bus(xg, K, True, False)
                p.took("bus %d shared in" % K, expand(xg, K, N))
                for h in (p.b, p.twin):
                    h.process_block_bus(xn, K, False, True)
                p.took("bus %d mix out" % K, xn)
                for h in (p.b, p.twin):
                    h.process_block_bus(xg, K, True, True)
                p.took("bus %d both" % K, expand(xg, K, N))
                pg, po = pinned((S, ch, g)), pinned((S, ch, g))
                pg[...] = xg
                for h in (p.b, p.twin):
                    assert h.process_block_bus_dev(int(pg.ctypes.data), int(po.ctypes.data), S, K) == 0
                p.took("bus %d device entry" % K, expand(xg, K, N))
            # instance-major
            xi = np.ascontiguousarray(T.words(rng, (N, S, ch)))
            for h in (p.b, p.twin):
                h.process_block_imajor(xi)
            p.took("instance-major", np.ascontiguousarray(xi.transpose(1, 2, 0)))
            assert (lib.fxstub_meter_launches() - before[0], p.b.info("meter_launches") - before[1]) == (p.launches, 0), "fx_meter ran for the twin only"
            assert lib.fxstub_meter_target_launches() >= p.launches
            # the target dropped: fx_meter again, the four go on
            assert p.b.meter_clear_target() == 0 and lib.fxb_meter_target_pos(p.b._h) == FX_E_ARG
            for h in (p.b, p.twin):
                h.process_block(x)
            assert p.b.info("meter_launches") - before[1] == 1 and same_meters(p.b.meter_read(), p.twin.meter_read())
            pinned.free()
            p.close()
    clean(lib)
    print("target routes ok")


def child_pieces():
    A, lib = stub_library()
    rng = np.random.default_rng(67)
    # 96 samples of 262 144 instances on a bus: two pieces of 48 samples; a pageable block of 32 MiB: eight pieces
    N, S, K = 262144, 96, 64
    p = Pair(A, lib, N, 1)
    p.target(T.words(rng, (50, 1, N // 64)), 64, True)
    xg = T.words(rng, (S, 1, p.b.bus_groups(K)))
    for h in (p.b, p.twin):
        h.process_block_bus(xg, K)
    p.took("bus, two pieces", expand(xg, K, N), launches=2)
    x = T.words(rng, (32, 1, N))
    for h in (p.b, p.twin):
        h.process_block(x)
    p.took("pipelined host block", x, launches=8)
    p.close()
    # an armed control track: the interpreter tier cuts the block at the change points - five segments, five target launches, the
    # position carried through them; the translated tier reads the schedule by itself - one
    for tier, segments in (("asm", 5), (None, 1)):
        if tier:
            os.environ["FX_KERNEL"] = tier
        p = Pair(A, lib, 197, 1)
        os.environ.pop("FX_KERNEL", None)
        assert (p.b.info("kernel") >= 9) == (tier is None), p.b.info("kernel")
        p.target(T.words(rng, (40, 1, 66)), 3, True)
        for route in ("pageable", "bus"):
            for h in (p.b, p.twin):
                assert h.set_register_track("vol", [0.1, 0.2, 0.3, 0.4, 0.5], 8) == 0
            if route == "pageable":
                x = T.words(rng, (33, 1, 197))
                for h in (p.b, p.twin):
                    h.process_block(x)
                p.took("armed, " + route, x, launches=segments)
            else:
                xg = T.words(rng, (33, 1, p.b.bus_groups(64)))
                for h in (p.b, p.twin):
                    h.process_block_bus(xg, 64)
                p.took("armed, " + route, expand(xg, 64, 197), launches=segments)
        p.close()
    clean(lib)
    print("target pieces ok")


def child_refusals():
    os.environ["FX_BUILDER"] = "0"   # (allocations are counted below: none may come from the handle's builder thread meanwhile)
    A, lib = stub_library()
    rng = np.random.default_rng(71)
    N, S, ch = 197, 33, 2
    b = A.Batch(N, ch, 0)
    assert b.load_text(STEREO), b.errors()
    x = T.words(rng, (S, ch, N))
    t = T.words(rng, (20, ch, 66))
    err, cross = np.full((ch, N), 9.0), np.full((ch, N), 9.0)
    buf = np.full(N + 8, T.MARK, dtype=np.int64)
    win, val = np.full(N, -5, dtype=np.int64), np.full(N, 9.0)

    def queries(h):
        return (lib.fxb_meter_read_match(h, ptr(err), ptr(cross), 0), lib.fxb_meter_select_match(h, 0, C.c_double(0.0), 0, N, ptr(buf), N, 0),
                lib.fxb_meter_select_match(h, 0, C.c_double(0.0), 0, 0, None, 0, 0), lib.fxb_meter_best(h, 0, 3, ptr(win), ptr(val), 0), lib.fxb_meter_target_seek(h, 0), lib.fxb_meter_target_pos(h))

    def untouched():
        return (err == 9.0).all() and (cross == 9.0).all() and (buf == T.MARK).all() and (win == -5).all() and (val == 9.0).all()

    # metering off: the set is refused; so is every query; clear has nothing to drop
    live = lib.fxstub_live_allocations()
    assert lib.fxb_meter_set_target(b._h, ptr(t), 20, 3, 0) == FX_E_ARG and "metering is off" in b.last_error()
    assert set(queries(b._h)) == {FX_E_ARG} and untouched() and lib.fxb_meter_clear_target(b._h) == 0
    assert b.meter_enable() == 0
    # metering on, no target: every query is refused, nothing launched, nothing written
    assert set(queries(b._h)) == {FX_E_ARG} and "no target" in b.last_error() and untouched()
    live = lib.fxstub_live_allocations()
    # the refusals of the set: nothing changes
    big = 1 << 31
    for what, word, tp, n_samples, group, flags in (("a null target", "null", None, 20, 3, 0), ("n_samples = 0", "n_samples", t, 0, 3, 0), ("n_samples < 0", "n_samples", t, -4, 3, 0),
                                                   ("group = 0", "group", t, 20, 0, 0), ("group < 0", "group", t, 20, -1, 0), ("an unknown flag", "flags", t, 20, 3, 2),
                                                   ("an unknown high flag", "flags", t, 20, 3, 1 << 31), ("2^31 words", "2^31", t, big // (2 * 66) + 1, 3, 0), ("n_samples = 2^62", "2^31", t, 1 << 62, N, 0)):
        assert lib.fxb_meter_set_target(b._h, ptr(tp), n_samples, group, flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
        assert lib.fxstub_live_allocations() == live and set(queries(b._h)) == {FX_E_ARG} and untouched(), what
    assert all(f(None, *a) == FX_E_ARG for f, a in ((lib.fxb_meter_set_target, (ptr(t), 20, 3, 0)), (lib.fxb_meter_clear_target, ()), (lib.fxb_meter_target_seek, (0,)), (lib.fxb_meter_target_pos, ()),
                                                    (lib.fxb_meter_read_match, (None, None, 0)), (lib.fxb_meter_select_match, (0, C.c_double(0.0), 0, 0, None, 0, 0)), (lib.fxb_meter_best, (0, 1, None, None, 0))))
    b.process_block(x)
    assert b.info("meter_launches") == 1 and [b.info(k) for k in COUNTERS] == [0, 0, 0]
    live = lib.fxstub_live_allocations()   # (the block's own buffers exist now)
    # an allocation that fails at each allocation of the set (the target block, the match rows): FX_E_MEMORY, no target, usable
    for nth in (0, 1):
        lib.fxstub_fail_mallocs(nth, 1)
        assert lib.fxb_meter_set_target(b._h, ptr(t), 20, 3, 0) == FX_E_MEMORY and b.last_error()
        lib.fxstub_fail_mallocs(-1, 0)
        assert lib.fxstub_live_allocations() == live and set(queries(b._h)) == {FX_E_ARG} and untouched(), nth
        b.process_block(x)
        assert b.info("meter_target_launches") == 0
    # set: all device allocation of the feature happens here - none inside a block
    assert b.meter_set_target(t, 3) == 0 and lib.fxstub_live_allocations() == live + 2
    b.process_block(x)
    assert lib.fxstub_live_allocations() == live + 2 and b.meter_target_pos() == S
    want, _ = T.match_model(x, t, 3, 0, False)
    assert T.same_match(b.meter_read_match(), want)
    # the refusals of the queries with a target set: nothing launched, nothing written
    seen = ([b.info(k) for k in COUNTERS], lib.fxstub_match_selects(), lib.fxstub_match_bests())
    for what, word, stat, thr, first, n_range, L, cap, flags in (("stat = 2", "stat", 2, 0.0, 0, N, buf, N, 0), ("stat = -1", "stat", -1, 0.0, 0, N, buf, N, 0), ("a NaN threshold", "NaN", 0, np.nan, 0, N, buf, N, 0),
                                                                 ("an unknown flag", "flags", 0, 0.0, 0, N, buf, N, 2), ("first < 0", "first", 0, 0.0, -1, 4, buf, 4, 0), ("first + n_range = N + 1", "n_range", 0, 0.0, 1, N, buf, N, 0),
                                                                 ("cap < 0", "cap", 0, 0.0, 0, N, buf, -1, 0), ("a null list with cap > 0", "null list", 0, 0.0, 0, N, None, 1, 0)):
        assert lib.fxb_meter_select_match(b._h, stat, C.c_double(thr), first, n_range, ptr(L), cap, flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
    for what, word, stat, group, flags in (("stat = 2", "stat", 2, 3, 0), ("stat = -1", "stat", -1, 3, 0), ("group = 0", "group", 0, 0, 0), ("flag bit 0", "flags", 0, 3, 1), ("a high flag", "flags", 0, 3, 1 << 30)):
        assert lib.fxb_meter_best(b._h, stat, group, ptr(win), ptr(val), flags) == FX_E_ARG and word in b.last_error(), (what, b.last_error())
    for pos in (-1, 21, 1 << 40):
        assert lib.fxb_meter_target_seek(b._h, pos) == FX_E_ARG and b.meter_target_pos() == S
    assert lib.fxb_meter_select(b._h, 4, C.c_double(0.0), 0, N, ptr(buf), N, 0) == FX_E_ARG, "fxb_meter_select keeps refusing stat = 4"
    assert seen == ([b.info(k) for k in COUNTERS], lib.fxstub_match_selects(), lib.fxstub_match_bests()) and (buf == T.MARK).all() and (win == -5).all() and (val == 9.0).all()
    # seek: 0 .. n_samples without LOOP; either pointer of read_match may be NULL
    assert b.meter_target_seek(20) == 0 and b.meter_target_pos() == 20 and b.meter_target_seek(4) == 0
    assert lib.fxb_meter_read_match(b._h, ptr(err), None, 0) == 0 and (cross == 9.0).all() and np.array_equal(err.view(np.uint64), want["err"].view(np.uint64))
    assert lib.fxb_meter_read_match(b._h, None, ptr(cross), 0) == 0 and np.array_equal(cross.view(np.uint64), want["cross"].view(np.uint64))
    assert lib.fxb_meter_best(b._h, 0, 3, None, None, 0) == 0
    # read_match with reset zeroes only the two new rows and leaves the position; fxb_meter_read(reset) zeroes all six
    four = b.meter_read()
    assert T.same_match(b.meter_read_match(reset=True), want) and T.same_match(b.meter_read_match(), T.match_zero(ch, N))
    assert same_meters(b.meter_read(), four) and b.meter_samples() == 3 * S + S and b.meter_target_pos() == 4
    b.process_block(x)
    want, pos = T.match_model(x, t, 3, 4, False)
    assert T.same_match(b.meter_read_match(), want) and pos == b.meter_target_pos() == 4 + S
    b.meter_read(reset=True)
    assert T.same_match(b.meter_read_match(), T.match_zero(ch, N)) and b.meter_samples() == 0 and b.meter_target_pos() == 4 + S and not b.meter_read()["energy"].any()
    # with LOOP, pos = n_samples is refused (the queries above have their staging by now: counted from here)
    live = lib.fxstub_live_allocations() - 2
    assert b.meter_set_target(t, 3, loop=True) == 0 and lib.fxstub_live_allocations() == live + 2 and b.meter_target_pos() == 0
    assert lib.fxb_meter_target_seek(b._h, 20) == FX_E_ARG and b.meter_target_seek(19) == 0
    # a second set that cannot allocate leaves the first in force
    lib.fxstub_fail_mallocs(0, 1)
    assert lib.fxb_meter_set_target(b._h, ptr(t), 10, 1000, 0) == FX_E_MEMORY
    lib.fxstub_fail_mallocs(-1, 0)
    assert b.meter_target_pos() == 19 and lib.fxstub_live_allocations() == live + 2
    # a program load drops the target (and keeps metering on); so does fxb_meter_enable(0); both free the two blocks
    assert b.load_text(MORE), b.errors()
    assert lib.fxstub_live_allocations() <= live and set(queries(b._h)) == {FX_E_ARG} and b.meter_samples() == 0
    launches = b.info("meter_target_launches")
    b.process_block(x)
    assert b.info("meter_target_launches") == launches
    live = lib.fxstub_live_allocations()
    assert b.meter_set_target(t, 3) == 0 and lib.fxstub_live_allocations() == live + 2
    assert b.meter_enable(False) == 0 and lib.fxstub_live_allocations() == live - 1
    assert b.meter_enable() == 0 and set(queries(b._h)) == {FX_E_ARG}
    b.close()
    clean(lib)
    print("target refusals ok")


def child_streams():
    """a list reset behind a slow block returns while that block is still running; when everything has run, the match columns
    of the listed voices - and only those - are zero behind block 1, and block 2 has been added to all"""
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(73)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    n, S = 1000, 8
    b = A.Batch(n, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    assert b.meter_enable() == 0
    t = T.words(rng, (40, 1, 334))
    assert b.meter_set_target(t, 3, loop=True) == 0
    b.process_block(T.words(rng, (S, 1, n)))
    b.meter_reset_list([1, 2])   # (the staging exists before anything is timed)
    b.meter_read(reset=True)
    assert b.meter_target_seek(0) == 0

    def fresh():
        p, o = pinned((S, 1, n)), pinned((S, 1, n))
        p[...] = T.words(rng, (S, 1, n))
        o[...] = -7.0
        return p, o

    first, second = fresh(), fresh()
    L = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:63]]).astype(np.int64)
    zeros = (lib.fxstub_meter_zeros(), lib.fxstub_match_zeros())
    lib.fxstub_set_kernel_micros(150000)
    assert lib.fxb_process_block_dev(b._h, ptr(first[0]), ptr(first[1]), S, streams[0]) == 0
    assert b.meter_reset_list(L) == 0
    given = L.copy()
    L[:] = 7
    assert (first[1][S - 1] == -7.0).all(), "the list reset returned while the block in front of it was still running"
    assert (lib.fxstub_meter_zeros(), lib.fxstub_match_zeros()) == zeros, "... and both zeroing launches are queued behind that block"
    lib.fxstub_set_kernel_micros(150)
    assert lib.fxb_process_block_dev(b._h, ptr(second[0]), ptr(second[1]), S, streams[1]) == 0
    got = b.meter_read_match()
    assert (lib.fxstub_meter_zeros(), lib.fxstub_match_zeros()) == (zeros[0] + 1, zeros[1] + 1)
    one, pos = T.match_model(first[0], t, 3, 0, True)
    want, pos = T.match_model(second[0], t, 3, pos, True, T.zeroed(one, given))
    assert T.same_match(got, want) and not T.same_match(got, T.match_model(second[0], t, 3, S, True, one)[0]) and b.meter_target_pos() == pos
    rest = np.setdiff1d(np.arange(n), given)
    assert np.array_equal(got["err"][:, rest], T.match_model(second[0], t, 3, S, True, one)[0]["err"][:, rest])
    # without a target the list reset launches fx_meter_zero alone
    assert b.meter_clear_target() == 0 and b.meter_reset_list(given) == 0 and b.sync() == 0
    assert (lib.fxstub_meter_zeros(), lib.fxstub_match_zeros()) == (zeros[0] + 2, zeros[1] + 1)
    pinned.free()
    b.close()
    clean(lib)
    print("target streams ok")


def child_queries():
    A, lib = stub_library()
    rng = np.random.default_rng(79)
    for ch, N in ((1, 200), (2, 257)):
        p = Pair(A, lib, N, ch)
        p.target(T.words(rng, (33, ch, -(-N // 3))), 3, False)
        x = T.words(rng, (33, ch, N))
        # equal settings: ties inside a group
        x[:, :, 9:12] = x[:, :, 9:10]
        x[:, :, 64:70] = x[:, :, 64:65]
        for h in (p.b, p.twin):
            h.process_block(x)
        p.took("one block", x)
        rows = p.b.meter_read_match()
        assert (T.V(rows, 1) < 0).any() and (T.V(rows, 1) > 0).any(), "cross values of both signs"
        before = (p.b.info("meter_match_selects"), lib.fxstub_match_selects())
        assert T.check_selects(lib, p.b, rows, N) >= 6
        assert p.b.info("meter_match_selects") - before[0] == lib.fxstub_match_selects() - before[1] > 50 and p.b.info("meter_selects") == 0
        got, m = p.b.meter_select_match(A.MATCH_ERROR, np.inf, below=True)
        assert m == N and np.array_equal(got, np.arange(N))
        assert lib.fxb_meter_select_match(p.b._h, 1, C.c_double(0.0), 0, N, None, 0, 0) == T.select(rows, 1, 0.0, False).size, "a count query"
        bests = (p.b.info("meter_match_bests"), lib.fxstub_match_bests())
        for group in (1, 3, 64, 65, N, N + 1, 1 << 62):
            for stat in (0, 1):
                for largest in (False, True):
                    got = p.b.meter_best(stat, group, largest)
                    assert T.same_best(got, T.best(rows, stat, group, largest)), (N, group, stat, largest, got[0][:8])
        assert p.b.info("meter_match_bests") - bests[0] == 28 == lib.fxstub_match_bests() - bests[1]
        w, v = p.b.meter_best(0, 3)
        assert w[3] == 9 and w[64 // 3] <= 64 and T.V(rows, 0)[9] == T.V(rows, 0)[11], "the smallest number of equal ones"
        assert T.same_match(p.b.meter_read_match(), rows), "the queries change nothing"
        p.close()
    clean(lib)
    print("target queries ok")


def child_shards():
    """three shards starting at 320 and 576: group = 3 (320 = 3 * 106 + 2) and group = 65 straddle both borders, group = 64 does not"""
    os.environ["FX_BUILDER"] = "0"
    A, lib = stub_library()
    rng = np.random.default_rng(83)
    N, S, ch = 3 * 256 + 40, 33, 2
    for group, tlen, loop in ((3, 40, True), (64, 20, False), (65, 33, False), (5000, 5, True)):
        p = Pair(A, lib, N, ch, devices=[0, 1, 2])
        assert [(d, f) for d, f, _ in p.b.shards()] == [(0, 0), (1, 320), (2, 576)], p.b.shards()
        p.target(T.words(rng, (tlen, ch, -(-N // min(group, N)))), group, loop)
        x = T.words(rng, (S, ch, N))
        x[:, :, 318:323] = x[:, :, 318:319]   # equal settings across the first border
        for h in (p.b, p.twin):
            h.process_block(x[:16])
        p.took("pageable, 16 samples", x[:16])
        for h in (p.b, p.twin):
            h.process_block(x[16:])
        p.took("pageable, 17 more", x[16:])
        xg = T.words(rng, (S, ch, p.b.bus_groups(64)))
        for h in (p.b, p.twin):
            h.process_block_bus(xg, 64)
        p.took("bus 64", expand(xg, 64, N))
        rows = p.b.meter_read_match()
        T.check_selects(lib, p.b, rows, N, "three shards")
        for first, n_range in ((300, 300), (319, 2), (319, 258), (575, 2), (600, 50)):
            for stat, t in ((0, float(np.median(T.V(rows, 0)))), (1, 0.0)):
                want = T.check_one(lib, p.b, rows, stat, t, False, first, n_range, n_range)
                for cap in {0, 1, want.size // 2, max(want.size - 1, 0), want.size + 3}:
                    T.check_one(lib, p.b, rows, stat, t, True, first, n_range, cap)
        for g in (1, 3, 64, 65, 320, 321, N, 1 << 40):
            for stat in (0, 1):
                for largest in (False, True):
                    assert T.same_best(p.b.meter_best(stat, g, largest), T.best(rows, stat, g, largest)), (group, g, stat, largest)
        w, _ = p.b.meter_best(0, 5)
        assert w[318 // 5 + 1] == 320 or T.V(rows, 0)[320:325].argmin() != 0
        w, _ = p.b.meter_best(0, 321)
        assert T.V(rows, 0)[w[0]] == T.V(rows, 0)[:321].min() and (w[0] != 320 or T.V(rows, 0)[318] != T.V(rows, 0)[320]), "a tie across the border stays with the smaller number"
        # list reset, read with reset, seek on every shard
        L = np.array([0, 319, 320, 575, 576, N - 1], dtype=np.int64)
        for h in (p.b, p.twin):
            assert h.meter_reset_list(L) == 0
        p.acc = T.zeroed(p.acc, L)
        p.took("a list reset", np.zeros((0, ch, N), dtype=np.float32), launches=0)
        assert p.b.meter_target_seek(2) == 0
        p.pos = 2
        for h in (p.b, p.twin):
            h.process_block(x)
        p.took("after a seek", x)
        p.close()
    # an allocation that fails on whichever shard (two per shard): FX_E_MEMORY, no target on any shard, then the same call works
    t = T.words(rng, (20, ch, -(-N // 3)))
    x = T.words(rng, (S, ch, N))
    for nth in range(6):
        c = A.Batch(N, ch, devices=[0, 1, 2])
        assert c.load_text(STEREO) and c.meter_enable() == 0
        c.process_block(x)   # (the block's own buffers exist before allocations are counted)
        live = lib.fxstub_live_allocations()
        lib.fxstub_fail_mallocs(nth, 1)
        rc = lib.fxb_meter_set_target(c._h, ptr(t), 20, 3, 0)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.last_error() and lib.fxstub_live_allocations() == live, nth
        assert lib.fxb_meter_target_pos(c._h) == FX_E_ARG and lib.fxb_meter_read_match(c._h, None, None, 0) == FX_E_ARG
        c.process_block(x)
        assert c.info("meter_target_launches") == 0 and c.info("meter_launches") == 6, "no shard meters against a target"
        assert c.meter_set_target(t, 3) == 0 and lib.fxstub_live_allocations() == live + 6
        c.process_block(x)
        assert T.same_match(c.meter_read_match(), T.match_model(x, t, 3, 0, False)[0]) and c.info("meter_target_launches") == 3
        assert c.load_text(MORE) and lib.fxstub_live_allocations() <= live and lib.fxb_meter_target_pos(c._h) == FX_E_ARG
        c.close()
    clean(lib)
    print("target shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "pieces": child_pieces, "refusals": child_refusals, "streams": child_streams, "queries": child_queries, "shards": child_shards}[sys.argv[1]]()
