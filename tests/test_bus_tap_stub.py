"""Bus taps without a GPU: the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc
stublib`), driven through the C ABI in a child process like tests/test_bus_stub.py (this file is also that child).  The stand-in of
the tap kernel (tests/hipstub/fx_bus_tap_stub.cpp) gathers in stream order with an addressing of its own, so what is checked here
is the host side: which rows and columns a block's taps go to on every route (pinned in place, pageable through the staging, the
device entry, the pieces of a block above the scratch limit, three shards on the columns of their entries), the state machine of
fxb_bus_set_taps, that a tapped block leaves everything else as an untapped one does, and that a refusal changes nothing.

The yardstick is an existing path: a second handle runs fxb_process_block on the expanded input and gives y; the taps must be
y[:, :, list] as 32-bit patterns - NaN payloads included - and the mix what mix_model / gain_mix_model of y give.  Parity on the
device is tests/test_gpu_bus_tap.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MIX_OUT, PROGRAM, ROOT, SHARED_IN, STEREO, Pinned, bus, expand, mix_model, same_words, stub_library  # noqa: E402
from test_bus_gain_stub import SHAPES, gain_mix_model, gains_for  # noqa: E402

TAPS = (1, 3, 64, 65, 130)   # the wavefront boundary of the column ownership and its ragged tail
MOST_TAPS = 65536


def tap_list(rng, N, T):
    """T instance numbers: the last instance, the first, the last again (a repeat), then random ones - unsorted from the start -
    as far as T reaches (T = 1 holds the last instance only)"""
    lst = [N - 1, 0, N - 1] + [int(v) for v in rng.integers(0, N, max(T - 3, 0))]
    if T > 4:
        lst[3], lst[4] = max(lst[3], lst[4]), min(lst[3], lst[4])   # (a descending pair whatever was drawn)
    return np.array(lst[:T], dtype=np.int64)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all()


def signal(rng, shape):
    """finite words of every magnitude, and NaNs with payloads, infinities and a negative zero: a tap moves patterns"""
    y = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 6, shape)).astype(np.float32)
    flat = y.reshape(-1).view(np.uint32)
    for k, word in enumerate((0x80000000, 0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x7f812345, 0x00000001)):
        flat[(k * 7) % flat.size] = word
    return y


def test_tap_lists_are_what_they_say():
    rng = np.random.default_rng(1)
    for N, _ in SHAPES:
        for T in TAPS:
            lst = tap_list(rng, N, T)
            assert lst.size == T and lst.min() >= 0 and lst.max() < N and lst[0] == N - 1
            if T >= 3:
                assert lst[1] == 0 and lst[2] == N - 1 and (N == 1 or (np.diff(lst) < 0).any())


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_tap_values_and_routes_on_the_hip_stand_in():
    run_child("routes", "tap routes ok")


def test_tap_rows_of_the_pieces_of_a_block_on_the_hip_stand_in():
    run_child("pieces", "tap pieces ok")


def test_tap_state_machine_on_the_hip_stand_in():
    """set, replace, off, set before a load, the list round trip"""
    run_child("state", "tap state ok")


def test_tapping_leaves_meters_gains_and_state_alone_on_the_hip_stand_in():
    run_child("unaffected", "tap unaffected ok")


def test_tap_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "tap refusals ok")


def test_taps_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "tap shards ok", devices=3)


def test_tap_set_that_runs_out_of_memory_on_one_shard_on_the_hip_stand_in():
    run_child("memory", "tap memory ok", devices=3)


def test_tap_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/bus_tap_checks.cpp (csrc/Makefile `stubasantaps`): the list shapes, the refusals and an allocation failure at
    every allocation of a set and of a staged block, through the C ABI on exactly-sized heap blocks, on one handle and on three
    shards, under AddressSanitizer + UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded
    and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasantaps"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "bus_tap_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "bus tap checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def tap_library():
    A, lib = stub_library()
    for f in ("fxstub_bus_taps", "fxstub_bus_tap_strays", "fxstub_bus_gain_mixes", "fxstub_live_allocations"):
        getattr(lib, f).restype = C.c_long
    return A, lib


class TapCounts:
    """what has happened since the last look: (emulation launches, expands, mixes plain and weighted, tap launches, staged, in
    place, bus blocks, bus blocks with taps)"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_bus_expands(), self.lib.fxstub_bus_mixes() + self.lib.fxstub_bus_gain_mixes(), self.lib.fxstub_bus_taps(),
                self.b.info("host_staged_blocks"), self.b.info("host_inplace_blocks"), self.b.info("bus_blocks"), self.b.info("bus_tap_blocks"))

    def expect(self, what, *want):
        now = self.now()
        got = tuple(x - y for x, y in zip(now, self.seen))
        assert got == want, (what, got, want)
        self.seen = now

    def skip(self):
        """(what another handle has launched meanwhile is not this one's)"""
        self.seen = self.now()


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def tapped(lib, b, x, y, t, S, K, flags):
    return lib.fxb_process_block_bus_tap(b._h, ptr(x), ptr(y), ptr(t), S, K, flags)


def tapped_dev(lib, b, x, y, t, S, K, flags, stream=None):
    return lib.fxb_process_block_bus_tap_dev(b._h, ptr(x), ptr(y), ptr(t), S, K, flags, stream)


def set_taps(lib, b, lst):
    lst = np.ascontiguousarray(lst, dtype=np.int64)
    return lib.fxb_bus_set_taps(b._h, ptr(lst) if lst.size else None, lst.size)


def child_routes():
    A, lib = tap_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(51)
    S = 9   # (rows of 9 and 18: a whole chunk of eight rows of the kernel and a ragged one)
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N, K in SHAPES:
            b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
            assert b.load_text(text) and plain.load_text(text), b.errors()
            G = b.bus_groups(K)
            count = TapCounts(lib, b)
            for T in TAPS:
                lst = tap_list(rng, N, T)
                given = lst.copy()
                assert set_taps(lib, b, given) == 0, b.last_error()
                given[...] = -1   # the caller's list is free on return
                assert (b.bus_get_taps() == lst).all()
                for shared in (True, False):
                    flags = MIX_OUT | (SHARED_IN if shared else 0)
                    x = signal(rng, (S, ch, G if shared else N))
                    y = plain.process_block(expand(x, K, N) if shared else x)
                    count.skip()
                    want_mix, want_taps = mix_model(y, K), y[:, :, lst]
                    # pageable: the mix and the tap rows are staged
                    out, taps = b.process_block_bus(x, K, shared, True, taps=True)
                    assert same_words(out, want_mix) and same_bits(taps, want_taps), (ch, N, K, T, shared, "staged")
                    count.expect("staged", 1, int(shared), 1, 1, 1, 0, 1, 1)
                    # pinned: everything in place
                    px, po, pt = pinned(x.shape), pinned((S, ch, G)), pinned((S, ch, T))
                    px[...] = x
                    pt[...] = -7.0
                    assert tapped(lib, b, px, po, pt, S, K, flags) == 0, b.last_error()
                    assert same_words(po, want_mix) and same_bits(pt, want_taps), (ch, N, K, T, shared, "in place")
                    count.expect("in place", 1, int(shared), 1, 1, 0, 1, 1, 1)
                    # pinned PCM, pageable tap rows: the two sides keep their route, the taps are staged
                    page = np.full((S, ch, T), -7.0, dtype=np.float32)
                    assert tapped(lib, b, px, po, page, S, K, flags) == 0, b.last_error()
                    assert same_words(po, want_mix) and same_bits(page, want_taps), (ch, N, K, T, shared, "pinned PCM, pageable taps")
                    count.expect("pinned PCM, pageable taps", 1, int(shared), 1, 1, 0, 1, 1, 1)
                    # pageable PCM, pinned tap rows
                    pt[...] = -7.0
                    out = np.zeros((S, ch, G), dtype=np.float32)
                    assert tapped(lib, b, x, out, pt, S, K, flags) == 0, b.last_error()
                    assert same_words(out, want_mix) and same_bits(pt, want_taps), (ch, N, K, T, shared, "pageable PCM, pinned taps")
                    count.expect("pageable PCM, pinned taps", 1, int(shared), 1, 1, 1, 0, 1, 1)
                    # the device entry on the handle's own stream, twice (the second time: buffers that have passed once)
                    for rep in range(2):
                        pt[...] = -7.0
                        assert tapped_dev(lib, b, px, po, pt, S, K, flags) == 0 and b.sync() == 0, b.last_error()
                        assert same_words(po, want_mix) and same_bits(pt, want_taps), (ch, N, K, T, shared, "device entry")
                    count.expect("device entry", 2, 2 * int(shared), 2, 2, 0, 0, 2, 2)
                    # tap_out == NULL is fxb_process_block_bus
                    assert tapped(lib, b, px, po, None, S, K, flags) == 0 and same_words(po, want_mix)
                    count.expect("no tap rows", 1, int(shared), 1, 0, 0, 1, 1, 0)
                    assert tapped(lib, b, px, po, pt, 0, K, flags) == 0
                    count.expect("zero samples", 0, 0, 0, 0, 0, 0, 0, 0)
                    pinned.free()
            b.close()
            plain.close()
    assert lib.fxstub_bus_tap_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("tap routes ok")


def child_pieces():
    A, lib = tap_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(53)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples
    N, S, K, T = 262144, 96, 64, 65
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    lst = tap_list(rng, N, T)
    assert set_taps(lib, b, lst) == 0
    count = TapCounts(lib, b)
    xg = rng.standard_normal((S, 1, G)).astype(np.float32)
    y = expand(xg, K, N)   # (the stand-in's emulation launch copies in to out; tests/test_gpu_bus_tap.py runs the plain path)
    want_mix, want_taps = mix_model(y, K), y[:, :, lst]
    out, taps = b.process_block_bus(xg, K, taps=True)
    assert same_words(out, want_mix) and same_bits(taps, want_taps)
    count.expect("two pieces, staged", 2, 2, 2, 2, 1, 0, 1, 1)
    pg, po, pt = pinned((S, 1, G)), pinned((S, 1, G)), pinned((S, 1, T))
    pg[...] = xg
    assert tapped(lib, b, pg, po, pt, S, K, 3) == 0 and same_words(po, want_mix) and same_bits(pt, want_taps)
    count.expect("two pieces, in place", 2, 2, 2, 2, 0, 1, 1, 1)
    pt[...] = -7.0
    assert tapped(lib, b, pg, po, pt, 65, K, 3) == 0 and same_bits(pt[:65], want_taps[:65]) and (pt[65:] == -7.0).all()
    count.expect("65 samples: two pieces", 2, 2, 2, 2, 0, 1, 1, 1)
    assert b.set_register_track("vol", [0.1, 0.2], 48) == 0
    pt[...] = -7.0
    assert tapped(lib, b, pg, po, pt, S, K, 3) == 0 and same_words(po, want_mix) and same_bits(pt, want_taps), b.last_error()
    count.expect("armed: one piece", 1, 1, 1, 1, 0, 1, 1, 1)
    assert lib.fxstub_bus_tap_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("tap pieces ok")


def child_state():
    A, lib = tap_library()
    rng = np.random.default_rng(57)
    N, K, S = 777, 130, 5
    b, plain = A.Batch(N, 2, 0), A.Batch(N, 2, 0)
    live = lib.fxstub_live_allocations()
    assert lib.fxb_bus_get_taps(b._h, None, 0) == 0 and b.bus_get_taps().size == 0, "off by default"
    first = tap_list(rng, N, 65)
    assert set_taps(lib, b, first) == 0, "before a program is loaded"
    assert lib.fxstub_live_allocations() == live + 1, "the list is the only allocation of a set"
    assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()
    assert (b.bus_get_taps() == first).all(), "the taps survive a program load"
    G = b.bus_groups(K)

    def block(lst):
        x = signal(rng, (S, 2, G))
        y = plain.process_block(expand(x, K, N))
        out, taps = b.process_block_bus(x, K, taps=True)
        assert same_words(out, mix_model(y, K)) and same_bits(taps, y[:, :, lst])

    block(first)
    # the round trip with less room than entries, and with more
    some = np.full(10, -1, dtype=np.int64)
    assert lib.fxb_bus_get_taps(b._h, ptr(some), 7) == 65 and (some[:7] == first[:7]).all() and (some[7:] == -1).all()
    room = np.full(70, -1, dtype=np.int64)
    assert lib.fxb_bus_get_taps(b._h, ptr(room), 70) == 65 and (room[:65] == first).all() and (room[65:] == -1).all()
    second = tap_list(rng, N, 3)
    assert set_taps(lib, b, second) == 0 and (b.bus_get_taps() == second).all(), "replaced"
    block(second)
    third = tap_list(rng, N, 130)
    assert b.bus_set_taps(third) == 0 and (b.bus_get_taps() == third).all()
    block(third)
    # off: any list with count 0; the memory goes; tapped blocks are refused, untapped ones go on
    held = lib.fxstub_live_allocations()
    assert lib.fxb_bus_set_taps(b._h, ptr(third), 0) == 0 and b.bus_get_taps().size == 0
    assert lib.fxstub_live_allocations() == held - 2 and b.info("bus_tap_blocks") == 3, "the device list and the staging of pageable rows are freed"
    x = signal(rng, (S, 2, G))
    t = np.zeros((S, 2, 3), dtype=np.float32)
    assert tapped(lib, b, x, np.zeros_like(x), t, S, K, 3) == FX_E_ARG and "taps are off" in b.last_error()
    assert same_words(b.process_block_bus(x, K), mix_model(plain.process_block(expand(x, K, N)), K))
    assert set_taps(lib, b, []) == 0 and b.bus_set_taps(None) == 0, "off twice"
    assert set_taps(lib, b, first) == 0
    block(first)
    # the largest set there is
    most = rng.integers(0, N, MOST_TAPS).astype(np.int64)
    assert set_taps(lib, b, most) == 0 and (b.bus_get_taps() == most).all()
    x = signal(rng, (1, 2, G))
    out, taps = b.process_block_bus(x, K, taps=True)
    assert same_bits(taps, plain.process_block(expand(x, K, N))[:, :, most])
    b.close()
    plain.close()
    assert lib.fxstub_live_allocations() < live, "nothing of the taps outlives the handle"
    assert lib.fxstub_bus_tap_strays() == 0
    print("tap state ok")


def child_unaffected():
    """a tapped and an untapped handle through the same calls: the mix, the meters, the gains with a ramp left pending by a block
    without FXB_BUS_MIX_OUT, the state image and every counter there was before agree"""
    A, lib = tap_library()
    rng = np.random.default_rng(59)
    N, K, ch = 200, 63, 2
    a, b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0), A.Batch(N, ch, 0)
    assert plain.load_text(STEREO), plain.errors()
    G = a.bus_groups(K)
    lst = tap_list(rng, N, 65)
    assert set_taps(lib, b, lst) == 0
    for h in (a, b):
        assert h.load_text(STEREO), h.errors()
        assert h.meter_enable(True) == 0
    g0, g1, g2 = gains_for(rng, ch, N), gains_for(rng, ch, N), gains_for(rng, ch, N)
    g1[:, 70] = 0.0   # a muted voice, tapped below: pre-fader
    lst[5] = 70
    assert set_taps(lib, b, lst) == 0
    gains = g0
    for step, (S, ramp, g) in enumerate(((33, 0, g0), (1, 1, g1), (33, 1, g2), (7, None, None))):
        if g is not None:
            assert a.bus_set_gains(g, bool(ramp)) == 0 and b.bus_set_gains(g, bool(ramp)) == 0
        x = signal(rng, (S, ch, G))
        y = plain.process_block(expand(x, K, N))
        want = gain_mix_model(y, gains, g if g is not None else gains, bool(ramp), S, K)
        gains = g if g is not None else gains
        out_a = a.process_block_bus(x, K)
        out_b, taps = b.process_block_bus(x, K, taps=True)
        assert same_words(out_a, want) and same_words(out_b, out_a), step
        assert same_bits(taps, y[:, :, lst]), (step, "pre-fader: the muted voice and the NaNs are heard")
    # a ramp that a block without FXB_BUS_MIX_OUT leaves pending, and a refused tapped block behind it
    assert a.bus_set_gains(g0, True) == 0 and b.bus_set_gains(g0, True) == 0
    x = signal(rng, (4, ch, G))
    assert same_words(a.process_block_bus(x, K, True, False), b.process_block_bus(x, K, True, False))
    t = np.zeros((4, ch, lst.size), dtype=np.float32)
    assert tapped(lib, b, x, np.zeros((4, ch, N), dtype=np.float32), t, 4, K, SHARED_IN) == FX_E_ARG
    assert same_words(a.bus_get_gains(), b.bus_get_gains()) and same_words(a.bus_get_gains(), gains), "the ramp is still pending"
    out_a = a.process_block_bus(x, K)
    out_b, taps = b.process_block_bus(x, K, taps=True)
    assert same_words(out_a, gain_mix_model(expand(x, K, N), gains, g0, True, 4, K)) and same_words(out_b, out_a)
    ma, mb = a.meter_read(), b.meter_read()
    for key in ("energy", "peak", "full_scale", "nonfinite"):
        assert (ma[key].view(np.uint8) == mb[key].view(np.uint8)).all(), key
    assert mb["nonfinite"].sum() > 0 and a.meter_samples() == b.meter_samples()
    assert (a.save_state() == b.save_state()).all()
    # instance calls do not touch the taps
    assert b.copy_instances([0, 1], [70, 131]) == 0 and b.reset_instances([5]) == 0 and b.sync() == 0
    assert (b.bus_get_taps() == lst).all()
    for what in ("host_staged_blocks", "host_inplace_blocks", "bus_blocks", "meter_launches", "bus_gain_blocks", "imajor_blocks", "num_rows", "kernel", "grid", "xlate_code_hash"):
        assert a.info(what) == b.info(what), what
    assert a.info("bus_tap_blocks") == 0 and b.info("bus_tap_blocks") == 5
    print("tap unaffected ok")


def child_refusals():
    A, lib = tap_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(61)
    N, S, K, T = 300, 8, 64, 65
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    lst = tap_list(rng, N, T)
    xg, yg, xn, pt = pinned((S, 1, G)), pinned((S, 1, G)), pinned((S, 1, N)), pinned((S, 1, T))
    both = pinned((4 * S, 1, N))
    xg[...] = 0.5
    at = lambda a, off: C.c_void_p(a.ctypes.data + off * 4)
    page = np.zeros((S, 1, T), dtype=np.float32)

    def untouched():
        ok = (pt == -7.0).all() and (page == -7.0).all() and (both == -7.0).all()
        pt[...] = -7.0
        page[...] = -7.0
        both[...] = -7.0
        return ok

    untouched()
    # while taps are off
    count = TapCounts(lib, b)
    for what, call in (("host entry, taps off", lambda: tapped(lib, b, xg, yg, pt, S, K, 3)), ("device entry, taps off", lambda: tapped_dev(lib, b, xg, yg, pt, S, K, 3)),
                       ("zero samples, taps off", lambda: tapped(lib, b, xg, yg, pt, 0, K, 3))):
        assert call() == FX_E_ARG and "taps are off" in b.last_error(), what
        count.expect(what, 0, 0, 0, 0, 0, 0, 0, 0)
        assert untouched() and b.bus_get_taps().size == 0, what
    # sets that are refused: nothing changes, neither from "off" nor from a list in force
    live = lib.fxstub_live_allocations()
    bad_entry, negative = lst.copy(), lst.copy()
    bad_entry[T - 1], negative[0] = N, -1
    too_many = np.zeros(MOST_TAPS + 1, dtype=np.int64)
    for state in ("off", "on"):
        if state == "on":
            assert set_taps(lib, b, lst) == 0
            live = lib.fxstub_live_allocations()
        for what, call in (("count < 0", lambda: lib.fxb_bus_set_taps(b._h, ptr(lst), -1)), ("count above the cap", lambda: lib.fxb_bus_set_taps(b._h, ptr(too_many), too_many.size)),
                           ("null list", lambda: lib.fxb_bus_set_taps(b._h, None, 3)), ("entry == N", lambda: lib.fxb_bus_set_taps(b._h, ptr(bad_entry), T)),
                           ("entry < 0", lambda: lib.fxb_bus_set_taps(b._h, ptr(negative), T)), ("null handle", lambda: lib.fxb_bus_set_taps(None, ptr(lst), T))):
            assert call() == FX_E_ARG, (state, what)
            assert lib.fxstub_live_allocations() == live, (state, what)
            assert (b.bus_get_taps() == (lst if state == "on" else lst[:0])).all(), (state, what)
    assert lib.fxb_bus_get_taps(None, None, 0) == FX_E_ARG and lib.fxb_bus_get_taps(b._h, None, 4) == FX_E_ARG and lib.fxb_bus_get_taps(b._h, ptr(too_many), -1) == FX_E_ARG
    assert tapped(lib, b, xg, yg, pt, S, K, 3) == 0, b.last_error()
    ms = b.last_kernel_ms()
    want_taps = expand(xg, K, N)[:, :, lst]
    assert same_bits(pt, want_taps)
    untouched()
    count = TapCounts(lib, b)
    rows = S * T   # words of the tap rows
    refused = [
        ("no FXB_BUS_MIX_OUT", lambda: tapped(lib, b, xg, xn, pt, S, K, SHARED_IN)), ("no flags", lambda: tapped(lib, b, xn, xn, pt, S, K, 0)),
        ("no FXB_BUS_MIX_OUT, device entry", lambda: tapped_dev(lib, b, xg, xn, pt, S, K, SHARED_IN)),
        ("no FXB_BUS_MIX_OUT, zero samples", lambda: tapped(lib, b, xg, xn, pt, 0, K, SHARED_IN)),
        # tap rows that share a byte with the input or the output
        ("tap rows == in", lambda: lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, 0), S, K, MIX_OUT)),
        ("tap rows == out", lambda: lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, 2 * S * N), S, K, MIX_OUT)),
        ("last tap word on the first of in", lambda: lib.fxb_process_block_bus_tap(b._h, at(both, rows - 1), at(both, 2 * S * N), at(both, 0), S, K, MIX_OUT)),
        ("first tap word on the last of in", lambda: lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, S * N - 1), S, K, MIX_OUT)),
        ("first tap word on the last of out", lambda: lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, 2 * S * N + S * G - 1), S, K, MIX_OUT)),
        ("tap rows over the output, device entry", lambda: lib.fxb_process_block_bus_tap_dev(b._h, at(both, 0), at(both, 2 * S * N), at(both, 2 * S * N - rows + 1), S, K, MIX_OUT, None)),
        # every refusal the untapped entries have
        ("group 0", lambda: tapped(lib, b, xg, yg, pt, S, 0, 3)), ("unknown flag", lambda: tapped(lib, b, xg, yg, pt, S, K, 7)),
        ("null in", lambda: tapped(lib, b, None, yg, pt, S, K, 3)), ("null out", lambda: tapped(lib, b, xg, None, pt, S, K, 3)),
        ("negative length", lambda: tapped(lib, b, xg, yg, pt, -1, K, 3)),
        ("in and out overlap", lambda: lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 3), ptr(pt), S, K, 3)),
        ("device entry, group 0", lambda: tapped_dev(lib, b, xg, yg, pt, S, 0, 3)), ("device entry, null", lambda: tapped_dev(lib, b, None, yg, pt, S, K, 3)),
        ("device entry, pageable in", lambda: tapped_dev(lib, b, np.zeros((S, 1, G), dtype=np.float32), yg, pt, S, K, 3)),
        # tap rows the device cannot address over the whole block
        ("device entry, pageable tap rows", lambda: tapped_dev(lib, b, xg, yg, page, S, K, 3)),
        ("device entry, tap rows beyond their allocation", lambda: lib.fxb_process_block_bus_tap_dev(b._h, ptr(xg), ptr(yg), at(pt, 1), S, K, 3, None)),
        ("null handle", lambda: lib.fxb_process_block_bus_tap(None, ptr(xg), ptr(yg), ptr(pt), S, K, 3)),
    ]
    for what, call in refused:
        assert call() == FX_E_ARG, (what, b.last_error())
        count.expect(what, 0, 0, 0, 0, 0, 0, 0, 0)
        assert untouched(), what
        assert (b.bus_get_taps() == lst).all() and b.last_kernel_ms() == ms, what
    # ... and blocks that touch without overlapping are not among them; the next tapped block is right
    assert lib.fxb_process_block_bus_tap(b._h, at(both, rows), at(both, 2 * S * N), at(both, 0), S, K, MIX_OUT) == 0, b.last_error()
    assert lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, S * N), S, K, MIX_OUT) == 0, b.last_error()
    assert tapped_dev(lib, b, xg, yg, pt, S, K, 3) == 0 and b.sync() == 0 and same_bits(pt, want_taps), b.last_error()
    # a staged tap block that cannot be had: FX_E_MEMORY, nothing launched, the handle goes on
    count = TapCounts(lib, b)
    page[...] = -7.0
    lib.fxstub_fail_mallocs(0, 1)
    rc = tapped(lib, b, xg, yg, page, S, K, 3)
    lib.fxstub_fail_mallocs(-1, 0)
    assert rc == FX_E_MEMORY and (page == -7.0).all(), b.last_error()
    count.expect("staging refused", 0, 0, 0, 0, 0, 0, 0, 0)
    assert tapped(lib, b, xg, yg, page, S, K, 3) == 0 and same_bits(page, want_taps), b.last_error()
    # a handle of several shards has no device entry (here: one device, three shards)
    three = A.Batch(N, 1, devices=[0, 0, 0])
    assert three.load_text(PROGRAM) and set_taps(lib, three, lst) == 0
    k0 = lib.fxstub_kernels_run()
    assert tapped_dev(lib, three, xg, yg, pt, S, K, 3) == FX_E_ARG and lib.fxstub_kernels_run() == k0
    assert lib.fxstub_bus_tap_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("tap refusals ok")


def child_shards():
    A, lib = tap_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(67)
    N, S = 3 * 256 + 40, 9
    b, plain = A.Batch(N, 2, devices=[0, 1, 2]), A.Batch(N, 2, 0)
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()
    lists = {
        "every shard": (np.concatenate([tap_list(rng, N, 65), [319, 320, 575, 576]]), 3),
        "the middle shard skipped": (np.array([807, 0, 576, 319, 0, 700, 5, 4], dtype=np.int64), 2),
        "the first shard only, one entry": (np.array([319], dtype=np.int64), 1),
        "repeats across shards": (np.array([320, 0, 320, 576, 0, 576, 320, 807, 807, 1] * 13, dtype=np.int64), 3),
    }
    count = TapCounts(lib, b)
    for what, (lst, owners) in lists.items():
        T = lst.size
        assert set_taps(lib, b, lst) == 0 and (b.bus_get_taps() == lst).all(), (what, b.last_error())
        for K in (64, 32):
            G = b.bus_groups(K)
            x = signal(rng, (S, 2, G))
            y = plain.process_block(expand(x, K, N))
            count.skip()
            want_mix, want_taps = mix_model(y, K), y[:, :, lst]
            px, po, pt = pinned((S, 2, G)), pinned((S, 2, G)), pinned((S, 2, T))
            px[...] = x
            pt[...] = -7.0
            assert tapped(lib, b, px, po, pt, S, K, 3) == 0, (what, b.last_error())
            assert same_words(po, want_mix) and same_bits(pt, want_taps), (what, K, "in place")
            # (a shard launches the tap kernel only for entries of its own, and writes only their columns)
            count.expect(what + ", in place", 3, 3, 3, owners, 0, 3, 3, 3)
            out, taps = b.process_block_bus(x, K, taps=True)
            assert same_words(out, want_mix) and same_bits(taps, want_taps), (what, K, "staged")
            count.expect(what + ", staged", 3, 3, 3, owners, 3, 0, 3, 3)
            page = np.full((S, 2, T), -7.0, dtype=np.float32)
            assert tapped(lib, b, px, po, page, S, K, 3) == 0 and same_bits(page, want_taps), (what, K, "pinned PCM, pageable taps")
            count.expect(what + ", pinned PCM, pageable taps", 3, 3, 3, owners, 0, 3, 3, 3)
            pinned.free()
    lst = lists["the middle shard skipped"][0]
    assert set_taps(lib, b, lst) == 0
    # refusals that go by the whole batch launch nothing on any shard
    count = TapCounts(lib, b)
    px, po, pt = pinned((S, 2, N)), pinned((S, 2, N)), pinned((S, 2, lst.size))
    assert tapped(lib, b, px, po, pt, S, 100, 3) == FX_E_ARG and "straddles" in b.last_error()
    assert tapped(lib, b, px, po, pt, S, 64, SHARED_IN) == FX_E_ARG and tapped_dev(lib, b, px, po, pt, S, 64, 3) == FX_E_ARG
    assert lib.fxb_process_block_bus_tap(b._h, ptr(px), ptr(po), ptr(px), S, 64, MIX_OUT) == FX_E_ARG
    count.expect("refused", 0, 0, 0, 0, 0, 0, 0, 0)
    assert set_taps(lib, b, []) == 0 and b.bus_get_taps().size == 0
    assert tapped(lib, b, px, po, pt, S, 64, 3) == FX_E_ARG
    count.expect("refused, taps off", 0, 0, 0, 0, 0, 0, 0, 0)
    assert lib.fxstub_bus_tap_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("tap shards ok")


def child_memory():
    """an allocation that fails inside a set, on whichever shard it happens: FX_E_MEMORY, the old taps stay in force on all of
    them, nothing leaks"""
    A, lib = tap_library()
    rng = np.random.default_rng(71)
    N, S, K = 3 * 256 + 40, 5, 64
    b = A.Batch(N, 1, devices=[0, 1, 2])
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    x = signal(rng, (S, 1, G))
    b.process_block_bus(x, K)   # (code generated, scratch and staging allocated)
    assert b.prepare(S, True) == 0   # (... and the builder thread is idle: nothing else allocates while allocations are counted)
    old = np.array([807, 0, 400, 0], dtype=np.int64)
    new = tap_list(rng, N, 130)
    new[7] = 400   # (an entry of the middle shard, whatever was drawn)
    for state in ("off", "on"):
        if state == "on":
            assert set_taps(lib, b, old) == 0
        for nth in range(3):   # one allocation per shard
            live = lib.fxstub_live_allocations()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = set_taps(lib, b, new)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY, (state, nth, rc, b.last_error())
            assert lib.fxstub_live_allocations() == live, (state, nth)
            assert (b.bus_get_taps() == (old if state == "on" else old[:0])).all(), (state, nth)
            if state == "on":
                out, taps = b.process_block_bus(x, K, taps=True)
                assert same_bits(taps, expand(x, K, N)[:, :, old]), (state, nth)
    assert set_taps(lib, b, new) == 0 and (b.bus_get_taps() == new).all()
    out, taps = b.process_block_bus(x, K, taps=True)
    assert same_bits(taps, expand(x, K, N)[:, :, new]) and same_words(out, mix_model(expand(x, K, N), K))
    assert lib.fxstub_bus_tap_strays() == 0 and lib.fxstub_cross_device_errors() == 0
    print("tap memory ok")


if __name__ == "__main__":
    {"routes": child_routes, "pieces": child_pieces, "state": child_state, "unaffected": child_unaffected, "refusals": child_refusals, "shards": child_shards,
     "memory": child_memory}[sys.argv[1]]()
