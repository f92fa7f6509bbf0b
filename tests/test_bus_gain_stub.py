"""Bus gains without a GPU: the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc
stublib`), driven through the C ABI in a child process like tests/test_bus_stub.py (this file is also that child).  The stand-in's
emulation kernel copies in to out and the stand-in of the weighted mix (tests/hipstub/fx_bus_gain_stub.cpp) does the real
arithmetic in stream order, so out == gain_mix_model(expand(in), a, b, ramp, S, K) must hold word for word on every route: that
checks the gain state of the handle - current and target, the pending ramp, who consumes it - its ordering against queued blocks,
the pieces of a block above the scratch limit (one S for all of them), the columns of three shards, and the stand-in against the
numpy model below, which is itself checked against the definition of include/fx8010_amd.h written out one operation at a time.
NaN matches NaN; there is no tolerance anywhere.  Parity of the real kernel is tests/test_gpu_bus_gain.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MIX_OUT, PROGRAM, ROOT, SHARED_IN, STEREO, Pinned, bus, expand, mix_model, same_words, stub_library  # noqa: E402
from route_models import DENORMAL, TINY, HUGE, gain_weights, gain_mix_model, gains_for  # noqa: E402,F401  (the models live there; the tests of them stay here)

SHAPES = ((1, 1), (5, 2), (65, 64), (200, 63), (200, 65), (777, 130), (300, 1000))   # (N, K)


def signal(rng, shape):
    y = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 6, shape)).astype(np.float32)
    y.flat[0] = -0.0
    return y


def test_gain_mix_model_is_the_definition_it_says():
    """the vectorised model against the definition written out one operation at a time"""
    rng = np.random.default_rng(5)
    f = np.float32
    for N, K in SHAPES:
        for C_ in (1, 2):
            for S in (1, 2, 33):
                a, b = gains_for(rng, C_, N), gains_for(rng, C_, N)
                b[0, N // 2] = a[0, N // 2]                    # a member that does not move
                y = signal(rng, (S, C_, N))
                y[S // 2, 0, (N - 1) // 2] = np.nan
                y[S - 1, C_ - 1, N - 1] = np.inf
                k = min(K, N)
                G = -(-N // k)
                for ramp in (False, True):
                    want = np.zeros((S, C_, G), dtype=np.float32)
                    r = f(f(1.0) / f(S))
                    with np.errstate(all="ignore"):
                        for s in range(S):
                            for c in range(C_):
                                for g in range(G):
                                    p = [f(0.0)] * 64
                                    for m, n in enumerate(range(g * k, min((g + 1) * k, N))):
                                        if not ramp or s == S - 1:
                                            w = b[c, n]
                                        else:
                                            t = f(f(s + 1) * r)
                                            d = f(b[c, n] - a[c, n])
                                            w = f(a[c, n] + f(d * t))
                                        term = f(0.0) if w == 0.0 else f(w * y[s, c, n])
                                        p[m % 64] = f(p[m % 64] + term)
                                    for step in (32, 16, 8, 4, 2, 1):
                                        for l in range(step):
                                            p[l] = f(p[l] + p[l + step])
                                    want[s, c, g] = p[0]
                    assert same_words(gain_mix_model(y, a, b, ramp, S, K), want), (N, K, C_, S, ramp)
    # the consequences the header states
    y = signal(rng, (33, 2, 200))
    y[3, 1, 7] = np.nan
    ones = np.ones((2, 200), dtype=np.float32)
    for ramp in (False, True):
        assert same_words(gain_mix_model(y, ones, ones, ramp, 33, 64), mix_model(y, 64)), "gains of 1.0f: the unweighted sum"
    a, b = gains_for(rng, 2, 200), gains_for(rng, 2, 200)
    assert same_words(gain_mix_model(y, a, b, True, 33, 64)[32], gain_mix_model(y, a, b, False, 33, 64)[32]), "the last sample carries exactly b"
    muted = ones.copy()
    muted[1, 7] = -0.0
    got = gain_mix_model(y, muted, muted, False, 33, 64)
    assert np.isfinite(got).all() and np.isnan(mix_model(y, 64)).any(), "a muted member contributes +0.0f whatever it holds"
    parts = np.concatenate([gain_mix_model(y[:16], a, b, True, 16, 64), gain_mix_model(y[16:], b, b, False, 17, 64)])
    assert not same_words(parts, gain_mix_model(y, a, b, True, 33, 64)), "a ramp is per call"


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_gain_values_and_routes_on_the_hip_stand_in():
    run_child("routes", "gain routes ok")


def test_gain_state_machine_on_the_hip_stand_in():
    """gains of 1.0f and NULL, a replaced target, ramp = 0 cancelling a ramp, a block without FXB_BUS_MIX_OUT, get before and after"""
    run_child("state", "gain state ok")


def test_gain_ramp_across_the_pieces_of_a_block_on_the_hip_stand_in():
    run_child("pieces", "gain pieces ok")


def test_gains_set_behind_a_block_on_another_stream_on_the_hip_stand_in():
    run_child("streams", "gain streams ok")


def test_gain_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "gain refusals ok")


def test_gains_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "gain shards ok", devices=3)


def test_gain_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/bus_gain_checks.cpp (csrc/Makefile `stubasangains`): the indexing shapes, the refusals and the allocation
    failures through the C ABI on exactly-sized heap blocks, on one handle and on three shards, under AddressSanitizer + UBSan +
    LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasangains"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "bus_gain_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "bus gain checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def gain_library():
    A, lib = stub_library()
    for f in ("fxstub_bus_gain_mixes", "fxstub_bus_gain_ramps", "fxstub_live_allocations"):
        getattr(lib, f).restype = C.c_long
    return A, lib


class GainCounts:
    """what has happened since the last look: (emulation launches, plain mixes, weighted mixes, of those ramping, bus blocks, bus
    blocks mixed with gains)"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_bus_mixes(), self.lib.fxstub_bus_gain_mixes(), self.lib.fxstub_bus_gain_ramps(),
                self.b.info("bus_blocks"), self.b.info("bus_gain_blocks"))

    def expect(self, what, *want):
        now = self.now()
        got = tuple(x - y for x, y in zip(now, self.seen))
        assert got == want, (what, got, want)
        self.seen = now


def set_gains(lib, b, g, ramp):
    return lib.fxb_bus_set_gains(b._h, C.c_void_p(g.ctypes.data) if g is not None else None, ramp)


def child_routes():
    A, lib = gain_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(41)
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N, K in SHAPES:
            b = A.Batch(N, ch, 0)
            # before a program is loaded: only N and the channel count are needed
            a = np.ones((ch, N), dtype=np.float32)
            g0 = gains_for(rng, ch, N)
            assert b.bus_set_gains(g0) == 0 and same_words(b.bus_get_gains(), g0)
            assert b.load_text(text), b.errors()
            assert same_words(b.bus_get_gains(), g0), "the gains survive a program load"
            a = g0
            G = b.bus_groups(K)
            count = GainCounts(lib, b)
            for S in (33, 1):
                for ramp in (0, 1):
                    # pageable, staged; shared in and per-instance in
                    g = gains_for(rng, ch, N)
                    given = g.copy()
                    assert set_gains(lib, b, given, ramp) == 0
                    given[...] = np.nan   # the caller's array is free on return
                    xg = signal(rng, (S, ch, G))
                    want = gain_mix_model(expand(xg, K, N), a, g, ramp, S, K)
                    assert same_words(b.process_block_bus(xg, K, True, True), want), (ch, N, K, S, ramp, "staged")
                    count.expect("staged", 1, 0, 1, ramp, 1, 1)
                    a = g
                    xn = signal(rng, (S, ch, N))
                    assert same_words(b.process_block_bus(xn, K, False, True), gain_mix_model(xn, a, a, False, S, K)), (ch, N, K, S, "static after the ramp")
                    count.expect("static", 1, 0, 1, 0, 1, 1)
                    # pinned, in place
                    g = gains_for(rng, ch, N)
                    assert set_gains(lib, b, g, ramp) == 0
                    pg, po = pinned((S, ch, G)), pinned((S, ch, G))
                    pg[...] = signal(rng, (S, ch, G))
                    want = gain_mix_model(expand(pg, K, N), a, g, ramp, S, K)
                    assert bus(lib, b, pg, po, S, K, SHARED_IN | MIX_OUT) == 0 and same_words(po, want), (ch, N, K, S, ramp, "in place")
                    count.expect("in place", 1, 0, 1, ramp, 1, 1)
                    a = g
                    # the device entry on the handle's own stream
                    g = gains_for(rng, ch, N)
                    assert set_gains(lib, b, g, ramp) == 0
                    want = gain_mix_model(expand(pg, K, N), a, g, ramp, S, K)
                    assert b.process_block_bus_dev(int(pg.ctypes.data), int(po.ctypes.data), S, K) == 0 and b.sync() == 0
                    assert same_words(po, want), (ch, N, K, S, ramp, "device entry")
                    count.expect("device entry", 1, 0, 1, ramp, 1, 1)
                    a = g
                    assert same_words(b.bus_get_gains(), a)
                    pinned.free()
            b.close()
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain routes ok")


def child_state():
    A, lib = gain_library()
    rng = np.random.default_rng(43)
    N, K, S, ch = 200, 63, 33, 2
    b = A.Batch(N, ch, 0)
    assert b.load_text(STEREO), b.errors()
    G = b.bus_groups(K)
    count = GainCounts(lib, b)
    ones = np.ones((ch, N), dtype=np.float32)
    block = lambda: signal(rng, (S, ch, G))
    # gains of 1.0f equal gains off
    xg = block()
    off = b.process_block_bus(xg, K)
    count.expect("gains off: the plain mix", 1, 1, 0, 0, 1, 0)
    assert same_words(off, mix_model(expand(xg, K, N), K))
    assert b.bus_set_gains(ones) == 0
    assert same_words(b.process_block_bus(xg, K), off)
    count.expect("gains of 1.0f", 1, 0, 1, 0, 1, 1)
    assert b.bus_set_gains(ones, ramp=True) == 0
    assert same_words(b.process_block_bus(xg, K), off)
    count.expect("a ramp from 1.0f to 1.0f", 1, 0, 1, 1, 1, 1)
    # NULL turns them off again: the plain launch, the counter stands still, get is refused, the blocks are freed
    assert b.bus_set_gains(None) == 0
    assert same_words(b.process_block_bus(xg, K), off)
    count.expect("off again", 1, 1, 0, 0, 1, 0)
    assert lib.fxb_bus_get_gains(b._h, C.c_void_p(ones.ctypes.data)) == FX_E_ARG and b.bus_set_gains(None) == 0
    # a ramp out of "off" starts at 1.0f
    g1 = gains_for(rng, ch, N)
    assert b.bus_set_gains(g1, ramp=True) == 0
    assert same_words(b.bus_get_gains(), ones), "get before the consuming block: the gains in force"
    xg = block()
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), ones, g1, True, S, K))
    count.expect("ramp from off", 1, 0, 1, 1, 1, 1)
    assert same_words(b.bus_get_gains(), g1), "get after the consuming block: its target"
    # a replaced target: the ramp starts where it would have started
    g2, g3 = gains_for(rng, ch, N), gains_for(rng, ch, N)
    assert b.bus_set_gains(g2, ramp=True) == 0 and b.bus_set_gains(g3, ramp=True) == 0
    assert same_words(b.bus_get_gains(), g1)
    xg = block()
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g1, g3, True, S, K))
    count.expect("replaced target", 1, 0, 1, 1, 1, 1)
    # ... and the next block is static at that target
    xg = block()
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g3, g3, False, S, K))
    count.expect("static", 1, 0, 1, 0, 1, 1)
    # ramp = 0 cancels a pending ramp
    g4, g5 = gains_for(rng, ch, N), gains_for(rng, ch, N)
    assert b.bus_set_gains(g4, ramp=True) == 0 and b.bus_set_gains(g5, ramp=False) == 0
    assert same_words(b.bus_get_gains(), g5)
    xg = block()
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g5, g5, False, S, K))
    count.expect("cancelled ramp", 1, 0, 1, 0, 1, 1)
    # a block without FXB_BUS_MIX_OUT ignores the gains and leaves the ramp pending; so does a plain block
    g6 = gains_for(rng, ch, N)
    assert b.bus_set_gains(g6, ramp=True) == 0
    xg = block()
    assert same_words(b.process_block_bus(xg, K, True, False), expand(xg, K, N))
    count.expect("shared in only", 1, 0, 0, 0, 1, 0)
    xn = signal(rng, (S, ch, N))
    assert same_words(b.process_block(xn), xn)
    assert same_words(b.bus_get_gains(), g5), "still pending"
    xg = block()
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g5, g6, True, S, K))
    count.expect("the ramp, one block later", 2, 0, 1, 1, 1, 1)
    assert same_words(b.bus_get_gains(), g6)
    # two ramps in a row swap the roles of the two blocks; S = 1: w = b
    g7 = gains_for(rng, ch, N)
    assert b.bus_set_gains(g7, ramp=True) == 0
    xg = signal(rng, (1, ch, G))
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g6, g7, True, 1, K))
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g7, g7, False, 1, K))
    count.expect("S = 1", 2, 0, 2, 1, 2, 2)
    # instance calls do not touch the gains: a gain belongs to the mixer slot
    assert b.copy_instances([0, 1], [5, 6]) == 0 and b.reset_instances([7]) == 0
    assert same_words(b.bus_get_gains(), g7)
    # an allocation that fails inside the call: FX_E_MEMORY, gains stay off, nothing leaks; on a handle with gains on nothing is
    # allocated; NULL frees (a handle without a program: no builder thread allocates meanwhile)
    fresh = A.Batch(N, ch, 0)
    live = lib.fxstub_live_allocations()
    for nth in (0, 1, 2):
        lib.fxstub_fail_mallocs(nth, 1)
        assert set_gains(lib, fresh, g7, 0) == FX_E_MEMORY and fresh.last_error()
        lib.fxstub_fail_mallocs(-1, 0)
        assert lib.fxstub_live_allocations() == live and lib.fxb_bus_get_gains(fresh._h, C.c_void_p(ones.ctypes.data)) == FX_E_ARG
    assert fresh.bus_set_gains(g7) == 0 and lib.fxstub_live_allocations() == live + 3
    lib.fxstub_fail_mallocs(0, 100)
    assert fresh.bus_set_gains(g6, ramp=True) == 0 and fresh.bus_set_gains(g5) == 0
    lib.fxstub_fail_mallocs(-1, 0)
    assert same_words(fresh.bus_get_gains(), g5)
    assert fresh.bus_set_gains(None) == 0 and lib.fxstub_live_allocations() == live
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain state ok")


def child_pieces():
    A, lib = gain_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(47)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples, one S
    N, S, K = 262144, 96, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    a, g = gains_for(rng, 1, N), gains_for(rng, 1, N)
    assert b.bus_set_gains(a) == 0 and b.bus_set_gains(g, ramp=True) == 0
    count = GainCounts(lib, b)
    pg, po = pinned((S, 1, G)), pinned((S, 1, G))
    pg[...] = rng.standard_normal((S, 1, G)).astype(np.float32)
    x = expand(pg, K, N)
    want = gain_mix_model(x, a, g, True, S, K)
    assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, want), "a ramp across two pieces"
    count.expect("two pieces, in place", 2, 0, 2, 2, 1, 1)
    assert same_words(po[S - 1], gain_mix_model(x, g, g, False, S, K)[S - 1]), "the last row equals a static block at b"
    assert same_words(b.bus_get_gains(), g)
    assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, gain_mix_model(x, g, g, False, S, K)), "the next block is static"
    count.expect("static, two pieces", 2, 0, 2, 0, 1, 1)
    # with a schedule armed the block stays whole
    assert b.bus_set_gains(a, ramp=True) == 0 and b.set_register_track("vol", [0.1, 0.2], 48) == 0
    assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, gain_mix_model(x, g, a, True, S, K)), b.last_error()
    count.expect("armed: one piece", 1, 0, 1, 1, 1, 1)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("gain pieces ok")


def child_streams():
    A, lib = gain_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(53)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(st), 1) == 0 and st.value
    N, S, K = 1000, 8, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    dev = lambda x, y, st: lib.fxb_process_block_bus_dev(b._h, C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), S, K, 3, st)

    def fresh():
        p, o = pinned((S, 1, G)), pinned((S, 1, G))
        p[...] = rng.standard_normal((S, 1, G)).astype(np.float32)
        o[...] = -7.0
        return p, o
    g = [gains_for(rng, 1, N) for _ in range(6)]
    assert b.bus_set_gains(g[0]) == 0
    assert b.process_block_bus(np.zeros((S, 1, G), dtype=np.float32), K) is not None   # (code generated, scratch allocated)
    lib.fxstub_set_kernel_micros(30000)   # the emulation launch takes 30 ms: a set that does not wait for the block in front of it is caught
    # a block on one stream, then a set, then a block on another stream, fxb_sync only at the end
    (pa, ya), (pb, yb), (pc, yc), (pd, yd) = fresh(), fresh(), fresh(), fresh()
    assert dev(pa, ya, streams[0]) == 0
    assert b.bus_set_gains(g[1]) == 0
    assert dev(pb, yb, streams[1]) == 0
    # ... a ramp set behind it, consumed by a third block on the first stream; a second ramp behind that (the blocks swap roles)
    assert b.bus_set_gains(g[2], ramp=True) == 0
    assert dev(pc, yc, streams[0]) == 0
    assert b.bus_set_gains(g[3], ramp=True) == 0
    assert dev(pd, yd, None) == 0
    assert b.sync() == 0
    assert same_words(ya, gain_mix_model(expand(pa, K, N), g[0], g[0], False, S, K)), "the first block has the gains it was queued with"
    assert same_words(yb, gain_mix_model(expand(pb, K, N), g[1], g[1], False, S, K)), "the second block has the new gains"
    assert same_words(yc, gain_mix_model(expand(pc, K, N), g[1], g[2], True, S, K)), "the ramp behind it"
    assert same_words(yd, gain_mix_model(expand(pd, K, N), g[2], g[3], True, S, K)), "the second ramp"
    # get right behind a device-entry block waits as fxb_sync does
    assert b.bus_set_gains(g[4], ramp=True) == 0 and dev(pa, ya, streams[1]) == 0
    assert same_words(b.bus_get_gains(), g[4]) and same_words(ya, gain_mix_model(expand(pa, K, N), g[3], g[4], True, S, K))
    # off right behind a block: the block keeps its gains
    assert dev(pb, yb, streams[0]) == 0 and b.bus_set_gains(None) == 0
    assert same_words(yb, gain_mix_model(expand(pb, K, N), g[4], g[4], False, S, K))
    assert dev(pc, yc, streams[0]) == 0 and b.sync() == 0 and same_words(yc, mix_model(expand(pc, K, N), K))
    lib.fxstub_set_kernel_micros(150)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("gain streams ok")


def child_refusals():
    A, lib = gain_library()
    rng = np.random.default_rng(59)
    N, S, K, ch = 300, 8, 64, 2
    b = A.Batch(N, ch, 0)   # (no program yet: nothing but the calls below allocates)
    G = b.bus_groups(K)
    out = np.zeros((ch, N), dtype=np.float32)
    live = lib.fxstub_live_allocations()
    count = GainCounts(lib, b)
    g = gains_for(rng, ch, N)
    for state in ("off", "on", "pending"):
        if state == "on":
            assert b.bus_set_gains(g) == 0
        if state == "pending":
            assert b.bus_set_gains(np.ones((ch, N), dtype=np.float32), ramp=True) == 0
        live = lib.fxstub_live_allocations()
        for what, value, at in (("NaN", np.nan, (0, 0)), ("Inf", np.inf, (ch - 1, N - 1)), ("-Inf", -np.inf, (0, N // 2))):
            bad = gains_for(rng, ch, N)
            bad[at] = value
            for ramp in (0, 1):
                assert set_gains(lib, b, bad, ramp) == FX_E_ARG and "finite" in b.last_error(), (state, what)
        for ramp in (2, -1, 256):
            assert set_gains(lib, b, g, ramp) == FX_E_ARG and "ramp" in b.last_error(), (state, ramp)
            assert set_gains(lib, b, None, ramp) == FX_E_ARG, (state, ramp)
        assert lib.fxstub_live_allocations() == live
        if state == "off":
            assert lib.fxb_bus_get_gains(b._h, C.c_void_p(out.ctypes.data)) == FX_E_ARG and "off" in b.last_error()
        else:
            assert lib.fxb_bus_get_gains(b._h, None) == FX_E_ARG
            assert same_words(b.bus_get_gains(), g), state
        count.expect("refused: " + state, 0, 0, 0, 0, 0, 0)
    assert lib.fxb_bus_set_gains(None, C.c_void_p(g.ctypes.data), 0) == FX_E_ARG and lib.fxb_bus_get_gains(None, C.c_void_p(out.ctypes.data)) == FX_E_ARG
    # the pending ramp is still the one that was set
    assert b.load_text(STEREO), b.errors()
    xg = signal(rng, (S, ch, G))
    assert same_words(b.process_block_bus(xg, K), gain_mix_model(expand(xg, K, N), g, np.ones((ch, N), dtype=np.float32), True, S, K))
    count.expect("the handle goes on", 1, 0, 1, 1, 1, 1)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain refusals ok")


def child_shards():
    A, lib = gain_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(61)
    N, S, ch = 3 * 256 + 40, 16, 2
    b = A.Batch(N, ch, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    g0 = gains_for(rng, ch, N)
    assert b.bus_set_gains(g0) == 0 and same_words(b.bus_get_gains(), g0), "get assembles by global instance"
    assert b.load_text(STEREO), b.errors()
    count = GainCounts(lib, b)
    a = g0
    for K in (64, 32, 1):
        G = b.bus_groups(K)
        for ramp in (0, 1):
            g = gains_for(rng, ch, N)
            assert set_gains(lib, b, g, ramp) == 0
            pg, po = pinned((S, ch, G)), pinned((S, ch, G))
            pg[...] = signal(rng, (S, ch, G))
            assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, gain_mix_model(expand(pg, K, N), a, g, ramp, S, K)), (K, ramp, b.last_error())
            count.expect("in place, every shard on its columns", 3, 0, 3, 3 * ramp, 3, 3)
            a = g
            xn = signal(rng, (S, ch, N))
            assert same_words(b.process_block_bus(xn, K, False, True), gain_mix_model(xn, a, a, False, S, K)), K
            count.expect("pageable", 3, 0, 3, 0, 3, 3)
            assert same_words(b.bus_get_gains(), a)
            pinned.free()
    # all or nothing: an allocation that fails on whichever shard leaves gains off on all of them (no program yet: no builder
    # thread allocates meanwhile)
    c = A.Batch(N, ch, devices=[0, 1, 2])
    live = lib.fxstub_live_allocations()
    out = np.zeros((ch, N), dtype=np.float32)
    for nth in (0, 4, 8):
        lib.fxstub_fail_mallocs(nth, 1)
        rc = set_gains(lib, c, g0, 1)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.last_error(), (nth, rc)
        assert lib.fxstub_live_allocations() == live and lib.fxb_bus_get_gains(c._h, C.c_void_p(out.ctypes.data)) == FX_E_ARG
    bad = g0.copy()
    bad[1, 600] = np.nan   # (in the last shard's columns: refused for the whole batch, in front of every shard)
    assert set_gains(lib, c, bad, 0) == FX_E_ARG and lib.fxstub_live_allocations() == live
    assert c.bus_set_gains(g0) == 0 and lib.fxstub_live_allocations() == live + 9
    assert c.bus_set_gains(None) == 0 and lib.fxstub_live_allocations() == live
    assert c.load_text(STEREO), c.errors()
    xg = signal(rng, (S, ch, c.bus_groups(64)))
    mixes = lib.fxstub_bus_mixes()
    assert same_words(c.process_block_bus(xg, 64), mix_model(expand(xg, 64, N), 64)) and lib.fxstub_bus_mixes() == mixes + 3
    assert c.info("bus_gain_blocks") == 0 and b.info("bus_gain_blocks") == 3 * 12
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "state": child_state, "pieces": child_pieces, "streams": child_streams, "refusals": child_refusals, "shards": child_shards}[sys.argv[1]]()
