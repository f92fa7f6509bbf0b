"""Bus feeds without a GPU: the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc
stublib`), driven through the C ABI in a child process like tests/test_bus_send_stub.py (this file is also that child).  The
stand-in of the feed kernel (tests/hipstub/fx_bus_feed_stub.cpp) does the real arithmetic in stream order, entry by entry, and
checks the host's tables against the structure they must describe, so what is checked here is the definition as numpy
(feed_model) and the host side: the structure and its tables (map and CSR form), the routes of the source block (pinned,
pageable, device memory), the pieces of a block above the scratch limit, the state machine of fxb_bus_set_feeds /
fxb_bus_set_feed_gains, that a feed block leaves everything as fxb_process_block_bus_aux on feed_model's block does, the
refusals, and three shards.  Words are compared as uint32: there is no tolerance anywhere.

Parity on the device is tests/test_gpu_bus_feed.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MIX_OUT, PROGRAM, ROOT, SHARED_IN, STEREO, Pinned, expand, mix_model, same_words, stub_library  # noqa: E402
from test_bus_gain_stub import gain_mix_model, gain_weights, gains_for  # noqa: E402
from test_bus_tap_stub import same_bits, signal, tap_list  # noqa: E402
from test_bus_send_stub import send_model, structure  # noqa: E402
from route_models import feed_model  # noqa: E402,F401  (the models live there; the tests of them stay here)

MOST_ENTRIES = 1 << 24
COUNTS = (0, 1, 2, 5, 65)   # entries of an instance: none, the moved word, one add, a short list, more than a wavefront is wide


def feed_structure(rng, N, M, counts=COUNTS):
    """CSR by instance: every instance draws its number of entries from `counts`, instances 0 and N - 1 are always fed; the
    lists are unsorted and repeat columns (always where a list is longer than M)"""
    count = rng.choice(np.array(counts), N)
    fed = [c for c in counts if c > 0]
    count[0], count[N - 1] = fed[-1], fed[0]
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    sources = rng.integers(0, M, int(offsets[-1])).astype(np.int64)
    if sources.size > 1:
        sources[1] = sources[0]
    return offsets, sources


def source_block(rng, shape):
    """finite words of every magnitude, denormals and both zeros among them"""
    x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 6, shape)).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    for k, word in enumerate((0x80000000, 0x00000001, 0x80000003, 0x00000000, 0x007fffff)):
        flat[(k * 5) % flat.size] = word
    return x


def test_feed_model_against_the_sum_written_out_one_add_at_a_time():
    """one instance with five entries, static and ramping; and the words that must move as patterns"""
    rng = np.random.default_rng(3)
    f = np.float32
    S, M = 4, 7
    src = source_block(rng, (S, 1, M))
    sources = np.array([6, 0, 6, 3, 1], dtype=np.int64)
    a, b = gains_for(rng, 1, 5), gains_for(rng, 1, 5)
    b[0, 2] = f(0.0)
    r = f(f(1.0) / f(S))
    for ramp in (False, True):
        for s in range(S):
            t = f(f(s + 1) * r)
            acc = None
            for k in range(5):
                w = b[0, k] if (not ramp or s == S - 1) else f(a[0, k] + f(f(b[0, k] - a[0, k]) * t))
                term = f(0.0) if w == 0.0 else f(w * src[s, 0, sources[k]])
                acc = term if k == 0 else f(acc + term)
            got = feed_model(src, [0, 5], sources, a, b, ramp, S)
            assert same_bits(got[s, 0], np.array([acc], dtype=np.float32)), (ramp, s)
    # unweighted: no entry is +0.0, one entry moves the pattern (a NaN payload, -0), two entries are one add from term_0 on
    words = np.array([0x7fc12345, 0x80000000, 0x7f812345, 0x3f800000], dtype=np.uint32).view(np.float32).reshape(1, 1, 4)
    got = feed_model(words, [0, 0, 1, 2, 3, 5], [0, 1, 2, 1, 1], None, None, False, 1)
    assert (got.view(np.uint32)[0, 0] == np.array([0, 0x7fc12345, 0x80000000, 0x7f812345, 0x80000000], dtype=np.uint32)).all()   # (-0 + -0 = -0: no zero in front)
    # the map n / K is the shared input
    x = source_block(rng, (3, 2, 4))
    assert same_bits(feed_model(x, np.arange(11), np.arange(10) // 3, None, None, False, 3), expand(x, 3, 10))


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_the_map_n_over_k_is_the_shared_input_on_the_hip_stand_in():
    run_child("shared", "feed shared ok")


def test_feed_routes_and_results_against_a_plain_handle_on_the_hip_stand_in():
    """pinned, pageable and device src; the mix, taps, sends, meters, bus gains with a pending ramp and the state image"""
    run_child("routes", "feed routes ok")


def test_feed_rows_of_the_pieces_of_a_block_on_the_hip_stand_in():
    run_child("pieces", "feed pieces ok")


def test_feed_ramps_and_state_machine_on_the_hip_stand_in():
    run_child("state", "feed state ok")


def test_feed_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "feed refusals ok")


def test_feeds_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "feed shards ok", devices=3)


def test_feed_set_that_runs_out_of_memory_on_one_shard_on_the_hip_stand_in():
    run_child("memory", "feed memory ok", devices=3)


def test_feed_structures_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/bus_feed_checks.cpp (csrc/Makefile `stubasanfeeds`): structure shapes, the refusals and an allocation failure
    at every allocation of a set and of the source staging, through the C ABI on exactly-sized heap blocks, on one handle and on
    three shards, under AddressSanitizer + UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is
    preloaded and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasanfeeds"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "bus_feed_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "bus feed checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def feed_library():
    A, lib = stub_library()
    for f in ("fxstub_bus_taps", "fxstub_bus_gain_mixes", "fxstub_live_allocations", "fxstub_bus_sends", "fxstub_bus_feeds", "fxstub_bus_feed_ramps", "fxstub_bus_feed_maps",
              "fxstub_bus_feed_strays"):
        getattr(lib, f).restype = C.c_long
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipFree.argtypes = [C.c_void_p]
    return A, lib


class FeedCounts:
    """what has happened since the last look: (emulation launches, expands, feed launches, mixes plain and weighted, staged, in
    place, bus blocks, feed blocks)"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_bus_expands(), self.lib.fxstub_bus_feeds(), self.lib.fxstub_bus_mixes() + self.lib.fxstub_bus_gain_mixes(),
                self.b.info("host_staged_blocks"), self.b.info("host_inplace_blocks"), self.b.info("bus_blocks"), self.b.info("bus_feed_blocks"))

    def expect(self, what, *want):
        now = self.now()
        got = tuple(x - y for x, y in zip(now, self.seen))
        assert got == want, (what, got, want)
        self.seen = now

    def skip(self):
        self.seen = self.now()


NOTHING = (0,) * 8


def ptr(a):
    return C.c_void_p(a if isinstance(a, int) else (a.ctypes.data if a is not None else 0))


def fed(lib, b, src, y, t, a, S, K, flags):
    return lib.fxb_process_block_bus_feed(b._h, ptr(src), ptr(y), ptr(t), ptr(a), S, K, flags)


def fed_dev(lib, b, src, y, t, a, S, K, flags, stream=None):
    return lib.fxb_process_block_bus_feed_dev(b._h, ptr(src), ptr(y), ptr(t), ptr(a), S, K, flags, stream)


def set_feeds(lib, b, M, offsets, sources, gains):
    offsets, sources = np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(sources, dtype=np.int64)
    return lib.fxb_bus_set_feeds(b._h, M, ptr(offsets), ptr(sources) if sources.size else None, ptr(gains))


def feeds_are(b, M, offsets, sources, gains):
    m, off, src, g = b.bus_get_feeds()
    return m == M and (off == offsets).all() and (src == sources).all() and same_bits(g, gains)


class DeviceBlock:
    """a block of the stand-in's device memory holding a copy of `x`"""

    def __init__(self, lib, x):
        self.lib, self.p = lib, C.c_void_p(0)
        assert lib.hipMalloc(C.byref(self.p), max(x.nbytes, 4)) == 0
        assert lib.hipMemcpy(self.p, ptr(x), x.nbytes, 1) == 0
        self.address = self.p.value

    def free(self):
        self.lib.hipFree(self.p)


def child_shared():
    """unweighted feeds with M = G, one entry per instance and sources[n] = n / K: FXB_BUS_SHARED_IN with group K, word for
    word - out and the state image"""
    A, lib = feed_library()
    rng = np.random.default_rng(201)
    S = 9
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N in (777, 200):
            for K in (1, 63, 64, 130):
                a, b = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
                assert a.load_text(text) and b.load_text(text), a.errors()
                G = a.bus_groups(K)
                assert b.bus_set_feeds(G, np.arange(N + 1), np.arange(N) // min(K, N)) == 0, b.last_error()
                maps = lib.fxstub_bus_feed_maps()
                for mix in (False, True):
                    for rep in range(2):
                        x = signal(rng, (S, ch, G))   # (NaNs with payloads, infinities, -0: the words move)
                        want = a.process_block_bus(x, K, True, mix)
                        got = b.process_block_bus_feed(x, K, mix)
                        assert same_bits(got, want) if not mix else same_words(got, want), (ch, N, K, mix, rep)
                        assert (a.save_state() == b.save_state()).all(), (ch, N, K, mix, rep)
                assert lib.fxstub_bus_feed_maps() == maps + 4, "the host noticed the map form"
                assert a.info("bus_blocks") == b.info("bus_blocks") and b.info("bus_feed_blocks") == 4 and a.info("bus_feed_blocks") == 0
                a.close()
                b.close()
    assert lib.fxstub_bus_feed_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("feed shared ok")


def child_routes():
    A, lib = feed_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(203)
    S, K = 9, 130
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N, M in ((1, 1), (200, 3), (777, 70)):
            b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
            assert b.load_text(text) and plain.load_text(text), b.errors()
            G = b.bus_groups(K)
            offsets, sources = feed_structure(rng, N, M)
            E = int(offsets[-1])
            g = gains_for(rng, ch, max(E, 1))[:, :E].copy()
            soff, smem = structure(rng, N, (65, 0, 3))
            sg = gains_for(rng, ch, int(soff[-1]))
            taps = tap_list(rng, N, 5)
            bg0, bg1 = gains_for(rng, ch, N), gains_for(rng, ch, N)
            for h in (b, plain):
                assert h.bus_set_sends(soff, smem, sg) == 0 and h.bus_set_taps(taps) == 0 and h.meter_enable(True) == 0 and h.bus_set_gains(bg0) == 0
            count = FeedCounts(lib, b)
            for weights in (None, g):
                given = (offsets.copy(), sources.copy(), None if weights is None else weights.copy())
                assert set_feeds(lib, b, M, *given) == 0, b.last_error()
                for arr in given:
                    if arr is not None:
                        arr[...] = -1   # the caller's arrays are free on return
                assert feeds_are(b, M, offsets, sources, np.ones((ch, E), dtype=np.float32) if weights is None else weights)
                where = (ch, N, M, weights is not None)
                src = source_block(rng, (S, ch, M))
                block = feed_model(src, offsets, sources, weights, weights, False, S)
                # unmixed, pageable: the words of the plain handle on feed_model's block
                want = plain.process_block(block)
                count.skip()
                assert same_words(b.process_block_bus_feed(src), want), where + ("unmixed",)
                count.expect("unmixed, pageable", 1, 0, 1, 0, 1, 0, 1, 1)
                # mixed with taps and sends, a ramp of the bus gains pending on both handles
                assert b.bus_set_gains(bg1, True) == 0 and plain.bus_set_gains(bg1, True) == 0
                w_out, w_taps, w_aux = plain.process_block_bus(block, K, False, True, taps=True, aux=True)
                count.skip()
                out, tp, aux = b.process_block_bus_feed(src, K, True, taps=True, aux=True)
                assert same_words(out, w_out) and same_bits(tp, w_taps) and same_words(aux, w_aux), where + ("pageable",)
                count.expect("mixed, pageable", 1, 0, 1, 1, 1, 0, 1, 1)
                assert same_bits(b.bus_get_gains(), plain.bus_get_gains()), "the ramp of the bus gains was consumed on both"
                # pinned src and out: the output in place, the source rows copied to the device all the same
                w_out = plain.process_block_bus(block, K, False, True)
                ps, po = pinned(src.shape), pinned((S, ch, G))
                ps[...] = src
                count.skip()
                assert fed(lib, b, ps, po, None, None, S, K, MIX_OUT) == 0 and same_words(po, w_out), where + ("pinned",)
                count.expect("pinned", 1, 0, 1, 1, 0, 1, 1, 1)
                # the device entry: pinned src (copied), then src in device memory (gathered in place), twice
                w_out = plain.process_block_bus(block, K, False, True)
                assert fed_dev(lib, b, ps, po, None, None, S, K, MIX_OUT) == 0 and b.sync() == 0 and same_words(po, w_out), where + ("device entry, pinned",)
                dev = DeviceBlock(lib, src)
                live = lib.fxstub_live_allocations()
                for rep in range(2):
                    w_out = plain.process_block_bus(block, K, False, True)
                    po[...] = -7.0
                    assert fed_dev(lib, b, dev.address, po, None, None, S, K, MIX_OUT) == 0 and b.sync() == 0 and same_words(po, w_out), where + ("device memory", rep)
                assert lib.fxstub_live_allocations() == live
                # ... and handed to the host entry
                w_out = plain.process_block_bus(block, K, False, True)
                assert fed(lib, b, dev.address, po, None, None, S, K, MIX_OUT) == 0 and same_words(po, w_out), where + ("host entry, device memory",)
                dev.free()
                count.skip()
                assert fed(lib, b, ps, po, None, None, 0, K, MIX_OUT) == 0
                count.expect("zero samples", *NOTHING)
                ma, mb = plain.meter_read(), b.meter_read()
                for key in ("energy", "peak", "full_scale", "nonfinite"):
                    assert (ma[key].view(np.uint8) == mb[key].view(np.uint8)).all(), key
                assert (plain.save_state() == b.save_state()).all(), where
                pinned.free()
            b.close()
            plain.close()
    assert lib.fxstub_bus_feed_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("feed routes ok")


def child_pieces():
    A, lib = feed_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(205)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples
    N, S, M = 262144, 96, 70
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    offsets, sources = feed_structure(rng, N, M, counts=(0, 1, 2))
    E = int(offsets[-1])
    g0, g1 = gains_for(rng, 1, E), gains_for(rng, 1, E)
    assert set_feeds(lib, b, M, offsets, sources, g0) == 0, b.last_error()
    src = source_block(rng, (S, 1, M))
    count = FeedCounts(lib, b)
    # (the stand-in's emulation launch copies in to out: tests/test_gpu_bus_feed.py runs the plain path)
    assert same_words(b.process_block_bus_feed(src), feed_model(src, offsets, sources, g0, g0, False, S))
    count.expect("two pieces", 2, 0, 2, 0, 1, 0, 1, 1)
    # a ramp across the two pieces: t goes by the sample of the CALL
    assert b.bus_set_feed_gains(g1, True) == 0
    po = pinned((S, 1, N))
    assert fed(lib, b, src, po, None, None, S, 1, 0) == 0 and same_words(po, feed_model(src, offsets, sources, g0, g1, True, S))
    count.expect("two pieces, ramping", 2, 0, 2, 0, 0, 1, 1, 1)
    assert lib.fxstub_bus_feed_ramps() == 2
    po[...] = -7.0
    assert fed(lib, b, src, po, None, None, 65, 1, 0) == 0 and same_words(po[:65], feed_model(src[:65], offsets, sources, g1, g1, False, 65)) and (po[65:] == -7.0).all()
    count.expect("65 samples: two pieces", 2, 0, 2, 0, 0, 1, 1, 1)
    assert lib.fxstub_bus_feed_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("feed pieces ok")


def child_state():
    A, lib = feed_library()
    rng = np.random.default_rng(207)
    N, M, S, ch = 777, 70, 5, 2
    b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
    live = lib.fxstub_live_allocations()
    nM = C.c_int64(-1)
    assert lib.fxb_bus_get_feeds(b._h, C.byref(nM), None, 0, None, None, 0) == 0 and nM.value == 0 and b.bus_get_feeds()[0] == 0, "off by default"
    off1, src1 = feed_structure(rng, N, M)
    E = int(off1[-1])
    g1, g2, g3, g4 = (gains_for(rng, ch, E) for _ in range(4))
    ones = np.ones((ch, E), dtype=np.float32)
    assert set_feeds(lib, b, M, off1, src1, g1) == 0, "before a program is loaded"
    assert lib.fxstub_live_allocations() == live + 1, "one device block is the only allocation of a set"
    assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()
    assert b.prepare(S, True) == 0 and plain.prepare(S, True) == 0
    assert feeds_are(b, M, off1, src1, g1), "the feeds survive a program load"

    def block(a, bb, ramp, S=S, off=off1, src=src1, M=M):
        x = source_block(rng, (S, ch, M))
        want = plain.process_block(feed_model(x, off, src, a, bb, ramp, S))
        assert same_words(b.process_block_bus_feed(x), want), (ramp, S)

    block(g1, g1, False)
    # the round trip with less room than there is
    some_off, some_src, some_g = np.full(12, -1, dtype=np.int64), np.full(10, -1, dtype=np.int64), np.full((ch, E), -7.0, dtype=np.float32)
    assert lib.fxb_bus_get_feeds(b._h, C.byref(nM), ptr(some_off), 4, ptr(some_src), ptr(some_g), 7) == E and nM.value == M
    assert (some_off[:4] == off1[:4]).all() and (some_off[4:] == -1).all() and (some_src[:7] == src1[:7]).all() and (some_src[7:] == -1).all()
    assert same_bits(some_g[:, :7], g1[:, :7]) and (some_g[:, 7:] == -7.0).all()
    # static gains replace a and b; a ramp makes the old b the a of the next FEED block and ends on its target
    assert b.bus_set_feed_gains(g2) == 0 and feeds_are(b, M, off1, src1, g2)
    block(g2, g2, False)
    assert b.bus_set_feed_gains(g3, True) == 0 and feeds_are(b, M, off1, src1, g2), "a while the ramp is pending"
    # a block that is not a feed block leaves it pending
    x = signal(rng, (S, ch, N))
    assert same_words(b.process_block_bus(x, 64, False, True), plain.process_block_bus(x, 64, False, True)) and feeds_are(b, M, off1, src1, g2)
    assert b.bus_set_feed_gains(g4, True) == 0 and feeds_are(b, M, off1, src1, g2), "a second ramp set replaces the target, a stays"
    # 16 + 17 samples are not 33 while a ramp is pending ...
    x33 = source_block(rng, (33, ch, M))
    whole = feed_model(x33, off1, src1, g2, g4, True, 33)
    parts = np.concatenate([feed_model(x33[:16], off1, src1, g2, g4, True, 16), feed_model(x33[16:], off1, src1, g4, g4, False, 17)])
    assert not same_words(whole, parts)
    assert same_bits(whole[32], feed_model(x33[32:], off1, src1, g4, g4, False, 1)[0]), "the last sample of a ramp carries exactly b"
    assert same_words(b.process_block_bus_feed(x33), plain.process_block(whole))
    assert feeds_are(b, M, off1, src1, g4), "consumed: the target is in force"
    # ... and without one they are
    got = np.concatenate([b.process_block_bus_feed(x33[:16]), b.process_block_bus_feed(x33[16:])])
    assert same_words(got, plain.process_block(feed_model(x33, off1, src1, g4, g4, False, 33)))
    assert b.bus_set_feed_gains(g2, True) == 0
    block(g4, g2, True, S=1)   # a ramp of one sample is its target
    assert b.bus_set_feed_gains(g3, True) == 0 and b.bus_set_feed_gains(g1, False) == 0 and feeds_are(b, M, off1, src1, g1), "ramp = 0 drops a pending ramp"
    block(g1, g1, False)
    # NULL: back to unweighted, and a pending ramp is gone; a ramp out of unweighted starts from 1.0f
    assert b.bus_set_feed_gains(g3, True) == 0 and b.bus_set_feed_gains(None) == 0 and feeds_are(b, M, off1, src1, ones)
    block(None, None, False)
    assert b.bus_set_feed_gains(g2, True) == 0 and feeds_are(b, M, off1, src1, ones)
    block(ones, g2, True, S=7)
    # a new structure cancels a pending ramp
    assert b.bus_set_feed_gains(g3, True) == 0
    off2, src2 = feed_structure(rng, N, 3, counts=(1,))
    assert set_feeds(lib, b, 3, off2, src2, None) == 0 and feeds_are(b, 3, off2, src2, np.ones((ch, N), dtype=np.float32)), "replaced, by a map"
    block(None, None, False, off=off2, src=src2, M=3)
    assert lib.fxstub_bus_feed_ramps() == 3
    bad = g1.copy()
    bad[1, 5] = np.inf
    assert lib.fxb_bus_set_feed_gains(b._h, ptr(bad[:, :N].copy()), 0) == FX_E_ARG and lib.fxb_bus_set_feed_gains(b._h, ptr(ones), 2) == FX_E_ARG
    assert feeds_are(b, 3, off2, src2, np.ones((ch, N), dtype=np.float32))
    # instance calls do not touch the feeds
    assert b.copy_instances([0, 1], [70, 131]) == 0 and plain.copy_instances([0, 1], [70, 131]) == 0 and b.sync() == 0 and feeds_are(b, 3, off2, src2, np.ones((ch, N), dtype=np.float32))
    # off: the memory goes; feed blocks are refused, others go on
    held = lib.fxstub_live_allocations()
    assert lib.fxb_bus_set_feeds(b._h, 0, None, None, None) == 0 and b.bus_get_feeds()[0] == 0
    assert lib.fxstub_live_allocations() == held - 2, "the structure and the device copy of the source rows are freed"
    x = source_block(rng, (S, ch, 3))
    assert fed(lib, b, x, np.zeros((S, ch, N), dtype=np.float32), None, None, S, 1, 0) == FX_E_ARG and "feeds are off" in b.last_error()
    assert lib.fxb_bus_set_feed_gains(b._h, ptr(ones), 0) == FX_E_ARG and "feeds are off" in b.last_error()
    assert b.bus_set_feeds(0, None, None) == 0, "off twice"
    assert b.bus_set_feeds(M, off1, src1, g1) == 0
    block(g1, g1, False)
    n_fed = b.info("bus_feed_blocks")
    b.close()
    plain.close()
    assert n_fed == 11, n_fed
    assert lib.fxstub_live_allocations() < live, "nothing of the feeds outlives the handle"
    assert lib.fxstub_bus_feed_strays() == 0
    print("feed state ok")


def child_refusals():
    A, lib = feed_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(209)
    N, S, K, M, T = 300, 8, 64, 7, 5
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    assert b.prepare(S, True) == 0
    G = b.bus_groups(K)
    offsets, sources = feed_structure(rng, N, M)
    E = int(offsets[-1])
    g = gains_for(rng, 1, E)
    soff, smem = structure(rng, N, (65, 3))
    assert b.bus_set_taps(tap_list(rng, N, T)) == 0 and b.bus_set_sends(soff, smem) == 0
    ps, po, pn, pt, pa = pinned((S, 1, M)), pinned((S, 1, G)), pinned((S, 1, N)), pinned((S, 1, T)), pinned((S, 1, 2))
    both = pinned((4 * S, 1, N))
    ps[...] = source_block(rng, (S, 1, M))
    at = lambda a, off: C.c_void_p(a.ctypes.data + off * 4)

    def untouched():
        ok = (po == -7.0).all() and (pn == -7.0).all() and (both == -7.0).all() and (pt == -7.0).all() and (pa == -7.0).all()
        for arr in (po, pn, both, pt, pa):
            arr[...] = -7.0
        return ok

    untouched()
    count = FeedCounts(lib, b)
    for what, call in (("host entry, feeds off", lambda: fed(lib, b, ps, pn, None, None, S, K, 0)), ("device entry, feeds off", lambda: fed_dev(lib, b, ps, pn, None, None, S, K, 0)),
                       ("zero samples, feeds off", lambda: fed(lib, b, ps, pn, None, None, 0, K, 0)), ("feed gains, feeds off", lambda: lib.fxb_bus_set_feed_gains(b._h, ptr(g), 0))):
        assert call() == FX_E_ARG and "feeds are off" in b.last_error(), what
        count.expect(what, *NOTHING)
        assert untouched() and b.bus_get_feeds()[0] == 0, what
    # sets that are refused: nothing changes, neither from "off" nor from a structure in force
    i64 = lambda *v: np.array(v, dtype=np.int64)
    bad_source, negative, not_finite, nan = sources.copy(), sources.copy(), g.copy(), g.copy()
    bad_source[E - 1], negative[0], not_finite[0, 3], nan[0, E - 1] = M, -1, np.inf, np.nan
    long_off = np.concatenate([np.zeros(N, dtype=np.int64), [MOST_ENTRIES + 1]])
    decreasing, first_one = offsets.copy(), offsets.copy()
    decreasing[5] = decreasing[4] - 1 if decreasing[4] > 0 else decreasing[6] + 1
    first_one[0] = 1
    sets = (
        ("n_src < 0", lambda: lib.fxb_bus_set_feeds(b._h, -1, ptr(offsets), ptr(sources), ptr(g))),
        ("a source row of 4 GiB", lambda: lib.fxb_bus_set_feeds(b._h, 1 << 30, ptr(offsets), ptr(sources), ptr(g))),
        ("more entries than the cap", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(long_off), ptr(sources), None)),
        ("null offsets", lambda: lib.fxb_bus_set_feeds(b._h, M, None, ptr(sources), ptr(g))),
        ("null sources", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(offsets), None, ptr(g))),
        ("offsets[0] != 0", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(first_one), ptr(sources), None)),
        ("offsets decreasing", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(decreasing), ptr(sources), None)),
        ("source == M", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(offsets), ptr(bad_source), ptr(g))),
        ("source < 0", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(offsets), ptr(negative), ptr(g))),
        ("an infinite gain", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(offsets), ptr(sources), ptr(not_finite))),
        ("a NaN gain", lambda: lib.fxb_bus_set_feeds(b._h, M, ptr(offsets), ptr(sources), ptr(nan))),
        ("null handle", lambda: lib.fxb_bus_set_feeds(None, M, ptr(offsets), ptr(sources), ptr(g))),
    )
    live = lib.fxstub_live_allocations()
    for state in ("off", "on"):
        if state == "on":
            assert set_feeds(lib, b, M, offsets, sources, g) == 0
            live = lib.fxstub_live_allocations()
        for what, call in sets:
            assert call() == FX_E_ARG, (state, what)
            assert lib.fxstub_live_allocations() == live, (state, what)
            assert feeds_are(b, M, offsets, sources, g) if state == "on" else b.bus_get_feeds()[0] == 0, (state, what)
    assert lib.fxb_bus_get_feeds(None, None, None, 0, None, None, 0) == FX_E_ARG and lib.fxb_bus_get_feeds(b._h, None, None, -1, None, None, 0) == FX_E_ARG
    assert lib.fxb_bus_get_feeds(b._h, None, None, 0, None, None, -1) == FX_E_ARG
    assert b.bus_set_feed_gains(g, True) == 0   # (a pending ramp that no refusal may consume)
    assert fed(lib, b, ps, po, pt, pa, S, K, MIX_OUT) == 0, b.last_error()
    assert b.bus_set_feed_gains(g, True) == 0
    ms = b.last_kernel_ms()
    untouched()
    count = FeedCounts(lib, b)
    rows = S * M   # words of the source block
    refused = [
        ("FXB_BUS_SHARED_IN", lambda: fed(lib, b, ps, pn, None, None, S, K, SHARED_IN)), ("both flags", lambda: fed(lib, b, ps, po, None, None, S, K, 3)),
        ("FXB_BUS_SHARED_IN, device entry", lambda: fed_dev(lib, b, ps, po, None, None, S, K, 3)),
        ("null src", lambda: fed(lib, b, None, po, None, None, S, K, MIX_OUT)), ("null out", lambda: fed(lib, b, ps, None, None, None, S, K, MIX_OUT)),
        ("device entry, null src", lambda: fed_dev(lib, b, None, po, None, None, S, K, MIX_OUT)),
        # src sharing a byte with out, the tap rows or the aux rows: there is no in-place form
        ("src == out", lambda: lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, 0), None, None, S, K, 0)),
        ("last src word on the first of out", lambda: lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, rows - 1), None, None, S, K, 0)),
        ("first src word on the last of out", lambda: lib.fxb_process_block_bus_feed(b._h, at(both, S * G - 1), at(both, 0), None, None, S, K, MIX_OUT)),
        ("src == tap rows", lambda: lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, 2 * S * N), at(both, 0), None, S, K, MIX_OUT)),
        ("first tap word on the last of src", lambda: lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, 2 * S * N), at(both, rows - 1), None, S, K, MIX_OUT)),
        ("src == aux rows", lambda: lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, 0), S, K, MIX_OUT)),
        ("last aux word on the first of src, device entry", lambda: lib.fxb_process_block_bus_feed_dev(b._h, at(both, 2 * S - 1), at(both, 2 * S * N), None, at(both, 0), S, K, MIX_OUT, None)),
        # every refusal fxb_process_block_bus_aux has
        ("group 0", lambda: fed(lib, b, ps, po, pt, pa, S, 0, MIX_OUT)), ("unknown flag", lambda: fed(lib, b, ps, po, pt, pa, S, K, 6)), ("flag 4", lambda: fed(lib, b, ps, pn, None, None, S, K, 4)),
        ("negative length", lambda: fed(lib, b, ps, po, pt, pa, -1, K, MIX_OUT)),
        ("tap rows without FXB_BUS_MIX_OUT", lambda: fed(lib, b, ps, pn, pt, None, S, K, 0)), ("aux rows without FXB_BUS_MIX_OUT", lambda: fed(lib, b, ps, pn, None, pa, S, K, 0)),
        ("aux rows == tap rows", lambda: lib.fxb_process_block_bus_feed(b._h, ptr(ps), ptr(po), at(both, 0), at(both, 0), S, K, MIX_OUT)),
        ("tap rows over the output", lambda: lib.fxb_process_block_bus_feed(b._h, ptr(ps), at(both, 0), at(both, 0), None, S, K, MIX_OUT)),
        ("device entry, pageable src", lambda: fed_dev(lib, b, np.zeros((S, 1, M), dtype=np.float32), po, None, None, S, K, MIX_OUT)),
        ("device entry, src beyond its allocation", lambda: lib.fxb_process_block_bus_feed_dev(b._h, at(ps, 1), ptr(po), None, None, S, K, MIX_OUT, None)),
        ("device entry, pageable out", lambda: fed_dev(lib, b, ps, np.zeros((S, 1, G), dtype=np.float32), None, None, S, K, MIX_OUT)),
        ("null handle", lambda: lib.fxb_process_block_bus_feed(None, ptr(ps), ptr(po), None, None, S, K, MIX_OUT)),
    ]
    for what, call in refused:
        assert call() == FX_E_ARG, (what, b.last_error())
        count.expect(what, *NOTHING)
        assert untouched(), what
        assert feeds_are(b, M, offsets, sources, g) and b.last_kernel_ms() == ms, what
    assert lib.fxstub_bus_feed_ramps() == 1, "no refusal consumed the pending ramp"
    # ... and blocks that touch without overlapping are not among them
    assert lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, rows), None, None, S, K, 0) == 0, b.last_error()
    assert lib.fxstub_bus_feed_ramps() == 2
    # the device copy of a larger source block that cannot be had: FX_E_MEMORY, nothing launched, the handle goes on
    src2 = source_block(rng, (2 * S, 1, M))
    out2 = np.full((2 * S, 1, N), -7.0, dtype=np.float32)
    count = FeedCounts(lib, b)
    lib.fxstub_fail_mallocs(0, 1)
    rc = fed(lib, b, src2, out2, None, None, 2 * S, K, 0)
    lib.fxstub_fail_mallocs(-1, 0)
    assert rc == FX_E_MEMORY and (out2 == -7.0).all(), b.last_error()
    count.expect("source rows refused", *NOTHING)
    assert fed(lib, b, src2, out2, None, None, 2 * S, K, 0) == 0 and same_words(out2, feed_model(src2, offsets, sources, g, g, False, 2 * S)), b.last_error()
    # a handle of several shards has no device entry (here: one device, three shards)
    three = A.Batch(N, 1, devices=[0, 0, 0])
    assert three.load_text(PROGRAM) and three.bus_set_feeds(M, offsets, sources) == 0
    k0 = lib.fxstub_kernels_run()
    assert fed_dev(lib, three, ps, po, None, None, S, K, MIX_OUT) == FX_E_ARG and lib.fxstub_kernels_run() == k0
    assert lib.fxstub_bus_feed_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("feed refusals ok")


def child_shards():
    A, lib = feed_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(211)
    N, S, ch, M = 3 * 256 + 40, 9, 2, 70
    b, plain = A.Batch(N, ch, devices=[0, 1, 2]), A.Batch(N, ch, 0)
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()
    count = FeedCounts(lib, b)
    for what in ("lists on every shard", "the middle shard has no entry", "a map"):
        offsets, sources = feed_structure(rng, N, M, counts=(1,) if what == "a map" else COUNTS)
        if what == "the middle shard has no entry":
            cnt = np.diff(offsets)
            cnt[320:576] = 0
            offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
            sources = sources[:int(offsets[-1])]
        E = int(offsets[-1])
        g, g2 = gains_for(rng, ch, E), gains_for(rng, ch, E)
        assert set_feeds(lib, b, M, offsets, sources, g) == 0 and feeds_are(b, M, offsets, sources, g), (what, b.last_error())
        for K in (64, 100):   # (100 straddles the shards: only a mixed output minds)
            src = source_block(rng, (S, ch, M))
            block = feed_model(src, offsets, sources, g, g, False, S)
            want = plain.process_block(block)
            count.skip()
            assert same_words(b.process_block_bus_feed(src, K), want), (what, K, "staged")
            count.expect(what + ", unmixed", 3, 0, 3, 0, 3, 0, 3, 3)
            if K == 64:
                want = plain.process_block_bus(block, K, False, True)
                ps, po = pinned((S, ch, M)), pinned((S, ch, b.bus_groups(K)))
                ps[...] = src
                count.skip()
                assert fed(lib, b, ps, po, None, None, S, K, MIX_OUT) == 0 and same_words(po, want), (what, K, "in place")
                count.expect(what + ", mixed in place", 3, 0, 3, 3, 0, 3, 3, 3)
                pinned.free()
            else:
                po = np.zeros((S, ch, b.bus_groups(K)), dtype=np.float32)
                assert fed(lib, b, src, po, None, None, S, K, MIX_OUT) == FX_E_ARG and "straddles" in b.last_error()
        # the feed gains go to every shard's entries, and a ramp is consumed on all of them
        assert b.bus_set_feed_gains(g2, True) == 0 and feeds_are(b, M, offsets, sources, g)
        src = source_block(rng, (S, ch, M))
        assert same_words(b.process_block_bus_feed(src), plain.process_block(feed_model(src, offsets, sources, g, g2, True, S))) and feeds_are(b, M, offsets, sources, g2), what
    assert (b.save_state() == plain.save_state()).all()
    assert b.bus_set_feeds(0, None, None) == 0 and b.bus_get_feeds()[0] == 0
    assert lib.fxstub_bus_feed_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("feed shards ok")


def child_memory():
    """an allocation that fails inside a set, on whichever shard it happens: FX_E_MEMORY, the old feeds stay in force on all of
    them, nothing leaks"""
    A, lib = feed_library()
    rng = np.random.default_rng(213)
    N, S, M = 3 * 256 + 40, 5, 7
    b = A.Batch(N, 1, devices=[0, 1, 2])
    assert b.load_text(PROGRAM), b.errors()
    b.process_block_bus(signal(rng, (S, 1, b.bus_groups(64))), 64)   # (code generated, scratch and staging allocated)
    assert b.prepare(S, True) == 0
    old_off, old_src = feed_structure(rng, N, 3, counts=(1,))
    new_off, new_src = feed_structure(rng, N, M)
    old_g, new_g = gains_for(rng, 1, N), gains_for(rng, 1, int(new_off[-1]))
    src_old, src_new = source_block(rng, (S, 1, 3)), source_block(rng, (S, 1, M))
    for state in ("off", "on"):
        if state == "on":
            assert set_feeds(lib, b, 3, old_off, old_src, old_g) == 0
            b.process_block_bus_feed(src_old)   # (the device copies of the source rows exist)
        for nth in range(3):   # one allocation per shard
            live = lib.fxstub_live_allocations()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = set_feeds(lib, b, M, new_off, new_src, new_g)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY, (state, nth, rc, b.last_error())
            assert lib.fxstub_live_allocations() == live, (state, nth)
            assert feeds_are(b, 3, old_off, old_src, old_g) if state == "on" else b.bus_get_feeds()[0] == 0, (state, nth)
            if state == "on":
                assert same_words(b.process_block_bus_feed(src_old), feed_model(src_old, old_off, old_src, old_g, old_g, False, S)), (state, nth)
    assert set_feeds(lib, b, M, new_off, new_src, new_g) == 0 and feeds_are(b, M, new_off, new_src, new_g)
    assert same_words(b.process_block_bus_feed(src_new), feed_model(src_new, new_off, new_src, new_g, new_g, False, S))
    assert lib.fxstub_bus_feed_strays() == 0 and lib.fxstub_cross_device_errors() == 0
    print("feed memory ok")


if __name__ == "__main__":
    {"shared": child_shared, "routes": child_routes, "pieces": child_pieces, "state": child_state, "refusals": child_refusals, "shards": child_shards,
     "memory": child_memory}[sys.argv[1]]()
