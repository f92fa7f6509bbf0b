"""Bus sends without a GPU: the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc
stublib`), driven through the C ABI in a child process like tests/test_bus_tap_stub.py (this file is also that child).  The
stand-in of the send kernels (tests/hipstub/fx_bus_send_stub.cpp) does the real arithmetic in stream order with an addressing of
its own, so what is checked here is the definition as numpy (tree, send_model) against the existing gain_mix_model, and the host
side: the structure and its tables, which rows and columns a block's sends go to on every route (pinned in place, pageable
through the staging, the device entry, the pieces of a block above the scratch limit, three shards on the columns of their
buses), the state machine of fxb_bus_set_sends / fxb_bus_set_send_gains, that a block with sends leaves everything else as one
without does, and that a refusal changes nothing.  Words are compared as uint32: there is no tolerance anywhere.

The yardstick is an existing path: a second handle runs fxb_process_block on the expanded input and gives y.  Parity on the
device is tests/test_gpu_bus_send.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, MIX_OUT, PROGRAM, ROOT, SHARED_IN, STEREO, Pinned, expand, mix_model, same_words, stub_library  # noqa: E402
from test_bus_gain_stub import SHAPES, gain_mix_model, gain_weights, gains_for  # noqa: E402
from test_bus_tap_stub import same_bits, signal, tap_list  # noqa: E402
from route_models import CHUNK, tree, send_model  # noqa: E402,F401  (the models live there; the tests of them stay here)

SIZES = (0, 1, 63, 64, 65, 1024, 1025, 2049)   # the lane boundary, the chunk boundary, Q = 2 and Q = 3 with a one-entry last chunk
MOST_BUSES, MOST_ENTRIES = 65536, 1 << 24


def structure(rng, N, sizes):
    """CSR of buses of the given sizes: every non-empty list holds the last instance, the first one (from two entries on) and
    random ones - repeats where a list is longer than N - and is not sorted"""
    offsets, members = [0], []
    for M in sizes:
        lst = tap_list(rng, N, max(M, 3))[:M] if M else np.zeros(0, dtype=np.int64)
        members.append(lst)
        offsets.append(offsets[-1] + M)
    return np.array(offsets, dtype=np.int64), (np.concatenate(members) if members else np.zeros(0)).astype(np.int64)


def test_send_model_is_the_group_mix_on_buses_that_list_the_groups():
    """a bus per group, ascending members, the group's gains, every K <= 1 024: the words of gain_mix_model - static and ramping"""
    rng = np.random.default_rng(7)
    for N, K in SHAPES:
        k = min(K, N)
        assert k <= CHUNK
        G = -(-N // k)
        offsets = np.minimum(np.arange(G + 1) * k, N)
        members = np.arange(N)
        for C_ in (1, 2):
            for S, ramp in ((1, False), (2, True), (33, True), (33, False)):
                a, b = gains_for(rng, C_, N), gains_for(rng, C_, N)
                y = signal(rng, (S, C_, N))
                got, want = send_model(y, offsets, members, a, b, ramp, S), gain_mix_model(y, a, b, ramp, S, K)
                assert same_words(got, want), (N, K, C_, S, ramp)
                ones = np.ones((C_, N), dtype=np.float32)
                finite = np.nan_to_num(y, nan=1.0, posinf=2.0, neginf=-2.0)   # (1.0f * y is y, but the plain mix moves no NaN through a product)
                assert same_words(send_model(finite, offsets, members, ones, ones, False, S), mix_model(finite, K)), (N, K, C_, S)


def test_tree_and_the_chunks_written_out_one_add_at_a_time():
    rng = np.random.default_rng(9)
    f = np.float32

    def slow(seq):
        p = [f(0.0)] * 64
        for m, v in enumerate(seq):
            p[m % 64] = f(p[m % 64] + v)
        for step in (32, 16, 8, 4, 2, 1):
            for l in range(step):
                p[l] = f(p[l] + p[l + step])
        return p[0]

    for M in SIZES + (3000,):
        v = (rng.standard_normal(M) * 10.0 ** rng.integers(-6, 6, M)).astype(np.float32)
        w = gains_for(rng, 1, max(M, 1))[:, :M]
        want = slow([f(0.0) if g == 0.0 else f(g * x) for g, x in zip(w[0], v)][:CHUNK]) if M <= CHUNK else \
            slow([slow([f(0.0) if g == 0.0 else f(g * x) for g, x in zip(w[0, q:q + CHUNK], v[q:q + CHUNK])]) for q in range(0, M, CHUNK)])
        got = send_model(v.reshape(1, 1, M), [0, M], np.arange(M), w, w, False, 1)
        assert got.shape == (1, 1, 1) and same_bits(got[0, 0], np.array([want], dtype=np.float32)), M
    assert same_bits(tree(np.zeros((2, 0), dtype=np.float32)), np.zeros(2, dtype=np.float32)), "an empty bus is +0.0"


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_send_values_and_routes_on_the_hip_stand_in():
    run_child("routes", "send routes ok")


def test_aux_rows_of_the_pieces_of_a_block_on_the_hip_stand_in():
    run_child("pieces", "send pieces ok")


def test_send_state_machine_on_the_hip_stand_in():
    """set, replace, off, set before a load, the round trip, send gains with and without ramp, a ramp left pending, a ramp cancelled"""
    run_child("state", "send state ok")


def test_sends_leave_the_mix_taps_meters_gains_and_state_alone_on_the_hip_stand_in():
    run_child("unaffected", "send unaffected ok")


def test_send_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "send refusals ok")


def test_sends_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "send shards ok", devices=3)


def test_send_set_that_runs_out_of_memory_on_one_shard_on_the_hip_stand_in():
    run_child("memory", "send memory ok", devices=3)


def test_send_structures_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/bus_send_checks.cpp (csrc/Makefile `stubasansends`): structure shapes, the refusals and an allocation failure
    at every allocation of a set, of the chunk sums and of a staged aux_out, through the C ABI on exactly-sized heap blocks, on
    one handle and on three shards, under AddressSanitizer + UBSan + LeakSanitizer.  The program links the sanitizer runtime
    itself: nothing is preloaded and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasansends"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "bus_send_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "bus send checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def send_library():
    A, lib = stub_library()
    for f in ("fxstub_bus_taps", "fxstub_bus_tap_strays", "fxstub_bus_gain_mixes", "fxstub_live_allocations", "fxstub_bus_sends", "fxstub_bus_send_ramps", "fxstub_bus_send_strays"):
        getattr(lib, f).restype = C.c_long
    return A, lib


class SendCounts:
    """what has happened since the last look: (emulation launches, expands, mixes plain and weighted, tap launches, send launches,
    staged, in place, bus blocks, bus blocks with taps, bus blocks with sends)"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_bus_expands(), self.lib.fxstub_bus_mixes() + self.lib.fxstub_bus_gain_mixes(), self.lib.fxstub_bus_taps(),
                self.lib.fxstub_bus_sends(), self.b.info("host_staged_blocks"), self.b.info("host_inplace_blocks"), self.b.info("bus_blocks"), self.b.info("bus_tap_blocks"),
                self.b.info("bus_send_blocks"))

    def expect(self, what, *want):
        now = self.now()
        got = tuple(x - y for x, y in zip(now, self.seen))
        assert got == want, (what, got, want)
        self.seen = now

    def skip(self):
        self.seen = self.now()


NOTHING = (0,) * 10


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def auxed(lib, b, x, y, t, a, S, K, flags):
    return lib.fxb_process_block_bus_aux(b._h, ptr(x), ptr(y), ptr(t), ptr(a), S, K, flags)


def auxed_dev(lib, b, x, y, t, a, S, K, flags, stream=None):
    return lib.fxb_process_block_bus_aux_dev(b._h, ptr(x), ptr(y), ptr(t), ptr(a), S, K, flags, stream)


def set_sends(lib, b, offsets, members, gains):
    offsets, members = np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(members, dtype=np.int64)
    return lib.fxb_bus_set_sends(b._h, offsets.size - 1, ptr(offsets), ptr(members) if members.size else None, ptr(gains))


def sends_are(b, offsets, members, gains):
    off, mem, g = b.bus_get_sends()
    return (off == offsets).all() and (mem == members).all() and same_bits(g, gains)


def child_routes():
    A, lib = send_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(151)
    S = 9   # (rows of 9 and 18: a whole group of eight rows of the kernel and a ragged one)
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N, K in ((1, 1), (65, 64), (200, 63), (777, 130)):
            b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
            assert b.load_text(text) and plain.load_text(text), b.errors()
            G = b.bus_groups(K)
            count = SendCounts(lib, b)
            for sizes in ((1,), SIZES, (3,) * 65, (0, 0)):
                offsets, members = structure(rng, N, sizes)
                E, nA = int(offsets[-1]), len(sizes)
                g = gains_for(rng, ch, max(E, 1))[:, :E].copy()
                given = (offsets.copy(), members.copy(), g.copy())
                assert set_sends(lib, b, *given) == 0, b.last_error()
                for arr in given:
                    arr[...] = -1   # the caller's arrays are free on return
                assert sends_are(b, offsets, members, g)
                taps = tap_list(rng, N, 5)
                assert b.bus_set_taps(taps) == 0
                for shared in (True, False):
                    flags = MIX_OUT | (SHARED_IN if shared else 0)
                    x = signal(rng, (S, ch, G if shared else N))
                    y = plain.process_block(expand(x, K, N) if shared else x)
                    count.skip()
                    want_mix, want_aux, want_taps = mix_model(y, K), send_model(y, offsets, members, g, g, False, S), y[:, :, taps]
                    where = (ch, N, K, sizes[:3], shared)
                    # pageable: the mix and the aux rows are staged
                    out, aux = b.process_block_bus(x, K, shared, True, aux=True)
                    assert same_words(out, want_mix) and same_words(aux, want_aux), where + ("staged",)
                    count.expect("staged", 1, int(shared), 1, 0, 1, 1, 0, 1, 0, 1)
                    # ... with taps in the same block: one more element at the end of the result
                    out, tp, aux = b.process_block_bus(x, K, shared, True, taps=True, aux=True)
                    assert same_words(out, want_mix) and same_bits(tp, want_taps) and same_words(aux, want_aux), where + ("staged, tapped",)
                    count.expect("staged, tapped", 1, int(shared), 1, 1, 1, 1, 0, 1, 1, 1)
                    # pinned: everything in place
                    px, po, pt, pa = pinned(x.shape), pinned((S, ch, G)), pinned((S, ch, 5)), pinned((S, ch, nA))
                    px[...] = x
                    pa[...] = -7.0
                    assert auxed(lib, b, px, po, pt, pa, S, K, flags) == 0, b.last_error()
                    assert same_words(po, want_mix) and same_bits(pt, want_taps) and same_words(pa, want_aux), where + ("in place",)
                    count.expect("in place", 1, int(shared), 1, 1, 1, 0, 1, 1, 1, 1)
                    # pinned PCM, pageable aux rows: the two sides keep their route, the aux rows are staged
                    page = np.full((S, ch, nA), -7.0, dtype=np.float32)
                    assert auxed(lib, b, px, po, None, page, S, K, flags) == 0, b.last_error()
                    assert same_words(po, want_mix) and same_words(page, want_aux), where + ("pinned PCM, pageable aux",)
                    count.expect("pinned PCM, pageable aux", 1, int(shared), 1, 0, 1, 0, 1, 1, 0, 1)
                    # pageable PCM and tap rows, pinned aux rows
                    pa[...] = -7.0
                    out, tp = np.zeros((S, ch, G), dtype=np.float32), np.zeros((S, ch, 5), dtype=np.float32)
                    assert auxed(lib, b, x, out, tp, pa, S, K, flags) == 0, b.last_error()
                    assert same_words(out, want_mix) and same_bits(tp, want_taps) and same_words(pa, want_aux), where + ("pageable PCM, pinned aux",)
                    count.expect("pageable PCM, pinned aux", 1, int(shared), 1, 1, 1, 1, 0, 1, 1, 1)
                    # the device entry on the handle's own stream, twice (the second time: buffers that have passed once)
                    for rep in range(2):
                        pa[...] = -7.0
                        assert auxed_dev(lib, b, px, po, pt if rep else None, pa, S, K, flags) == 0 and b.sync() == 0, b.last_error()
                        assert same_words(po, want_mix) and same_words(pa, want_aux), where + ("device entry",)
                    count.expect("device entry", 2, 2 * int(shared), 2, 1, 2, 0, 0, 2, 1, 2)
                    # aux_out == NULL is fxb_process_block_bus_tap
                    assert auxed(lib, b, px, po, pt, None, S, K, flags) == 0 and same_words(po, want_mix) and same_bits(pt, want_taps)
                    count.expect("no aux rows", 1, int(shared), 1, 1, 0, 0, 1, 1, 1, 0)
                    assert auxed(lib, b, px, po, pt, pa, 0, K, flags) == 0
                    count.expect("zero samples", *NOTHING)
                    pinned.free()
            b.close()
            plain.close()
    assert lib.fxstub_bus_send_strays() == 0 and lib.fxstub_bus_tap_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("send routes ok")


def child_pieces():
    A, lib = send_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(153)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples
    N, S, K = 262144, 96, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    offsets = np.array([0, N, N + 65], dtype=np.int64)   # all instances ascending (Q = 256), and a bus of 65
    members = np.concatenate([np.arange(N), tap_list(rng, N, 65)]).astype(np.int64)
    a0, a1 = gains_for(rng, 1, N + 65), gains_for(rng, 1, N + 65)
    assert set_sends(lib, b, offsets, members, a0) == 0, b.last_error()
    count = SendCounts(lib, b)
    xg = rng.standard_normal((S, 1, G)).astype(np.float32)
    y = expand(xg, K, N)   # (the stand-in's emulation launch copies in to out; tests/test_gpu_bus_send.py runs the plain path)
    want_mix, want_aux = mix_model(y, K), send_model(y, offsets, members, a0, a0, False, S)
    out, aux = b.process_block_bus(xg, K, aux=True)
    assert same_words(out, want_mix) and same_words(aux, want_aux)
    count.expect("two pieces, staged", 2, 2, 2, 0, 2, 1, 0, 1, 0, 1)
    pg, po, pa = pinned((S, 1, G)), pinned((S, 1, G)), pinned((S, 1, 2))
    pg[...] = xg
    # a ramp across the two pieces: t goes by the sample of the CALL
    assert b.bus_set_send_gains(a1, True) == 0
    assert auxed(lib, b, pg, po, None, pa, S, K, 3) == 0 and same_words(po, want_mix) and same_words(pa, send_model(y, offsets, members, a0, a1, True, S))
    count.expect("two pieces, in place, ramping", 2, 2, 2, 0, 2, 0, 1, 1, 0, 1)
    assert lib.fxstub_bus_send_ramps() == 2
    pa[...] = -7.0
    assert auxed(lib, b, pg, po, None, pa, 65, K, 3) == 0 and same_words(pa[:65], send_model(y[:65], offsets, members, a1, a1, False, 65)) and (pa[65:] == -7.0).all()
    count.expect("65 samples: two pieces", 2, 2, 2, 0, 2, 0, 1, 1, 0, 1)
    assert b.set_register_track("vol", [0.1, 0.2], 48) == 0
    assert auxed(lib, b, pg, po, None, pa, S, K, 3) == 0 and same_words(pa, send_model(y, offsets, members, a1, a1, False, S)), b.last_error()
    count.expect("armed: one piece", 1, 1, 1, 0, 1, 0, 1, 1, 0, 1)
    assert lib.fxstub_bus_send_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("send pieces ok")


def child_state():
    A, lib = send_library()
    rng = np.random.default_rng(157)
    N, K, S, ch = 777, 130, 5, 2
    b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
    live = lib.fxstub_live_allocations()
    nA = C.c_int64(-1)
    assert lib.fxb_bus_get_sends(b._h, C.byref(nA), None, 0, None, None, 0) == 0 and nA.value == 0 and b.bus_get_sends()[1].size == 0, "off by default"
    off1, mem1 = structure(rng, N, SIZES)
    g1 = gains_for(rng, ch, int(off1[-1]))
    assert set_sends(lib, b, off1, mem1, g1) == 0, "before a program is loaded"
    assert lib.fxstub_live_allocations() == live + 1, "one device block is the only allocation of a set"
    assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()
    assert b.prepare(S, True) == 0 and plain.prepare(S, True) == 0   # (the builder threads are idle while allocations are counted)
    assert sends_are(b, off1, mem1, g1), "the sends survive a program load"
    G = b.bus_groups(K)

    def block(offsets, members, a, bb, ramp, S=S, aux=True):
        x = signal(rng, (S, ch, G))
        y = plain.process_block(expand(x, K, N))
        if not aux:
            assert same_words(b.process_block_bus(x, K), mix_model(y, K))
            return
        out, got = b.process_block_bus(x, K, aux=True)
        assert same_words(out, mix_model(y, K)) and same_words(got, send_model(y, offsets, members, a, bb, ramp, S)), (ramp, S)

    block(off1, mem1, g1, g1, False)
    # the round trip with less room than there is, and with more
    E = int(off1[-1])
    some_off, some_mem, some_g = np.full(12, -1, dtype=np.int64), np.full(10, -1, dtype=np.int64), np.full((ch, E), -7.0, dtype=np.float32)
    assert lib.fxb_bus_get_sends(b._h, C.byref(nA), ptr(some_off), 4, ptr(some_mem), ptr(some_g), 7) == E and nA.value == len(SIZES)
    assert (some_off[:4] == off1[:4]).all() and (some_off[4:] == -1).all() and (some_mem[:7] == mem1[:7]).all() and (some_mem[7:] == -1).all()
    assert same_bits(some_g[:, :7], g1[:, :7]) and (some_g[:, 7:] == -7.0).all()
    room_off, room_mem = np.full(len(SIZES) + 5, -1, dtype=np.int64), np.full(E + 5, -1, dtype=np.int64)
    assert lib.fxb_bus_get_sends(b._h, None, ptr(room_off), room_off.size, ptr(room_mem), None, E + 5) == E
    assert (room_off[:len(SIZES) + 1] == off1).all() and (room_off[len(SIZES) + 1:] == -1).all() and (room_mem[:E] == mem1).all() and (room_mem[E:] == -1).all()
    # send gains: static replaces a and b; a ramp makes the old b the a of the next block with aux rows and ends on its target
    g2, g3, g4 = gains_for(rng, ch, E), gains_for(rng, ch, E), gains_for(rng, ch, E)
    assert b.bus_set_send_gains(g2) == 0 and sends_are(b, off1, mem1, g2)
    block(off1, mem1, g2, g2, False)
    assert b.bus_set_send_gains(g3, True) == 0 and sends_are(b, off1, mem1, g2), "a while the ramp is pending"
    block(off1, mem1, None, None, False, aux=False)   # a block without aux rows leaves it pending
    assert sends_are(b, off1, mem1, g2)
    assert b.bus_set_send_gains(g4, True) == 0 and sends_are(b, off1, mem1, g2), "a second ramp set replaces the target, a stays"
    block(off1, mem1, g2, g4, True, S=33)
    assert sends_are(b, off1, mem1, g4), "consumed: the target is in force"
    block(off1, mem1, g4, g4, False, S=1)
    assert b.bus_set_send_gains(g2, True) == 0
    block(off1, mem1, g4, g2, True, S=1)   # a ramp of one sample is its target
    assert b.bus_set_send_gains(g3, True) == 0 and b.bus_set_send_gains(g1, False) == 0 and sends_are(b, off1, mem1, g1), "ramp = 0 drops a pending ramp"
    block(off1, mem1, g1, g1, False)
    # a new structure cancels a pending ramp; NULL gains are 1.0f everywhere
    assert b.bus_set_send_gains(g3, True) == 0
    off2, mem2 = structure(rng, N, (3,) * 65 + (0,))
    ones = np.ones((ch, int(off2[-1])), dtype=np.float32)
    assert set_sends(lib, b, off2, mem2, None) == 0 and sends_are(b, off2, mem2, ones), "replaced"
    block(off2, mem2, ones, ones, False)
    assert lib.fxstub_bus_send_ramps() == 2
    bad = g1.copy()
    bad[1, 5] = np.inf
    assert b._lib.fxb_bus_set_send_gains(b._h, ptr(bad[:, :ones.shape[1]].copy()), 0) == FX_E_ARG and sends_are(b, off2, mem2, ones)
    assert b._lib.fxb_bus_set_send_gains(b._h, ptr(ones), 2) == FX_E_ARG and b._lib.fxb_bus_set_send_gains(b._h, None, 0) == FX_E_ARG
    # instance calls do not touch the sends
    assert b.copy_instances([0, 1], [70, 131]) == 0 and b.reset_instances([5]) == 0 and b.sync() == 0 and sends_are(b, off2, mem2, ones)
    # off: the memory goes; blocks with aux rows are refused, others go on
    held = lib.fxstub_live_allocations()
    assert lib.fxb_bus_set_sends(b._h, 0, None, None, None) == 0 and b.bus_get_sends()[1].size == 0
    assert lib.fxstub_live_allocations() == held - 3, "the structure, the chunk sums and the staging of pageable rows are freed"
    x = signal(rng, (S, ch, G))
    t = np.zeros((S, ch, 3), dtype=np.float32)
    assert auxed(lib, b, x, np.zeros_like(x), None, t, S, K, 3) == FX_E_ARG and "sends are off" in b.last_error()
    assert lib.fxb_bus_set_send_gains(b._h, ptr(ones), 0) == FX_E_ARG and "sends are off" in b.last_error()
    block(None, None, None, None, False, aux=False)
    assert b.bus_set_sends(None, None) == 0 and b.bus_set_sends([0], []) == 0, "off twice"
    assert b.bus_set_sends(off1, mem1, g1) == 0
    block(off1, mem1, g1, g1, False)
    # the widest structure there is in buses: 65 536 of them, most of them empty
    offw = np.minimum(np.arange(MOST_BUSES + 1), 100).astype(np.int64)
    memw = rng.integers(0, N, 100).astype(np.int64)
    assert b.bus_set_sends(offw, memw) == 0 and (b.bus_get_sends()[0] == offw).all()
    block(offw, memw, np.ones((ch, 100), dtype=np.float32), np.ones((ch, 100), dtype=np.float32), False, S=1)
    sent = b.info("bus_send_blocks")
    b.close()
    plain.close()
    assert sent == 9, sent
    assert lib.fxstub_live_allocations() < live, "nothing of the sends outlives the handle"
    assert lib.fxstub_bus_send_strays() == 0
    print("send state ok")


def child_unaffected():
    """a handle with sends and one without through the same calls: the mix, the taps, the meters, the bus gains with a ramp left
    pending by a block without FXB_BUS_MIX_OUT, the state image and every counter there was before agree; the sends are pre-fader"""
    A, lib = send_library()
    rng = np.random.default_rng(159)
    N, K, ch = 200, 63, 2
    a, b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0), A.Batch(N, ch, 0)
    assert plain.load_text(STEREO), plain.errors()
    G = a.bus_groups(K)
    offsets, members = structure(rng, N, (65, 1025, 0, 3))
    sg = gains_for(rng, ch, int(offsets[-1]))
    taps = tap_list(rng, N, 65)
    assert set_sends(lib, b, offsets, members, sg) == 0
    for h in (a, b):
        assert h.load_text(STEREO), h.errors()
        assert h.meter_enable(True) == 0 and h.bus_set_taps(taps) == 0
    g0, g1, g2 = gains_for(rng, ch, N), gains_for(rng, ch, N), gains_for(rng, ch, N)
    g1[:, N - 1] = 0.0   # a voice muted on its group bus and still on every aux bus: pre-fader
    gains = g0
    for step, (S, ramp, g) in enumerate(((33, 0, g0), (1, 1, g1), (33, 1, g2), (7, None, None))):
        if g is not None:
            assert a.bus_set_gains(g, bool(ramp)) == 0 and b.bus_set_gains(g, bool(ramp)) == 0
        x = signal(rng, (S, ch, G))
        y = plain.process_block(expand(x, K, N))
        want = gain_mix_model(y, gains, g if g is not None else gains, bool(ramp), S, K)
        gains = g if g is not None else gains
        out_a, taps_a = a.process_block_bus(x, K, taps=True)
        out_b, taps_b, aux = b.process_block_bus(x, K, taps=True, aux=True)
        assert same_words(out_a, want) and same_words(out_b, out_a) and same_bits(taps_a, taps_b), step
        assert same_words(aux, send_model(y, offsets, members, sg, sg, False, S)), (step, "the bus gains and their ramp do not act on the sends")
    # a ramp of the bus gains that a block without FXB_BUS_MIX_OUT leaves pending, and a refused block with aux rows behind it
    assert a.bus_set_gains(g0, True) == 0 and b.bus_set_gains(g0, True) == 0
    x = signal(rng, (4, ch, G))
    assert same_words(a.process_block_bus(x, K, True, False), b.process_block_bus(x, K, True, False))
    t = np.zeros((4, ch, len(offsets) - 1), dtype=np.float32)
    assert auxed(lib, b, x, np.zeros((4, ch, N), dtype=np.float32), None, t, 4, K, SHARED_IN) == FX_E_ARG
    assert same_words(a.bus_get_gains(), b.bus_get_gains()) and same_words(a.bus_get_gains(), gains), "the ramp is still pending"
    out_a = a.process_block_bus(x, K)
    out_b, aux = b.process_block_bus(x, K, aux=True)
    assert same_words(out_a, gain_mix_model(expand(x, K, N), gains, g0, True, 4, K)) and same_words(out_b, out_a)
    ma, mb = a.meter_read(), b.meter_read()
    for key in ("energy", "peak", "full_scale", "nonfinite"):
        assert (ma[key].view(np.uint8) == mb[key].view(np.uint8)).all(), key
    assert mb["nonfinite"].sum() > 0 and a.meter_samples() == b.meter_samples()
    assert (a.save_state() == b.save_state()).all()
    for what in ("host_staged_blocks", "host_inplace_blocks", "bus_blocks", "meter_launches", "bus_gain_blocks", "bus_tap_blocks", "imajor_blocks", "num_rows", "kernel", "grid",
                 "xlate_code_hash"):
        assert a.info(what) == b.info(what), what
    assert a.info("bus_send_blocks") == 0 and b.info("bus_send_blocks") == 5
    print("send unaffected ok")


def child_refusals():
    A, lib = send_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(161)
    N, S, K, T = 300, 8, 64, 5
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    assert b.prepare(S, True) == 0   # (the builder thread is idle while allocations are counted)
    G = b.bus_groups(K)
    offsets, members = structure(rng, N, (65, 0, 1025, 2, 1))
    nA, E = offsets.size - 1, int(offsets[-1])
    g = gains_for(rng, 1, E)
    taps = tap_list(rng, N, T)
    assert b.bus_set_taps(taps) == 0
    xg, yg, xn, pt, pa = pinned((S, 1, G)), pinned((S, 1, G)), pinned((S, 1, N)), pinned((S, 1, T)), pinned((S, 1, nA))
    both = pinned((4 * S, 1, N))
    xg[...] = 0.5
    at = lambda a, off: C.c_void_p(a.ctypes.data + off * 4)
    page = np.zeros((S, 1, nA), dtype=np.float32)

    def untouched():
        ok = (pa == -7.0).all() and (page == -7.0).all() and (both == -7.0).all() and (pt == -7.0).all()
        pa[...] = -7.0
        page[...] = -7.0
        both[...] = -7.0
        pt[...] = -7.0
        return ok

    untouched()
    # while sends are off
    count = SendCounts(lib, b)
    for what, call in (("host entry, sends off", lambda: auxed(lib, b, xg, yg, None, pa, S, K, 3)), ("device entry, sends off", lambda: auxed_dev(lib, b, xg, yg, None, pa, S, K, 3)),
                       ("zero samples, sends off", lambda: auxed(lib, b, xg, yg, None, pa, 0, K, 3)), ("send gains, sends off", lambda: lib.fxb_bus_set_send_gains(b._h, ptr(g), 0))):
        assert call() == FX_E_ARG and "sends are off" in b.last_error(), what
        count.expect(what, *NOTHING)
        assert untouched() and b.bus_get_sends()[1].size == 0, what
    # sets that are refused: nothing changes, neither from "off" nor from a structure in force
    i64 = lambda *v: np.array(v, dtype=np.int64)
    bad_member, negative, not_finite, nan = members.copy(), members.copy(), g.copy(), g.copy()
    bad_member[E - 1], negative[0], not_finite[0, 3], nan[0, E - 1] = N, -1, np.inf, np.nan
    wide_off = np.zeros(MOST_BUSES + 2, dtype=np.int64)
    long_off = i64(0, MOST_ENTRIES + 1)
    sets = (
        ("n_aux < 0", lambda: lib.fxb_bus_set_sends(b._h, -1, ptr(offsets), ptr(members), ptr(g))),
        ("n_aux above the cap", lambda: lib.fxb_bus_set_sends(b._h, MOST_BUSES + 1, ptr(wide_off), ptr(members), None)),
        ("more entries than the cap", lambda: lib.fxb_bus_set_sends(b._h, 1, ptr(long_off), ptr(members), None)),
        ("null offsets", lambda: lib.fxb_bus_set_sends(b._h, nA, None, ptr(members), ptr(g))),
        ("null members", lambda: lib.fxb_bus_set_sends(b._h, nA, ptr(offsets), None, ptr(g))),
        ("offsets[0] != 0", lambda: lib.fxb_bus_set_sends(b._h, 2, ptr(i64(1, 2, 3)), ptr(members), None)),
        ("offsets decreasing", lambda: lib.fxb_bus_set_sends(b._h, 3, ptr(i64(0, 5, 4, 6)), ptr(members), None)),
        ("member == N", lambda: lib.fxb_bus_set_sends(b._h, nA, ptr(offsets), ptr(bad_member), ptr(g))),
        ("member < 0", lambda: lib.fxb_bus_set_sends(b._h, nA, ptr(offsets), ptr(negative), ptr(g))),
        ("an infinite gain", lambda: lib.fxb_bus_set_sends(b._h, nA, ptr(offsets), ptr(members), ptr(not_finite))),
        ("a NaN gain", lambda: lib.fxb_bus_set_sends(b._h, nA, ptr(offsets), ptr(members), ptr(nan))),
        ("null handle", lambda: lib.fxb_bus_set_sends(None, nA, ptr(offsets), ptr(members), ptr(g))),
    )
    live = lib.fxstub_live_allocations()
    for state in ("off", "on"):
        if state == "on":
            assert set_sends(lib, b, offsets, members, g) == 0
            live = lib.fxstub_live_allocations()
        for what, call in sets:
            assert call() == FX_E_ARG, (state, what)
            assert lib.fxstub_live_allocations() == live, (state, what)
            assert sends_are(b, offsets, members, g) if state == "on" else b.bus_get_sends()[0].size == 1, (state, what)
    assert lib.fxb_bus_get_sends(None, None, None, 0, None, None, 0) == FX_E_ARG and lib.fxb_bus_get_sends(b._h, None, None, -1, None, None, 0) == FX_E_ARG
    assert lib.fxb_bus_get_sends(b._h, None, None, 0, None, None, -1) == FX_E_ARG
    assert auxed(lib, b, xg, yg, pt, pa, S, K, 3) == 0, b.last_error()
    ms = b.last_kernel_ms()
    want_aux = send_model(expand(xg, K, N), offsets, members, g, g, False, S)
    assert same_words(pa, want_aux)
    untouched()
    count = SendCounts(lib, b)
    rows = S * nA   # words of the aux rows
    refused = [
        ("no FXB_BUS_MIX_OUT", lambda: auxed(lib, b, xg, xn, None, pa, S, K, SHARED_IN)), ("no flags", lambda: auxed(lib, b, xn, xn, None, pa, S, K, 0)),
        ("no FXB_BUS_MIX_OUT, device entry", lambda: auxed_dev(lib, b, xg, xn, None, pa, S, K, SHARED_IN)),
        ("no FXB_BUS_MIX_OUT, zero samples", lambda: auxed(lib, b, xg, xn, None, pa, 0, K, SHARED_IN)),
        # aux rows that share a byte with the input, the output or the tap rows
        ("aux rows == in", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, 0), S, K, MIX_OUT)),
        ("aux rows == out", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, 2 * S * N), S, K, MIX_OUT)),
        ("last aux word on the first of in", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, rows - 1), at(both, 2 * S * N), None, at(both, 0), S, K, MIX_OUT)),
        ("first aux word on the last of in", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, S * N - 1), S, K, MIX_OUT)),
        ("first aux word on the last of out", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, 2 * S * N + S * G - 1), S, K, MIX_OUT)),
        ("aux rows == tap rows", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), at(both, 3 * S * N), at(both, 3 * S * N), S, K, MIX_OUT)),
        ("first aux word on the last tap word", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), at(both, 3 * S * N), at(both, 3 * S * N + S * T - 1), S, K, MIX_OUT)),
        ("last aux word on the first tap word, device entry",
         lambda: lib.fxb_process_block_bus_aux_dev(b._h, at(both, 0), at(both, 2 * S * N), at(both, 3 * S * N + rows - 1), at(both, 3 * S * N), S, K, MIX_OUT, None)),
        # every refusal the tap entry has
        ("group 0", lambda: auxed(lib, b, xg, yg, pt, pa, S, 0, 3)), ("unknown flag", lambda: auxed(lib, b, xg, yg, pt, pa, S, K, 7)),
        ("null in", lambda: auxed(lib, b, None, yg, pt, pa, S, K, 3)), ("null out", lambda: auxed(lib, b, xg, None, pt, pa, S, K, 3)),
        ("negative length", lambda: auxed(lib, b, xg, yg, pt, pa, -1, K, 3)),
        ("in and out overlap", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 3), ptr(pt), ptr(pa), S, K, 3)),
        ("tap rows over the input", lambda: lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), at(both, 0), ptr(pa), S, K, MIX_OUT)),
        ("device entry, group 0", lambda: auxed_dev(lib, b, xg, yg, pt, pa, S, 0, 3)), ("device entry, null", lambda: auxed_dev(lib, b, None, yg, pt, pa, S, K, 3)),
        ("device entry, pageable in", lambda: auxed_dev(lib, b, np.zeros((S, 1, G), dtype=np.float32), yg, pt, pa, S, K, 3)),
        ("device entry, pageable tap rows", lambda: auxed_dev(lib, b, xg, yg, np.zeros((S, 1, T), dtype=np.float32), pa, S, K, 3)),
        # aux rows the device cannot address over the whole block
        ("device entry, pageable aux rows", lambda: auxed_dev(lib, b, xg, yg, pt, page, S, K, 3)),
        ("device entry, aux rows beyond their allocation", lambda: lib.fxb_process_block_bus_aux_dev(b._h, ptr(xg), ptr(yg), None, at(pa, 1), S, K, 3, None)),
        ("null handle", lambda: lib.fxb_process_block_bus_aux(None, ptr(xg), ptr(yg), ptr(pt), ptr(pa), S, K, 3)),
    ]
    for what, call in refused:
        assert call() == FX_E_ARG, (what, b.last_error())
        count.expect(what, *NOTHING)
        assert untouched(), what
        assert sends_are(b, offsets, members, g) and b.last_kernel_ms() == ms, what
    # ... and blocks that touch without overlapping are not among them; the next block with aux rows is right
    assert lib.fxb_process_block_bus_aux(b._h, at(both, rows), at(both, 2 * S * N), None, at(both, 0), S, K, MIX_OUT) == 0, b.last_error()
    assert lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), at(both, 3 * S * N), at(both, 3 * S * N + S * T), S, K, MIX_OUT) == 0, b.last_error()
    assert auxed_dev(lib, b, xg, yg, pt, pa, S, K, 3) == 0 and b.sync() == 0 and same_words(pa, want_aux), b.last_error()
    # a staged aux block that cannot be had: FX_E_MEMORY, nothing launched, the handle goes on
    count = SendCounts(lib, b)
    page[...] = -7.0
    lib.fxstub_fail_mallocs(0, 1)
    rc = auxed(lib, b, xg, yg, None, page, S, K, 3)
    lib.fxstub_fail_mallocs(-1, 0)
    assert rc == FX_E_MEMORY and (page == -7.0).all(), b.last_error()
    count.expect("staging refused", *NOTHING)
    assert auxed(lib, b, xg, yg, None, page, S, K, 3) == 0 and same_words(page, want_aux), b.last_error()
    # ... and the chunk sums of a larger structure
    off2, mem2 = structure(rng, N, (2049, 2049))   # (six chunks: more than the five there was room for)
    assert set_sends(lib, b, off2, mem2, None) == 0
    count = SendCounts(lib, b)
    pa2 = pinned((S, 1, 2))
    pa2[...] = -7.0
    lib.fxstub_fail_mallocs(0, 1)
    rc = auxed(lib, b, xg, yg, None, pa2, S, K, 3)
    lib.fxstub_fail_mallocs(-1, 0)
    assert rc == FX_E_MEMORY and (pa2 == -7.0).all(), b.last_error()
    count.expect("chunk sums refused", *NOTHING)
    ones = np.ones((1, int(off2[-1])), dtype=np.float32)
    assert auxed(lib, b, xg, yg, None, pa2, S, K, 3) == 0 and same_words(pa2, send_model(expand(xg, K, N), off2, mem2, ones, ones, False, S)), b.last_error()
    # a handle of several shards has no device entry (here: one device, three shards)
    three = A.Batch(N, 1, devices=[0, 0, 0])
    assert three.load_text(PROGRAM) and three.bus_set_sends([0, 2], [1, 2]) == 0
    k0 = lib.fxstub_kernels_run()
    assert auxed_dev(lib, three, xg, yg, None, pa2, S, K, 3) == FX_E_ARG and lib.fxstub_kernels_run() == k0
    assert lib.fxstub_bus_send_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("send refusals ok")


def child_shards():
    A, lib = send_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(167)
    N, S, ch = 3 * 256 + 40, 9, 2
    b, plain = A.Batch(N, ch, devices=[0, 1, 2]), A.Batch(N, ch, 0)
    bounds = [(0, 320), (320, 576), (576, N)]
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()

    def within(shard, M):
        lo, hi = bounds[shard]
        lst = rng.integers(lo, hi, M)
        if M >= 2:
            lst[0], lst[1] = hi - 1, lo
        return lst.astype(np.int64)

    def build(spec):
        lists = [within(s, M) if M else np.zeros(0, dtype=np.int64) for s, M in spec]
        return np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.int64), np.concatenate(lists).astype(np.int64)

    structures = {
        "buses on every shard, interleaved": ([(2, 65), (0, 1025), (1, 3), (0, 0), (2, 2049), (1, 64), (0, 1)], 3),
        "the middle shard has none": ([(2, 5), (0, 70), (2, 1), (0, 2)], 2),
        "only empty buses and one on the last shard": ([(0, 0), (2, 130), (0, 0)], 2),   # (empty buses go to the first shard: it writes their +0.0f)
        "65 buses of the last shard": ([(2, 3)] * 65, 1),
    }
    count = SendCounts(lib, b)
    for what, (spec, owners) in structures.items():
        offsets, members = build(spec)
        nA, E = len(spec), int(offsets[-1])
        g, g2 = gains_for(rng, ch, E), gains_for(rng, ch, E)
        assert set_sends(lib, b, offsets, members, g) == 0 and sends_are(b, offsets, members, g), (what, b.last_error())
        for K in (64, 32):
            G = b.bus_groups(K)
            x = signal(rng, (S, ch, G))
            y = plain.process_block(expand(x, K, N))
            count.skip()
            want_mix, want_aux = mix_model(y, K), send_model(y, offsets, members, g, g, False, S)
            px, po, pa = pinned((S, ch, G)), pinned((S, ch, G)), pinned((S, ch, nA))
            px[...] = x
            pa[...] = -7.0
            assert auxed(lib, b, px, po, None, pa, S, K, 3) == 0, (what, b.last_error())
            assert same_words(po, want_mix) and same_words(pa, want_aux), (what, K, "in place")
            # (a shard launches the send kernels only for buses of its own, and writes only their columns)
            count.expect(what + ", in place", 3, 3, 3, 0, owners, 0, 3, 3, 0, 3)
            out, aux = b.process_block_bus(x, K, aux=True)
            assert same_words(out, want_mix) and same_words(aux, want_aux), (what, K, "staged")
            count.expect(what + ", staged", 3, 3, 3, 0, owners, 3, 0, 3, 0, 3)
            page = np.full((S, ch, nA), -7.0, dtype=np.float32)
            assert auxed(lib, b, px, po, None, page, S, K, 3) == 0 and same_words(page, want_aux), (what, K, "pinned PCM, pageable aux")
            count.expect(what + ", pinned PCM, pageable aux", 3, 3, 3, 0, owners, 0, 3, 3, 0, 3)
            pinned.free()
        # the send gains go to every shard's entries, and a ramp is consumed on all of them
        assert b.bus_set_send_gains(g2, True) == 0 and sends_are(b, offsets, members, g)
        x = signal(rng, (S, ch, b.bus_groups(64)))
        y = plain.process_block(expand(x, 64, N))
        out, aux = b.process_block_bus(x, 64, aux=True)
        assert same_words(aux, send_model(y, offsets, members, g, g2, True, S)) and sends_are(b, offsets, members, g2), what
    # a bus whose members fall into two shards is refused, by name, and nothing changes
    offsets, members = build(structures["the middle shard has none"][0])
    g = gains_for(rng, ch, int(offsets[-1]))
    assert set_sends(lib, b, offsets, members, g) == 0
    live = lib.fxstub_live_allocations()
    straddling = members.copy()
    straddling[offsets[2] - 1] = 319   # the last entry of bus 1 ... is fine: bus 1 is of the first shard
    assert set_sends(lib, b, offsets, straddling, g) == 0 and set_sends(lib, b, offsets, members, g) == 0
    straddling[offsets[2] - 1] = 320
    assert set_sends(lib, b, offsets, straddling, g) == FX_E_ARG and "aux bus 1 " in b.last_error() and "more than one shard" in b.last_error(), b.last_error()
    assert lib.fxstub_live_allocations() == live and sends_are(b, offsets, members, g)
    # refusals that go by the whole batch launch nothing on any shard
    count = SendCounts(lib, b)
    px, po, pa = pinned((S, ch, N)), pinned((S, ch, N)), pinned((S, ch, 4))
    assert auxed(lib, b, px, po, None, pa, S, 100, 3) == FX_E_ARG and "straddles" in b.last_error()
    assert auxed(lib, b, px, po, None, pa, S, 64, SHARED_IN) == FX_E_ARG and auxed_dev(lib, b, px, po, None, pa, S, 64, 3) == FX_E_ARG
    assert lib.fxb_process_block_bus_aux(b._h, ptr(px), ptr(po), None, ptr(px), S, 64, MIX_OUT) == FX_E_ARG
    count.expect("refused", *NOTHING)
    assert b.bus_set_sends(None, None) == 0 and b.bus_get_sends()[1].size == 0
    assert auxed(lib, b, px, po, None, pa, S, 64, 3) == FX_E_ARG
    count.expect("refused, sends off", *NOTHING)
    assert lib.fxstub_bus_send_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("send shards ok")


def child_memory():
    """an allocation that fails inside a set, on whichever shard it happens: FX_E_MEMORY, the old sends stay in force on all of
    them, nothing leaks"""
    A, lib = send_library()
    rng = np.random.default_rng(171)
    N, S, K = 3 * 256 + 40, 5, 64
    b = A.Batch(N, 1, devices=[0, 1, 2])
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    x = signal(rng, (S, 1, G))
    b.process_block_bus(x, K)   # (code generated, scratch and staging allocated)
    assert b.prepare(S, True) == 0   # (... and the builder thread is idle: nothing else allocates while allocations are counted)
    old_off, old_mem = np.array([0, 2, 4, 5], dtype=np.int64), np.array([807, 576, 0, 1, 400], dtype=np.int64)
    new_off = np.array([0, 70, 1100, 1103], dtype=np.int64)
    new_mem = np.concatenate([rng.integers(0, 320, 70), rng.integers(320, 576, 1030), rng.integers(576, N, 3)]).astype(np.int64)
    old_g, new_g = gains_for(rng, 1, 5), gains_for(rng, 1, 1103)
    y = expand(x, K, N)
    for state in ("off", "on"):
        if state == "on":
            assert set_sends(lib, b, old_off, old_mem, old_g) == 0
        for nth in range(3):   # one allocation per shard
            live = lib.fxstub_live_allocations()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = set_sends(lib, b, new_off, new_mem, new_g)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY, (state, nth, rc, b.last_error())
            assert lib.fxstub_live_allocations() == live, (state, nth)
            assert sends_are(b, old_off, old_mem, old_g) if state == "on" else b.bus_get_sends()[0].size == 1, (state, nth)
            if state == "on":
                out, aux = b.process_block_bus(x, K, aux=True)
                assert same_words(aux, send_model(y, old_off, old_mem, old_g, old_g, False, S)), (state, nth)
    assert set_sends(lib, b, new_off, new_mem, new_g) == 0 and sends_are(b, new_off, new_mem, new_g)
    out, aux = b.process_block_bus(x, K, aux=True)
    assert same_words(aux, send_model(y, new_off, new_mem, new_g, new_g, False, S)) and same_words(out, mix_model(y, K))
    assert lib.fxstub_bus_send_strays() == 0 and lib.fxstub_cross_device_errors() == 0
    print("send memory ok")


if __name__ == "__main__":
    {"routes": child_routes, "pieces": child_pieces, "state": child_state, "unaffected": child_unaffected, "refusals": child_refusals, "shards": child_shards,
     "memory": child_memory}[sys.argv[1]]()
