"""Delay-line windows by list without a GPU: fxb_set_tram_list / fxb_get_tram_list on the library's host sources linked against
tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like
tests/test_register_list_stub.py (this file is also that child).  The stand-ins of the two kernels
(tests/hipstub/fx_tram_stub.cpp) move the words in stream order with an addressing of their own.

The model is a TWIN handle that receives the same words through fxb_save_instances, an edit of the record words
stateRows (+ iSlots) + slot, and fxb_load_instances - the parent's only way to the same effect.  Which slot a logical index means
is worked out here in numpy from fxb_get_cursors_i with `%`, for the reference addressing and for FX_OPT_TRAM_DANE.  After every
step fxb_get_tram_i of every instance, the whole save_state() image and a block's output are compared; there is no tolerance.
The stand-in's emulation launch copies its input and moves no position: positions that differ per instance are loaded with the
state image.  Parity with the emulation itself is tests/test_gpu_tram_list.py.  The Python-driven cases do not run under a
sanitizer: that is tests/hipstub/tram_list_checks.cpp, a program of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, ROOT, Pinned, same_words  # noqa: E402
from test_bus_tap_stub import same_bits  # noqa: E402
from test_instances_rot_stub import LONG, OFFSET, PLAIN, filled, handle, rings  # noqa: E402

FX_E_NOTREADY = -2
LOGICAL, BROADCAST = 1, 2
N = 200
RINGS = [1, 7, 11, 63, 64, 65, 500]
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7149f2ca, 0xf149f2ca, 0x7fc12345, 0x7f812345, 0x3fc00000], dtype=np.uint32)
#          +0, -0, the smallest and the largest denormal (the latter negative), +-1e30, a quiet NaN with a payload, a signalling NaN, 1.5
SCRATCH = 64 << 20


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("cols", (64, 128, 256))
def test_windows_equal_the_twin_on_the_hip_stand_in(cols):
    """ring sizes 1, 7, 11, 63, 64, 65, 500; n_words 1, 63, 64, 65, Z; lists of 1, {0, N-1}, 63, 64, 65 and all N; both addressings"""
    run_child("twin-%d" % cols, "tram list twin ok")


def test_broadcast_equals_the_set_of_repeated_windows_on_the_hip_stand_in():
    run_child("broadcast", "tram list broadcast ok")


def test_window_set_behind_a_block_on_another_stream_on_the_hip_stand_in():
    run_child("streams", "tram list streams ok")


def test_window_call_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "tram list refusals ok")


def test_window_calls_above_the_staging_limit_run_in_pieces_on_the_hip_stand_in():
    run_child("pieces", "tram list pieces ok")


def test_window_calls_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "tram list shards ok", devices=3)


def test_window_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/tram_list_checks.cpp (csrc/Makefile `stubasantramlist`): window and list shapes through the C ABI on
    exactly-sized heap blocks, both addressings, the refusals and the allocation failures, on one handle and on three shards, under
    AddressSanitizer + UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded and no
    interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasantramlist"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "tram_list_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "tram list checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def list_library():
    import test_instances_rot_stub as rot
    base, A, lib = rot.stub_library()
    for f in ("fxstub_tram_scatters", "fxstub_tram_gathers", "fxstub_tram_strays", "fxstub_live_allocations", "fxstub_bad_pcm_launches"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return base, A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def raw_set(lib, b, which, L, first, n_words, v, flags, count=None):
    return lib.fxb_set_tram_list(b._h, which, ptr(L), (0 if L is None else L.size) if count is None else count, first, n_words, ptr(v), flags)


def raw_get(lib, b, which, L, first, n_words, v, flags, count=None):
    return lib.fxb_get_tram_list(b._h, which, ptr(L), (0 if L is None else L.size) if count is None else count, first, n_words, ptr(v), flags)


def lists_of(rng, n):
    """the lists of the issue over 0..n-1: one entry; {0, n-1}; 63, 64 and 65 entries around a wavefront's width, the first and the
    last instance among them; all n in a shuffled order"""
    out = [[n // 2], [0, n - 1]]
    for k in (63, 64, 65):
        out.append(np.concatenate([[n - 1], rng.permutation(np.arange(1, n - 1))[:k - 2], [0]]))
    out.append(rng.permutation(n))
    return [np.asarray(L, dtype=np.int64) for L in out]


def windows_for(rng, count, n_words):
    """[count, n_words] float32 holding random 32-bit patterns; the specials walk through the first words of every window"""
    v = rng.integers(0, 1 << 32, (count, n_words), dtype=np.uint64).astype(np.uint32)
    for i in range(count):
        m = min(n_words, SPECIALS.size)
        v[i, :m] = np.roll(SPECIALS, i)[:m]
    return v.view(np.float32)


def slots_of(b, which, L, Z, first, n_words, logical, dane):
    """[count, n_words]: the slot of every window word, per listed instance, from the definition in include/fx8010_amd.h"""
    a = first + np.arange(n_words, dtype=np.int64)
    if not logical:
        return np.tile(a, (len(L), 1))
    p = np.array([b.get_cursors_i(int(i))[2 * which] for i in L], dtype=np.int64)[:, None]
    return (p + 1 + a) % Z if dane else (p - 1 - a) % Z


class Twin:
    """a handle that takes windows by list beside one that takes the same words through save_instances / edit / load_instances"""

    def __init__(self, base, A, lib, text, n, cols, rng, seed, positions, dane=False, devices=None):
        self.base, self.lib, self.n, self.rng, self.dane = base, lib, n, rng, dane
        self.b = handle(A, text, n, cols, devices=devices, dane=dane)
        self.t = handle(A, text, n, cols, dane=dane)
        self.img, _ = filled(base, A, self.b, text, seed, positions)
        filled(base, A, self.t, text, seed, positions)
        self.sizes = (self.b.info("itram_slots"), self.b.info("xtram_slots"))

    def set(self, which, L, first, v, logical, broadcast=False, slots=None):
        """v: [count, n_words], or with broadcast [n_words]; slots: worked out by the caller (reading the positions waits for the queued blocks)"""
        L = np.ascontiguousarray(L, dtype=np.int64)
        v = np.ascontiguousarray(v, dtype=np.float32)
        n_words = v.shape[-1]
        rows = np.tile(v, (L.size, 1)) if broadcast else v
        if slots is None:
            slots = slots_of(self.b, which, L, self.sizes[which], first, n_words, logical, self.dane)
        given_L, given_v = L.copy(), v.copy()
        shards = len(self.b.shards())
        before, ran = self.b.info("tram_list_sets"), self.lib.fxstub_tram_scatters()
        flags = (LOGICAL if logical else 0) | (BROADCAST if broadcast else 0)
        assert raw_set(self.lib, self.b, which, given_L, first, n_words, given_v, flags) == 0, self.b.last_error()
        given_L[...] = -5            # the arrays are the caller's again on return
        given_v.view(np.uint32)[...] = 0xdeadbeef
        launched = self.b.info("tram_list_sets") - before
        assert 1 <= launched <= shards and (shards > 1 or launched == 1), launched
        W = self.img.words
        image = self.t.save_instances(L)
        rec = self.base.instance_records(image, W)
        off = self.img.rows + (self.img.islots if which else 0)
        for i in range(L.size):
            rec[i, off + slots[i]] = rows[i].view(np.uint32)
        assert self.t.load_instances(L, image) == 0
        return ran + launched

    def same(self, what, S=3):
        for which in (0, 1):
            A = self.sizes[which]
            if A:
                for i in range(self.n):
                    assert same_bits(self.b.get_tram_i(which, i, A), self.t.get_tram_i(which, i, A)), (what, which, i)
        assert (self.b.save_state() == self.t.save_state()).all(), what
        x = self.rng.standard_normal((S, self.n)).astype(np.float32)
        assert same_words(self.b.process_block(x), self.t.process_block(x)), what

    def same_get(self, which, L, first, n_words, logical, what):
        L = np.asarray(L, dtype=np.int64)
        got = self.b.get_tram_list(which, L, first, n_words, logical=logical)
        assert got.shape == (L.size, n_words)
        slots = slots_of(self.b, which, L, self.sizes[which], first, n_words, logical, self.dane)
        for i, inst in enumerate(L):
            line = self.t.get_tram_i(which, int(inst), self.sizes[which])
            assert same_bits(got[i], line[slots[i]]), (what, i, inst)
            if not logical:
                assert same_bits(got[i], self.b.get_tram_i(which, int(inst), first + n_words)[first:]), (what, i, inst)

    def close(self):
        self.b.close()
        self.t.close()


def positions_at(n, zi, zx, first):
    """positions [n, 4]: the write position of instance i is where the wrap of a logical window that begins at `first` falls at
    window word 0, 1, 2, 62, 63, 64, 65, 66 or 100 (mod the size) - the start of, inside and the end of a word tile of 64 - and
    then at every further place (instance numbers times 7); the read positions stand elsewhere"""
    wraps = np.array([0, 1, 2, 62, 63, 64, 65, 66, 100], dtype=np.int64)
    at = np.where(np.arange(n) < 3 * wraps.size, wraps[np.arange(n) % wraps.size], np.arange(n) * 7)
    return np.stack([(at + first) % zi, (at * 3 + 1) % zi, (at + first) % zx, (at * 5 + 2) % zx], axis=1)


def child_twin(cols):
    base, A, lib = list_library()
    rng = np.random.default_rng(500 + cols)
    gathers0, step = lib.fxstub_tram_gathers(), 0
    total_gets = 0
    for dane in (False, True):
        pairs = list(zip(RINGS, RINGS[1:] + RINGS[:1]))
        if dane:
            pairs = [(7, 11), (64, 65), (500, 63)]
        for zi, zx in pairs:
            text = rings(zi, zx)
            w = Twin(base, A, lib, text, N, cols, rng, 1000 * zi + zx, positions_at(N, zi, zx, 3), dane=dane)
            assert w.b.info("instance_rings") == 3 and w.sizes == (zi, zx) and w.b.info("inst_per_lane") == cols // 64
            lists = lists_of(rng, N)
            for which, Z in ((0, zi), (1, zx)):
                for n_words in sorted({1, 63, 64, 65, Z}):
                    if n_words > Z:
                        continue
                    # (first, the list and the block length cycle on one counter: every (ring, n_words, mode) meets ONE first and ONE
                    # list - a diagonal through the cross product, not all of it.  Where the wrap falls does not hang on that: the
                    # per-instance positions of positions_at() put it at the start of, inside and at the end of a word tile)
                    for logical in (True, False):
                        firsts = sorted({0, 3 % Z, Z - 1, Z // 2}) if logical else sorted({0, (Z - n_words) // 2, Z - n_words})
                        first = firsts[step % len(firsts)]
                        L = lists[step % len(lists)]
                        step += 1
                        what = (cols, dane, zi, zx, which, n_words, first, logical, L.size)
                        ran = w.set(which, L, first, windows_for(rng, L.size, n_words), logical)
                        w.same_get(which, L[:65], first, n_words, logical, what)   # (synchronous: the set has run)
                        assert lib.fxstub_tram_scatters() == ran, what
                        w.same(what, (33, 1, 2)[step % 3])
            total_gets += w.b.info("tram_list_gets")
            # repeats are fine in a get; count == 0 and, in physical mode, n_words == 0 return 0 and launch nothing
            L = np.array([7, 7, 0, N - 1, 7], dtype=np.int64)
            got = w.b.get_tram_list(1, L, 0, zx, logical=True)
            assert same_bits(got[0], got[1]) and same_bits(got[0], got[4])
            total_gets += 1
            sets = (w.b.info("tram_list_sets"), w.b.info("tram_list_gets"))
            assert raw_set(lib, w.b, 0, None, 0, 1, None, 0) == 0 and raw_get(lib, w.b, 1, None, 0, 1, None, LOGICAL) == 0
            assert raw_set(lib, w.b, 0, L[:1].copy(), 0, 0, None, 0) == 0 and raw_get(lib, w.b, 0, L, zi, 0, None, 0) == 0
            assert (w.b.info("tram_list_sets"), w.b.info("tram_list_gets")) == sets
            w.same("after the empty calls")
            w.close()
    assert lib.fxstub_tram_gathers() - gathers0 == total_gets
    # a line that is no ring beside one that is (xTRAM written at offset 3: 503 slots for a line of 500): physical windows reach
    # every allocated slot, the ring takes logical ones
    w = Twin(base, A, lib, OFFSET, N, cols, rng, 77, positions_at(N, 64, 500, 0))
    assert w.b.info("instance_rings") == 1 and w.sizes == (64, 503)
    L = lists_of(rng, N)[4]
    w.set(1, L, 438, windows_for(rng, L.size, 65), False)
    w.same_get(1, L, 438, 65, False, "the last slots of a line that is no ring")
    w.set(0, L, 60, windows_for(rng, L.size, 64), True)
    w.same_get(0, L, 60, 64, True, "the ring beside it")
    w.same("a line that is no ring")
    w.close()
    assert lib.fxstub_tram_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("tram list twin ok")


def child_broadcast():
    base, A, lib = list_library()
    rng = np.random.default_rng(521)
    for dane in (False, True):
        w = Twin(base, A, lib, rings(64, 500), N, 64, rng, 5, positions_at(N, 64, 500, 0), dane=dane)
        for which, first, n_words, logical in ((1, 0, 500, True), (1, 499, 130, True), (0, 1, 63, False), (1, 100, 400, False), (0, 63, 64, True)):
            for L in lists_of(rng, N):
                one = windows_for(rng, 1, n_words)[0]
                w.set(which, L, first, one, logical, broadcast=True)
                got = w.b.get_tram_list(which, L, first, n_words, logical=logical)
                assert same_bits(got, np.tile(one, (L.size, 1))), (which, first, n_words, logical, L.size)
            w.same((which, first, n_words, logical))
        # the burst of a note-on and the zeros that cut a tail, through the Python methods
        burst = windows_for(rng, 1, 64)[0]
        assert w.b.set_tram_list(0, [3, 150], 0, burst, logical=True) == 0
        assert same_bits(w.b.get_tram_list(0, [150, 3], 0, 64, logical=True), np.tile(burst, (2, 1)))
        assert w.b.set_tram_list(1, [3], 0, np.zeros(500, dtype=np.float32)) == 0
        assert not w.b.get_tram_i(1, 3, 500).view(np.uint32).any() and w.b.get_tram_i(1, 4, 500).view(np.uint32).any()
        w.close()
    assert lib.fxstub_tram_strays() == 0
    print("tram list broadcast ok")


def child_streams():
    """a window set behind a slow block on stream A returns while that block is still running (its last output row still holds the
    mark it was given) and has not run yet; a block on stream B and a get behind it wait for it"""
    base, A, lib = list_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(523)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    n, S = 1000, 8
    SLOW = 150000   # the emulation launch takes 150 ms: a set that waits for the block in front of it is caught, and so is one that is not ordered behind it
    w = Twin(base, A, lib, rings(64, 500), n, 64, rng, 9, positions_at(n, 64, 500, 0))
    w.set(1, np.array([1, 2], dtype=np.int64), 0, windows_for(rng, 2, 500), True)   # (code and staging exist before anything is timed)
    w.same("warm-up", S)

    def fresh():
        p, o = pinned((S, 1, n)), pinned((S, 1, n))
        p[...] = rng.standard_normal((S, 1, n)).astype(np.float32)
        o[...] = -7.0
        return p, o

    def dev(bufs, stream):
        return lib.fxb_process_block_dev(w.b._h, ptr(bufs[0]), ptr(bufs[1]), S, stream)

    first, second, third = fresh(), fresh(), fresh()
    L = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:63]]).astype(np.int64)
    v1, v2 = windows_for(rng, L.size, 300), windows_for(rng, L.size, 300)
    slots = slots_of(w.b, 1, L, 500, 450, 300, True, False)
    lib.fxstub_set_kernel_micros(SLOW)
    assert dev(first, streams[0]) == 0
    ran = w.set(1, L, 450, v1, True, slots=slots)
    assert (first[1][S - 1] == -7.0).all(), "the window set returned while the block in front of it was still running"
    assert lib.fxstub_tram_scatters() == ran - 1, "... and it is queued behind that block: it has not run"
    lib.fxstub_set_kernel_micros(150)
    assert dev(second, streams[1]) == 0
    got = w.b.get_tram_list(1, L, 450, 300, logical=True)   # waits for everything queued
    assert lib.fxstub_tram_scatters() == ran and not (first[1][S - 1] == -7.0).any(), "the get waited for the set, the set for the block"
    assert same_bits(got, v1)
    # a second set, a block on the default stream, sync
    ran = w.set(1, L[::-1].copy(), 450, v2, True, slots=slots[::-1])
    assert dev(third, None) == 0
    assert w.b.sync() == 0 and lib.fxstub_tram_scatters() == ran
    for bufs in (first, second, third):
        assert same_words(bufs[1], bufs[0])   # (the stand-in's emulation launch copies its input)
    assert same_bits(w.b.get_tram_list(1, L[::-1].copy(), 450, 300, logical=True), v2)
    w.same("after the streams", S)
    # every call that touches state observes a window set that is still queued behind a slow block
    for name, call in (("get_tram_i", lambda h: h.get_tram_i(1, 0, 500)), ("save_state", lambda h: h.save_state()), ("copy_instances", lambda h: h.copy_instances([0], [9])),
                       ("save_instances", lambda h: h.save_instances([0, n - 1]))):
        lib.fxstub_set_kernel_micros(30000)
        assert dev(first, streams[0]) == 0
        ran = w.set(1, L, 17, windows_for(rng, L.size, 65), False)
        lib.fxstub_set_kernel_micros(150)
        call(w.b)
        assert lib.fxstub_tram_scatters() == ran, name
        call(w.t)
        assert w.b.sync() == 0
        w.same(name + " behind a queued window set", S)
    pinned.free()
    w.close()
    assert lib.fxstub_tram_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("tram list streams ok")


def refusals_of(n, zi, ax, good_L, good_v, out):
    """(what, fn name, words the message must hold, which, L, first, n_words, values, flags, count) - iTRAM a ring of zi, xTRAM no ring with ax slots"""
    twice = np.array([5, 9, 5], dtype=np.int64)
    big = np.zeros(1, dtype=np.int64)
    cases = [("an instance listed twice", "set", "entry 2", 0, twice, 0, 4, good_v, 0, None),
             ("an instance listed twice, logical", "set", "entry 2", 0, twice, 0, 4, good_v, LOGICAL, None),
             ("broadcast on a get", "get", "flags", 0, good_L, 0, 4, out, BROADCAST, None)]
    for fn, v in (("set", good_v), ("get", out)):
        cases += [
            ("an instance of N", fn, "entry 1", 0, np.array([0, n, 1], dtype=np.int64), 0, 4, v, 0, None),
            ("an instance of -1", fn, "entry 2", 0, np.array([0, 1, -1], dtype=np.int64), 0, 4, v, LOGICAL, None),
            ("count < 0", fn, "count", 0, good_L, 0, 4, v, 0, -1),
            ("count = 2^31", fn, "count", 0, big, 0, 4, v, 0, 1 << 31),
            ("a null list", fn, "list", 0, None, 0, 4, v, 0, 3),
            ("null values", fn, "values", 0, good_L, 0, 4, None, 0, None),
            ("which = 2", fn, "which", 2, good_L, 0, 4, v, 0, None),
            ("which = -1", fn, "which", -1, good_L, 0, 4, v, 0, None),
            ("an unknown flag bit", fn, "flags", 0, good_L, 0, 4, v, 4, None),
            ("an unknown high flag bit", fn, "flags", 0, good_L, 0, 4, v, 1 << 31, None),
            ("first < 0", fn, "first", 0, good_L, -1, 4, v, 0, None),
            ("n_words < 0", fn, "n_words", 0, good_L, 0, -1, v, 0, None),
            ("n_words = 0, logical", fn, "n_words", 0, good_L, 0, 0, v, LOGICAL, None),
            ("physical: one word past the slots", fn, "n_words", 0, good_L, zi - 3, 4, v, 0, None),
            ("physical: first at the end", fn, "first", 0, good_L, zi, 1, v, 0, None),
            ("physical: one word past the slots of the line that is no ring", fn, "n_words", 1, good_L, ax - 3, 4, v, 0, None),
            ("logical: first = Z", fn, "first", 0, good_L, zi, 1, v, LOGICAL, None),
            ("logical: n_words = Z + 1", fn, "n_words", 0, good_L, 0, zi + 1, v, LOGICAL, None),
            ("logical on a line that is no ring", fn, "ring", 1, good_L, 0, 4, v, LOGICAL, None),
        ]
    return cases


def child_refusals():
    base, A, lib = list_library()
    rng = np.random.default_rng(541)
    fns = {"set": raw_set, "get": raw_get}
    good_L = np.array([3, 0, N - 1], dtype=np.int64)
    good_v = windows_for(rng, 3, 65 * 3)
    out = np.zeros_like(good_v)
    # no program loaded
    e = A.Batch(N, 1, 0)
    assert raw_set(lib, e, 0, good_L, 0, 4, good_v, 0) == FX_E_NOTREADY and raw_get(lib, e, 0, good_L, 0, 4, out, 0) == FX_E_NOTREADY
    assert raw_set(lib, e, 0, None, 0, 4, None, 0) == FX_E_NOTREADY, "count == 0 without a program, as fxb_set_registers_list"
    e.close()
    w = Twin(base, A, lib, OFFSET, N, 64, rng, 3, positions_at(N, 64, 500, 0))
    w.set(0, good_L, 0, good_v[:, :4], True)
    w.same("before the refusals")
    b = w.b
    counters = lambda: (b.info("tram_list_sets"), b.info("tram_list_gets"), lib.fxstub_tram_scatters(), lib.fxstub_tram_gathers())  # noqa: E731
    seen, image = counters(), b.save_state()
    for what, fn, word, which, L, first, n_words, v, flags, count in refusals_of(N, 64, 503, good_L, good_v, out):
        before = out.copy()
        got = fns[fn](lib, b, which, L, first, n_words, v, flags, count=count)
        assert got == FX_E_ARG and word in b.last_error(), (what, fn, got, b.last_error())
        assert counters() == seen and same_bits(out, before) and (b.save_state() == image).all(), (what, fn)
    assert lib.fxb_set_tram_list(None, 0, ptr(good_L), 3, 0, 4, ptr(good_v), 0) == FX_E_ARG
    assert lib.fxb_get_tram_list(None, 0, ptr(good_L), 3, 0, 4, ptr(out), 0) == FX_E_ARG
    # a line the program does not have
    p = handle(A, PLAIN, N)
    for fn in (raw_set, raw_get):
        assert fn(lib, p, 0, good_L, 0, 1, good_v, LOGICAL) == FX_E_ARG and "does not have" in p.last_error()
        assert fn(lib, p, 1, good_L, 0, 1, good_v, 0) == FX_E_ARG and "n_words" in p.last_error()
    assert p.info("tram_list_sets") == 0 and p.info("tram_list_gets") == 0
    p.close()
    # repeats are a refusal of the set only
    assert raw_get(lib, b, 0, np.array([5, 9, 5], dtype=np.int64), 0, 4, np.zeros((3, 4), dtype=np.float32), LOGICAL) == 0
    w.same("after the refusals")
    w.close()
    # an allocation that fails, at each allocation of the call (the device staging, the pinned staging): FX_E_MEMORY, nothing
    # changed, then the same call succeeds
    for fn in (raw_set, raw_get):
        for nth in (0, 1):
            w = Twin(base, A, lib, OFFSET, N, 64, rng, 4, positions_at(N, 64, 500, 0))
            w.same("in front of the failure")
            live = lib.fxstub_live_allocations()
            held = out.copy()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = fn(lib, w.b, 0, good_L, 5, 64, good_v.copy() if fn is raw_set else out, LOGICAL)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and w.b.last_error(), (fn.__name__, nth, rc)
            assert w.b.info("tram_list_sets") == 0 and w.b.info("tram_list_gets") == 0 and lib.fxstub_live_allocations() <= live + 1 and same_bits(out, held)
            w.same("after an allocation failure")
            w.set(0, good_L, 5, good_v[:, :64], True)
            w.same_get(0, good_L, 5, 64, True, "the same call goes through afterwards")
            w.same("the same call goes through afterwards")
            w.close()
    assert lib.fxstub_tram_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("tram list refusals ok")


def child_pieces():
    """windows of 8 192 words: 2 048 of them fill the 64 MiB of staging, so 2 200 run in two pieces - the set blocks between them,
    and the words arrive as from one"""
    base, A, lib = list_library()
    rng = np.random.default_rng(547)
    n, Z = 2200, 8192
    per = SCRATCH // (Z * 4)
    assert per == 2048
    b = A.Batch(n, 1, 0)
    assert b.load_text(LONG), b.errors()
    assert b.info("instance_rings") == 3 and b.info("xtram_slots") == Z
    L = rng.permutation(n).astype(np.int64)
    v = rng.integers(0, 1 << 32, (n, Z), dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert b.set_tram_list(1, L, 100, v, logical=True) == 0
    assert b.info("tram_list_sets") == 2 and lib.fxstub_tram_scatters() >= 1, "the first piece has run when the call returns: the second waited for it"
    assert b.sync() == 0 and lib.fxstub_tram_scatters() == 2
    p = b.get_cursors_i(0)[2]
    slots = (p - 1 - (100 + np.arange(Z))) % Z
    for k in (0, 1, per - 1, per, per + 1, n - 1):
        assert same_bits(b.get_tram_i(1, int(L[k]), Z)[slots], v[k]), k
    got = b.get_tram_list(1, L[::-1].copy(), 100, Z, logical=True)
    assert b.info("tram_list_gets") == 2 and same_bits(got, v[::-1])
    assert b.set_tram_list(1, L[:per], 0, v[:per]) == 0 and b.info("tram_list_sets") == 3, "exactly a piece"
    assert b.set_tram_list(1, L[:per + 1], 0, v[:per + 1]) == 0 and b.info("tram_list_sets") == 5, "one window more than a piece holds"
    assert same_bits(b.get_tram_i(1, int(L[per]), Z), v[per])
    one = v[7].copy()
    assert b.set_tram_list(0, L, 0, one) == 0 and b.info("tram_list_sets") == 7, "a broadcast window is staged once per piece"
    assert same_bits(b.get_tram_list(0, L[[0, per, n - 1]], 0, Z), np.tile(one, (3, 1)))
    b.close()
    assert lib.fxstub_tram_strays() == 0
    print("tram list pieces ok")


def child_shards():
    """three shards against the twin - a single handle that takes the words through records: one list on every shard, one wholly
    inside the middle shard, refusals in front of every shard, allocation failures on whichever shard"""
    base, A, lib = list_library()
    rng = np.random.default_rng(557)
    n = 3 * 256 + 40
    w = Twin(base, A, lib, OFFSET, n, 64, rng, 6, positions_at(n, 64, 500, 0), devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in w.b.shards()] == [(0, 0), (1, 320), (2, 576)], w.b.shards()
    inside = rng.permutation(np.arange(330, 400)).astype(np.int64)
    everywhere = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:128]]).astype(np.int64)
    for which, first, n_words, logical in ((0, 61, 64, True), (1, 400, 103, False), (0, 0, 1, False)):
        before = w.b.info("tram_list_sets")
        w.set(which, inside, first, windows_for(rng, inside.size, n_words), logical)
        assert w.b.info("tram_list_sets") == before + 1, "a shard without an entry launches nothing"
        w.same_get(which, inside, first, n_words, logical, "inside the middle shard")
        w.set(which, everywhere, first, windows_for(rng, everywhere.size, n_words), logical)
        assert w.b.info("tram_list_sets") == before + 4
        w.same_get(which, np.concatenate([everywhere[:40], inside[:10], everywhere[:40]]), first, n_words, logical, "a get with repeats on every shard")
        w.set(which, everywhere, first, windows_for(rng, 1, n_words)[0], logical, broadcast=True)
        w.same((which, first, n_words, logical))
    # refused for the whole handle, in front of every shard
    seen, image = (w.b.info("tram_list_sets"), lib.fxstub_tram_scatters()), w.b.save_state()
    v = windows_for(rng, 3, 8)
    assert raw_set(lib, w.b, 0, np.array([0, n - 1, 0], dtype=np.int64), 0, 8, v, 0) == FX_E_ARG and "entry 2" in w.b.last_error()
    assert raw_set(lib, w.b, 0, np.array([0, 700, n], dtype=np.int64), 0, 8, v, 0) == FX_E_ARG and "entry 2" in w.b.last_error()
    assert raw_set(lib, w.b, 1, np.array([700], dtype=np.int64), 0, 8, v, LOGICAL) == FX_E_ARG, "asked of every shard, also those without an entry"
    assert raw_set(lib, w.b, 0, np.array([700], dtype=np.int64), 60, 8, v, 0) == FX_E_ARG
    assert (w.b.info("tram_list_sets"), lib.fxstub_tram_scatters()) == seen and (w.b.save_state() == image).all()
    w.close()
    # an allocation that fails on whichever shard - two per shard, each shard has entries: FX_E_MEMORY, and no shard has changed
    for nth in range(6):
        c = Twin(base, A, lib, OFFSET, n, 64, rng, 8, positions_at(n, 64, 500, 0), devices=[0, 1, 2])
        g = windows_for(rng, everywhere.size, 64)
        c.b.sync()
        lib.fxstub_fail_mallocs(nth, 1)
        rc = raw_set(lib, c.b, 0, everywhere, 9, 64, g, LOGICAL)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.b.last_error(), (nth, rc)
        assert c.b.info("tram_list_sets") == 0
        c.same("after an allocation failure on a shard")
        c.set(0, everywhere, 9, g, True)
        assert c.b.info("tram_list_sets") == 3
        c.same("the same call goes through afterwards")
        c.close()
    assert lib.fxstub_tram_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("tram list shards ok")


if __name__ == "__main__":
    which = sys.argv[1]
    if which.startswith("twin-"):
        child_twin(int(which[5:]))
    else:
        {"broadcast": child_broadcast, "streams": child_streams, "refusals": child_refusals, "pieces": child_pieces, "shards": child_shards}[which]()
