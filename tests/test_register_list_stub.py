"""Register calls by list without a GPU: fxb_set_registers_list / fxb_get_registers_list on the library's host sources linked
against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like
tests/test_bus_gain_list_stub.py (this file is also that child).  The stand-ins of the two kernels
(tests/hipstub/fx_registers_stub.cpp) move the words in stream order with an addressing of their own.

The model is a TWIN handle that receives the same writes through fxb_set_register_i or fxb_set_register_array - the definition of
the set in include/fx8010_amd.h "Register sets by list".  After every step every word of a block's output, every
get_register_array row, save_state() and the counters of the code in force are compared; there is no tolerance.  What the stand-in
cannot show is which register values a block computed with (its emulation kernel copies the input and reads no register): that a
queued block keeps the values it was queued with is tests/test_gpu_register_list.py; here the ORDER in which the stand-in ran the
launches is observed instead.  The Python-driven cases do not run under a sanitizer: that is
tests/hipstub/register_list_checks.cpp, a program of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, PROGRAM, ROOT, STEREO, Pinned, same_words, stub_library  # noqa: E402
from test_bus_tap_stub import same_bits  # noqa: E402

FX_E_NOTREADY = -2
N = 200
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7149f2ca, 0xf149f2ca, 0x7fc12345, 0x3f000000], dtype=np.uint32).view(np.float32)
#          +0, -0, the smallest and the largest denormal (the latter negative), +-1e30, a quiet NaN with a payload, 0.5


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("channels", (1, 2))
def test_list_sets_equal_the_twin_on_the_hip_stand_in(channels):
    """every list (1 entry, {0, N-1}, 63, 64, 65, all N shuffled) with one key, two keys and every register, in front of blocks"""
    run_child("twin-%d" % channels, "register list twin ok")


def test_list_sets_and_the_code_in_force_on_the_hip_stand_in():
    """a folded register, a broadcast write behind a list set, a cold control under the lean variant, an armed track, a reset"""
    run_child("code", "register list code ok")


def test_list_set_behind_a_block_on_another_stream_on_the_hip_stand_in():
    run_child("streams", "register list streams ok")


def test_list_call_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "register list refusals ok")


def test_list_calls_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "register list shards ok", devices=3)


def test_list_call_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/register_list_checks.cpp (csrc/Makefile `stubasanreglist`): the list and key shapes through the C ABI on
    exactly-sized heap blocks, the refusals and the allocation failures, on one handle and on three shards, under AddressSanitizer +
    UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasanreglist"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "register_list_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "register list checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def list_library():
    A, lib = stub_library()
    for f in ("fxstub_reg_scatters", "fxstub_reg_gathers", "fxstub_reg_strays", "fxstub_live_allocations"):
        getattr(lib, f).restype = C.c_long
    return A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def key_table(keys):
    return (C.c_char_p * max(len(keys), 1))(*[k.encode() for k in keys])


def raw_set(lib, b, keys, L, v, n_keys=None, count=None, table=True):
    return lib.fxb_set_registers_list(b._h, key_table(keys) if table else None, len(keys) if n_keys is None else n_keys, ptr(L), (0 if L is None else L.size) if count is None else count, ptr(v))


def raw_get(lib, b, keys, L, v, n_keys=None, count=None, table=True):
    return lib.fxb_get_registers_list(b._h, key_table(keys) if table else None, len(keys) if n_keys is None else n_keys, ptr(L), (0 if L is None else L.size) if count is None else count, ptr(v))


def lists_of(rng, n):
    """the lists of the issue over 0..n-1: one entry; {0, n-1}; 63, 64 and 65 entries around a wavefront's width, the first and the
    last instance among them; all n in a shuffled order"""
    out = [[n // 2], [0, n - 1]]
    for k in (63, 64, 65):
        out.append(np.concatenate([[n - 1], rng.permutation(np.arange(1, n - 1))[:k - 2], [0]]))
    out.append(rng.permutation(n))
    return [np.asarray(L, dtype=np.int64) for L in out]


def values_for(rng, n_keys, count):
    """[n_keys, count] words of every magnitude; the specials walk through the first columns of every row"""
    v = (rng.standard_normal((n_keys, count)) * 10.0 ** rng.integers(-8, 8, (n_keys, count))).astype(np.float32)
    for k in range(n_keys):
        m = min(count, SPECIALS.size)
        v[k, :m] = np.roll(SPECIALS, k)[:m]
    return v


def register_names(A, text, ch):
    f = A.FrontEnd(ch)
    assert f.load_text(text), f.errors()
    return [r[0] for r in f.registers()]


class Twin:
    """a handle that takes list sets beside one that takes the same writes through the calls the definition names"""
    COUNTERS = ("xlate_builds", "num_rows", "control_rows", "kernel", "num_lane_regs", "num_uniform_regs")

    def __init__(self, A, lib, text, n, ch, rng, devices=None):
        self.A, self.lib, self.n, self.ch, self.rng = A, lib, n, ch, rng
        self.b = A.Batch(n, ch, devices=devices) if devices else A.Batch(n, ch, 0)
        self.t = A.Batch(n, ch, 0)
        assert self.b.load_text(text) and self.t.load_text(text), self.b.errors()
        self.names = register_names(A, text, ch)

    def settle(self, S=8):
        """the builder threads are idle: what they deliver does not depend on when a test looks"""
        assert self.b.prepare(S, True) == 0 and self.t.prepare(S, True) == 0

    def set(self, keys, L, v):
        keys, L, v = list(keys), np.ascontiguousarray(L, dtype=np.int64), np.ascontiguousarray(v, dtype=np.float32).reshape(len(keys), -1)
        given_L, given_v = L.copy(), v.copy()
        shards = len(self.b.shards())
        before, ran = self.b.info("register_list_sets"), self.lib.fxstub_reg_scatters()
        assert raw_set(self.lib, self.b, keys, given_L, given_v) == 0, self.b.last_error()
        given_L[...] = -5            # the arrays are the caller's again on return
        given_v[...] = np.nan
        launched = self.b.info("register_list_sets") - before
        assert 1 <= launched <= shards and (shards > 1 or launched == 1), launched
        for k, key in enumerate(keys):
            if L.size <= 3:
                for i, inst in enumerate(L):
                    # (a Python float carries a quiet NaN's payload through ctypes; SPECIALS holds no signalling one)
                    assert self.t.set_register_i(key, int(inst), float(v[k, i])) == 0
                    assert same_bits(np.float32(self.t.get_register_i(key, int(inst))), v[k, i])
            else:
                row = self.t.get_register_array(key)
                row[L] = v[k]
                assert self.t.set_register_array(key, row) == 0
        return ran + launched   # what fxstub_reg_scatters says once the set has run

    def same_registers(self, what):
        for key in self.names:
            assert same_bits(self.b.get_register_array(key), self.t.get_register_array(key)), (what, key)

    def same_get(self, keys, L, what):
        """fxb_get_registers_list against fxb_get_register_i of both handles (large lists: against the twin's rows)"""
        keys, L = list(keys), np.asarray(L, dtype=np.int64)
        got = self.b.get_registers_list(keys, L)
        assert got.shape == (len(keys), L.size)
        for k, key in enumerate(keys):
            if L.size <= 65:
                want_b = np.array([self.b.get_register_i(key, int(i)) for i in L], dtype=np.float32)
                want_t = np.array([self.t.get_register_i(key, int(i)) for i in L], dtype=np.float32)
                assert same_bits(got[k], want_b) and same_bits(got[k], want_t), (what, key)
            else:
                assert same_bits(got[k], self.t.get_register_array(key)[L]), (what, key)

    def block(self, S, what):
        x = (self.rng.standard_normal((S, self.ch, self.n)) if self.ch > 1 else self.rng.standard_normal((S, self.n))).astype(np.float32)
        assert same_words(self.b.process_block(x), self.t.process_block(x)), what
        self.same_registers(what)
        assert (self.b.save_state() == self.t.save_state()).all(), what
        if len(self.b.shards()) == 1:
            assert [self.b.info(c) for c in self.COUNTERS] == [self.t.info(c) for c in self.COUNTERS], (what, self.COUNTERS, [self.b.info(c) for c in self.COUNTERS], [self.t.info(c) for c in self.COUNTERS])

    def close(self):
        self.b.close()
        self.t.close()


def child_twin(ch):
    A, lib = list_library()
    rng = np.random.default_rng(401 + ch)
    text = STEREO if ch == 2 else PROGRAM
    w = Twin(A, lib, text, N, ch, rng)
    names = w.names
    assert "vol" in names and "a" in names, names
    gathers = lib.fxstub_reg_gathers()
    w.block(8, "the first block")
    step = 0
    for keys in (["vol"], ["a", "vol"], names):
        for L in lists_of(rng, N):
            S = (33, 1, 2)[step % 3]
            step += 1
            what = (keys, L.size, S)
            v = values_for(rng, len(keys), L.size)
            ran = w.set(keys, L, v)
            w.same_get(keys, L, what)   # (synchronous: the set has run)
            assert lib.fxstub_reg_scatters() == ran, what
            w.same_registers(what)
            w.settle(S)
            w.block(S, what)
            w.same_get(keys, L, what)
    assert lib.fxstub_reg_gathers() > gathers and w.b.info("register_list_gets") == lib.fxstub_reg_gathers() - gathers
    # repeats are fine in a get: instances and keys
    L = np.array([7, 7, 0, N - 1, 7], dtype=np.int64)
    got = w.b.get_registers_list(["vol", "a", "vol"], L)
    assert same_bits(got[0], got[2]) and same_bits(got[0], w.t.get_register_array("vol")[L]) and same_bits(got[1], w.t.get_register_array("a")[L])
    # count == 0 and n_keys == 0 return 0 once the keys have been looked up
    sets = w.b.info("register_list_sets")
    assert raw_set(lib, w.b, ["vol"], None, None) == 0 and raw_set(lib, w.b, [], L[:1].copy(), None) == 0 and raw_get(lib, w.b, ["a"], None, None) == 0
    assert raw_set(lib, w.b, ["nosuch"], None, None) == 1 and "nosuch" in w.b.last_error()
    assert w.b.info("register_list_sets") == sets
    w.block(5, "after the empty calls")
    w.close()
    assert lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("register list twin ok")


def child_code():
    A, lib = list_library()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import fx8010_programs as P
    rng = np.random.default_rng(409)
    # a register the code in force has folded in: the next block generates other code, once; later sets are plain scatters
    w = Twin(A, lib, STEREO, N, 2, rng)
    w.settle()
    w.block(8, "vol folded in")
    # (a change of code is a translation, on either thread, or - vol is a declared control, whose variant is built ahead - code found cached)
    changes = lambda: w.b.info("xlate_builds") + w.b.info("xlate_background_builds") + w.b.info("code_cache_hits")  # noqa: E731
    rows, builds = w.b.info("num_rows"), changes()
    L = lists_of(rng, N)[3]
    w.set(["vol"], L, values_for(rng, 1, L.size))
    w.block(8, "the first list set of vol")
    assert w.b.info("num_rows") == rows + 1, "vol has a row now"
    assert changes() == builds + 1, "one change of code"
    w.settle()
    w.block(8, "the builder has caught up")
    builds = (w.b.info("xlate_builds"), w.b.info("xlate_background_builds"), w.b.info("code_cache_hits"))
    for L in lists_of(rng, N):
        w.set(["vol"], L, values_for(rng, 1, L.size))
        w.block(8, "a later set of vol")
    assert (w.b.info("xlate_builds"), w.b.info("xlate_background_builds"), w.b.info("code_cache_hits")) == builds, "later sets are plain scatters"
    # a broadcast write behind a list set wins, and the row is given back
    ran = w.set(["vol"], np.array([3, 0, N - 1], dtype=np.int64), values_for(rng, 1, 3))
    assert w.b.set_register("vol", 0.375) == 0 and w.t.set_register("vol", 0.375) == 0
    assert lib.fxstub_reg_scatters() == ran, "the broadcast write waited for the scatter in front of it"
    assert same_bits(w.b.get_register_array("vol"), np.full(N, 0.375, dtype=np.float32))
    w.same_get(["vol"], np.arange(N), "a broadcast write behind a list set")
    w.block(8, "a broadcast write behind a list set")
    assert w.b.info("num_rows") == rows, "the row is given back"
    # a reset of instances behind a list set: the listed instances are back at the last broadcast value
    L = np.array([5, 64, N - 1, 0], dtype=np.int64)
    w.set(["vol", "a"], L, values_for(rng, 2, L.size))
    for h in (w.b, w.t):
        assert h.reset_instances(L[:2]) == 0
    w.same_registers("a reset behind a list set")
    assert same_bits(w.b.get_registers_list(["vol"], L[:2]), np.full((1, 2), 0.375, dtype=np.float32))
    w.block(8, "a reset behind a list set")
    # a register with an armed track: the track's step at sample 0 wins over the list set in front of the block
    track = np.array([0.25, 0.75], dtype=np.float32)
    for h in (w.b, w.t):
        assert h.set_register_track("vol", track, 4) == 0
    w.set(["vol"], L, values_for(rng, 1, L.size))
    w.block(8, "a list set on a register with an armed track")   # (what the host knows afterwards; that the step at sample 0 wins in the block's words is the GPU's to show)
    assert w.b.get_register_i("nosuch", 0) == 1.0 and same_bits(np.float32(w.b.get_register_i("vol", N)), np.float32(0.75)), "the track's last step is the value the host holds for all"
    w.close()
    # a list set on a declared control while the lean variant is active (tests/hipstub/host_logic.py has the recipe): the cold
    # control needs its row in the next block, from the full variant that is still there - no translation on the caller's thread
    n = 262144 // 64
    w = Twin(A, lib, P.config5(), n, 1, rng)
    x = P.stimulus(n, 32)

    def both(f):
        for h in (w.b, w.t):
            f(h)

    def settle(want):
        for _ in range(3):
            both(lambda h: (h.prepare(32, True), h.process_block(x)))
        assert w.b.info("control_rows") == want and w.t.info("control_rows") == want, (w.b.info("control_rows"), w.t.info("control_rows"), want)

    both(lambda h: (h.prepare(32, True), h.process_block(x)))
    both(lambda h: (h.set_register("decay", 0.4), h.process_block(x)))
    assert w.b.info("control_rows") == 3
    settle(1)
    L = np.array([5, 70, n - 1], dtype=np.int64)
    w.set(["diff"], L, np.array([[0.55, 0.5, 0.45]], dtype=np.float32))
    both(lambda h: h.process_block(x))
    assert w.b.info("control_rows") == 3 and w.t.info("control_rows") == 3, "the cold control has its row in the very next block"
    assert w.b.info("xlate_builds") == 1 and w.t.info("xlate_builds") == 1
    settle(2)
    w.same_get(["diff", "decay", "damp"], L, "under the lean variant")
    assert same_bits(w.b.get_registers_list(["diff"], [5, 6]), np.array([[0.55, 0.6]], dtype=np.float32))
    w.same_registers("under the lean variant")
    assert (w.b.save_state() == w.t.save_state()).all()
    w.close()
    assert lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("register list code ok")


def child_streams():
    """a list set behind a slow block on stream A returns while that block is still running (its last output row still holds the
    mark it was given) and has not run yet; a block on stream B and a get behind it wait for it"""
    A, lib = list_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(419)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    n, S, ch = 1000, 8, 1
    SLOW = 150000   # the emulation launch takes 150 ms: a set that waits for the block in front of it is caught, and so is one that is not ordered behind it
    w = Twin(A, lib, PROGRAM, n, ch, rng)
    L0 = np.array([1, 2], dtype=np.int64)
    w.set(["vol", "a"], L0, values_for(rng, 2, 2))   # (rows, code and staging exist before anything is timed)
    w.settle(S)
    w.block(S, "warm-up")

    def fresh():
        p, o = pinned((S, ch, n)), pinned((S, ch, n))
        p[...] = rng.standard_normal((S, ch, n)).astype(np.float32)
        o[...] = -7.0
        return p, o

    def dev(bufs, stream):
        return lib.fxb_process_block_dev(w.b._h, ptr(bufs[0]), ptr(bufs[1]), S, stream)

    first, second, third = fresh(), fresh(), fresh()
    L = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:63]]).astype(np.int64)
    v1, v2 = values_for(rng, 2, L.size), values_for(rng, 2, L.size)
    old = w.t.get_register_array("vol").copy()
    lib.fxstub_set_kernel_micros(SLOW)
    assert dev(first, streams[0]) == 0
    ran = w.set(["vol", "a"], L, v1)
    assert (first[1][S - 1] == -7.0).all(), "the list set returned while the block in front of it was still running"
    assert lib.fxstub_reg_scatters() == ran - 1, "... and it is queued behind that block: it has not run"
    lib.fxstub_set_kernel_micros(150)
    assert dev(second, streams[1]) == 0
    got = w.b.get_registers_list(["vol", "a"], L)   # waits for everything queued
    assert lib.fxstub_reg_scatters() == ran and not (first[1][S - 1] == -7.0).any(), "the get waited for the set, the set for the block"
    assert same_bits(got, v1) and not same_bits(got[0], old[L])
    # a second set, a block on the default stream, sync
    ran = w.set(["vol", "a"], L[::-1].copy(), v2)
    assert dev(third, None) == 0
    assert w.b.sync() == 0 and lib.fxstub_reg_scatters() == ran
    for bufs in (first, second, third):
        assert same_words(bufs[1], bufs[0])   # (the stand-in's emulation launch copies its input)
    w.same_registers("after the streams")
    assert same_bits(w.b.get_registers_list(["a", "vol"], L[::-1].copy()), v2[::-1])
    # every call that touches registers or state observes a list set that is still queued behind a slow block
    for name, call in (("set_register_i", lambda h: h.set_register_i("vol", 3, 0.125)), ("set_register_array", lambda h: h.set_register_array("a", np.linspace(0, 1, n).astype(np.float32))),
                       ("get_register_array", lambda h: h.get_register_array("vol")), ("save_state", lambda h: h.save_state()), ("copy_instances", lambda h: h.copy_instances([0], [9]))):
        lib.fxstub_set_kernel_micros(30000)
        assert dev(first, streams[0]) == 0
        ran = w.set(["vol", "a"], L, values_for(rng, 2, L.size))
        lib.fxstub_set_kernel_micros(150)
        call(w.b)
        call(w.t)
        assert w.b.sync() == 0 and lib.fxstub_reg_scatters() == ran
        w.same_registers(name + " behind a queued list set")
        assert (w.b.save_state() == w.t.save_state()).all(), name
    pinned.free()
    w.close()
    assert lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("register list streams ok")


def child_refusals():
    A, lib = list_library()
    rng = np.random.default_rng(421)
    S = 8
    # no program loaded
    e = A.Batch(N, 2, 0)
    good_L, good_v = np.array([3, 0, N - 1], dtype=np.int64), values_for(rng, 2, 3)
    out = np.zeros((2, 3), dtype=np.float32)
    assert raw_set(lib, e, ["vol", "a"], good_L, good_v) == FX_E_NOTREADY and raw_get(lib, e, ["vol", "a"], good_L, out) == FX_E_NOTREADY
    e.close()
    w = Twin(A, lib, STEREO, N, 2, rng)
    w.set(["vol"], good_L, good_v[:1])
    w.settle(S)
    w.block(S, "before the refusals")
    b = w.b
    counters = lambda: (b.info("register_list_sets"), b.info("register_list_gets"), lib.fxstub_reg_scatters(), lib.fxstub_reg_gathers())  # noqa: E731
    seen = counters()
    big = np.zeros(1, dtype=np.int64)
    refused = [
        ("an instance listed twice", raw_set, FX_E_ARG, dict(keys=["vol", "a"], L=np.array([5, 9, 5], dtype=np.int64), v=good_v)),
        ("two keys that name one register", raw_set, FX_E_ARG, dict(keys=["vol", "vol"], L=good_L, v=good_v)),
        ("a key that is no register", raw_set, 1, dict(keys=["vol", "nosuch"], L=good_L, v=good_v)),
        ("a key that is no register", raw_get, 1, dict(keys=["nosuch", "a"], L=good_L, v=out)),
        ("a key that is no register, nothing listed", raw_set, 1, dict(keys=["nosuch"], L=None, v=None)),
    ]
    for fn, v in ((raw_set, good_v), (raw_get, out)):
        refused += [
            ("an instance of N", fn, FX_E_ARG, dict(keys=["vol", "a"], L=np.array([0, N, 1], dtype=np.int64), v=v)),
            ("an instance of -1", fn, FX_E_ARG, dict(keys=["vol", "a"], L=np.array([0, 1, -1], dtype=np.int64), v=v)),
            ("count < 0", fn, FX_E_ARG, dict(keys=["vol", "a"], L=good_L, v=v, count=-1)),
            ("n_keys < 0", fn, FX_E_ARG, dict(keys=["vol", "a"], L=good_L, v=v, n_keys=-1)),
            ("null keys", fn, FX_E_ARG, dict(keys=["vol", "a"], L=good_L, v=v, table=False)),
            ("a null list", fn, FX_E_ARG, dict(keys=["vol", "a"], L=None, v=v, count=3)),
            ("null values", fn, FX_E_ARG, dict(keys=["vol", "a"], L=good_L, v=None)),
            ("n_keys * count = 2^31", fn, FX_E_ARG, dict(keys=["vol", "a"], L=big, v=v, count=1 << 30)),
            ("count = 2^31", fn, FX_E_ARG, dict(keys=["vol"], L=big, v=v, count=1 << 31)),
        ]
    for what, fn, rc, kw in refused:
        before = out.copy()
        got = fn(lib, b, kw["keys"], kw["L"], kw["v"], n_keys=kw.get("n_keys"), count=kw.get("count"), table=kw.get("table", True))
        assert got == rc and b.last_error(), (what, fn.__name__, got, b.last_error())
        assert counters() == seen and same_bits(out, before), (what, fn.__name__)
        assert rc != 1 or "nosuch" in b.last_error(), (what, b.last_error())
    assert lib.fxb_set_registers_list(None, key_table(["vol"]), 1, ptr(good_L), 3, ptr(good_v)) == FX_E_ARG
    assert lib.fxb_get_registers_list(None, key_table(["vol"]), 1, ptr(good_L), 3, ptr(out)) == FX_E_ARG
    # repeats are a refusal of the set only
    assert raw_get(lib, b, ["vol", "vol"], np.array([5, 9, 5], dtype=np.int64), np.zeros((2, 3), dtype=np.float32)) == 0
    seen = counters()
    w.same_registers("after the refusals")
    w.block(S, "after the refusals")
    w.close()
    # an allocation that fails, at each allocation of the call (the device staging, the pinned staging): FX_E_MEMORY, nothing
    # changed, then the same call succeeds (the builder threads are idle while allocations are made to fail)
    for fn in (raw_set, raw_get):
        for nth in (0, 1):
            w = Twin(A, lib, STEREO, N, 2, rng)
            if fn is raw_get:
                assert w.b.set_register_i("vol", 1, 0.25) == 0 and w.t.set_register_i("vol", 1, 0.25) == 0 and w.b.set_register_i("a", 1, 0.25) == 0 and w.t.set_register_i("a", 1, 0.25) == 0
            w.settle(S)
            w.block(S, "in front of the failure")
            w.settle(S)
            live = lib.fxstub_live_allocations()
            held = out.copy()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = fn(lib, w.b, ["vol", "a"], good_L, good_v.copy() if fn is raw_set else out)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and w.b.last_error(), (fn.__name__, nth, rc)
            assert w.b.info("register_list_sets") == 0 and w.b.info("register_list_gets") == 0 and lib.fxstub_live_allocations() <= live + 1 and same_bits(out, held)
            w.same_registers("after an allocation failure")
            w.block(S, "after an allocation failure")
            if fn is raw_set:
                w.set(["vol", "a"], good_L, good_v)
            w.same_get(["vol", "a"], good_L, "the same call goes through afterwards")
            w.block(S, "the same call goes through afterwards")
            w.close()
    assert lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("register list refusals ok")


def child_shards():
    """three shards against the twin - a single handle that takes the writes through the existing calls: one list on every shard,
    one wholly inside the middle shard, allocation failures on whichever shard"""
    A, lib = list_library()
    rng = np.random.default_rng(431)
    n, S, ch = 3 * 256 + 40, 9, 2
    w = Twin(A, lib, STEREO, n, ch, rng, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in w.b.shards()] == [(0, 0), (1, 320), (2, 576)], w.b.shards()
    w.block(S, "the first block")
    inside = rng.permutation(np.arange(330, 400)).astype(np.int64)
    everywhere = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:128]]).astype(np.int64)
    for keys in (["vol"], ["a", "vol"], w.names):
        before = w.b.info("register_list_sets")
        w.set(keys, inside, values_for(rng, len(keys), inside.size))
        assert w.b.info("register_list_sets") == before + 1, "a shard without an entry launches nothing"
        w.same_get(keys, inside, "inside the middle shard")
        w.block(S, "inside the middle shard")
        w.set(keys, everywhere, values_for(rng, len(keys), everywhere.size))
        assert w.b.info("register_list_sets") == before + 4
        w.same_get(keys, everywhere, "on every shard")
        w.same_get(keys, np.concatenate([everywhere, inside, everywhere]), "a get with repeats on every shard")
        w.block(S, "on every shard")
    # refused for the whole handle, in front of every shard
    seen = (w.b.info("register_list_sets"), lib.fxstub_reg_scatters())
    v = values_for(rng, 1, 3)
    assert raw_set(lib, w.b, ["vol"], np.array([0, n - 1, 0], dtype=np.int64), v) == FX_E_ARG and raw_set(lib, w.b, ["vol"], np.array([n], dtype=np.int64), v) == FX_E_ARG
    assert raw_set(lib, w.b, ["nosuch"], np.array([0], dtype=np.int64), v) == 1 and "nosuch" in w.b.last_error()
    assert (w.b.info("register_list_sets"), lib.fxstub_reg_scatters()) == seen
    # an allocation that fails on whichever shard - two per shard, each shard has entries: FX_E_MEMORY, and no shard has changed
    for nth in range(6):
        c = Twin(A, lib, STEREO, n, ch, rng, devices=[0, 1, 2])
        c.settle(S)
        c.block(S, "in front of the failure")
        c.settle(S)
        g = values_for(rng, 2, everywhere.size)
        lib.fxstub_fail_mallocs(nth, 1)
        rc = raw_set(lib, c.b, ["vol", "a"], everywhere, g)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.b.last_error(), (nth, rc)
        assert c.b.info("register_list_sets") == 0
        c.same_registers("after an allocation failure on a shard")
        c.block(S, "after an allocation failure on a shard")   # (save_state included: no shard has noted a per-instance write)
        c.set(["vol", "a"], everywhere, g)
        assert c.b.info("register_list_sets") == 3
        c.block(S, "the same call goes through afterwards")
        c.close()
    w.set(w.names, rng.permutation(n).astype(np.int64), values_for(rng, len(w.names), n))
    w.block(S, "everything")
    w.close()
    assert lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("register list shards ok")


if __name__ == "__main__":
    which = sys.argv[1]
    if which.startswith("twin-"):
        child_twin(int(which[5:]))
    else:
        {"code": child_code, "streams": child_streams, "refusals": child_refusals, "shards": child_shards}[which]()
