"""Gain sets by list without a GPU: fxb_bus_set_gains_list / _send_gains_list / _feed_gains_list on the library's host sources
linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like
tests/test_bus_gain_stub.py (this file is also that child).  The stand-in of the scatter kernel
(tests/hipstub/fx_gain_scatter_stub.cpp) moves the words in stream order with an addressing of its own; the stand-ins of the mix,
the sends and the feeds do the real arithmetic.  Every test keeps a / b / pending in the state model below, written from the
definition of include/fx8010_amd.h "Gain sets by list", and hands a and b to the models of the existing test modules
(gain_mix_model, send_model, feed_model).  Every word is compared; there is no tolerance.  The Python-driven cases do not run
under a sanitizer: that is tests/hipstub/gain_list_checks.cpp, a program of its own.  Parity of the real kernel is
tests/test_gpu_bus_gain_list.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, PROGRAM, ROOT, STEREO, Pinned, bus, expand, mix_model, same_words, stub_library  # noqa: E402
from test_bus_gain_stub import gain_mix_model, gains_for, signal  # noqa: E402
from test_bus_tap_stub import same_bits  # noqa: E402
from test_bus_send_stub import auxed_dev, send_model, set_sends  # noqa: E402
from test_bus_feed_stub import fed_dev, feed_model, feed_structure, set_feeds, source_block  # noqa: E402


class GainState:
    """a, b and pending of one structure, as include/fx8010_amd.h "Gain sets by list" defines them ([C, W] float32).  While no
    ramp is pending a counts as b, and is kept equal to it here."""

    def __init__(self, g):
        self.a, self.b, self.pending = g.copy(), g.copy(), False

    def full(self, g, ramp):
        if ramp:
            if not self.pending:
                self.a = self.b.copy()
            self.b, self.pending = g.copy(), True
        else:
            self.a, self.b, self.pending = g.copy(), g.copy(), False

    def listed(self, L, g, ramp):
        L = np.asarray(L, dtype=np.int64)
        if ramp:
            if not self.pending:
                self.a = self.b.copy()
            self.b[:, L] = g
            self.pending = True
        else:
            self.a[:, L] = g
            self.b[:, L] = g   # (a pending ramp stays pending for the others)

    def in_force(self):
        return self.a if self.pending else self.b

    def consume(self):
        """what the block that consumes the ramp is given: (a, b, ramp); afterwards a = b"""
        a, b, ramp = self.a.copy(), self.b.copy(), self.pending
        self.a, self.pending = self.b.copy(), False
        return a, b, ramp


def lists_of(rng, W):
    """the lists of the issue over 0..W-1 (W >= 66): one entry; the first and the last index; 63, 64 and 65 entries straddling a
    wavefront's range; all indices in a shuffled order"""
    out = [[W // 2], [0, W - 1]]
    for n in (63, 64, 65):
        out.append(np.concatenate([[W - 1], rng.permutation(np.arange(1, W - 1))[:n - 2], [0]]))
    out.append(rng.permutation(W))
    return [np.asarray(L, dtype=np.int64) for L in out]


def test_state_model_is_the_definition_it_says():
    """the dozen lines above against the cases of the definition, spelled out"""
    rng = np.random.default_rng(3)
    g0, g1, g2 = (gains_for(rng, 2, 10) for _ in range(3))
    L = np.array([7, 0, 9])
    s = GainState(g0)
    s.listed(L, g1[:, :3], 1)   # ramp 1, none pending
    want_b = g0.copy()
    want_b[:, L] = g1[:, :3]
    assert s.pending and same_bits(s.a, g0) and same_bits(s.b, want_b) and same_bits(s.in_force(), g0)
    s.listed([3], g2[:, :1], 1)   # ramp 1, one pending: a stays
    want_b[:, 3] = g2[:, 0]
    assert s.pending and same_bits(s.a, g0) and same_bits(s.b, want_b)
    s.listed([3, 4], g1[:, 4:6], 0)   # ramp 0 while pending: a = b on L, still pending elsewhere
    want_a = g0.copy()
    want_a[:, [3, 4]] = g1[:, 4:6]
    want_b[:, [3, 4]] = g1[:, 4:6]
    assert s.pending and same_bits(s.a, want_a) and same_bits(s.b, want_b)
    a, b, ramp = s.consume()
    assert ramp and same_bits(a, want_a) and same_bits(b, want_b) and not s.pending and same_bits(s.in_force(), want_b)
    s.listed([1], g2[:, 1:2], 0)   # ramp 0, none pending
    want_b[:, 1] = g2[:, 1]
    assert not s.pending and same_bits(s.in_force(), want_b) and same_bits(s.a, s.b)
    # a full set with ramp = 0 cancels the ramp - the one difference - and a list set of everything with ramp = 1 is the full set
    t, u = GainState(g0), GainState(g0)
    t.full(g1, 1)
    u.listed(np.arange(10)[::-1], g1[:, ::-1], 1)
    assert t.pending and u.pending and same_bits(t.a, u.a) and same_bits(t.b, u.b)
    t.full(g2, 0)
    u.listed(np.arange(10), g2, 0)
    assert not t.pending and u.pending and same_bits(t.b, u.b) and same_bits(u.a, u.b)


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("kind", ("gains", "sends", "feeds"))
def test_list_set_state_machine_on_the_hip_stand_in(kind):
    """every transition with every list: ramp 1 / 0 with none / one pending, list sets around full sets, feeds going from
    unweighted, get_* after every step, the full-list equivalence"""
    run_child("state-" + kind, "gain list state ok")


def test_list_sets_behind_a_block_on_another_stream_on_the_hip_stand_in():
    run_child("streams", "gain list streams ok")


def test_ramp_started_by_a_list_set_across_the_pieces_of_a_block_on_the_hip_stand_in():
    run_child("pieces", "gain list pieces ok")


def test_list_set_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "gain list refusals ok")


def test_list_sets_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "gain list shards ok", devices=3)


def test_list_set_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/gain_list_checks.cpp (csrc/Makefile `stubasangainlist`): the indexing shapes for C = 1 and 2 with the three
    pitches, the refusals and the allocation failures through the C ABI on exactly-sized heap blocks, on one handle and on three
    shards, under AddressSanitizer + UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded
    and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasangainlist"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "gain_list_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "gain list checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def list_library():
    A, lib = stub_library()
    for f in ("fxstub_gain_scatters", "fxstub_gain_scatter_strays", "fxstub_live_allocations", "fxstub_bus_gain_mixes", "fxstub_bus_sends", "fxstub_bus_feeds"):
        getattr(lib, f).restype = C.c_long
    return A, lib


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


class Structure:
    """one of the three structures on a handle `b` beside a plain handle: full sets, list sets, get, and a block whose words are
    compared with the model of the structure for the (a, b, ramp) of the state model"""
    K = 63

    def __init__(self, kind, lib, b, plain, rng, N, ch):
        self.kind, self.lib, self.b, self.plain, self.rng, self.N, self.ch = kind, lib, b, plain, rng, N, ch
        if kind == "gains":
            self.W = N
        elif kind == "sends":
            # three buses: one entry, 64, and 1 030 (across the 1 024 chunk boundary)
            sizes = (1, 64, 1030)
            self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            self.mem = rng.integers(0, N, int(self.off[-1])).astype(np.int64)
            self.mem[[0, 1, -1]] = (N - 1, 0, N - 1)
            self.W = int(self.off[-1])
        else:
            self.M = 7
            self.off, self.src = feed_structure(rng, N, self.M, counts=(0, 1, 3))
            self.W = int(self.off[-1])
        self.weighted = True

    def install(self, g):
        """the structure with the weights g (feeds: g None = unweighted)"""
        if self.kind == "gains":
            assert self.b.bus_set_gains(g) == 0
        elif self.kind == "sends":
            assert set_sends(self.lib, self.b, self.off, self.mem, g) == 0, self.b.last_error()
        else:
            assert set_feeds(self.lib, self.b, self.M, self.off, self.src, g) == 0, self.b.last_error()
            self.weighted = g is not None

    def full(self, g, ramp):
        fn = {"gains": self.b.bus_set_gains, "sends": self.b.bus_set_send_gains, "feeds": self.b.bus_set_feed_gains}[self.kind]
        assert fn(g, bool(ramp)) == 0, self.b.last_error()
        self.weighted = True

    def raw_list(self, L, g, ramp, count=None):
        fn = {"gains": self.lib.fxb_bus_set_gains_list, "sends": self.lib.fxb_bus_set_send_gains_list, "feeds": self.lib.fxb_bus_set_feed_gains_list}[self.kind]
        return fn(self.b._h, ptr(L), (0 if L is None else L.size) if count is None else count, ptr(g), ramp)

    def listed(self, L, g, ramp):
        L, g = np.ascontiguousarray(L, dtype=np.int64), np.ascontiguousarray(g, dtype=np.float32)
        given_L, given_g = L.copy(), g.copy()
        assert self.raw_list(given_L, given_g, ramp) == 0, self.b.last_error()
        given_L[...] = -5          # the arrays are the caller's again on return
        given_g[...] = np.nan
        self.weighted = True

    def get(self):
        if self.kind == "gains":
            return self.b.bus_get_gains()
        return self.b.bus_get_sends()[2] if self.kind == "sends" else self.b.bus_get_feeds()[3]

    def block(self, a, bb, ramp, S):
        """one block with the structure; returns what it delivered, having compared it with the model"""
        rng, b, plain, N, K, ch = self.rng, self.b, self.plain, self.N, self.K, self.ch
        if self.kind == "feeds":
            x = source_block(rng, (S, ch, self.M))
            want = plain.process_block(feed_model(x, self.off, self.src, a, bb, ramp, S) if self.weighted else feed_model(x, self.off, self.src, None, None, False, S))
            got = b.process_block_bus_feed(x)
            assert same_words(got, want), (self.kind, ramp, S)
            return got
        x = signal(rng, (S, ch, b.bus_groups(K)))
        y = plain.process_block(expand(x, K, N))
        if self.kind == "gains":
            got = b.process_block_bus(x, K)
            assert same_words(got, gain_mix_model(y, a, bb, ramp, S, K)), (self.kind, ramp, S)
            return got
        out, got = b.process_block_bus(x, K, aux=True)
        assert same_words(out, mix_model(y, K)), "the group mix is unchanged"
        assert same_words(got, send_model(y, self.off, self.mem, a, bb, ramp, S)), (self.kind, ramp, S)
        return got


def handles(A, N, ch):
    b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
    text = STEREO if ch == 2 else PROGRAM
    assert b.load_text(text) and plain.load_text(text), b.errors()
    assert b.prepare(8, True) == 0 and plain.prepare(8, True) == 0   # (the builder threads are idle while allocations are counted)
    return b, plain


def child_state(kind):
    A, lib = list_library()
    rng = np.random.default_rng({"gains": 301, "sends": 303, "feeds": 305}[kind])
    N, ch = (65 if kind == "feeds" else 200), 2
    b, plain = handles(A, N, ch)
    st = Structure(kind, lib, b, plain, rng, N, ch)
    W = st.W
    assert W >= 66, W
    g0 = gains_for(rng, ch, W)
    st.install(g0)
    m = GainState(g0)
    sets = [b.info("gain_list_sets"), lib.fxstub_gain_scatters()]

    def values(L):
        return gains_for(rng, ch, W)[:, :len(L)]   # (the specials of gains_for sit in the first columns: +-0, denormals, +-1e30)

    def listed(L, ramp):
        g = values(L)
        st.listed(L, g, ramp)
        m.listed(L, g, ramp)
        sets[0] += 1
        sets[1] += 1
        assert b.info("gain_list_sets") == sets[0]
        assert same_bits(st.get(), m.in_force()), (kind, "get after a list set", ramp)
        assert b.sync() == 0 and lib.fxstub_gain_scatters() == sets[1]   # (the stand-in counts a launch when it has run)

    def full(ramp):
        g = gains_for(rng, ch, W)
        st.full(g, ramp)
        m.full(g, ramp)
        assert b.info("gain_list_sets") == sets[0]
        assert same_bits(st.get(), m.in_force()), (kind, "get after a full set", ramp)

    def block(S):
        st.block(*m.consume(), S)
        assert same_bits(st.get(), m.in_force()), (kind, "get after a block")

    lists = lists_of(rng, W)
    for n, L in enumerate(lists):
        other = lists[(n + 2) % len(lists)]
        S = (33, 1, 2)[n % 3]
        listed(L, 1)          # ramp 1, none pending
        listed(other, 1)      # ramp 1, one pending: a stays everywhere
        block(S)
        block(S)              # ... and the next block is static at the target
        listed(L, 0)          # ramp 0, none pending
        block(S)
        listed(other, 1)
        listed(L, 0)          # ramp 0 while pending: the ramp stays pending for the others
        assert m.pending
        block(S)
        # list sets around full sets
        listed(L, 1)
        full(1)               # a full ramp set behind a list set replaces every target, a stays
        block(S)
        full(1)
        listed(L, 1)
        listed(other, 0)
        block(S)
        listed(L, 1)
        full(0)               # a full set with ramp = 0 cancels the ramp the list set began
        assert not m.pending
        block(S)
        full(0)
        listed(other, 0)
        block(S)
    # count == 0: returns 0 and changes nothing
    assert st.raw_list(None, None, 1) == 0 and st.raw_list(np.zeros(1, dtype=np.int64), g0, 0, count=0) == 0
    assert b.info("gain_list_sets") == sets[0] and same_bits(st.get(), m.in_force()) and not m.pending
    block(5)
    # full-list equivalence: every index with ramp = 1 leaves what the full set with ramp = 1 leaves
    c, plain2 = handles(A, N, ch)
    st2 = Structure(kind, lib, c, plain2, rng, N, ch)
    if kind != "gains":
        st2.off = st.off
        st2.mem, st2.src = getattr(st, "mem", None), getattr(st, "src", None)
    base, g = m.in_force().copy(), gains_for(rng, ch, W)
    st2.install(base)
    perm = rng.permutation(W)
    st.full(g, 1)
    st2.listed(perm, g[:, perm], 1)
    assert same_bits(st.get(), st2.get()) and same_bits(st.get(), base)
    x_state = rng.bit_generator.state
    one = st.block(base, g, True, 9)
    rng.bit_generator.state = x_state   # (the same input block)
    two = st2.block(base, g, True, 9)
    assert same_words(one, two) and same_bits(st.get(), st2.get()) and same_bits(st.get(), g)
    if kind == "feeds":
        # feeds going from unweighted: the call makes them weighted first, a = b = 1.0f everywhere; count 0 does not
        ones = np.ones((ch, W), dtype=np.float32)
        for ramp in (1, 0):
            st.install(None)
            u = GainState(ones)
            st.block(None, None, False, 5)
            assert st.raw_list(None, None, ramp) == 0 and same_bits(st.get(), ones)
            st.block(None, None, False, 5)
            L = lists[2]
            gl = values(L)
            st.listed(L, gl, ramp)
            u.listed(L, gl, ramp)
            assert same_bits(st.get(), u.in_force()) and u.pending == bool(ramp)
            st.block(*u.consume(), 7)
            st.block(*u.consume(), 7)
            assert same_bits(st.get(), u.in_force())
    assert lib.fxstub_gain_scatter_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain list state ok")


def child_streams():
    """a list set behind a slow block on another stream: the block keeps its weights, the next block has the new ones, and the
    call returns while the block is still running (its last output row still holds the mark it was given)"""
    A, lib = list_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(311)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    N, S, K, ch = 1000, 8, 64, 1
    SLOW = 150000   # the emulation launch takes 150 ms: a set that waits for the block in front of it is caught, and so is one that is not ordered behind it
    for kind in ("gains", "sends", "feeds"):
        b, plain = handles(A, N, ch)
        st = Structure(kind, lib, b, plain, rng, N, ch)
        W, G = st.W, b.bus_groups(K)
        g0 = gains_for(rng, ch, W)
        st.install(g0)
        m = GainState(g0)
        st.block(*m.consume(), S)   # (code generated, scratch and staging allocated)
        width_in = st.M if kind == "feeds" else G
        width_out = N if kind == "feeds" else G

        def fresh():
            p, o, a = pinned((S, ch, width_in)), pinned((S, ch, width_out)), pinned((S, ch, 3))
            p[...] = source_block(rng, (S, ch, width_in)) if kind == "feeds" else signal(rng, (S, ch, width_in))
            o[...] = -7.0
            a[...] = -7.0
            return p, o, a

        def dev(bufs, stream):
            p, o, a = bufs
            if kind == "gains":
                return lib.fxb_process_block_bus_dev(b._h, ptr(p), ptr(o), S, K, 3, stream)
            if kind == "sends":
                return auxed_dev(lib, b, p, o, None, a, S, K, 3, stream)
            return fed_dev(lib, b, p, o, None, None, S, K, 0, stream)

        def want(bufs, a, bb, ramp):
            p = bufs[0]
            if kind == "feeds":
                return plain.process_block(feed_model(p, st.off, st.src, a, bb, ramp, S))
            y = plain.process_block(expand(p, K, N))
            return gain_mix_model(y, a, bb, ramp, S, K) if kind == "gains" else send_model(y, st.off, st.mem, a, bb, ramp, S)

        result = (lambda bufs: bufs[2]) if kind == "sends" else (lambda bufs: bufs[1])
        first, second, third, fourth = fresh(), fresh(), fresh(), fresh()
        L1, L2 = np.array([0, W - 1, W // 2], dtype=np.int64), rng.permutation(W)[:65].astype(np.int64)
        v1, v2, v3 = gains_for(rng, ch, W)[:, :3], gains_for(rng, ch, W)[:, :65], gains_for(rng, ch, W)[:, :3]
        lib.fxstub_set_kernel_micros(SLOW)
        assert dev(first, streams[0]) == 0
        args1 = m.consume()
        st.listed(L1, v1, 0)
        assert (result(first)[S - 1] == -7.0).all(), "the list set returned while the block in front of it was still running"
        lib.fxstub_set_kernel_micros(150)
        m.listed(L1, v1, 0)
        assert dev(second, streams[1]) == 0
        args2 = m.consume()
        # a ramp by list behind it, consumed by a block on the first stream; then ramp = 0 by list while a second ramp is pending
        st.listed(L2, v2, 1)
        m.listed(L2, v2, 1)
        assert dev(third, streams[0]) == 0
        args3 = m.consume()
        st.listed(L2, v2[:, ::-1].copy(), 1)
        m.listed(L2, v2[:, ::-1], 1)
        st.listed(L1, v3, 0)
        m.listed(L1, v3, 0)
        assert dev(fourth, None) == 0
        args4 = m.consume()
        assert b.sync() == 0
        for what, bufs, args in (("first", first, args1), ("second", second, args2), ("third", third, args3), ("fourth", fourth, args4)):
            assert same_words(result(bufs), want(bufs, *args)), (kind, what, "block: the weights it was queued with")
        assert same_bits(st.get(), m.in_force())
        if kind != "gains":
            # the full set drains a list set still in flight before it writes
            lib.fxstub_set_kernel_micros(30000)
            assert dev(first, streams[0]) == 0
            args1 = m.consume()
            st.listed(L2, v2, 1)
            m.listed(L2, v2, 1)
            g = gains_for(rng, ch, W)
            st.full(g, 1)
            m.full(g, 1)
            lib.fxstub_set_kernel_micros(150)
            assert dev(second, streams[1]) == 0 and b.sync() == 0
            assert same_words(result(first), want(first, *args1)) and same_words(result(second), want(second, *m.consume())), (kind, "a full set behind a list set")
        pinned.free()
        b.close()
        plain.close()
    assert lib.fxstub_gain_scatter_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain list streams ok")


def child_pieces():
    A, lib = list_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(313)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples, one S
    N, S, K = 262144, 96, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    g0 = gains_for(rng, 1, N)
    assert b.bus_set_gains(g0) == 0
    m = GainState(g0)
    L = np.concatenate([[0, N - 1], rng.permutation(np.arange(1, N - 1))[:1022]]).astype(np.int64)
    v = gains_for(rng, 1, N)[:, :L.size].copy()
    assert lib.fxb_bus_set_gains_list(b._h, ptr(L), L.size, ptr(v), 1) == 0
    m.listed(L, v, 1)
    mixes = lib.fxstub_bus_gain_mixes()
    pg, po = pinned((S, 1, G)), pinned((S, 1, G))
    pg[...] = rng.standard_normal((S, 1, G)).astype(np.float32)
    x = expand(pg, K, N)
    a, bb, ramp = m.consume()
    assert ramp and bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, gain_mix_model(x, a, bb, True, S, K)), "a ramp begun by a list set across two pieces"
    assert lib.fxstub_bus_gain_mixes() == mixes + 2
    assert same_bits(b.bus_get_gains(), bb) and b.info("gain_list_sets") == 1
    assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, gain_mix_model(x, bb, bb, False, S, K)), "the next block is static"
    # a few entries out of many instances (the repeats are then looked for in a sorted copy, not in a bitmap over the range)
    few, twice = np.array([N - 1, 7, 0], dtype=np.int64), np.array([N - 1, 7, N - 1], dtype=np.int64)
    assert lib.fxb_bus_set_gains_list(b._h, ptr(twice), 3, ptr(v), 0) == FX_E_ARG and "more than once" in b.last_error()
    assert b.info("gain_list_sets") == 1 and same_bits(b.bus_get_gains(), bb)
    assert lib.fxb_bus_set_gains_list(b._h, ptr(few), 3, ptr(v), 0) == 0
    m.listed(few, v[:, :3], 0)
    assert same_bits(b.bus_get_gains(), m.in_force()) and b.info("gain_list_sets") == 2
    pinned.free()
    print("gain list pieces ok")


def child_refusals():
    A, lib = list_library()
    rng = np.random.default_rng(317)
    N, ch, S = 200, 2, 8
    for kind in ("gains", "sends", "feeds"):
        b, plain = handles(A, N, ch)
        st = Structure(kind, lib, b, plain, rng, N, ch)
        W = st.W
        good_L, good_g = np.array([3, 0, W - 1], dtype=np.int64), gains_for(rng, ch, W)[:, :3].copy()
        # the mode being off: a list call does not switch it on
        for ramp in (0, 1):
            assert st.raw_list(good_L, good_g, ramp) == FX_E_ARG and "off" in b.last_error(), (kind, b.last_error())
        if kind == "gains":
            assert lib.fxb_bus_get_gains(b._h, ptr(np.zeros((ch, N), dtype=np.float32))) == FX_E_ARG
        g0 = gains_for(rng, ch, W)
        st.install(g0)
        m = GainState(g0)
        for state in ("static", "pending"):
            if state == "pending":
                g1 = gains_for(rng, ch, W)
                st.full(g1, 1)
                m.full(g1, 1)
            sets, scatters = b.info("gain_list_sets"), lib.fxstub_gain_scatters()
            refused = []
            for ramp in (0, 1):
                refused.append(("a repeated index", np.array([5, 9, 5], dtype=np.int64), good_g, ramp, None))
                refused.append(("an index of W", np.array([0, W, 1], dtype=np.int64), good_g, ramp, None))
                refused.append(("an index of -1", np.array([0, 1, -1], dtype=np.int64), good_g, ramp, None))
                for value, at in ((np.nan, (0, 0)), (np.inf, (ch - 1, 2)), (-np.inf, (0, 1))):
                    bad = good_g.copy()
                    bad[at] = value
                    refused.append(("a value that is not finite", good_L, bad, ramp, None))
                refused.append(("count < 0", good_L, good_g, ramp, -1))
                refused.append(("a null list", None, good_g, ramp, 3))
                refused.append(("null gains", good_L, None, ramp, 3))
            for ramp in (2, -1, 256):
                refused.append(("a bad ramp", good_L, good_g, ramp, None))
                refused.append(("a bad ramp with nothing listed", None, None, ramp, 0))
            for what, L, g, ramp, count in refused:
                assert st.raw_list(L, g, ramp, count) == FX_E_ARG and b.last_error(), (kind, state, what)
                assert b.info("gain_list_sets") == sets and lib.fxstub_gain_scatters() == scatters, (kind, state, what)
            assert {"gains": lib.fxb_bus_set_gains_list, "sends": lib.fxb_bus_set_send_gains_list, "feeds": lib.fxb_bus_set_feed_gains_list}[kind](None, ptr(good_L), 3, ptr(good_g), 0) == FX_E_ARG
            assert same_bits(st.get(), m.in_force()), (kind, state)
            st.block(*m.consume(), S)
            st.block(*m.consume(), S)
        # an allocation that fails, at each allocation of the call (the device staging, the pinned staging): FX_E_MEMORY, nothing
        # changed (a handle without a program: no builder thread allocates meanwhile; the program comes afterwards)
        for ramp in (1, 0):
            for nth in (0, 1):
                c, plain2 = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
                st2 = Structure(kind, lib, c, plain2, rng, N, ch)
                for name in ("off", "mem", "src"):
                    if hasattr(st, name):
                        setattr(st2, name, getattr(st, name))
                st2.install(g0)
                m2 = GainState(g0)
                lib.fxstub_fail_mallocs(nth, 1)
                rc = st2.raw_list(good_L, good_g, ramp)
                lib.fxstub_fail_mallocs(-1, 0)
                assert rc == FX_E_MEMORY and c.last_error(), (kind, ramp, nth, rc)
                assert c.info("gain_list_sets") == 0 and same_bits(st2.get(), g0)
                assert c.load_text(STEREO) and plain2.load_text(STEREO), c.errors()
                st2.block(*m2.consume(), S)
                st2.listed(good_L, good_g, ramp)   # ... and the same call goes through afterwards
                m2.listed(good_L, good_g, ramp)
                assert same_bits(st2.get(), m2.in_force()) and c.info("gain_list_sets") == 1
                st2.block(*m2.consume(), S)
                c.close()
                plain2.close()
        b.close()
        plain.close()
    assert lib.fxstub_gain_scatter_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain list refusals ok")


def child_shards():
    """three shards against the model, which the single handle of the other children equals: lists on every shard, a list wholly
    inside one shard that starts a ramp (get and a ramp block on all shards), allocation failures on whichever shard"""
    A, lib = list_library()
    rng = np.random.default_rng(331)
    N, S, ch = 3 * 256 + 40, 9, 2
    bounds = [(0, 320), (320, 576), (576, N)]
    for kind in ("gains", "sends", "feeds"):
        b, plain = A.Batch(N, ch, devices=[0, 1, 2]), A.Batch(N, ch, 0)
        single, plain1 = handles(A, N, ch)
        assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
        assert b.load_text(STEREO) and plain.load_text(STEREO), b.errors()
        st = Structure(kind, lib, b, plain, rng, N, ch)
        st.K = 64
        if kind == "sends":
            # a bus is summed where its members live: buses on the last, the first and the middle shard, and an empty one
            spec = ((2, 65), (0, 1030), (1, 3), (0, 0), (1, 64))
            lists = [rng.integers(bounds[s][0], bounds[s][1], n) for s, n in spec]
            st.off = np.concatenate([[0], np.cumsum([n for _, n in spec])]).astype(np.int64)
            st.mem = np.concatenate(lists).astype(np.int64)
            st.W = int(st.off[-1])
            inside = np.arange(st.off[2], st.off[3])                 # the entries of the bus of the middle shard
        elif kind == "feeds":
            inside = np.arange(st.off[330], st.off[560])[:70]        # entries of instances of the middle shard
        else:
            inside = np.arange(330, 400)
        st1 = Structure(kind, lib, single, plain1, rng, N, ch)
        st1.K = 64
        for name in ("off", "mem", "src", "W", "M"):
            if hasattr(st, name):
                setattr(st1, name, getattr(st, name))
        W = st.W
        g0 = gains_for(rng, ch, W)
        st.install(g0)
        st1.install(g0)
        m = GainState(g0)
        inside = rng.permutation(inside).astype(np.int64)
        everywhere = np.concatenate([[0, W - 1], rng.permutation(np.arange(1, W - 1))[:128]]).astype(np.int64)
        scatters = lib.fxstub_gain_scatters()

        def listed(L, ramp):
            g = gains_for(rng, ch, W)[:, :L.size].copy()
            st.listed(L, g, ramp)
            st1.listed(L, g, ramp)
            m.listed(L, g, ramp)
            assert same_bits(st.get(), m.in_force()) and same_bits(st1.get(), m.in_force()), (kind, "get assembles one state from all shards")

        def block():
            args = m.consume()
            state = rng.bit_generator.state
            one = st.block(*args, S)
            rng.bit_generator.state = state   # (the same input block)
            assert same_words(one, st1.block(*args, S)), (kind, "three shards equal the single handle")
            assert same_bits(st.get(), m.in_force()) and same_bits(st1.get(), m.in_force())

        before = b.info("gain_list_sets")
        listed(inside, 1)   # wholly inside the middle shard, and it starts a ramp: every shard follows
        assert b.info("gain_list_sets") == before + 1, "a shard without an entry launches nothing"
        block()
        block()
        listed(everywhere, 1)
        listed(inside, 1)
        block()
        listed(everywhere, 1)
        listed(inside, 0)   # ramp = 0 while pending, inside one shard
        block()
        listed(inside, 0)
        listed(everywhere, 0)
        block()
        assert lib.fxstub_gain_scatters() - scatters == b.info("gain_list_sets") - before + single.info("gain_list_sets")
        # refused for the whole handle, in front of every shard
        sets = b.info("gain_list_sets")
        bad = np.array([0, W - 1, 0], dtype=np.int64)
        assert st.raw_list(bad, g0[:, :3].copy(), 1) == FX_E_ARG and st.raw_list(np.array([W], dtype=np.int64), g0[:, :1].copy(), 1) == FX_E_ARG
        # an allocation that fails on whichever shard - two per shard, each shard has entries: FX_E_MEMORY, and no shard has
        # changed (handles without a program: no builder thread allocates meanwhile)
        for nth in range(6):
            c = A.Batch(N, ch, devices=[0, 1, 2])
            st2 = Structure(kind, lib, c, None, rng, N, ch)
            for name in ("off", "mem", "src", "W", "M"):
                if hasattr(st, name):
                    setattr(st2, name, getattr(st, name))
            st2.install(g0)
            g = gains_for(rng, ch, W)[:, :everywhere.size].copy()
            lib.fxstub_fail_mallocs(nth, 1)
            rc = st2.raw_list(everywhere, g, 1)
            lib.fxstub_fail_mallocs(-1, 0)
            assert rc == FX_E_MEMORY and c.last_error(), (kind, nth, rc)
            assert c.info("gain_list_sets") == 0 and same_bits(st2.get(), g0)
            st2.listed(everywhere, g, 0)   # (had the ramp begun on some shard, get would now show its a there)
            want = g0.copy()
            want[:, everywhere] = g
            assert same_bits(st2.get(), want) and c.info("gain_list_sets") == 3
            c.close()
        assert b.info("gain_list_sets") == sets
        block()
        listed(rng.permutation(W).astype(np.int64), 1)
        block()
        assert (b.save_state() == single.save_state()).all()
        for h in (b, plain, single, plain1):
            h.close()
    assert lib.fxstub_gain_scatter_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("gain list shards ok")


if __name__ == "__main__":
    which = sys.argv[1]
    if which.startswith("state-"):
        child_state(which[6:])
    else:
        {"streams": child_streams, "pieces": child_pieces, "refusals": child_refusals, "shards": child_shards}[which]()
