"""Group buses without a GPU: the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc
stublib`), driven through the C ABI in a child process (the binding reads FX8010_AMD_LIB once, at import; this file is also that
child).  The stand-in's emulation kernel copies in to out and the stand-ins of the two bus kernels (tests/hipstub/fx_bus_stub.cpp)
do their real work in stream order, so out == mix_model(expand(in)) must hold word for word: that checks the host routing - in
place on pinned buffers, staged for pageable ones, the device entry, pieces of a block above the scratch limit, shards on three
devices - and the stand-in's mix against the numpy model below.  Launches are counted per route; refusals launch nothing.  Parity
with the emulation itself is tests/test_gpu_bus.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from route_models import mix_model, expand, same_words  # noqa: E402,F401  (the models live there; the tests of them stay here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_NODEVICE, FX_E_ARG, FX_E_MEMORY = -1, -3, -5
SHARED_IN, MIX_OUT = 1, 2
HIP_LAUNCH_FAILURE = 719
PROGRAM = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
STEREO = PROGRAM.replace("output out 0", "input in1 1\noutput out 0\noutput out1 1").replace("\nend", "\nmacs out1, in1, a, 0.5\nend")


def test_mix_model_is_the_order_it_says():
    """the vectorised model against the order written out one add at a time"""
    rng = np.random.default_rng(3)
    for N, K in ((1, 1), (5, 2), (64, 64), (65, 64), (200, 63), (200, 65), (777, 130), (777, 777), (300, 1000)):
        y = (rng.standard_normal((3, N)) * 10.0 ** rng.integers(-6, 6, (3, N))).astype(np.float32)
        y[0, 0] = -0.0
        k = min(K, N)
        want = np.zeros((3, -(-N // k)), dtype=np.float32)
        for r in range(3):
            for g in range(want.shape[1]):
                p = [np.float32(0.0)] * 64
                for m, v in enumerate(y[r, g * k:min((g + 1) * k, N)]):
                    p[m % 64] = np.float32(p[m % 64] + v)
                for step in (32, 16, 8, 4, 2, 1):
                    for l in range(step):
                        p[l] = np.float32(p[l] + p[l + step])
                want[r, g] = p[0]
        assert same_words(mix_model(y, K), want), (N, K)
    assert np.signbit(mix_model(np.full((1, 2), -0.0, dtype=np.float32), 1)).sum() == 0, "+0.0 + -0.0 is +0.0"
    assert np.isnan(mix_model(np.array([[1.0, np.nan, np.inf, -np.inf]], dtype=np.float32), 2)).tolist() == [[True, True]]


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_bus_values_and_routes_on_the_hip_stand_in():
    run_child("routes", "bus routes ok")


def test_bus_refusals_launch_nothing_on_the_hip_stand_in():
    run_child("refusals", "bus refusals ok")


def test_bus_pieces_and_error_paths_on_the_hip_stand_in():
    run_child("pieces", "bus pieces ok")


def test_bus_blocks_on_a_second_stream_on_the_hip_stand_in():
    """fxb_sync alone covers a device-entry block on the caller's stream, and the one scratch block is not refilled while the
    previous bus block - on whatever stream - still works on it"""
    run_child("streams", "bus streams ok")


def test_bus_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "bus shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_kernels_run", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_bus_expands", "fxstub_bus_mixes"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_launches.argtypes = [C.c_long, C.c_long, C.c_int]
    lib.fxstub_fail_launches.restype = None
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    return A, lib


class Pinned:
    """float32 numpy views of fxb_host_alloc memory, freed together"""

    def __init__(self, lib):
        self.lib, self.held = lib, []

    def __call__(self, shape):
        count = int(np.prod(shape))
        p = self.lib.fxb_host_alloc(max(count, 1) * 4)
        assert p, self.lib.fx_last_create_error()
        self.held.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(max(count, 1),))[:count].reshape(shape)

    def free(self):
        for p in self.held:
            self.lib.fxb_host_free(p)
        self.held = []


class Counts:
    """what has happened since the last look: (emulation launches, expands, mixes, staged, in place, bus blocks)"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_bus_expands(), self.lib.fxstub_bus_mixes(),
                self.b.info("host_staged_blocks"), self.b.info("host_inplace_blocks"), self.b.info("bus_blocks"))

    def expect(self, what, *want):
        now = self.now()
        got = tuple(a - b for a, b in zip(now, self.seen))
        assert got == want, (what, got, want)
        self.seen = now


def bus(lib, b, x, y, S, K, flags):
    return lib.fxb_process_block_bus(b._h, C.c_void_p(x.ctypes.data if x is not None else 0), C.c_void_p(y.ctypes.data if y is not None else 0), S, K, flags)


def child_routes():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(11)
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N in (1, 63, 64, 65, 200, 1000):
            b = A.Batch(N, ch, 0)
            assert b.load_text(text), b.errors()
            count = Counts(lib, b)
            for K in (1, 2, 63, 64, 65, 128, 1000, N, N + 5):
                G = b.bus_groups(K)
                assert G == -(-N // K) and lib.fxb_bus_groups(b._h, 0) == FX_E_ARG
                for S in (1, 7):
                    xg = (rng.standard_normal((S, ch, G)) * 10.0 ** rng.integers(-8, 8, (S, ch, G))).astype(np.float32)
                    xn = expand(xg, K, N)
                    # pageable buffers: the [S][C][G] sides are staged, the [S][C][N] sides are copied to and from the scratch
                    assert same_words(b.process_block_bus(xg, K, True, False), xn), (N, K, S, "shared in")
                    count.expect("shared in, staged", 1, 1, 0, 1, 0, 1)
                    assert same_words(b.process_block_bus(xn, K, False, True), mix_model(xn, K)), (N, K, S, "mix out")
                    count.expect("mix out, staged", 1, 0, 1, 1, 0, 1)
                    assert same_words(b.process_block_bus(xg, K, True, True), mix_model(xn, K)), (N, K, S, "both")
                    count.expect("both, staged", 1, 1, 1, 1, 0, 1)
                # pinned buffers: in place, and on one buffer with one layout
                S = 5
                pg, po, pn = pinned((S, ch, G)), pinned((S, ch, G)), pinned((S, ch, N))
                pg[...] = (rng.standard_normal((S, ch, G)) * 4).astype(np.float32)
                want = mix_model(expand(pg, K, N), K)
                assert bus(lib, b, pg, po, S, K, SHARED_IN | MIX_OUT) == 0 and same_words(po, want), (N, K, b.last_error())
                count.expect("both, in place", 1, 1, 1, 0, 1, 1)
                assert bus(lib, b, pg, pn, S, K, SHARED_IN) == 0 and same_words(pn, expand(pg, K, N)), (N, K, b.last_error())
                count.expect("shared in, in place", 1, 1, 0, 0, 1, 1)
                assert bus(lib, b, pn, po, S, K, MIX_OUT) == 0 and same_words(po, want), (N, K, b.last_error())
                count.expect("mix out, in place", 1, 0, 1, 0, 1, 1)
                assert bus(lib, b, pg, pg, S, K, SHARED_IN | MIX_OUT) == 0 and same_words(pg, want), (N, K, b.last_error())
                count.expect("both, one buffer", 1, 1, 1, 0, 1, 1)
                # one pinned, one pageable: staged
                y = np.zeros((S, ch, G), dtype=np.float32)
                assert bus(lib, b, pn, y, S, K, MIX_OUT) == 0 and same_words(y, mix_model(pn, K))
                count.expect("pinned in, pageable out", 1, 0, 1, 1, 0, 1)
                # flags == 0 is fxb_process_block; zero samples: success, nothing launched
                assert bus(lib, b, pn, pn, S, K, 0) == 0
                small = S * ch * N <= 512   # (a few KB go through the library's own pinned pair, counted as staged)
                count.expect("no flags", 1, 0, 0, 1 if small else 0, 0 if small else 1, 0)
                assert bus(lib, b, pg, po, 0, K, SHARED_IN | MIX_OUT) == 0 and bus(lib, b, None, None, 0, K, MIX_OUT) == 0
                count.expect("zero samples", 0, 0, 0, 0, 0, 0)
                pinned.free()
            # the device entry: device-visible memory on the handle's own stream; a pageable pointer is refused
            K, S = 64, 4
            G = b.bus_groups(K)
            pg, po = pinned((S, ch, G)), pinned((S, ch, G))
            pg[...] = 0.375
            for rep in range(2):   # (the second time: the pair that has passed once)
                assert b.process_block_bus_dev(int(pg.ctypes.data), int(po.ctypes.data), S, K) == 0 and b.sync() == 0
                assert same_words(po, mix_model(expand(pg, K, N), K))
            count.expect("device entry", 2, 2, 2, 0, 0, 2)
            page = np.zeros((S, ch, G), dtype=np.float32)
            assert lib.fxb_process_block_bus_dev(b._h, C.c_void_p(page.ctypes.data), C.c_void_p(po.ctypes.data), S, K, 3, None) == FX_E_ARG
            assert "not memory of this handle's device" in b.last_error(), b.last_error()
            assert lib.fxb_process_block_bus_dev(b._h, C.c_void_p(pg.ctypes.data), C.c_void_p(po.ctypes.data), S + 1, K, 3, None) == FX_E_ARG   # beyond the allocation
            count.expect("device entry, refused", 0, 0, 0, 0, 0, 0)
            pinned.free()
    # a schedule armed for the block applies (the interpreter tier cuts the block at its steps, on the scratch)
    os.environ["FX_KERNEL"] = "asm"
    t = A.Batch(200, 1, 0)
    del os.environ["FX_KERNEL"]
    assert t.load_text(PROGRAM), t.errors()
    x = np.ones((32, 1, 4), dtype=np.float32)
    assert same_words(t.process_block_bus(x, 64), mix_model(expand(x, 64, 200), 64))
    assert t.set_register_track("vol", [0.1, 0.2, 0.3, 0.4], 8) == 0
    k0 = lib.fxstub_kernels_run()
    assert same_words(t.process_block_bus(x, 64), mix_model(expand(x, 64, 200), 64))
    assert lib.fxstub_kernels_run() - k0 == 4 and abs(t.get_register_i("vol", 3) - 0.4) < 1e-6
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("bus routes ok")


def child_refusals():
    A, lib = stub_library()
    pinned = Pinned(lib)
    N, S, K = 300, 8, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    xg, yg, xn = pinned((S, 1, G)), pinned((S, 1, G)), pinned((S, 1, N))
    both = pinned((2 * S, 1, N))
    xg[...] = 0.5
    assert bus(lib, b, xg, yg, S, K, 3) == 0
    ms = b.last_kernel_ms()
    count = Counts(lib, b)
    at = lambda a, off: C.c_void_p(a.ctypes.data + off * 4)
    refused = [
        ("group 0", lambda: bus(lib, b, xg, yg, S, 0, 3)), ("group < 0", lambda: bus(lib, b, xg, yg, S, -64, 3)),
        ("unknown flag", lambda: bus(lib, b, xg, yg, S, K, 4)), ("unknown flags", lambda: bus(lib, b, xg, yg, S, K, 3 | 1 << 31)),
        ("group 0 without flags", lambda: bus(lib, b, xn, xn, S, 0, 0)),
        ("null in", lambda: bus(lib, b, None, yg, S, K, 3)), ("null out", lambda: bus(lib, b, xg, None, S, K, 3)),
        ("negative length", lambda: bus(lib, b, xg, yg, -1, K, 3)),
        # one buffer, two layouts; footprints that share bytes
        ("one buffer, shared in only", lambda: lib.fxb_process_block_bus(b._h, at(both, 0), at(both, 0), S, K, SHARED_IN)),
        ("one buffer, mix out only", lambda: lib.fxb_process_block_bus(b._h, at(both, 0), at(both, 0), S, K, MIX_OUT)),
        ("shifted by three words", lambda: lib.fxb_process_block_bus(b._h, at(both, 0), at(both, 3), S, K, 3)),
        ("out inside in", lambda: lib.fxb_process_block_bus(b._h, at(both, 0), at(both, S * N - 1), S, K, MIX_OUT)),
        ("in inside out", lambda: lib.fxb_process_block_bus(b._h, at(both, S * N - 1), at(both, 0), S, K, SHARED_IN)),
        ("device entry, group 0", lambda: lib.fxb_process_block_bus_dev(b._h, at(xg, 0), at(yg, 0), S, 0, 3, None)),
        ("device entry, unknown flag", lambda: lib.fxb_process_block_bus_dev(b._h, at(xg, 0), at(yg, 0), S, K, 8, None)),
        ("device entry, null", lambda: lib.fxb_process_block_bus_dev(b._h, None, at(yg, 0), S, K, 3, None)),
        ("device entry, overlap", lambda: lib.fxb_process_block_bus_dev(b._h, at(both, 0), at(both, 1), S, K, 3, None)),
    ]
    for what, call in refused:
        assert call() == FX_E_ARG and b.last_error(), what
        count.expect(what, 0, 0, 0, 0, 0, 0)
        assert b.last_kernel_ms() == ms, what
    # ... and the block that touches without overlapping is not one of them
    assert lib.fxb_process_block_bus(b._h, at(both, 0), at(both, S * N), S, K, MIX_OUT) == 0, b.last_error()
    assert lib.fxb_process_block_bus(b._h, None, None, 0, K, 3) == 0
    # channels * row length * 4 must stay below 2^32 in every layout (refused in front of everything: no program needed)
    wide = A.Batch(1 << 28, 4, 0)
    k0 = lib.fxstub_kernels_run()
    for flags in (1, 2, 3):
        for K in (1, 64, 1 << 28):
            assert lib.fxb_process_block_bus(wide._h, at(xg, 0), at(yg, 0), 1, K, flags) == FX_E_ARG and "2^32" in wide.last_error(), (flags, K)
    assert lib.fxstub_kernels_run() == k0 and wide.info("bus_blocks") == 0
    assert lib.fxb_process_block_bus(None, at(xg, 0), at(yg, 0), 1, 1, 3) == FX_E_ARG and lib.fxb_bus_groups(None, 4) == FX_E_ARG
    assert bus(lib, b, xg, yg, S, K, 3) == 0, "the handle stays usable"
    pinned.free()
    print("bus refusals ok")


def child_pieces():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(17)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples
    N, S, K = 262144, 96, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    G = b.bus_groups(K)
    count = Counts(lib, b)
    xg = rng.standard_normal((S, 1, G)).astype(np.float32)
    want = mix_model(expand(xg, K, N), K)
    assert same_words(b.process_block_bus(xg, K), want)
    count.expect("two pieces, staged", 2, 2, 2, 1, 0, 1)
    pg, po = pinned((S, 1, G)), pinned((S, 1, G))
    pg[...] = xg
    assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, want)
    count.expect("two pieces, in place", 2, 2, 2, 0, 1, 1)
    assert bus(lib, b, pg, po, 64, K, 3) == 0 and same_words(po[:64], want[:64])
    count.expect("64 MiB exactly: one piece", 1, 1, 1, 0, 1, 1)
    assert bus(lib, b, pg, po, 65, K, 3) == 0 and same_words(po[:65], want[:65])
    count.expect("one sample more: two pieces", 2, 2, 2, 0, 1, 1)
    # with a schedule armed the block stays whole, on a scratch block grown for it
    assert b.set_register_track("vol", [0.1, 0.2], 48) == 0
    assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, want), b.last_error()
    count.expect("armed: one piece", 1, 1, 1, 0, 1, 1)
    # ... and FX_E_MEMORY where that block cannot be had; the handle stays usable
    big = A.Batch(N, 2, 0)
    assert big.load_text(STEREO), big.errors()
    x2 = np.zeros((S, 2, G), dtype=np.float32)
    assert big.process_block_bus(x2[:8], K) is not None
    assert big.set_register_track("vol", [0.1, 0.2], 48) == 0
    k0 = lib.fxstub_kernels_run()
    lib.fxstub_fail_mallocs(0, 1)
    y2 = np.zeros_like(x2)
    assert bus(lib, big, x2, y2, S, K, 3) == FX_E_MEMORY, big.last_error()
    lib.fxstub_fail_mallocs(-1, 0)
    assert lib.fxstub_kernels_run() == k0
    assert bus(lib, big, x2, y2, S, K, 3) == 0, big.last_error()
    # a launch that fails: reported on both routes, nothing left running on the caller's memory, the next block works
    for what, x, y in (("staged", xg, np.zeros_like(xg)), ("in place", pg, po)):
        lib.fxstub_fail_launches(0, 1, HIP_LAUNCH_FAILURE)
        rc = bus(lib, b, x, y, S, K, 3)
        lib.fxstub_fail_launches(-1, 0, 0)
        assert rc == FX_E_NODEVICE, (what, rc, b.last_error())
        assert bus(lib, b, x, y, S, K, 3) == 0 and same_words(y, want), (what, b.last_error())
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("bus pieces ok")


def child_streams():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(29)
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
    fresh = lambda: (rng.standard_normal((S, 1, G)).astype(np.float32), pinned((S, 1, G)), pinned((S, 1, G)))
    assert b.process_block_bus(np.zeros((S, 1, G), dtype=np.float32), K) is not None   # (code generated, scratch allocated)
    lib.fxstub_set_kernel_micros(30000)   # the emulation launch takes 30 ms: whatever does not wait for what follows it is caught
    for mode in ("both", "mix out", "shared in"):
        flags = {"both": 3, "mix out": MIX_OUT, "shared in": SHARED_IN}[mode]
        xg = rng.standard_normal((S, 1, G)).astype(np.float32)
        src = pinned((S, 1, G if flags & SHARED_IN else N))
        dst = pinned((S, 1, G if flags & MIX_OUT else N))
        src[...] = xg if flags & SHARED_IN else expand(xg, K, N)
        dst[...] = -7.0
        want = mix_model(expand(xg, K, N), K) if flags & MIX_OUT else expand(xg, K, N)
        assert lib.fxb_process_block_bus_dev(b._h, C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data), S, K, flags, streams[0]) == 0, b.last_error()
        assert b.sync() == 0 and same_words(dst, want), "fxb_sync returned before the last kernel of a bus block (%s)" % mode
    # a device-entry block on one stream, at once another on a second stream, at once a host-entry block: three fillings of one scratch
    (xa, pa, ya), (xb, pb, yb), (xc, pc, yc) = fresh(), fresh(), fresh()
    for x, p_ in ((xa, pa), (xb, pb), (xc, pc)):
        p_[...] = x
    assert dev(pa, ya, streams[0]) == 0 and dev(pb, yb, streams[1]) == 0, b.last_error()
    assert bus(lib, b, pc, yc, S, K, 3) == 0, b.last_error()
    assert same_words(yc, mix_model(expand(xc, K, N), K)), "host entry"
    assert b.sync() == 0
    assert same_words(ya, mix_model(expand(xa, K, N), K)), "the first block's scratch was refilled under it"
    assert same_words(yb, mix_model(expand(xb, K, N), K)), "the second block's scratch was refilled under it"
    # ... and a register read right behind a device-entry block sees the block done
    assert dev(pa, ya, streams[1]) == 0 and b.instruction_counter() >= 0 and same_words(ya, mix_model(expand(xa, K, N), K))
    lib.fxstub_set_kernel_micros(150)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("bus streams ok")


def child_shards():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(23)
    N, S = 3 * 256 + 40, 16
    b = A.Batch(N, 1, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    assert b.load_text(PROGRAM), b.errors()
    count = Counts(lib, b)
    for K in (64, 32, 1):
        G = b.bus_groups(K)
        pg, po, pn = pinned((S, 1, G)), pinned((S, 1, G)), pinned((S, 1, N))
        pg[...] = rng.standard_normal((S, 1, G)).astype(np.float32)
        want = mix_model(expand(pg, K, N), K)
        assert bus(lib, b, pg, po, S, K, 3) == 0 and same_words(po, want), (K, b.last_error())
        count.expect("both, in place, every shard on its group columns", 3, 3, 3, 0, 3, 3)
        assert bus(lib, b, pg, pn, S, K, SHARED_IN) == 0 and same_words(pn, expand(pg, K, N)), (K, b.last_error())
        count.expect("shared in", 3, 3, 0, 0, 3, 3)
        assert bus(lib, b, pn, po, S, K, MIX_OUT) == 0 and same_words(po, want), (K, b.last_error())
        count.expect("mix out", 3, 0, 3, 0, 3, 3)
        xg = np.ascontiguousarray(pg)
        assert same_words(b.process_block_bus(xg, K), want)
        count.expect("pageable: every shard stages its columns", 3, 3, 3, 3, 0, 3)
        pinned.free()
    # a group that straddles two shards; the device entry on a handle of several shards
    pg, po = pinned((S, 1, N)), pinned((S, 1, N))
    for K in (100, 128, N):
        assert bus(lib, b, pg, po, S, K, 3) == FX_E_ARG and "straddles" in b.last_error(), (K, b.last_error())
    assert lib.fxb_process_block_bus_dev(b._h, C.c_void_p(pg.ctypes.data), C.c_void_p(po.ctypes.data), S, 64, 3, None) == FX_E_ARG
    assert bus(lib, b, pg, pg, S, 64, MIX_OUT) == FX_E_ARG
    count.expect("refused", 0, 0, 0, 0, 0, 0)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("bus shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "refusals": child_refusals, "pieces": child_pieces, "shards": child_shards, "streams": child_streams}[sys.argv[1]]()
