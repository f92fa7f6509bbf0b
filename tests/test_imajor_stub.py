"""Instance-major blocks without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process (the binding reads FX8010_AMD_LIB once, at
import; this file is also that child).  The stand-in's emulation kernel copies in to out and the stand-ins of the two transposition
kernels (tests/hipstub/fx_imajor_stub.cpp) do their real work in stream order, so out[n, s, c] == in[n, s, c] must hold word for
word on every route - in place on pinned buffers, staged for pageable ones, the device entry, pieces of a block above the scratch
limit, shards on three devices - and the words between two runs of a padded stride must keep what they held.  Launches are counted
per route; refusals launch nothing.  Parity with the emulation itself is tests/test_gpu_imajor.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_NODEVICE, FX_E_ARG, FX_E_MEMORY = -1, -3, -5
PROGRAM = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
STEREO = PROGRAM.replace("output out 0", "input in1 1\noutput out 0\noutput out1 1").replace("\nend", "\nmacs out1, in1, a, 0.5\nend")
SENTINEL = 0x7FC0DEAD   # a NaN with a payload: survives only as a bit pattern


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_imajor_values_and_routes_on_the_hip_stand_in():
    run_child("routes", "imajor routes ok")


def test_imajor_refusals_launch_nothing_on_the_hip_stand_in():
    run_child("refusals", "imajor refusals ok")


def test_imajor_pieces_on_the_hip_stand_in():
    run_child("pieces", "imajor pieces ok")


def test_imajor_blocks_on_a_second_stream_and_between_bus_blocks_on_the_hip_stand_in():
    """fxb_sync alone covers a device-entry block on the caller's stream, and the one scratch block is not refilled - by a block of
    either kind, on whatever stream - while the previous block still works on it"""
    run_child("streams", "imajor streams ok")


def test_imajor_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "imajor shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_kernels_run", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_bus_expands", "fxstub_bus_mixes",
              "fxstub_imajor_gathers", "fxstub_imajor_scatters"):
        getattr(lib, f).restype = C.c_long
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
    """what has happened since the last look: (emulation launches, gathers, scatters, staged, in place, instance-major blocks, bus blocks)"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_imajor_gathers(), self.lib.fxstub_imajor_scatters(),
                self.b.info("host_staged_blocks"), self.b.info("host_inplace_blocks"), self.b.info("imajor_blocks"), self.b.info("bus_blocks"))

    def expect(self, what, *want):
        now = self.now()
        got = tuple(a - b for a, b in zip(now, self.seen))
        assert got == want, (what, got, want)
        self.seen = now


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def words(rng, shape):
    """every kind of word: the transposition moves patterns"""
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(np.float32)


def imajor(lib, b, x, y, S, in_stride=0, out_stride=0):
    ptr = lambda a: C.c_void_p(a if isinstance(a, int) else (a.ctypes.data if a is not None else 0))
    return lib.fxb_process_block_imajor(b._h, ptr(x), ptr(y), S, in_stride, out_stride)


def padded(alloc, N, stride, tail=0):
    """[N][stride] (+ tail words) full of the sentinel, flat"""
    a = alloc((N * stride + tail,))
    a.view(np.uint32)[...] = SENTINEL
    return a


def runs(flat, N, R, stride, first=0):
    """the N runs of R words at `stride` from word `first` on: a [N, R] view"""
    return np.lib.stride_tricks.as_strided(flat[first:], shape=(N, R), strides=(stride * 4, 4))


def only_runs_changed(flat, N, R, stride, first=0):
    """every word outside the N runs still holds the sentinel"""
    mask = np.ones(flat.size, dtype=bool)
    idx = (first + np.arange(N)[:, None] * stride + np.arange(R)[None, :]).ravel()
    mask[idx] = False
    return bool((flat.view(np.uint32)[mask] == SENTINEL).all())


def child_routes():
    A, lib = stub_library()
    pinned = Pinned(lib)
    pageable = lambda shape: np.zeros(shape, dtype=np.float32)
    rng = np.random.default_rng(11)
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N in (1, 63, 64, 65, 200, 1000):
            b = A.Batch(N, ch, 0)
            assert b.load_text(text), b.errors()
            count = Counts(lib, b)
            for S in (1, 7, 33):
                R = S * ch
                x = words(rng, (N, S, ch))
                # pageable buffers: the runs are staged as the rows of a 2-D copy
                assert same_bits(b.process_block_imajor(x), x), (N, S, "staged")
                count.expect("staged", 1, 1, 1, 1, 0, 1, 0)
                for route, alloc, staged in (("staged", pageable, 1), ("in place", pinned, 0)):
                    # padded strides, the padding pre-filled: intact afterwards on both buffers
                    si, so = R + 3, R + 5
                    fin, fout = padded(alloc, N, si), padded(alloc, N, so)
                    runs(fin, N, R, si)[...] = x.reshape(N, R)
                    assert imajor(lib, b, fin, fout, S, si, so) == 0, b.last_error()
                    count.expect(route + ", padded", 1, 1, 1, staged, 1 - staged, 1, 0)
                    assert same_bits(runs(fout, N, R, so), x.reshape(N, R)) and same_bits(runs(fin, N, R, si), x.reshape(N, R)), (N, S, route)
                    assert only_runs_changed(fin, N, R, si) and only_runs_changed(fout, N, R, so), (N, S, route, "padding")
                    # in == out, one stride
                    assert imajor(lib, b, fin, fin, S, si, si) == 0, b.last_error()
                    count.expect(route + ", one buffer", 1, 1, 1, staged, 1 - staged, 1, 0)
                    assert same_bits(runs(fin, N, R, si), x.reshape(N, R)) and only_runs_changed(fin, N, R, si)
                    # the binding: packed arrays as they are, into `out`
                    px, po = alloc((N, S, ch)), alloc((N, S, ch))
                    px[...] = x
                    assert b.process_block_imajor(px, out=po) is po and same_bits(po, x)
                    count.expect(route + ", packed", 1, 1, 1, staged, 1 - staged, 1, 0)
                    pinned.free()
            # a view into a longer per-instance allocation, walked in three blocks of unequal length
            frames = 40
            for route, alloc, staged in (("staged", pageable, 1), ("in place", pinned, 0)):
                whole_in, whole_out = alloc((N, frames, ch)), alloc((N, frames, ch))
                whole_in[...] = words(rng, (N, frames, ch))
                whole_out.view(np.uint32)[...] = SENTINEL
                f0 = 3
                for S in (5, 17, 11):
                    got = b.process_block_imajor(whole_in[:, f0:f0 + S, :], out=whole_out[:, f0:f0 + S, :])
                    assert got.ctypes.data == whole_out[:, f0:f0 + S, :].ctypes.data
                    count.expect(route + ", a view of %d frames" % S, 1, 1, 1, staged, 1 - staged, 1, 0)
                    f0 += S
                assert same_bits(whole_out[:, 3:f0, :], whole_in[:, 3:f0, :])
                assert (whole_out.view(np.uint32)[:, :3, :] == SENTINEL).all() and (whole_out.view(np.uint32)[:, f0:, :] == SENTINEL).all()
                pinned.free()
            # one pinned, one pageable: staged
            S = 5
            px, y = pinned((N, S, ch)), pageable((N, S, ch))
            px[...] = words(rng, (N, S, ch))
            assert imajor(lib, b, px, y, S) == 0 and same_bits(y, px)
            count.expect("pinned in, pageable out", 1, 1, 1, 1, 0, 1, 0)
            # zero samples: success, nothing launched
            assert imajor(lib, b, px, y, 0) == 0 and imajor(lib, b, None, None, 0) == 0
            count.expect("zero samples", 0, 0, 0, 0, 0, 0, 0)
            # the device entry: device-visible memory on the handle's own stream, views by their stride
            po = pinned((N, S + 2, ch))
            po.view(np.uint32)[...] = SENTINEL
            for rep in range(2):   # (the second time: the pair that has passed once)
                assert b.process_block_imajor_dev(int(px.ctypes.data), int(po.ctypes.data) + 4 * ch, S, None, (S + 2) * ch) == 0 and b.sync() == 0
                assert same_bits(po[:, 1:S + 1, :], px) and (po.view(np.uint32)[:, (0, S + 1), :] == SENTINEL).all()
            count.expect("device entry", 2, 2, 2, 0, 0, 2, 0)
            # alternating with bus blocks on the one scratch
            G = b.bus_groups(64)
            xg = rng.standard_normal((S, ch, G)).astype(np.float32)
            wide = b.process_block_bus(xg, 64, True, False)
            count.expect("a bus block", 1, 0, 0, 1, 0, 0, 1)
            assert same_bits(wide, xg[..., np.arange(N) // min(64, N)])
            assert same_bits(b.process_block_imajor(px), px)
            count.expect("... and an instance-major one behind it", 1, 1, 1, 1, 0, 1, 0)
            assert same_bits(b.process_block_bus(xg, 64, True, False), wide)
            count.expect("... and a bus block again", 1, 0, 0, 1, 0, 0, 1)
            pinned.free()
    # meters read the scratch block: the figures of the plain block on the transposed data
    N, S, ch = 200, 33, 2
    b, plain = A.Batch(N, ch, 0), A.Batch(N, ch, 0)
    assert b.load_text(STEREO) and plain.load_text(STEREO)
    b.meter_enable()
    plain.meter_enable()
    x = (rng.standard_normal((N, S, ch)) * 2).astype(np.float32)
    x[3, 4, 1], x[7, 0, 0] = np.nan, -np.inf
    m0 = b.info("meter_launches")
    assert same_bits(b.process_block_imajor(x), x)
    assert same_bits(plain.process_block(np.ascontiguousarray(x.transpose(1, 2, 0))), np.ascontiguousarray(x.transpose(1, 2, 0)))
    assert b.info("meter_launches") == m0 + 1
    got, want = b.meter_read(), plain.meter_read()
    for key in ("energy", "peak", "full_scale", "nonfinite"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["nonfinite"].sum() == 2 and b.meter_samples() == S
    # a schedule armed for the block applies (the interpreter tier cuts the block at its steps, on the scratch)
    os.environ["FX_KERNEL"] = "asm"
    t = A.Batch(200, 1, 0)
    del os.environ["FX_KERNEL"]
    assert t.load_text(PROGRAM), t.errors()
    x = words(rng, (200, 32, 1))
    assert same_bits(t.process_block_imajor(x), x)
    assert t.set_register_track("vol", [0.1, 0.2, 0.3, 0.4], 8) == 0
    k0 = lib.fxstub_kernels_run()
    assert same_bits(t.process_block_imajor(x), x)
    assert lib.fxstub_kernels_run() - k0 == 4 and abs(t.get_register_i("vol", 3) - 0.4) < 1e-6
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("imajor routes ok")


def child_refusals():
    A, lib = stub_library()
    pinned = Pinned(lib)
    N, S, ch = 300, 8, 2
    R = S * ch
    b = A.Batch(N, ch, 0)
    assert b.load_text(STEREO), b.errors()
    x, y = pinned((N, R)), pinned((N, R))
    both = pinned((4 * N * R,))
    page = np.zeros((N, R), dtype=np.float32)
    x[...] = 0.5
    y[...] = 0.25
    both[...] = 0.125
    assert imajor(lib, b, x, y, S) == 0 and same_bits(y, x)
    y[...] = 0.25
    ms = b.last_kernel_ms()
    count = Counts(lib, b)
    at = lambda a, off=0: a.ctypes.data + off * 4
    dev = lambda i, o, s, si, so: lib.fxb_process_block_imajor_dev(b._h, C.c_void_p(i), C.c_void_p(o), s, si, so, None)
    refused = [
        ("in stride below the run", lambda: imajor(lib, b, x, y, S, R - 1, 0)), ("out stride below the run", lambda: imajor(lib, b, x, y, S, 0, 1)),
        ("negative stride", lambda: imajor(lib, b, x, y, S, -R, 0)), ("negative length", lambda: imajor(lib, b, x, y, -1)),
        ("null in", lambda: imajor(lib, b, None, y, S)), ("null out", lambda: imajor(lib, b, x, None, S)),
        ("shifted by three words", lambda: imajor(lib, b, at(both), at(both, 3), S)),
        ("shifted by a run", lambda: imajor(lib, b, at(both), at(both, R), S)),
        ("out inside in", lambda: imajor(lib, b, at(both), at(both, N * R - 1), S)),
        ("in inside out", lambda: imajor(lib, b, at(both, N * R - 1), at(both), S)),
        ("one buffer, two strides", lambda: imajor(lib, b, at(both), at(both), S, R, 2 * R)),
        ("two strides that meet", lambda: imajor(lib, b, at(both), at(both, R), S, 3 * R, 2 * R)),
        ("one stride, runs that meet", lambda: imajor(lib, b, at(both), at(both, 2 * R + R // 2), S, 2 * R, 2 * R)),
        ("device entry, stride below the run", lambda: dev(at(x), at(y), S, R - 1, 0)),
        ("device entry, null", lambda: dev(0, at(y), S, 0, 0)),
        ("device entry, overlap", lambda: dev(at(both), at(both, 1), S, 0, 0)),
        ("device entry, a host pointer", lambda: dev(page.ctypes.data, at(y), S, 0, 0)),
        ("device entry, beyond the allocation", lambda: dev(at(x), at(y), S, 0, R + 1)),
    ]
    for what, call in refused:
        assert call() == FX_E_ARG and b.last_error(), what
        count.expect(what, 0, 0, 0, 0, 0, 0, 0)
        assert b.last_kernel_ms() == ms, what
        assert (x == 0.5).all() and (y == 0.25).all() and (both == 0.125).all() and (page == 0).all(), what
    assert "not memory of this handle's device" in b.last_error(), b.last_error()
    # ... and footprints that touch or interleave without sharing an element are not among them
    assert imajor(lib, b, at(both), at(both, N * R), S) == 0, b.last_error()
    assert imajor(lib, b, at(both), at(both, R), S, 2 * R, 2 * R) == 0, b.last_error()
    assert imajor(lib, b, at(both), at(both, R), S, 2 * R, 4 * R) == 0, b.last_error()
    count.expect("three that are fine", 3, 3, 3, 0, 3, 3, 0)
    assert lib.fxb_process_block_imajor(None, C.c_void_p(at(x)), C.c_void_p(at(y)), S, 0, 0) == FX_E_ARG
    assert dev(at(x), at(y), S, 0, 0) == 0 and b.sync() == 0 and same_bits(y, x), "the handle stays usable"
    pinned.free()
    print("imajor refusals ok")


def child_pieces():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(17)
    # 96 samples of 262 144 instances: a scratch block of 96 MiB, above the 64 MiB of a piece -> two pieces of 48 samples
    N, S = 262144, 96
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    count = Counts(lib, b)
    x = words(rng, (N, S + 4, 1))
    assert same_bits(b.process_block_imajor(x[:, 2:S + 2, :]), x[:, 2:S + 2, :])
    count.expect("two pieces, staged", 2, 2, 2, 1, 0, 1, 0)
    px, po = pinned((N, S + 4, 1)), pinned((N, S + 4, 1))
    px[...] = x
    po.view(np.uint32)[...] = SENTINEL

    def block(S_, want):
        po.view(np.uint32)[...] = SENTINEL
        assert imajor(lib, b, px.ctypes.data + 8, po.ctypes.data + 8, S_, S + 4, S + 4) == 0, b.last_error()
        assert same_bits(po[:, 2:S_ + 2, :], x[:, 2:S_ + 2, :]) and (po.view(np.uint32)[:, :2, :] == SENTINEL).all() and (po.view(np.uint32)[:, S_ + 2:, :] == SENTINEL).all()
        count.expect(*want)

    block(S, ("two pieces, in place", 2, 2, 2, 0, 1, 1, 0))
    block(64, ("64 MiB exactly: one piece", 1, 1, 1, 0, 1, 1, 0))
    block(65, ("one sample more: two pieces", 2, 2, 2, 0, 1, 1, 0))
    # with a schedule armed the block stays whole, on a scratch block grown for it
    assert b.set_register_track("vol", [0.1, 0.2], 48) == 0
    block(S, ("armed: one piece", 1, 1, 1, 0, 1, 1, 0))
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("imajor pieces ok")


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
    dev = lambda x, y, st: lib.fxb_process_block_imajor_dev(b._h, C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), S, 0, 0, st)

    def fresh():
        x, y = pinned((N, S, 1)), pinned((N, S, 1))
        x[...] = words(rng, (N, S, 1))
        y[...] = -7.0
        return x, y
    assert b.process_block_imajor(np.zeros((N, S, 1), dtype=np.float32)) is not None   # (code generated, scratch allocated)
    lib.fxstub_set_kernel_micros(30000)   # the emulation launch takes 30 ms: whatever does not wait for what follows it is caught
    xa, ya = fresh()
    assert dev(xa, ya, streams[0]) == 0, b.last_error()
    assert b.sync() == 0 and same_bits(ya, xa), "fxb_sync returned before the scatter of an instance-major block"
    # a device-entry block on one stream, at once another on a second stream, at once a bus block on the first, at once a
    # host-entry block: four fillings of one scratch
    (xa, ya), (xb, yb), (xc, yc) = fresh(), fresh(), fresh()
    bus_in, bus_out = pinned((S, 1, G)), pinned((S, 1, N))
    bus_in[...] = rng.standard_normal((S, 1, G)).astype(np.float32)
    assert dev(xa, ya, streams[0]) == 0 and dev(xb, yb, streams[1]) == 0, b.last_error()
    assert lib.fxb_process_block_bus_dev(b._h, C.c_void_p(bus_in.ctypes.data), C.c_void_p(bus_out.ctypes.data), S, K, 1, streams[0]) == 0, b.last_error()
    assert imajor(lib, b, xc, yc, S) == 0, b.last_error()
    assert same_bits(yc, xc), "host entry"
    assert b.sync() == 0
    assert same_bits(ya, xa), "the first block's scratch was refilled under it"
    assert same_bits(yb, xb), "the second block's scratch was refilled under it"
    assert same_bits(bus_out, bus_in[..., np.arange(N) // K]), "the bus block's scratch was refilled under it"
    # ... and a register read right behind a device-entry block sees the block done
    ya[...] = -7.0
    assert dev(xa, ya, streams[1]) == 0 and b.instruction_counter() >= 0 and same_bits(ya, xa)
    lib.fxstub_set_kernel_micros(150)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("imajor streams ok")


def child_shards():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(23)
    N, S = 3 * 256 + 40, 16
    b = A.Batch(N, 1, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    assert b.load_text(PROGRAM), b.errors()
    count = Counts(lib, b)
    x = words(rng, (N, S, 1))
    for stride in (S, S + 3):
        fin, fout = padded(pinned, N, stride), padded(pinned, N, stride)
        runs(fin, N, S, stride)[...] = x.reshape(N, S)
        assert imajor(lib, b, fin, fout, S, stride, stride) == 0, b.last_error()
        count.expect("in place, every shard on its runs", 3, 3, 3, 0, 3, 3, 0)
        assert same_bits(runs(fout, N, S, stride), x.reshape(N, S)) and only_runs_changed(fout, N, S, stride) and only_runs_changed(fin, N, S, stride)
        assert imajor(lib, b, fin, fin, S, stride, stride) == 0 and same_bits(runs(fin, N, S, stride), x.reshape(N, S))
        count.expect("one buffer", 3, 3, 3, 0, 3, 3, 0)
        pageable = lambda shape: np.empty(shape, dtype=np.float32)
        gin, gout = padded(pageable, N, stride), padded(pageable, N, stride)
        runs(gin, N, S, stride)[...] = x.reshape(N, S)
        assert imajor(lib, b, gin, gout, S, stride, stride) == 0, b.last_error()
        count.expect("pageable: every shard stages its runs", 3, 3, 3, 3, 0, 3, 0)
        assert same_bits(runs(gout, N, S, stride), x.reshape(N, S)) and only_runs_changed(gout, N, S, stride)
        pinned.free()
    # the device entry on a handle of several shards; an overlap that only the whole batch shows (shard 1's output on shard 0's input)
    px, po = pinned((N, S)), pinned((N, S))
    assert lib.fxb_process_block_imajor_dev(b._h, C.c_void_p(px.ctypes.data), C.c_void_p(po.ctypes.data), S, 0, 0, None) == FX_E_ARG
    assert "one shard" in b.last_error(), b.last_error()
    assert imajor(lib, b, px.ctypes.data, px.ctypes.data + 4 * S * 10, S) == FX_E_ARG
    assert imajor(lib, b, px, po, S, S - 1, 0) == FX_E_ARG
    count.expect("refused", 0, 0, 0, 0, 0, 0, 0)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    print("imajor shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "refusals": child_refusals, "pieces": child_pieces, "shards": child_shards, "streams": child_streams}[sys.argv[1]]()
