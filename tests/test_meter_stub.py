"""Output meters without a GPU: the library's host sources linked against tests/hipstub/ (`make -C fx8010-emulator-core_amd/csrc
stublib`), driven through the C ABI in a child process (the binding reads FX8010_AMD_LIB once, at import; this file is also that
child).  The stand-in's emulation kernel copies in to out and the stand-in of the meter kernel (tests/hipstub/fx_meter_stub.cpp)
does its real arithmetic in stream order, so the meters must equal meter_model() - the numpy restatement of the definition in
include/fx8010_amd.h - of whatever per-instance block the call returned, bit for bit: that checks the host routing (every route a
block can take, pieces, segments of an armed control track, shards on three devices), the accumulation across blocks, enable /
read / reset / reload and the refusals.  Meter launches are counted per route and per piece.  The kernel itself and its parity
on real programs: tests/test_gpu_meter.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from route_models import FIELDS, meter_zero, meter_model, same_meters  # noqa: E402,F401  (the models live there; the tests of them stay here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_ARG, FX_E_MEMORY = -3, -5
SHARED_IN, MIX_OUT = 1, 2
PROGRAM = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
STEREO = PROGRAM.replace("output out 0", "input in1 1\noutput out 0\noutput out1 1").replace("\nend", "\nmacs out1, in1, a, 0.5\nend")
MORE = "static zz\nmacs zz, zz, 0.5, 0.5\nend"   # a further load that succeeds: registers and instructions accumulate over loads


def test_meter_model_splits_and_counts():
    """the restatement itself: blocks of 16 + 17 samples give the bits of one block of 33; the written-out loop for one column"""
    rng = np.random.default_rng(5)
    y = (rng.standard_normal((33, 2, 70)) * 10.0 ** rng.integers(-20, 3, (33, 2, 70))).astype(np.float32)
    y[3, 0, 5], y[4, 0, 5], y[5, 1, 6], y[6, 0, 7], y[7, 0, 7], y[8, 0, 8] = np.nan, np.inf, -np.inf, 1.0, -1.0, np.float32(1e-42)
    whole = meter_model(y)
    assert same_meters(meter_model(y[16:], meter_model(y[:16])), whole)
    for c, n in ((0, 5), (1, 6), (0, 7), (0, 8), (1, 69)):
        e, p, f, nf = 0.0, np.float32(0.0), 0, 0
        for s in range(33):
            v = y[s, c, n]
            fin = bool(abs(v) < np.inf)
            w = abs(v) if fin else np.float32(0.0)
            e = e + float(w) * float(w)
            p = max(p, w)
            f += fin and abs(v) >= 1.0
            nf += not fin
        assert (e, p, f, nf) == (whole["energy"][c, n], whole["peak"][c, n], whole["full_scale"][c, n], whole["nonfinite"][c, n]), (c, n)
    assert whole["nonfinite"][0, 5] == 2 and whole["nonfinite"][1, 6] == 1 and whole["full_scale"][0, 7] >= 2 and np.isfinite(whole["energy"]).all()
    full = meter_zero(1, 2)
    full["full_scale"][0, 0] = full["nonfinite"][0, 1] = 0xFFFFFFFE
    sat = meter_model(np.array([[[2.0, np.nan]]] * 3, dtype=np.float32), full)
    assert sat["full_scale"][0, 0] == 0xFFFFFFFF and sat["nonfinite"][0, 1] == 0xFFFFFFFF


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_meters_on_every_route_on_the_hip_stand_in():
    run_child("routes", "meter routes ok")


def test_meter_pieces_and_track_segments_on_the_hip_stand_in():
    run_child("pieces", "meter pieces ok")


def test_meter_enable_read_reset_and_refusals_on_the_hip_stand_in():
    run_child("refusals", "meter refusals ok")


def test_meters_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "meter shards ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_kernels_run", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches", "fxstub_meter_launches", "fxstub_live_allocations"):
        getattr(lib, f).restype = C.c_long
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


class Watch:
    """a handle with meters on, the model of everything it has been through, and the launches since the last look"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.model = meter_zero(b.channels, b.n)
        self.samples = 0
        self.seen = self.now()

    def now(self):
        return (self.lib.fxstub_kernels_run(), self.lib.fxstub_meter_launches(), self.b.info("meter_launches"))

    def took(self, what, y, launches=1):
        """the call returned the per-instance block y, and took `launches` emulation launches: as many meter launches"""
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, self.b.channels, self.b.n)
        self.model = meter_model(y, self.model)
        self.samples += y.shape[0]
        got = self.b.meter_read()   # (synchronous: an asynchronous entry's launches have run when it returns)
        now = self.now()
        assert tuple(a - b for a, b in zip(now, self.seen)) == (launches, launches, launches), (what, now, self.seen)
        self.seen = now
        assert same_meters(got, self.model), what
        assert self.b.meter_samples() == self.samples, what


def signal(rng, shape):
    x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-12, 2, shape)).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = np.float32(np.nan)
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = np.float32(-np.inf)
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = np.float32(-1.0)
    return x


def expand(x, K, N):
    return np.ascontiguousarray(x[..., np.arange(N) // min(int(K), N)])


def child_routes():
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(41)
    S = 33
    for ch, text in ((1, PROGRAM), (2, STEREO)):
        for N in (5, 197, 256, 4133):
            b = A.Batch(N, ch, 0)
            assert b.load_text(text), b.errors()
            assert b.meter_enable() == 0 and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(ch, N))
            w = Watch(lib, b)
            # pageable host blocks (N = 5: a few KB through the library's pinned pair; else staged in one piece)
            x = signal(rng, (S, ch, N))
            w.took("pageable", b.process_block(x))
            x = signal(rng, (16, ch, N))
            w.took("pageable, 16 more samples", b.process_block(x))
            # pinned, in place (the meter kernel reads the caller's buffer)
            pin, pout = pinned((S, ch, N)), pinned((S, ch, N))
            pin[...] = signal(rng, (S, ch, N))
            assert b.process_block(pin, out=pout) is pout
            w.took("pinned in place", pout)
            assert b.process_block(pin, out=pin) is pin
            w.took("pinned, one buffer", pin)
            # device entry at pitch N and at pitch N + 59: asynchronous, fxb_meter_read waits
            assert b.process_block_dev(int(pin.ctypes.data), int(pout.ctypes.data), S) == 0
            w.took("device entry", pout)
            P = N + 59
            # (the stand-in's emulation copies without a pitch: on one buffer it copies nothing, and the block is known)
            win = pinned((S, ch, P))
            win[...] = signal(rng, (S, ch, P))
            assert b.process_block_dev_pitched(int(win.ctypes.data), int(win.ctypes.data), S, P) == 0
            w.took("device entry, pitch N + 59", win[:, :, :N])
            # bus blocks: the scratch block between the emulation and the mix / copy-out
            for K in (3, 64, 65):
                G = b.bus_groups(K)
                xg, xn = signal(rng, (S, ch, G)), signal(rng, (S, ch, N))
                b.process_block_bus(xg, K, True, False)
                w.took("bus %d shared in" % K, expand(xg, K, N))
                b.process_block_bus(xn, K, False, True)
                w.took("bus %d mix out" % K, xn)
                b.process_block_bus(xg, K, True, True)
                w.took("bus %d both" % K, expand(xg, K, N))
                pg, po = pinned((S, ch, G)), pinned((S, ch, G))
                pg[...] = xg
                assert b.process_block_bus_dev(int(pg.ctypes.data), int(po.ctypes.data), S, K) == 0
                w.took("bus %d device entry" % K, expand(xg, K, N))
            # zero samples and refused blocks: nothing metered
            assert lib.fxb_process_block(b._h, None, None, 0) == 0 and lib.fxb_process_block(b._h, None, None, 4) == FX_E_ARG
            w.took("nothing", np.zeros((0, ch, N), dtype=np.float32), launches=0)
            # meters off: no launch; on again: zeros
            assert b.meter_enable(False) == 0
            k0 = lib.fxstub_meter_launches()
            b.process_block(x)
            assert lib.fxstub_meter_launches() == k0 and lib.fxb_meter_samples(b._h) == FX_E_ARG
            assert b.meter_enable() == 0 and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(ch, N))
            pinned.free()
            b.close()
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("meter routes ok")


def child_pieces():
    A, lib = stub_library()
    rng = np.random.default_rng(43)
    # 96 samples of 262 144 instances on a bus: a scratch block of 96 MiB, two pieces of 48 samples, a meter launch behind each
    N, S, K = 262144, 96, 64
    b = A.Batch(N, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    assert b.meter_enable() == 0
    w = Watch(lib, b)
    xg = signal(rng, (S, 1, b.bus_groups(K)))
    b.process_block_bus(xg, K)
    w.took("bus, two pieces", expand(xg, K, N), launches=2)
    # a pageable block of 32 MiB: eight pieces on three streams
    x = signal(rng, (32, 1, N))
    w.took("pipelined host block", b.process_block(x), launches=8)
    b.close()
    # an armed control track: the interpreter tier cuts the block at the change points - one meter launch per segment, in order;
    # the translated tier reads the schedule by itself - one
    for tier, segments in (("asm", 5), (None, 1)):
        if tier:
            os.environ["FX_KERNEL"] = tier
        t = A.Batch(197, 1, 0)
        os.environ.pop("FX_KERNEL", None)
        assert t.load_text(PROGRAM), t.errors()
        assert (t.info("kernel") >= 9) == (tier is None), t.info("kernel")
        assert t.meter_enable() == 0
        w = Watch(lib, t)
        for route in ("pageable", "bus"):
            assert t.set_register_track("vol", [0.1, 0.2, 0.3, 0.4, 0.5], 8) == 0
            if route == "pageable":
                x = signal(rng, (33, 1, 197))
                w.took("armed, " + route, t.process_block(x), launches=segments)
            else:
                xg = signal(rng, (33, 1, t.bus_groups(64)))
                t.process_block_bus(xg, 64)
                w.took("armed, " + route, expand(xg, 64, 197), launches=segments)
        t.close()
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("meter pieces ok")


def child_refusals():
    os.environ["FX_BUILDER"] = "0"   # (allocations are counted below: none may come from the handle's builder thread meanwhile)
    A, lib = stub_library()
    rng = np.random.default_rng(47)
    N, S = 197, 33
    b = A.Batch(N, 2, 0)
    assert b.load_text(STEREO), b.errors()
    x = signal(rng, (S, 2, N))
    arrays = meter_zero(2, N)
    for a in arrays.values():
        a[...] = 9
    ptrs = [C.c_void_p(arrays[k].ctypes.data) for k in FIELDS]
    # off (the default): read and samples are refused and change nothing; a block launches no meter
    assert lib.fxb_meter_read(b._h, *ptrs, 0) == FX_E_ARG and "metering is off" in b.last_error()
    assert lib.fxb_meter_read(b._h, None, None, None, None, 1) == FX_E_ARG and lib.fxb_meter_samples(b._h) == FX_E_ARG
    assert all((a == 9).all() for a in arrays.values())
    b.process_block(x)
    assert lib.fxstub_meter_launches() == 0 and b.info("meter_launches") == 0
    assert lib.fxb_meter_enable(b._h, 0) == 0, "off while off"
    # a NULL handle
    assert lib.fxb_meter_enable(None, 1) == FX_E_ARG and lib.fxb_meter_read(None, *ptrs, 0) == FX_E_ARG and lib.fxb_meter_samples(None) == FX_E_ARG
    # an allocation that fails inside fxb_meter_enable: FX_E_MEMORY, metering stays off, the next block is fine
    live = lib.fxstub_live_allocations()
    lib.fxstub_fail_mallocs(0, 1)
    assert lib.fxb_meter_enable(b._h, 1) == FX_E_MEMORY and b.last_error()
    lib.fxstub_fail_mallocs(-1, 0)
    assert lib.fxb_meter_samples(b._h) == FX_E_ARG and lib.fxstub_live_allocations() == live
    y = b.process_block(x)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32)) and lib.fxstub_meter_launches() == 0
    # on: all device allocation happens here - none inside a block
    assert b.meter_enable() == 0 and lib.fxstub_live_allocations() == live + 1
    b.process_block(x)
    assert lib.fxstub_live_allocations() == live + 1 and b.meter_samples() == S
    want = meter_model(x)
    assert same_meters(b.meter_read(), want)
    # any pointer may be NULL
    for skip in range(4):
        for a in arrays.values():
            a[...] = 9
        args = [None if k == skip else p for k, p in enumerate(ptrs)]
        assert lib.fxb_meter_read(b._h, *args, 0) == 0
        for k, key in enumerate(FIELDS):
            assert (arrays[key] == 9).all() if k == skip else np.array_equal(arrays[key].view(np.uint8), want[key].view(np.uint8)), (skip, key)
    # enabling twice keeps the values
    assert b.meter_enable() == 0 and same_meters(b.meter_read(), want) and b.meter_samples() == S
    # the state image does not hold them: save and load leave them alone
    image = b.save_state()
    b.process_block(x)
    want = meter_model(x, want)
    b.load_state(image)
    assert same_meters(b.meter_read(), want) and b.meter_samples() == 2 * S
    # read with reset: the values, then zeros and 0 samples; all pointers NULL with reset is legal
    assert same_meters(b.meter_read(reset=True), want)
    assert same_meters(b.meter_read(), meter_zero(2, N)) and b.meter_samples() == 0
    b.process_block(x)
    assert lib.fxb_meter_read(b._h, None, None, None, None, 1) == 0 and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
    # a program load resets the meters and keeps them enabled
    b.process_block(x)
    assert b.meter_samples() == S
    assert b.load_text(MORE), b.errors()
    assert b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
    y = b.process_block(x)
    assert same_meters(b.meter_read(), meter_model(y)) and b.meter_samples() == S
    # disabling then enabling gives zeros
    live = lib.fxstub_live_allocations()
    assert b.meter_enable(False) == 0 and lib.fxstub_live_allocations() == live - 1
    assert b.meter_enable() == 0 and same_meters(b.meter_read(), meter_zero(2, N)) and b.meter_samples() == 0
    b.close()
    print("meter refusals ok")


def child_shards():
    os.environ["FX_BUILDER"] = "0"   # (allocations are counted below: none may come from the handles' builder threads meanwhile)
    A, lib = stub_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(53)
    N, S = 3 * 256 + 40, 33
    b = A.Batch(N, 2, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    assert b.load_text(STEREO), b.errors()
    # a shard that cannot allocate: FX_E_MEMORY, metering off on every shard, nothing left allocated
    live = lib.fxstub_live_allocations()
    lib.fxstub_fail_mallocs(1, 1)
    assert lib.fxb_meter_enable(b._h, 1) == FX_E_MEMORY and b.last_error()
    lib.fxstub_fail_mallocs(-1, 0)
    assert lib.fxb_meter_samples(b._h) == FX_E_ARG and lib.fxstub_live_allocations() == live
    assert lib.fxb_meter_read(b._h, None, None, None, None, 0) == FX_E_ARG
    assert b.meter_enable() == 0 and lib.fxstub_live_allocations() == live + 3
    w = Watch(lib, b)
    x = signal(rng, (S, 2, N))
    w.took("pageable: every shard stages its columns", b.process_block(x), launches=3)
    # (a shard works at the pitch of the whole batch, the stand-in's emulation copies without one: on one buffer it copies nothing)
    pin = pinned((S, 2, N))
    pin[...] = signal(rng, (S, 2, N))
    assert b.process_block(pin, out=pin) is pin
    w.took("pinned: every shard on its columns in place", pin, launches=3)
    for K in (64, 32):
        G = b.bus_groups(K)
        xg = signal(rng, (S, 2, G))
        b.process_block_bus(xg, K)
        w.took("bus %d, staged" % K, expand(xg, K, N), launches=3)
        pg, po = pinned((S, 2, G)), pinned((S, 2, G))
        pg[...] = xg
        assert lib.fxb_process_block_bus(b._h, C.c_void_p(pg.ctypes.data), C.c_void_p(po.ctypes.data), S, K, SHARED_IN | MIX_OUT) == 0, b.last_error()
        w.took("bus %d, in place" % K, expand(xg, K, N), launches=3)
    want = w.model
    assert same_meters(b.meter_read(reset=True), want) and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
    b.process_block(x)
    assert b.meter_samples() == S and b.load_text(MORE) and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
    live = lib.fxstub_live_allocations()
    assert b.meter_enable(False) == 0 and lib.fxstub_live_allocations() == live - 3
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    pinned.free()
    b.close()
    print("meter shards ok")


if __name__ == "__main__":
    {"routes": child_routes, "pieces": child_pieces, "refusals": child_refusals, "shards": child_shards}[sys.argv[1]]()
