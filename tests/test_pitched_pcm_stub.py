"""Routing of row-pitched host blocks without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`) with three stand-in devices, driven through the C ABI in a child process (the binding reads
FX8010_AMD_LIB once, at import; this file is also that child).  A sharded handle over fxb_host_alloc buffers launches once per shard
and stages nothing, every shard on its own device's view of the buffers; pageable buffers are staged; the argument refusals of
fxb_process_block_pitched / fxb_process_block_dev_pitched launch nothing.  PCM values are not checked (the stand-in kernel copies in
to out): parity is tests/test_gpu_pitched_pcm.py.

The second child walks every route a block can take through a single handle (fx_batch_io.cpp) and records, per route, launches,
the host_staged_blocks / host_inplace_blocks counters, return codes and that a staged copy writes nothing outside the handle's
columns: small pinned blocks, in place, staged in one piece at the natural and at a wider pitch, pipelined at both, a device
pointer handed to the host entry, the track fallback of the interpreter tier at a pitch, zero-sample blocks and refusals on every
entry point, a launch that fails on every route, and the staged launch the device refuses (run again without stages).  The third
pins what that retry does to the handle's sample clock."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_ARG = -3
PROGRAM = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"


def test_pitched_routing_on_the_hip_stand_in():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = "3"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "pitched routing ok" in r.stdout, r.stdout[-4000:]


def run_child(which, marker):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_every_block_route_on_the_hip_stand_in():
    run_child("routes", "block routes ok")


def test_a_refused_staged_launch_counts_its_block_once():
    """A staged launch the device refuses is run again without stages INSIDE the same block: the handle's sample clock advances by
    the block's length once.  A control written just before that block therefore cools after kCoolSamples (8 192) sample periods
    of real blocks, not after half of them (the retry used to go back through the public entry and ran the head-of-block
    bookkeeping a second time)."""
    run_child("retry", "retry clock ok")


def host_array(lib, shape):
    """a float32 numpy view of fxb_host_alloc memory (and the pointer to free)"""
    count = int(np.prod(shape))
    p = lib.fxb_host_alloc(count * 4)
    assert p, lib.fx_last_create_error()
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(count,)).reshape(shape), p


def child():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    lib.fxstub_kernels_run.restype = C.c_long
    lib.fxstub_cross_device_errors.restype = C.c_long
    lib.fxstub_bad_pcm_launches.restype = C.c_long
    vp = lambda a: C.c_void_p(a.ctypes.data)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    n, S = 1000, 16

    # three shards on three devices, buffers of fxb_host_alloc (every device sees them): one launch per shard, nothing staged
    b = A.Batch(n, 1, devices=[0, 1, 2])
    assert [d for d, _, _ in b.shards()] == [0, 1, 2]
    assert b.load_text(PROGRAM), b.errors()
    xin, pin = host_array(lib, (S, 1, n))
    yout, pout = host_array(lib, (S, 1, n))
    xin[...] = 0.25
    for blk in range(3):
        k0 = lib.fxstub_kernels_run()
        assert lib.fxb_process_block(b._h, fp(xin), fp(yout), S) == 0, b.last_error()
        assert lib.fxstub_kernels_run() - k0 == 3, "one launch per shard"
    assert b.info("host_inplace_blocks") == 9 and b.info("host_staged_blocks") == 0
    # ... in == out, and a column range [37, 37 + N) of a wider buffer at its pitch
    assert lib.fxb_process_block(b._h, fp(xin), fp(xin), S) == 0
    M = n + 100
    win, pwin = host_array(lib, (S, 1, M))
    wout, pwout = host_array(lib, (S, 1, M))
    k0 = lib.fxstub_kernels_run()
    assert lib.fxb_process_block_pitched(b._h, C.c_void_p(win.ctypes.data + 37 * 4), C.c_void_p(wout.ctypes.data + 37 * 4), S, M) == 0, b.last_error()
    assert lib.fxstub_kernels_run() - k0 == 3
    assert b.process_block(win[:, :, 37:37 + n], wout[:, :, 37:37 + n]) is not None   # (the binding passes the views as they are)
    assert b.info("host_inplace_blocks") == 18 and b.info("host_staged_blocks") == 0
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0

    # pageable buffers: every shard stages its columns
    px, py = np.full((S, 1, M), 0.5, dtype=np.float32), np.zeros((S, 1, M), dtype=np.float32)
    assert lib.fxb_process_block_pitched(b._h, C.c_void_p(px.ctypes.data + 37 * 4), C.c_void_p(py.ctypes.data + 37 * 4), S, M) == 0, b.last_error()
    assert b.info("host_staged_blocks") == 3 and b.info("host_inplace_blocks") == 18
    assert (py[:, :, :37] == 0).all() and (py[:, :, 37 + n:] == 0).all(), "a staged copy wrote outside the handle's columns"
    # pinned buffers that overlap without being one buffer (columns shifted by 5 < N): staged, not in place
    assert lib.fxb_process_block_pitched(b._h, C.c_void_p(win.ctypes.data), C.c_void_p(win.ctypes.data + 5 * 4), S, M) == 0
    assert b.info("host_staged_blocks") == 6

    # refusals: FX_E_ARG, no launch, the handle stays usable
    k0 = lib.fxstub_kernels_run()
    for pitch in (n - 1, 0, -5, 1 << 30):
        assert lib.fxb_process_block_pitched(b._h, vp(xin), vp(yout), S, pitch) == FX_E_ARG, pitch
    assert lib.fxb_process_block_dev_pitched(b._h, vp(xin), vp(yout), S, n, None) == FX_E_ARG
    assert "fxb_process_block_dev_shards" in b.last_error()
    single = A.Batch(n, 2, 0)
    assert single.load_text(PROGRAM.replace("output out 0", "input in1 1\noutput out 0\noutput out1 1").replace("\nend", "\nmacs out1, in1, a, 0.5\nend"))
    assert single.process_block(np.zeros((S, 2, n), dtype=np.float32)) is not None
    k1 = lib.fxstub_kernels_run()
    qx, qy = np.zeros((S, 2, M), dtype=np.float32), np.zeros((S, 2, M), dtype=np.float32)
    assert lib.fxb_process_block_dev_pitched(single._h, vp(qx), vp(qy), S, M, None) == FX_E_ARG        # pageable
    assert "not memory of this handle's device" in single.last_error(), single.last_error()
    assert lib.fxb_process_block_dev_pitched(single._h, vp(xin), vp(yout), S, n - 1, None) == FX_E_ARG
    assert lib.fxb_process_block_dev_pitched(single._h, vp(xin), vp(yout), S, 1 << 29, None) == FX_E_ARG  # 2 channels x 2^29 x 4 = 2^32
    assert lib.fxb_process_block_pitched(single._h, vp(xin), vp(yout), 1, 1 << 29) == FX_E_ARG
    assert lib.fxstub_kernels_run() == k1, "a refused call launched"
    # device-visible host memory is accepted (one launch), and so is in == out
    wide, pwide = host_array(lib, (S, 2, M))
    assert lib.fxb_process_block_dev_pitched(single._h, vp(wide), vp(wide), S, M, None) == 0 and single.sync() == 0
    assert lib.fxstub_kernels_run() == k1 + 1
    assert lib.fxb_process_block_dev_pitched(single._h, vp(wide), C.c_void_p(wide.ctypes.data + 3 * 4), S, M, None) == FX_E_ARG   # overlapping
    assert lib.fxstub_kernels_run() == k0 + 2   # (the plain block of `single` and the accepted dev_pitched one)
    assert lib.fxb_process_block(b._h, fp(xin), fp(yout), S) == 0
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    for p in (pin, pout, pwin, pwout, pwide):
        lib.fxb_host_free(p)
    print("pitched routing ok")


def chain_program(links):
    """a filter chain that a small batch runs as a pipeline of stages, with declared controls"""
    t = "input in 0\noutput out 0\ncontrol vol = 0.5\ncontrol mix = 0.25\ncontrol cut = 0.1\nstatic t\n"
    t += "".join("static s%d\n" % k for k in range(links))
    t += "interp s0, s0, cut, in\nmacs t, 0, s0, vol\n"
    for k in range(1, links):
        t += "interp s%d, s%d, cut, t\nmacs t, 0, s%d, 0.5\n" % (k, k, k)
    return t + "macs out, t, mix, 0.125\nend"


def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub)"
    lib = A.load()
    for f in ("fxstub_kernels_run", "fxstub_cross_device_errors", "fxstub_bad_pcm_launches"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_fail_launches.argtypes = [C.c_long, C.c_long, C.c_int]
    lib.fxstub_fail_launches.restype = None
    lib.fxb_process_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]   # (buffers by address, like the other entries)
    return A, lib


HIP_LAUNCH_OUT_OF_RESOURCES, HIP_LAUNCH_FAILURE = 701, 719
FX_E_NODEVICE = -1


def child_routes():
    A, lib = stub_library()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    at = lambda a, col: C.c_void_p(a.ctypes.data + col * 4)
    n, M, col = 200, 250, 7
    b = A.Batch(n, 1, 0)
    assert b.load_text(PROGRAM), b.errors()
    seen = {"k": lib.fxstub_kernels_run(), "staged": 0, "inplace": 0}

    def expect(what, launches, staged, inplace):
        k = lib.fxstub_kernels_run()
        got = (k - seen["k"], b.info("host_staged_blocks") - seen["staged"], b.info("host_inplace_blocks") - seen["inplace"])
        assert got == (launches, staged, inplace), (what, got)
        seen.update(k=k, staged=b.info("host_staged_blocks"), inplace=b.info("host_inplace_blocks"))

    rng = np.random.default_rng(5)
    pageable = lambda S, P: (rng.random((S, 1, P), dtype=np.float32) + 1.0, np.zeros((S, 1, P), dtype=np.float32))

    def pitched_ok(x, y, S):
        assert (y[:S, :, col:col + n] == x[:S, :, col:col + n]).all(), "the handle's columns did not come back"
        assert (y[:, :, :col] == 0).all() and (y[:, :, col + n:] == 0).all() and (y[S:] == 0).all(), "a staged copy wrote outside the handle's columns"

    # small blocks (at most 512 floats at the natural pitch): the library's own pinned pair, one untimed launch
    x, y = pageable(2, n)
    assert lib.fxb_process_block(b._h, vp(x), vp(y), 2) == 0, b.last_error()
    expect("small pinned block", 1, 1, 0)
    assert (y == x).all() and b.last_kernel_ms() == -1.0
    # ... the same few floats at a wider pitch: staged (2-D copies)
    x, y = pageable(2, M)
    assert lib.fxb_process_block_pitched(b._h, at(x, col), at(y, col), 2, M) == 0, b.last_error()
    expect("small pitched block", 1, 1, 0)
    pitched_ok(x, y, 2)
    # staged in one piece: 1-D copies at the natural pitch, 2-D at a wider one
    x, y = pageable(16, n)
    assert lib.fxb_process_block(b._h, vp(x), vp(y), 16) == 0, b.last_error()
    expect("staged, natural pitch", 1, 1, 0)
    assert (y == x).all() and b.last_kernel_ms() >= 0.0
    x, y = pageable(16, M)
    assert lib.fxb_process_block_pitched(b._h, at(x, col), at(y, col), 12, M) == 0, b.last_error()
    expect("staged, wider pitch", 1, 1, 0)
    pitched_ok(x, y, 12)
    # in place on pinned buffers, both pitches, and on one buffer
    px, ppx = host_array(lib, (16, 1, M))
    py, ppy = host_array(lib, (16, 1, M))
    px[...] = 0.5
    assert lib.fxb_process_block(b._h, vp(px), vp(py), 16) == 0, b.last_error()
    expect("in place", 1, 0, 1)
    assert lib.fxb_process_block_pitched(b._h, at(px, col), at(py, col), 16, M) == 0, b.last_error()
    expect("in place, wider pitch", 1, 0, 1)
    assert lib.fxb_process_block_pitched(b._h, at(px, col), at(px, col), 16, M) == 0, b.last_error()
    expect("in place, one buffer", 1, 0, 1)
    # memory of the device handed to the HOST entry is not "pinned host memory": staged
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    dx, dy = C.c_void_p(), C.c_void_p()
    assert lib.hipMalloc(C.byref(dx), 16 * n * 4) == 0 and lib.hipMalloc(C.byref(dy), 16 * n * 4) == 0
    assert lib.fxb_process_block(b._h, dx, dy, 16) == 0, b.last_error()
    expect("device memory on the host entry", 1, 1, 0)
    # ... and is what the device entries take, checked (dev_pitched) or not (dev)
    assert lib.fxb_process_block_dev(b._h, dx, dy, 16, None) == 0 and b.sync() == 0
    expect("device entry", 1, 0, 0)
    assert lib.fxb_process_block_dev_pitched(b._h, dx, dy, 16, n, None) == 0 and b.sync() == 0
    assert lib.fxb_process_block_dev_pitched(b._h, dx, dy, 16, n, None) == 0 and b.sync() == 0   # (the pair that has passed once)
    expect("checked device entry", 2, 0, 0)
    assert lib.fxb_process_block_dev_pitched(b._h, dx, dx, 17, n, None) == FX_E_ARG   # one sample period beyond the allocation
    assert "not memory of this handle's device" in b.last_error(), b.last_error()
    expect("checked device entry, footprint beyond the allocation", 0, 0, 0)

    # zero-sample blocks: success on every entry point (with or without buffers), nothing launched, no route counted
    for call in (lambda p, q, S: lib.fxb_process_block(b._h, p, q, S), lambda p, q, S: lib.fxb_process_block_pitched(b._h, p, q, S, M),
                 lambda p, q, S: lib.fxb_process_block_dev(b._h, p, q, S, None), lambda p, q, S: lib.fxb_process_block_dev_pitched(b._h, p, q, S, M, None)):
        assert call(vp(px), vp(py), 0) == 0 and call(None, None, 0) == 0, b.last_error()
        assert call(vp(px), vp(py), -1) == FX_E_ARG and call(None, vp(py), 4) == FX_E_ARG and call(vp(px), None, 4) == FX_E_ARG
    expect("zero-sample blocks and refusals", 0, 0, 0)

    # a launch that fails: reported on every route, nothing left running on the caller's memory, the next block works
    x, y = pageable(16, M)
    for what, call in (("small", lambda: lib.fxb_process_block(b._h, vp(x), vp(y), 2)), ("staged", lambda: lib.fxb_process_block_pitched(b._h, at(x, col), at(y, col), 16, M)),
                       ("in place", lambda: lib.fxb_process_block_pitched(b._h, at(px, col), at(py, col), 16, M)), ("device", lambda: lib.fxb_process_block_dev(b._h, dx, dy, 16, None))):
        lib.fxstub_fail_launches(0, 1, HIP_LAUNCH_FAILURE)
        rc = call()
        assert rc == FX_E_NODEVICE, (what, rc, b.last_error())
        lib.fxstub_fail_launches(-1, 0, 0)
        assert call() == 0 and b.sync() == 0, (what, b.last_error())
    seen.update(k=lib.fxstub_kernels_run(), staged=b.info("host_staged_blocks"), inplace=b.info("host_inplace_blocks"))

    # the interpreter tier has no schedules of its own: a block with one armed is cut at its steps - at the caller's pitch
    os.environ["FX_KERNEL"] = "asm"
    t = A.Batch(n, 1, 0)
    del os.environ["FX_KERNEL"]
    assert t.load_text(PROGRAM), t.errors()
    x, y = pageable(32, M)
    assert lib.fxb_process_block_pitched(t._h, at(x, col), at(y, col), 32, M) == 0 and 1 <= t.info("kernel") < 8
    for route in ("staged", "in place"):
        assert t.set_register_track("vol", [0.1, 0.2, 0.3, 0.4], 8) == 0
        k0 = lib.fxstub_kernels_run()
        if route == "staged":
            y[...] = 0
            assert lib.fxb_process_block_pitched(t._h, at(x, col), at(y, col), 32, M) == 0, t.last_error()
            pitched_ok(x, y, 32)
        else:
            wx, pwx = host_array(lib, (32, 1, M))
            wy, pwy = host_array(lib, (32, 1, M))
            assert lib.fxb_process_block_pitched(t._h, at(wx, col), at(wy, col), 32, M) == 0, t.last_error()
        assert lib.fxstub_kernels_run() - k0 == 4, (route, "one launch per step of the schedule")
        assert abs(t.get_register_i("vol", 3) - 0.4) < 1e-6
    assert (t.info("host_staged_blocks"), t.info("host_inplace_blocks")) == (2, 1)
    # ... a small block with a schedule is timed (its launches are waited for through their events)
    assert t.set_register_track("vol", [0.1, 0.2], 1) == 0
    x, y = pageable(2, n)
    assert lib.fxb_process_block(t._h, vp(x), vp(y), 2) == 0 and (y == x).all() and t.last_kernel_ms() >= 0.0

    # a block of 32 MiB in eight pieces on three streams, at the natural and at a wider pitch; a piece that fails
    N, S, W = 4096, 2048, 4096 + 64
    big = A.Batch(N, 1, 0)
    assert big.load_text(PROGRAM), big.errors()
    for P in (N, W):
        x = rng.random((S, 1, P), dtype=np.float32) + 1.0
        y = np.zeros((S, 1, P), dtype=np.float32)
        c0 = 0 if P == N else 16
        k0 = lib.fxstub_kernels_run()
        assert lib.fxb_process_block_pitched(big._h, at(x, c0), at(y, c0), S, P) == 0, big.last_error()
        assert lib.fxstub_kernels_run() - k0 == 8, "eight pieces"
        assert (y[:, :, c0:c0 + N] == x[:, :, c0:c0 + N]).all() and (y[:, :, :c0] == 0).all() and (y[:, :, c0 + N:] == 0).all()
        lib.fxstub_fail_launches(2, 1, HIP_LAUNCH_FAILURE)
        assert lib.fxb_process_block_pitched(big._h, at(x, c0), at(y, c0), S, P) == FX_E_NODEVICE
        lib.fxstub_fail_launches(-1, 0, 0)
    assert (big.info("host_staged_blocks"), big.info("host_inplace_blocks")) == (4, 0)

    # a staged launch the device will not start: the same block again without stages, one kernel, no stages from then on
    st = A.Batch(300, 1, 0)
    assert st.load_text(chain_program(14)), st.errors()
    x, y = pageable(64, 300)
    assert lib.fxb_process_block(st._h, vp(x), vp(y), 64) == 0 and st.info("waves_per_wg") >= 2, st.tier_note()
    builds = st.info("xlate_builds")
    y[...] = 0
    k0 = lib.fxstub_kernels_run()
    lib.fxstub_fail_launches(0, 1, HIP_LAUNCH_OUT_OF_RESOURCES)
    assert lib.fxb_process_block(st._h, vp(x), vp(y), 64) == 0, st.last_error()
    lib.fxstub_fail_launches(-1, 0, 0)
    assert lib.fxstub_kernels_run() - k0 == 1 and (y == x).all() and st.info("waves_per_wg") == 1 and st.info("xlate_builds") == builds + 1
    assert lib.fxb_process_block(st._h, vp(x), vp(y), 64) == 0 and st.info("waves_per_wg") == 1 and st.info("xlate_builds") == builds + 1
    # ... any other launch error is reported as it is and leaves the stages alone
    st2 = A.Batch(300, 1, 0)
    assert st2.load_text(chain_program(14)), st2.errors()
    assert lib.fxb_process_block(st2._h, vp(x), vp(y), 64) == 0 and st2.info("waves_per_wg") >= 2
    lib.fxstub_fail_launches(0, 1, HIP_LAUNCH_FAILURE)
    assert lib.fxb_process_block(st2._h, vp(x), vp(y), 64) == FX_E_NODEVICE
    lib.fxstub_fail_launches(-1, 0, 0)
    assert lib.fxb_process_block(st2._h, vp(x), vp(y), 64) == 0 and st2.info("waves_per_wg") >= 2

    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    for p in (ppx, ppy, pwx, pwy):
        lib.fxb_host_free(p)
    print("block routes ok")


def child_retry():
    A, lib = stub_library()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    n, S = 300, 4096   # kCoolSamples / 2 per block
    b = A.Batch(n, 1, 0)
    assert b.load_text(chain_program(14)), b.errors()
    x = np.full((S, 1, n), 0.25, dtype=np.float32)
    y = np.zeros_like(x)
    assert lib.fxb_process_block(b._h, vp(x), vp(y), S) == 0 and b.info("waves_per_wg") >= 2, b.tier_note()
    assert b.set_register("vol", 0.6) == 0        # the first touch of a control: every declared control gets its row ...
    assert lib.fxb_process_block(b._h, vp(x), vp(y), S) == 0
    assert b.prepare(S, True) == 0
    assert b.info("control_rows") == 1, b.info("control_rows")   # ... and the ones at rest are folded back in: `vol` alone keeps it
    assert b.set_register("vol", 0.7) == 0        # written at sample clock T
    lib.fxstub_fail_launches(0, 1, HIP_LAUNCH_OUT_OF_RESOURCES)
    assert lib.fxb_process_block(b._h, vp(x), vp(y), S) == 0, b.last_error()   # refused with stages, run without: T + 4 096
    lib.fxstub_fail_launches(-1, 0, 0)
    assert b.info("waves_per_wg") == 1
    assert b.prepare(S, True) == 0
    assert b.info("control_rows") == 1, "`vol` cooled after %d sample periods" % S
    assert lib.fxb_process_block(b._h, vp(x), vp(y), S) == 0                   # T + 8 192
    assert b.prepare(S, True) == 0
    assert b.info("control_rows") == 0, b.info("control_rows")
    print("retry clock ok")


if __name__ == "__main__":
    {"routes": child_routes, "retry": child_retry}.get(sys.argv[1] if len(sys.argv) > 1 else "", child)()
