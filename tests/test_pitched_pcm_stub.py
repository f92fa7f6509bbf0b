"""Routing of row-pitched host blocks without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`) with three stand-in devices, driven through the C ABI in a child process (the binding reads
FX8010_AMD_LIB once, at import; this file is also that child).  A sharded handle over fxb_host_alloc buffers launches once per shard
and stages nothing, every shard on its own device's view of the buffers; pageable buffers are staged; the argument refusals of
fxb_process_block_pitched / fxb_process_block_dev_pitched launch nothing.  PCM values are not checked (the stand-in kernel copies in
to out): parity is tests/test_gpu_pitched_pcm.py."""
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


if __name__ == "__main__":
    child()
