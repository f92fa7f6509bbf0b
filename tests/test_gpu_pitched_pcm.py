"""GPU tests of row-pitched PCM: a block's input and output are [sample][channel][P] floats with P >= N, the handle's instances
being columns 0..N-1 from the pointers passed in (fxb_process_block_pitched, fxb_process_block_dev_pitched).  Every tier addresses
PCM with P; P == N is what fxb_process_block has always done.  Every comparison is bit for bit, and every case also checks that
the columns outside the handle's range (the guard columns) still hold their sentinel words afterwards."""
import ctypes as C
import threading

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SENTINEL = np.uint32(0x7FBADBAD)   # a signalling-NaN pattern no program output has
CUTS = [0, 1, 34, 634]             # blocks of 1, 33 and 600 samples


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def multichannel(channels):
    """a delay-line program over `channels` inputs and outputs, with the control `decay`"""
    ins = "".join("input in%d %d\n" % (c, c) for c in range(channels))
    outs = "".join("output out%d %d\n" % (c, c) for c in range(channels))
    body = ("idelay read, rd, at, 0\nmacs a, in0, rd, decay\nmacs b, in%d, a, 0.5\nidelay write, b, at, 0\ninterp out0, out0, 0.25, a\n" % (channels - 1) +
            "".join("macs out%d, b, in%d, 0.125\n" % (c, c) for c in range(1, channels)))
    return "itramsize 100 \n" + ins + outs + "control decay = 0.45\nstatic rd\nstatic a\nstatic b\n" + body + "end"


def program(channels, n):
    """(text, control): config5 for the big mono batch, config2 (cut into stages at this size) for the small one"""
    if channels == 1:
        return (progs.config5(), "decay") if n > 1000 else (progs.config2(), "cutoff")
    return multichannel(channels), "decay"


def pinned(torch, shape):
    t = torch.empty(shape, dtype=torch.float32).pin_memory()
    t.numpy().view(np.uint32)[...] = SENTINEL
    return t


def drive(b, control, feed):
    """the block sequence of every case: a slider moves before the second block, a control schedule runs inside the third"""
    for k, (lo, hi) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        if k == 1:
            b.set_register(control, 0.3)
        if k == 2:
            b.set_register_track(control, np.array([0.2, 0.5, 0.1, 0.4], dtype=np.float32), 150)
        feed(lo, hi)


def oracle_column(text, control, x, inst, channels):
    o = Oracle(channels)
    assert o.load_text(text)
    ref = []
    for k, (lo, hi) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        if k == 1:
            o.set_register(control, 0.3)
        if k == 2:
            for t, v in enumerate((0.2, 0.5, 0.1, 0.4)):
                o.set_register(control, v)
                ref.append(o.process_block(x[lo + 150 * t:(lo + 150 * (t + 1) if t < 3 else hi), :, inst].copy()))
            continue
        ref.append(o.process_block(x[lo:hi, :, inst].copy()))
    return np.concatenate(ref, axis=0)


def dense_run(gpu, text, control, x, n, channels, devices=None):
    b = gpu.Batch(n, channels, 0) if devices is None else gpu.Batch(n, channels, devices=devices)
    assert b.load_text(text), b.errors()
    out = []
    drive(b, control, lambda lo, hi: out.append(b.process_block(x[lo:hi].copy())))
    assert b.ood_flags() == 0
    return np.concatenate(out, axis=0)


@pytest.fixture(params=["default", "asm", "hip1", "hip2", "hip4"])
def tier(request, monkeypatch):
    """tier 1 (translated, the default), tier 2 (the interpreter) and tier 3 (the HIP C++ kernel, 1 / 2 / 4 instances per lane:
    an odd first column takes its per-instance I/O)"""
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_HOST_PIPELINE", "FX_STAGES"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "asm":
        monkeypatch.setenv("FX_KERNEL", "asm")
    elif request.param.startswith("hip"):
        monkeypatch.setenv("FX_KERNEL", "hip")
        monkeypatch.setenv("FX_INST_PER_LANE", request.param[3:])
    return request.param


@pytest.mark.parametrize("n", [20000, 200])
@pytest.mark.parametrize("channels", [1, 2, 4])
def test_column_range_of_a_pinned_buffer_in_place(gpu, tier, channels, n):
    """one handle on columns [a, a + N) of a pinned [S][ch][M] buffer, M = N + 200, a in {0, 37, 64}: bit-exact against the same
    program fed dense copies, guard columns intact, every block in place"""
    import torch
    text, control = program(channels, n)
    S, M = CUTS[-1], n + 200
    x = progs.stimulus(n * channels, S).reshape(S, channels, n)
    want = dense_run(gpu, text, control, x, n, channels)
    kernel, waves = None, []
    for a in (0, 37, 64):
        pin_in, pin_out = pinned(torch, (S, channels, M)), pinned(torch, (S, channels, M))
        xin, yout = pin_in.numpy(), pin_out.numpy()
        xin[:, :, a:a + n] = x
        before = bits(xin).copy()
        b = gpu.Batch(n, channels, 0)
        assert b.load_text(text), b.errors()
        lib = gpu.load()

        def feed(lo, hi):
            off = (lo * channels * M + a) * 4
            rc = lib.fxb_process_block_pitched(b._h, C.c_void_p(xin.ctypes.data + off), C.c_void_p(yout.ctypes.data + off), hi - lo, M)
            assert rc == 0, b.last_error()
            waves.append(b.info("waves_per_wg"))
        drive(b, control, feed)
        assert b.ood_flags() == 0
        assert np.array_equal(bits(yout[:, :, a:a + n]), bits(want)), (tier, a)
        guard = np.ones(M, dtype=bool)
        guard[a:a + n] = False
        assert (bits(yout)[:, :, guard] == SENTINEL).all(), "a column outside the handle's range was written (a = %d)" % a
        assert np.array_equal(bits(xin), before), "the input buffer changed"
        assert b.info("host_inplace_blocks") == len(CUTS) - 1 and b.info("host_staged_blocks") == 0
        kernel = b.info("kernel")
    assert (kernel >= 9) if tier == "default" else ((1 <= kernel <= 8) if tier == "asm" else kernel == 0), (tier, kernel)
    if tier == "default" and channels == 1 and n == 200:
        assert max(waves) >= 2, "the small batch was never cut into stages: %s" % waves
    if tier == "default" and channels <= 2:
        for inst in (0, n - 1):
            assert np.array_equal(bits(oracle_column(text, control, x, inst, channels)), bits(want[:, :, inst])), inst


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_handle_in_place_on_pinned_buffers(gpu, shards, monkeypatch):
    """fxb_create_on_devices([0] * shards) over pinned dense buffers: every shard processes its columns in place (no staged
    block), in != out and in == out, bit-exact against a single handle; pageable buffers give the same bits, staged"""
    import torch
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_HOST_PIPELINE", "FX_STAGES"):
        monkeypatch.delenv(k, raising=False)
    n, S = 20000, CUTS[-1]
    text, control = progs.config5(), "decay"
    x = progs.stimulus(n, S).reshape(S, 1, n)
    want = dense_run(gpu, text, control, x, n, 1)
    for alias in (False, True):
        pin_in, pin_out = pinned(torch, (S, 1, n)), pinned(torch, (S, 1, n))
        xin, yout = pin_in.numpy(), pin_out.numpy()
        xin[...] = x
        b = gpu.Batch(n, 1, devices=[0] * shards)
        assert len(b.shards()) == shards
        assert b.load_text(text), b.errors()
        got = []

        def feed(lo, hi):
            if alias:
                buf = xin[lo:hi]
                got.append(b.process_block(buf, buf).copy())
            else:
                got.append(b.process_block(xin[lo:hi], yout[lo:hi]).copy())
        drive(b, control, feed)
        assert np.array_equal(bits(np.concatenate(got, axis=0)), bits(want)), alias
        assert b.info("host_staged_blocks") == 0, "a shard staged its columns of a pinned buffer"
        assert b.info("host_inplace_blocks") == shards * (len(CUTS) - 1)
    got = dense_run(gpu, text, control, x, n, 1, devices=[0] * shards)
    assert np.array_equal(bits(got), bits(want))
    b = gpu.Batch(n, 1, devices=[0] * shards)
    assert b.load_text(text)
    b.process_block(x[:33].copy())
    assert b.info("host_staged_blocks") == shards and b.info("host_inplace_blocks") == 0


def test_two_handles_two_programs_one_buffer(gpu, monkeypatch):
    """config5 (mono) and a stereo delay line on disjoint column ranges of ONE pinned [S][2][M] buffer, driven from two threads
    at once - the mono handle on channel 0's columns [a1, a1 + N1) with a pitch of 2M, the stereo one on columns [a2, a2 + N2) of
    both channels with a pitch of M: each bit-exact against its own dense run, the guard columns around and between them intact"""
    import torch
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_HOST_PIPELINE", "FX_STAGES"):
        monkeypatch.delenv(k, raising=False)
    S = CUTS[-1]
    n1, n2 = 20000, 7000
    a1, a2 = 16, 16 + n1 + 45
    M = a2 + n2 + 30
    t1, t2 = progs.config5(), multichannel(2)
    x1 = progs.stimulus(n1, S).reshape(S, 1, n1)
    x2 = progs.stimulus(n2 * 2, S, first_sample=5).reshape(S, 2, n2)
    w1 = dense_run(gpu, t1, "decay", x1, n1, 1)
    w2 = dense_run(gpu, t2, "decay", x2, n2, 2)
    pin_in, pin_out = pinned(torch, (S, 2, M)), pinned(torch, (S, 2, M))
    xin, yout = pin_in.numpy(), pin_out.numpy()
    xin[:, 0:1, a1:a1 + n1] = x1
    xin[:, :, a2:a2 + n2] = x2
    mono_in, mono_out = xin.reshape(S, 1, 2 * M), yout.reshape(S, 1, 2 * M)
    b1, b2 = gpu.Batch(n1, 1, 0), gpu.Batch(n2, 2, 0)
    assert b1.load_text(t1) and b2.load_text(t2)
    jobs = [(b1, lambda lo, hi: b1.process_block(mono_in[lo:hi, :, a1:a1 + n1], mono_out[lo:hi, :, a1:a1 + n1])),
            (b2, lambda lo, hi: b2.process_block(xin[lo:hi, :, a2:a2 + n2], yout[lo:hi, :, a2:a2 + n2]))]
    errors = []

    def worker(b, feed):
        try:
            drive(b, "decay", feed)
        except Exception as e:   # (re-raised on the main thread)
            errors.append(e)
    threads = [threading.Thread(target=worker, args=job) for job in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert np.array_equal(bits(yout[:, 0:1, a1:a1 + n1]), bits(w1))
    assert np.array_equal(bits(yout[:, :, a2:a2 + n2]), bits(w2))
    written = np.zeros((2, M), dtype=bool)
    written[0, a1:a1 + n1] = True
    written[:, a2:a2 + n2] = True
    assert (bits(yout)[:, ~written] == SENTINEL).all()
    for b in (b1, b2):
        assert b.info("host_inplace_blocks") == len(CUTS) - 1 and b.info("host_staged_blocks") == 0


@pytest.mark.parametrize("a", [0, 37])
def test_device_pitch_on_a_torch_column_slice(gpu, a, monkeypatch):
    """fxb_process_block_dev_pitched on t[:, :, a:a + N] of torch device tensors, on torch's current stream"""
    import torch
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_HOST_PIPELINE", "FX_STAGES"):
        monkeypatch.delenv(k, raising=False)
    n, ch, S = 20000, 2, CUTS[-1]
    M = n + 100
    text = multichannel(ch)
    x = progs.stimulus(n * ch, S).reshape(S, ch, n)
    want = dense_run(gpu, text, "decay", x, n, ch)
    host = np.full((S, ch, M), SENTINEL, dtype=np.uint32).view(np.float32)
    host[:, :, a:a + n] = x
    tin = torch.from_numpy(host).cuda()
    tout = torch.from_numpy(np.full((S, ch, M), SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
    b = gpu.Batch(n, ch, 0)
    assert b.load_text(text), b.errors()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    drive(b, "decay", lambda lo, hi: b.process_block_dev_pitched(tin[lo:hi, :, a:a + n], tout[lo:hi, :, a:a + n], hi - lo, stream=stream))
    torch.cuda.current_stream().synchronize()
    b.sync()
    y = tout.cpu().numpy()
    assert np.array_equal(bits(y[:, :, a:a + n]), bits(want))
    guard = np.ones(M, dtype=bool)
    guard[a:a + n] = False
    assert (bits(y)[:, :, guard] == SENTINEL).all()
    assert np.array_equal(bits(tin.cpu().numpy()), bits(host))


def test_refusals_leave_the_handle_usable(gpu, monkeypatch):
    """pitch < N, channels * P * 4 >= 2^32, a pageable pointer to dev_pitched, dev_pitched on two shards: FX_E_ARG without a
    launch, and the handle goes on working"""
    import torch
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_HOST_PIPELINE", "FX_STAGES"):
        monkeypatch.delenv(k, raising=False)
    lib = gpu.load()
    n, S = 1000, 8
    text = progs.config5()
    x = progs.stimulus(n, S).reshape(S, 1, n)
    b = gpu.Batch(n, 1, 0)
    assert b.load_text(text)
    first = b.process_block(x[:S].copy())
    grid = b.info("grid")
    page_in, page_out = x.copy(), np.empty_like(x)
    pin = torch.empty((S, 1, n), dtype=torch.float32).pin_memory().numpy()
    pin[...] = x
    dev = torch.from_numpy(x.copy()).cuda()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.fxb_process_block_pitched(b._h, vp(page_in), vp(page_out), S, n - 1) == FX_E_ARG
    assert lib.fxb_process_block_pitched(b._h, vp(page_in), vp(page_out), S, 0) == FX_E_ARG
    assert lib.fxb_process_block_pitched(b._h, vp(page_in), vp(page_out), S, 1 << 30) == FX_E_ARG
    assert lib.fxb_process_block_dev_pitched(b._h, C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr()), S, 1 << 30, None) == FX_E_ARG
    assert lib.fxb_process_block_dev_pitched(b._h, vp(page_in), C.c_void_p(dev.data_ptr()), S, n, None) == FX_E_ARG
    assert lib.fxb_process_block_dev_pitched(b._h, C.c_void_p(dev.data_ptr()), vp(page_out), S, n, None) == FX_E_ARG
    assert "not memory of this handle's device" in b.last_error()
    assert b.info("host_staged_blocks") == 1 and b.info("host_inplace_blocks") == 0
    # (the refused calls consumed no block: the next one continues from the first)
    second = b.process_block(x[:S].copy())
    ref = gpu.Batch(n, 1, 0)
    assert ref.load_text(text)
    ref.process_block(x[:S].copy())
    assert np.array_equal(bits(second), bits(ref.process_block(x[:S].copy())))
    assert b.info("grid") == grid
    # device-visible host memory is accepted by dev_pitched
    out = torch.empty((S, 1, n), dtype=torch.float32).pin_memory().numpy()
    assert lib.fxb_process_block_dev_pitched(b._h, vp(pin), vp(out), S, n, None) == 0 and b.sync() == 0
    assert np.array_equal(bits(out), bits(ref.process_block(x[:S].copy())))
    two = gpu.Batch(n, 1, devices=[0, 0])
    assert two.load_text(text)
    assert lib.fxb_process_block_dev_pitched(two._h, C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr()), S, n, None) == FX_E_ARG
    assert "fxb_process_block_dev_shards" in two.last_error()
    assert np.array_equal(bits(two.process_block(x[:S].copy())), bits(first))
