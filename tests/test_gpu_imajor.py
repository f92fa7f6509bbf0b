"""Instance-major blocks on the GPU: fxb_process_block_imajor* against a second handle that runs fxb_process_block on the
transposed input.  The two kernels around the launch move words, so the bar is equality of every 32-bit pattern, NaNs included,
and of all instance state afterwards; instances 0, 63, 64 and N - 1 are checked against the oracle as well, which consumes exactly
these [S][C] runs.  Where a stride is padded the padding holds a sentinel pattern that must survive on both buffers."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SENTINEL = 0x7FC0DEAD   # a NaN with a payload


def use_tier(monkeypatch, name):
    """the three kernel tiers: the program translated to gfx950 code (xlate, the default), the hand-written interpreter (asm), the
    HIP C++ kernel (hip) - selected through FX_KERNEL like tests/test_gpu_bus.py does"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    if name != "xlate":
        monkeypatch.setenv("FX_KERNEL", name)


@pytest.fixture(params=["xlate", "asm", "hip"])
def tier(request, monkeypatch):
    use_tier(monkeypatch, request.param)
    return request.param


def right_tier(b, tier):
    k = b.info("kernel")
    return k >= 9 if tier == "xlate" else (1 <= k < 9 if tier == "asm" else k == 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def stereo(text):
    """the mono configuration programs with a second channel that goes through their state"""
    assert text.endswith("\nend") and "static t" in text
    return text[:-3].replace("output out 0", "output out 0\ninput in1 1\noutput out1 1", 1) + "macs out1, in1, t, 0.5\nend"


def program(name, channels):
    text = progs.CONFIGS[name]()
    return text if channels == 1 else stereo(text)


def register_names(gpu, text, channels):
    f = gpu.FrontEnd(channels)
    assert f.load_text(text), f.errors()
    return [r[0] for r in f.registers()]


def cutoffs(N):
    """one setting per instance: no two streams go through the same filter"""
    return (0.05 + 0.9 * (progs.stimulus(N, 1, seed=4242)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32)


def streams(N, S, channels, clock, seed=7):
    """[N, S, channels]: every instance's own interleaved run"""
    wide = np.stack([progs.stimulus(N, S, first_sample=clock, seed=seed + 1000 * c) for c in range(channels)], axis=1)   # [S, channels, N]
    return np.ascontiguousarray(wide.transpose(2, 0, 1))


def sample_major(x):
    """[N, S, channels] -> [S, channels, N]: what fxb_process_block takes"""
    return np.ascontiguousarray(x.transpose(1, 2, 0))


def handles(gpu, text, N, channels, count, control="cutoff", devices=None):
    out = []
    for k in range(count):
        b = gpu.Batch(N, channels, 0) if devices is None or k == 0 else gpu.Batch(N, channels, devices=devices)
        assert b.load_text(text), b.errors()
        if control:
            assert b.set_register_array(control, cutoffs(N)) == 0
        out.append(b)
    return out


def same_state(a, b, names, instances, tram=0):
    for r in names:
        assert np.array_equal(bits(a.get_register_array(r)), bits(b.get_register_array(r))), "register %s" % r
    assert a.instruction_counter() == b.instruction_counter()
    for n in instances:
        assert a.instruction_counter_i(n) == b.instruction_counter_i(n), n
        assert a.get_cursors_i(n) == b.get_cursors_i(n), n
        if tram:
            assert np.array_equal(bits(a.get_tram_i(0, n, tram)), bits(b.get_tram_i(0, n, tram))), n
    assert a.ood_flags() == b.ood_flags()


class Buffers:
    """the caller's side of a block in one of the layouts: N runs of R = S * channels words in a flat buffer, pinned or pageable,
    whose every other word holds the sentinel"""

    def __init__(self, gpu, N, S, channels, layout, pinned):
        self.N, self.S, self.ch, self.R = N, S, channels, S * channels
        self.stride, self.first = {"packed": (self.R, 0), "odd": (self.R + 3, 0), "view": (3 * self.R, self.R)}[layout]
        self.held = []
        self.flat_in, self.flat_out = self.alloc(gpu, pinned), self.alloc(gpu, pinned)

    def alloc(self, gpu, pinned):
        if pinned:
            self.held.append(gpu.HostBuffer((self.N * self.stride,)))
            a = self.held[-1].array
        else:
            a = np.empty(self.N * self.stride, dtype=np.float32)
        a.view(np.uint32)[...] = SENTINEL
        return a

    def runs(self, flat):
        """[N, S, channels] view of the runs"""
        return np.lib.stride_tricks.as_strided(flat[self.first:], shape=(self.N, self.S, self.ch), strides=(self.stride * 4, self.ch * 4, 4))

    def padding_intact(self, flat):
        mask = np.ones(flat.size, dtype=bool)
        mask[(self.first + np.arange(self.N)[:, None] * self.stride + np.arange(self.R)[None, :]).ravel()] = False
        return bool((flat.view(np.uint32)[mask] == SENTINEL).all())

    def process(self, b, x, one_buffer=False):
        """x through `b` by way of these buffers (the binding passes the views with their stride); the padding is checked"""
        self.runs(self.flat_in)[...] = x
        out = self.flat_in if one_buffer else self.flat_out
        got = b.process_block_imajor(self.runs(self.flat_in), out=self.runs(out))
        assert got.ctypes.data == self.runs(out).ctypes.data, "the views went to the library as they are"
        assert self.padding_intact(self.flat_in) and self.padding_intact(out), "a word outside the runs was written"
        if not one_buffer:
            assert same_bits(self.runs(self.flat_in), x), "the input was written"
        return np.array(got)

    def close(self):
        for h in self.held:
            h.close()


# (N, S, channels, layout, pinned, program): every N of {1, 63, 64, 65, 200, 4133}, every S of {1, 31, 32, 33, 65, 100}, both
# channel counts and the three layouts on the translated tier - tile edges on both axes, the narrow tile (R <= 32) and the square
# one, rows that start at every alignment; the other two tiers take (65, 33) and (200, 100)
SHAPES = [
    ("xlate", 1, 1, 1, "packed", False, "config3"),
    ("xlate", 63, 31, 2, "odd", True, "config2"),
    ("xlate", 64, 32, 1, "view", True, "config3"),
    ("xlate", 65, 33, 2, "odd", False, "config3"),
    ("xlate", 200, 100, 1, "odd", True, "config2"),
    ("xlate", 4133, 65, 1, "view", False, "config3"),
    ("xlate", 4133, 32, 1, "odd", True, "config2"),
    ("xlate", 4133, 31, 2, "packed", True, "config3"),
    ("xlate", 65, 1, 2, "view", True, "config2"),
    ("asm", 65, 33, 1, "odd", True, "config3"),
    ("asm", 200, 100, 2, "view", False, "config2"),
    ("hip", 65, 33, 2, "view", True, "config2"),
    ("hip", 200, 100, 1, "odd", False, "config3"),
]


@pytest.mark.parametrize("tier_name,N,S,channels,layout,pinned,name", SHAPES, ids=lambda v: str(v))
def test_imajor_blocks_bit_exact(gpu, monkeypatch, tier_name, N, S, channels, layout, pinned, name):
    """two blocks on one pair of handles whose state carries over, then the same once more on one buffer"""
    use_tier(monkeypatch, tier_name)
    text = program(name, channels)
    names = register_names(gpu, text, channels)
    plain, im = handles(gpu, text, N, channels, 2)
    watched = sorted({0, min(63, N - 1), min(64, N - 1), N - 1})
    oracles = []
    for n in watched:
        o = Oracle(channels)
        assert o.load_text(text), o.errors()
        o.set_register("cutoff", float(cutoffs(N)[n]))
        oracles.append(o)
    buf = Buffers(gpu, N, S, channels, layout, pinned)
    before = (im.info("host_staged_blocks"), im.info("host_inplace_blocks"))
    for block in range(3):
        x = streams(N, S, channels, block * S)
        y = plain.process_block(sample_major(x))
        got = buf.process(im, x, one_buffer=block == 2)
        assert same_bits(sample_major(got), y), "block %d" % block
        for n, o in zip(watched, oracles):
            ref = o.process_block(np.ascontiguousarray(x[n]))
            assert same_bits(ref.reshape(S, channels), got[n]), "block %d: instance %d differs from the oracle" % (block, n)
    same_state(im, plain, names, watched, tram=1000 if name == "config3" else 0)
    assert im.info("imajor_blocks") == 3 and im.info("bus_blocks") == 0 and right_tier(im, tier_name)
    after = (im.info("host_staged_blocks"), im.info("host_inplace_blocks"))
    assert (after[0] - before[0], after[1] - before[1]) == ((0, 3) if pinned else (3, 0))
    buf.close()


NONFINITE = ("static a\ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic big = 100000000000000000000000000000000000000.0\n"
             "static tiny = 0.00000000000000000000000000000000000001\nstatic t\n"
             "macs a, 0, vol, in\nmacw t, big, in, big\nmacw out, a, t, tiny\nend")


def test_every_kind_of_word_passes_through(gpu, tier):
    """NaN with a payload, +-Inf, -0 and denormals on the input: the same words reach the program as on the plain handle, and what
    it makes of them (MACW does not saturate: Inf and NaN reach the output) comes back pattern for pattern"""
    N, S = 200, 33
    plain, im = handles(gpu, NONFINITE, N, 1, 2, control="vol")
    x = streams(N, S, 1, 0)
    xb = x.view(np.uint32)
    xb[1, 5, 0], xb[63, 9, 0], xb[64, 11, 0], xb[199, 32, 0] = 0x7FC12345, 0x7F800000, 0xFF800000, 0xFFA00001
    xb[2, 0, 0], xb[3, 1, 0], xb[65, 2, 0] = 0x80000000, 0x00000001, 0x807FFFFF
    x[7, 3, 0] = 3.0
    y = plain.process_block(sample_major(x))
    assert np.isnan(y).any() and np.isinf(y).any() and np.isfinite(y).any()
    buf = Buffers(gpu, N, S, 1, "odd", True)
    assert same_bits(sample_major(buf.process(im, x)), y)
    same_state(im, plain, ["a", "t", "out", "ccr"], (0, 63, 64, N - 1))
    buf.close()


def test_two_blocks_are_one_of_their_length(gpu, tier):
    """16 + 17 samples walked through a longer allocation equal one block of 33"""
    text = progs.config3()
    names = register_names(gpu, text, 1)
    N = 200
    twice, once = handles(gpu, text, N, 1, 2)
    whole = streams(N, 40, 1, 0)
    out = np.zeros_like(whole)
    twice.process_block_imajor(whole[:, 3:19, :], out=out[:, 3:19, :])
    twice.process_block_imajor(whole[:, 19:36, :], out=out[:, 19:36, :])
    assert same_bits(out[:, 3:36, :], once.process_block_imajor(whole[:, 3:36, :]))
    assert not out[:, :3, :].any() and not out[:, 36:, :].any()
    same_state(twice, once, names, (0, 63, 64, N - 1), tram=1000)


def test_an_armed_control_track_applies(gpu, tier):
    text = progs.config3()
    names = register_names(gpu, text, 1)
    N, S = 200, 64
    plain, im = handles(gpu, text, N, 1, 2, control=None)
    steps = np.linspace(0.05, 0.9, 8).astype(np.float32)
    per = (steps[:, None] * (0.5 + 0.5 * cutoffs(N))[None, :]).astype(np.float32)   # [steps, N]
    for block, (key, values) in enumerate((("cutoff", steps), ("fb", per), ("cutoff", per))):
        x = streams(N, S, 1, block * S)
        for b in (plain, im):
            assert b.set_register_track(key, values, 8) == 0
        assert same_bits(sample_major(im.process_block_imajor(x)), plain.process_block(sample_major(x))), key
    same_state(im, plain, names, (0, 63, 64, N - 1), tram=1000)


def test_device_entry_on_another_stream_then_sync(gpu):
    """torch tensors, views into a longer per-instance tensor, on a stream that is not the default one; fxb_sync alone covers it"""
    import torch

    text = progs.config4()
    N, S, frames = 4133, 33, 100
    plain, im = handles(gpu, text, N, 1, 2)
    stream = torch.cuda.Stream()
    whole = streams(N, frames, 1, 0)
    d_in = torch.from_numpy(whole).to("cuda")
    d_out = torch.full((N, frames, 1), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for f0 in (0, S, 2 * S - 5):   # (the third block re-reads five frames: what matters is that both handles hear the same)
        y = plain.process_block(sample_major(whole[:, f0:f0 + S, :]))
        assert im.process_block_imajor_dev(d_in[:, f0:f0 + S, :], d_out[:, f0:f0 + S, :], S, stream=stream.cuda_stream) == 0
        assert im.sync() == 0
        assert same_bits(sample_major(d_out[:, f0:f0 + S, :].cpu().numpy()), y), f0
    assert bool((d_out[:, 2 * S - 5 + S:, :] == -7.0).all()), "frames behind the blocks were written"
    assert im.info("imajor_blocks") == 3 and im.info("host_staged_blocks") == 0 and im.info("host_inplace_blocks") == 0
    # one tensor both ways, packed, by pointer
    x = streams(N, S, 1, 1000)
    d = torch.from_numpy(x).to("cuda")
    torch.cuda.synchronize()
    y = plain.process_block(sample_major(x))
    assert im.process_block_imajor_dev(d.data_ptr(), d.data_ptr(), S, stream=stream.cuda_stream) == 0 and im.sync() == 0
    assert same_bits(sample_major(d.cpu().numpy()), y)
    same_state(im, plain, ["x", "a", "b", "o", "ccr"], (0, 63, 64, N - 1))


def test_meters_read_the_scratch_block(gpu):
    text = program("config3", 2)
    N, S = 4133, 33
    plain, im = handles(gpu, text, N, 2, 2)
    plain.meter_enable()
    im.meter_enable()
    buf = Buffers(gpu, N, S, 2, "odd", True)
    for block in range(2):
        x = streams(N, S, 2, block * S)
        assert same_bits(sample_major(buf.process(im, x)), plain.process_block(sample_major(x)))
    got, want = im.meter_read(), plain.meter_read()
    for key in ("energy", "peak", "full_scale", "nonfinite"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert want["peak"].max() > 0 and im.meter_samples() == 2 * S and im.info("meter_launches") == 2
    buf.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_handles_equal_the_single_one(gpu, shards):
    text = progs.config3()
    names = register_names(gpu, text, 1)
    N, S = 4133, 33
    plan = gpu.shard_plan(N, shards)
    for pinned in (False, True):
        single, many = handles(gpu, text, N, 1, 2, devices=[0] * shards)
        one, split = Buffers(gpu, N, S, 1, "packed", False), Buffers(gpu, N, S, 1, "odd", pinned)
        for block in range(2):
            x = streams(N, S, 1, block * S)
            assert same_bits(split.process(many, x, one_buffer=block == 1), one.process(single, x)), (pinned, block)
        same_state(many, single, names, (0, 63, 64, plan[1][0] - 1, plan[1][0], N - 1), tram=1000)
        assert many.info("imajor_blocks") == 2 * shards and many.info("bus_blocks") == 0
        assert (many.info("host_staged_blocks"), many.info("host_inplace_blocks")) == ((0, 2 * shards) if pinned else (2 * shards, 0))
        split.close()
    d = np.zeros((N, S, 1), dtype=np.float32)
    rc = gpu.load().fxb_process_block_imajor_dev(many._h, C.c_void_p(d.ctypes.data), C.c_void_p(d.ctypes.data), S, 0, 0, None)
    assert rc == FX_E_ARG and "one shard" in many.last_error()


def test_a_block_above_the_scratch_limit_equals_the_uncut_result(gpu):
    """262 107 instances x 96 samples: a per-instance block of 96 MiB, run in two pieces on the 64 MiB scratch, in place on one
    pinned buffer with a padded stride"""
    text = progs.config3()
    N, S = 262107, 96
    plain, im = handles(gpu, text, N, 1, 2)
    x = streams(N, S, 1, 0)
    y = plain.process_block(sample_major(x))
    buf = Buffers(gpu, N, S, 1, "odd", True)
    assert same_bits(sample_major(buf.process(im, x, one_buffer=True)), y)
    same_state(im, plain, ["rd", "a", "t", "s31", "out", "ccr"], (0, 63, 64, 131072, N - 1), tram=1000)
    assert im.info("imajor_blocks") == 1 and im.info("host_inplace_blocks") == 1
    buf.close()


def test_refusals_change_nothing(gpu):
    lib = gpu.load()
    N, S = 300, 8
    (b,) = handles(gpu, progs.config3(), N, 1, 1)
    x, y, both = gpu.HostBuffer((N, S)), gpu.HostBuffer((N, S)), gpu.HostBuffer((4 * N * S,))
    x.array[...] = 0.25
    y.array[...] = 0.5
    both.array[...] = 0.125
    page = np.zeros((N, S), dtype=np.float32)
    assert lib.fxb_process_block_imajor(b._h, C.c_void_p(x.array.ctypes.data), C.c_void_p(y.array.ctypes.data), S, 0, 0) == 0
    first = y.array.copy()
    ms = b.last_kernel_ms()
    look = lambda: (b.info("host_staged_blocks"), b.info("host_inplace_blocks"), b.info("imajor_blocks"), b.info("bus_blocks"), b.instruction_counter())
    seen = look()
    p = lambda h, off=0: C.c_void_p(h.array.ctypes.data + 4 * off)
    host, dev = lib.fxb_process_block_imajor, lib.fxb_process_block_imajor_dev
    refused = {
        "in stride below the run": lambda: host(b._h, p(x), p(y), S, S - 1, 0),
        "out stride below the run": lambda: host(b._h, p(x), p(y), S, 0, 1),
        "negative stride": lambda: host(b._h, p(x), p(y), S, 0, -S),
        "negative length": lambda: host(b._h, p(x), p(y), -1, 0, 0),
        "null in": lambda: host(b._h, None, p(y), S, 0, 0),
        "null out": lambda: host(b._h, p(x), None, S, 0, 0),
        "shifted by three words": lambda: host(b._h, p(both), p(both, 3), S, 0, 0),
        "out inside in": lambda: host(b._h, p(both), p(both, N * S - 1), S, 0, 0),
        "in inside out": lambda: host(b._h, p(both, N * S - 1), p(both), S, 0, 0),
        "one buffer, two strides": lambda: host(b._h, p(both), p(both), S, S, 2 * S),
        "two strides that meet": lambda: host(b._h, p(both), p(both, S), S, 3 * S, 2 * S),
        "device entry: stride below the run": lambda: dev(b._h, p(x), p(y), S, S - 1, 0, None),
        "device entry: null": lambda: dev(b._h, p(x), None, S, 0, 0, None),
        "device entry: overlap": lambda: dev(b._h, p(both), p(both, 1), S, 0, 0, None),
        "device entry: a pageable pointer": lambda: dev(b._h, C.c_void_p(page.ctypes.data), p(y), S, 0, 0, None),
    }
    for what, call in refused.items():
        assert call() == FX_E_ARG and b.last_error(), what
        assert b.last_kernel_ms() == ms and look() == seen, what
        assert np.array_equal(y.array, first) and (x.array == 0.25).all() and (both.array == 0.125).all(), what
    assert "not memory of this handle's device" in b.last_error()
    # zero samples: lowers the program, returns 0; interleaved footprints that share no element are fine
    assert host(b._h, None, None, 0, 0, 0) == 0 and host(b._h, p(x), p(y), 0, 0, 0) == 0 and look() == seen
    assert host(b._h, p(both), p(both, S), S, 2 * S, 2 * S) == 0, b.last_error()
    # ... and the handle goes on as one that was never refused anything
    (again,) = handles(gpu, progs.config3(), N, 1, 1)
    xs = np.full((N, S, 1), 0.25, dtype=np.float32)
    assert same_bits(again.process_block_imajor(xs).reshape(N, S), first)
    for h in (x, y, both):
        h.close()
