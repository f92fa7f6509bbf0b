"""Output meters on the GPU (fxb_meter_*): the four accumulator arrays against meter_model() - the numpy restatement of the
definition in include/fx8010_amd.h, written out in tests/test_meter_stub.py - of the per-instance output block y.  y is what a
twin handle with meters off returns for the same block; for bus blocks it is the twin's plain process_block on the expanded
input.  Bar: every comparison bit for bit (fp64 and fp32 words as integers), no tolerances; and metering changes nothing else -
outputs and all instance state equal the twin's.  Shapes: N = 197 (three wavefronts plus five lanes, not a multiple of 4),
N = 256 (aligned), S = 33 (four rounds of eight loads plus one sample)."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_bus_stub import expand, mix_model
from test_meter_stub import FIELDS, meter_model, meter_zero, same_meters

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
MODES = ((True, False), (False, True), (True, True))
MORE = "static zz\nmacs zz, zz, 0.5, 0.5\nend"   # a further load that succeeds: registers and instructions accumulate over loads
NONFINITE = ("static a\ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic big = 100000000000000000000000000000000000000.0\n"
             "static tiny = 0.00000000000000000000000000000000000001\nstatic t\n"
             "macs a, 0, vol, in\nmacw t, big, in, big\nmacw out, a, t, tiny\nend")
PASS_THROUGH = "input in 0\noutput out 0\nmacs out, in, 0, 0\nend"   # MACS saturates: +-1.5 comes out as +-1


@pytest.fixture(params=["default", "asm", "hip"], ids=["xlate", "asm", "hip"])
def tier(request, monkeypatch):
    """the three kernel tiers, selected through FX_KERNEL like tests/test_gpu_bus.py does"""
    for name in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(name, raising=False)
    if request.param != "default":
        monkeypatch.setenv("FX_KERNEL", request.param)
    return request.param


def on_tier(b, tier):
    k = b.info("kernel")
    return k >= 9 if tier == "default" else (1 <= k < 9 if tier == "asm" else k == 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def same_words(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and bool((bits(got)[~nan] == bits(want)[~nan]).all())


def stereo(text):
    assert text.endswith("\nend") and "static t" in text
    return text[:-3].replace("output out 0", "output out 0\ninput in1 1\noutput out1 1", 1) + "macs out1, in1, t, 0.5\nend"


def cutoffs(N):
    return (0.05 + 0.9 * (progs.stimulus(N, 1, seed=4242)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32)


def pcm(width, S, channels, clock, seed=7):
    return np.ascontiguousarray(np.stack([progs.stimulus(width, S, first_sample=clock, seed=seed + 1000 * c) for c in range(channels)], axis=1))   # [S, channels, width]


def pair(gpu, text, N, channels, control="cutoff", values=None, devices=None):
    """(the handle with meters on, its twin with meters off)"""
    out = []
    for metered in (True, False):
        b = gpu.Batch(N, channels, 0) if devices is None or not metered else gpu.Batch(N, channels, devices=devices)
        assert b.load_text(text), b.errors()
        if control:
            assert b.set_register_array(control, cutoffs(N) if values is None else values) == 0
        if metered:
            assert b.meter_enable() == 0 and b.meter_samples() == 0
        out.append(b)
    return out


def register_names(gpu, text, channels):
    f = gpu.FrontEnd(channels)
    assert f.load_text(text), f.errors()
    return [r[0] for r in f.registers()]


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


@pytest.mark.parametrize("channels", [1, 2])
def test_every_route_meters_the_block_it_wrote(gpu, tier, channels):
    import torch

    text = progs.config3() if channels == 1 else stereo(progs.config3())
    names = register_names(gpu, text, channels)
    S = 33
    for N in (197, 256, 4133):
        m, t = pair(gpu, text, N, channels)
        model = meter_zero(channels, N)
        state = {"clock": 0, "samples": 0, "launches": 0}

        def took(what, y, launches=1):
            """both handles have processed a block (outputs compared by the caller): y is the per-instance block it wrote"""
            nonlocal model
            model = meter_model(y, model)
            state["samples"] += y.shape[0]
            state["launches"] += launches
            assert same_meters(m.meter_read(), model), "%s: N %d" % (what, N)
            assert m.meter_samples() == state["samples"] and m.info("meter_launches") == state["launches"], what

        def fresh(width, samples=S):
            x = pcm(width, samples, channels, state["clock"])
            state["clock"] += samples
            return x

        # pageable host blocks: staged; a few KB go through the library's own pinned pair
        x = fresh(N)
        y = t.process_block(x)
        got = m.process_block(x)
        assert same_bits(got, y)
        took("pageable", y)
        if N == 4133:
            same_state(m, t, names, (0, 63, 64, N - 1), tram=1000)
            continue
        x = fresh(N, 512 // (channels * N))
        y = t.process_block(x)
        got = m.process_block(x)
        assert same_bits(got, y)
        took("a few KB", y)
        # pinned host block, in place: the meter kernel reads the caller's buffer back
        pin_in, pin_out = gpu.HostBuffer((S, channels, N)), gpu.HostBuffer((S, channels, N))
        pin_in.array[...] = fresh(N)
        y = t.process_block(pin_in.array.copy())
        before = m.info("host_inplace_blocks")
        assert m.process_block(pin_in.array, out=pin_out.array) is pin_out.array and m.info("host_inplace_blocks") == before + 1
        assert same_bits(pin_out.array, y)
        took("pinned in place", y)
        pin_in.close()
        pin_out.close()
        # device entry at pitch N and at pitch N + 59
        for P in (N, N + 59):
            x = fresh(N)
            y = t.process_block(x)
            d_in = torch.zeros((S, channels, P), dtype=torch.float32, device="cuda")
            d_out = torch.full((S, channels, P), -7.0, dtype=torch.float32, device="cuda")
            d_in[:, :, :N] = torch.from_numpy(x).to("cuda")
            torch.cuda.synchronize()
            assert m.process_block_dev_pitched(d_in[:, :, :N], d_out[:, :, :N], S) == 0
            assert m.sync() == 0
            got = d_out.cpu().numpy()
            assert same_bits(got[:, :, :N], y) and (got[:, :, N:] == -7.0).all()
            took("device entry at pitch %d" % P, y)
        # bus blocks: the meters watch the scratch block between the emulation and the mix or the copy-out
        for K in (3, 64, 65):
            G = m.bus_groups(K)
            for shared_in, mix_out in MODES:
                xg = fresh(G)
                x = expand(xg, K, N) if shared_in else fresh(N)
                y = t.process_block(x)
                got = m.process_block_bus(xg if shared_in else x, K, shared_in, mix_out)
                assert same_words(got, mix_model(y, K) if mix_out else y), (N, K, shared_in, mix_out)
                took("bus K %d shared_in %d mix_out %d" % (K, shared_in, mix_out), y)
        same_state(m, t, names, (0, 63, 64, N - 1), tram=1000)
        assert on_tier(m, tier) and on_tier(t, tier)
        m.close()
        t.close()


def test_nonfinite_words_are_counted_and_kept_out_of_peak_and_energy(gpu, tier):
    """MACW does not saturate: an input of 3 puts +Inf on the output, a NaN input a NaN, -Inf itself - in a few columns"""
    N, S = 197, 33
    m, t = pair(gpu, NONFINITE, N, 1, control="vol")
    x = pcm(N, S, 1, 0)
    poisoned = {(5, 0): 3.0, (9, 63): np.nan, (11, 64): -np.inf, (12, 64): np.nan, (32, N - 1): 3.0, (0, 130): -np.inf}
    for (s, n), v in poisoned.items():
        x[s, 0, n] = v
    y = t.process_block(x)
    assert same_words(m.process_block(x), y)
    got, want = m.meter_read(), meter_model(y)
    assert same_meters(got, want)
    count = np.zeros((1, N), dtype=np.uint32)
    for (s, n) in poisoned:
        count[0, n] += 1
    assert np.array_equal(got["nonfinite"], count), "exactly the poisoned words"
    assert np.isfinite(got["energy"]).all() and np.isfinite(got["peak"]).all() and (got["energy"][0, [0, 63, 64, 130, N - 1]] > 0).all()
    same_state(m, t, ["a", "t", "out", "ccr"], (0, 63, 64, N - 1))
    # a saturating pass-through fed +-1.5: every sample sits at the rail
    m, t = pair(gpu, PASS_THROUGH, N, 1, control=None)
    x = np.where(pcm(N, S, 1, 0) < 0, np.float32(-1.5), np.float32(1.5)).astype(np.float32)
    y = t.process_block(x)
    assert same_bits(m.process_block(x), y) and (np.abs(y) == 1.0).all()
    got = m.meter_read()
    assert same_meters(got, meter_model(y))
    assert (got["full_scale"] == S).all() and (got["peak"].view(np.uint32) == 0x3F800000).all() and (got["energy"] == float(S)).all() and (got["nonfinite"] == 0).all()
    assert on_tier(m, tier)


def test_blocks_accumulate_and_resets_zero(gpu, tier):
    text = progs.config3()
    N = 197
    twice, _ = pair(gpu, text, N, 1)
    once, t = pair(gpu, text, N, 1)
    x = pcm(N, 33, 1, 0)
    y = t.process_block(x)
    twice.process_block(x[:16])
    twice.process_block(x[16:])
    once.process_block(x)
    want = meter_model(y)
    assert same_meters(once.meter_read(), want) and same_meters(twice.meter_read(), want), "16 + 17 samples are one block of 33"
    assert twice.meter_samples() == 33 and once.meter_samples() == 33
    assert twice.info("meter_launches") == 2 and once.info("meter_launches") == 1
    # read with reset: the values once more, then zeros and 0 samples
    assert same_meters(twice.meter_read(reset=True), want)
    assert same_meters(twice.meter_read(), meter_zero(1, N)) and twice.meter_samples() == 0
    # a program load resets the meters and keeps them enabled
    assert once.load_text(MORE) and t.load_text(MORE), once.errors()
    assert once.meter_samples() == 0 and same_meters(once.meter_read(), meter_zero(1, N))
    x = pcm(N, 17, 1, 33)
    y = t.process_block(x)
    assert same_bits(once.process_block(x), y) and same_meters(once.meter_read(), meter_model(y)) and once.meter_samples() == 17


def test_pieces_are_metered_in_order(gpu):
    """262 107 instances x 96 samples on a bus: a scratch block of 96 MiB in two pieces; then a pageable block of 34.6 MB, which
    takes the pipelined route in eight pieces.  The meters equal the model of the uncut plain output."""
    text = progs.config3()
    N, S, K = 262107, 96, 64
    m, t = pair(gpu, text, N, 1)
    xg = pcm(m.bus_groups(K), S, 1, 0)
    y = t.process_block(expand(xg, K, N))
    assert same_words(m.process_block_bus(xg, K), mix_model(y, K))
    model = meter_model(y)
    assert m.info("meter_launches") == 2 and m.meter_samples() == S
    assert same_meters(m.meter_read(), model)
    x = pcm(N, 33, 1, S)
    assert x.nbytes >= 32 << 20
    y = t.process_block(x)
    assert same_bits(m.process_block(x), y)
    assert m.info("meter_launches") == 2 + 8 and m.meter_samples() == S + 33
    assert same_meters(m.meter_read(), meter_model(y, model))
    same_state(m, t, ["rd", "a", "t", "s31", "out", "ccr"], (0, 63, 64, 131072, N - 1), tram=1000)


def test_an_armed_control_track_is_metered_segment_by_segment(gpu, tier):
    """a 33-sample block with a period-8 track: the interpreter and HIP tiers cut it into five segments, each metered once, in
    order; the translated tier reads the schedule by itself: one launch"""
    text = progs.config3()
    N, S = 197, 33
    m, t = pair(gpu, text, N, 1, control=None)
    steps = np.linspace(0.05, 0.9, 5).astype(np.float32)
    model = meter_zero(1, N)
    launches = 0
    for block, bus in enumerate((False, True)):
        for b in (m, t):
            assert b.set_register_track("cutoff", steps, 8) == 0
        if bus:
            xg = pcm(m.bus_groups(64), S, 1, block * S)
            y = t.process_block(expand(xg, 64, N))
            assert same_words(m.process_block_bus(xg, 64), mix_model(y, 64))
        else:
            x = pcm(N, S, 1, block * S)
            y = t.process_block(x)
            assert same_bits(m.process_block(x), y)
        model = meter_model(y, model)
        assert same_meters(m.meter_read(), model), bus
        assert on_tier(m, tier)
        launches += 1 if tier == "default" else 5
        assert m.info("meter_launches") == launches and m.meter_samples() == (block + 1) * S
    same_state(m, t, register_names(gpu, text, 1), (0, 63, 64, N - 1), tram=1000)


@pytest.mark.parametrize("shards,N", [(2, 64 * 10 + 17), (3, 64 * 16 + 17)])
def test_sharded_handles_equal_the_single_one(gpu, shards, N):
    text = stereo(progs.config3())
    S = 33
    many, t = pair(gpu, text, N, 2, devices=[0] * shards)
    one, _ = pair(gpu, text, N, 2)
    assert len(many.shards()) == shards
    model = meter_zero(2, N)
    pin_in, pin_out = gpu.HostBuffer((S, 2, N)), gpu.HostBuffer((S, 2, N))
    for block, route in enumerate(("pageable", "pinned", "bus")):
        x = pcm(N, S, 2, block * S)
        if route == "bus":
            xg = pcm(many.bus_groups(64), S, 2, block * S)
            x = expand(xg, 64, N)
            assert same_bits(many.process_block_bus(xg, 64), one.process_block_bus(xg, 64))
            y = t.process_block(x)
        elif route == "pinned":
            pin_in.array[...] = x
            y = t.process_block(x)
            assert many.process_block(pin_in.array, out=pin_out.array) is pin_out.array and same_bits(pin_out.array, y)
            assert same_bits(one.process_block(x), y)
        else:
            y = t.process_block(x)
            assert same_bits(many.process_block(x), y) and same_bits(one.process_block(x), y)
        model = meter_model(y, model)
        got = many.meter_read()
        assert same_meters(got, one.meter_read()) and same_meters(got, model), route
        assert many.meter_samples() == one.meter_samples() == (block + 1) * S
        assert many.info("meter_launches") == shards * (block + 1) and one.info("meter_launches") == block + 1
    assert same_meters(many.meter_read(reset=True), model) and many.meter_samples() == 0 and same_meters(many.meter_read(), meter_zero(2, N))
    pin_in.close()
    pin_out.close()


def test_refusals_change_nothing(gpu):
    lib = gpu.load()
    N, S = 197, 33
    b = gpu.Batch(N, 2, 0)
    assert b.load_text(stereo(progs.config3())), b.errors()
    x = pcm(N, S, 2, 0)
    arrays = meter_zero(2, N)
    for a in arrays.values():
        a[...] = 9
    ptrs = [C.c_void_p(arrays[k].ctypes.data) for k in FIELDS]
    # metering is off by default: read and samples are refused, nothing changes, a block launches no meter
    assert lib.fxb_meter_read(b._h, *ptrs, 0) == FX_E_ARG and "metering is off" in b.last_error()
    assert lib.fxb_meter_read(b._h, None, None, None, None, 1) == FX_E_ARG and lib.fxb_meter_samples(b._h) == FX_E_ARG
    assert all((a == 9).all() for a in arrays.values())
    y = b.process_block(x)
    assert b.info("meter_launches") == 0 and lib.fxb_meter_enable(b._h, 0) == 0
    # a NULL handle
    assert lib.fxb_meter_enable(None, 1) == FX_E_ARG and lib.fxb_meter_read(None, *ptrs, 0) == FX_E_ARG and lib.fxb_meter_samples(None) == FX_E_ARG
    # on; a read with all pointers NULL and reset is legal; any one pointer may be NULL
    assert b.meter_enable() == 0 and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
    y = b.process_block(x)
    want = meter_model(y)
    for skip in range(4):
        for a in arrays.values():
            a[...] = 9
        assert lib.fxb_meter_read(b._h, *[None if k == skip else p for k, p in enumerate(ptrs)], 0) == 0
        for k, key in enumerate(FIELDS):
            assert (arrays[key] == 9).all() if k == skip else np.array_equal(arrays[key].view(np.uint8), want[key].view(np.uint8)), (skip, key)
    # enabling twice keeps the values; the state image does not hold them
    assert b.meter_enable() == 0 and same_meters(b.meter_read(), want) and b.meter_samples() == S
    image = b.save_state()
    b.load_state(image)
    assert same_meters(b.meter_read(), want) and b.meter_samples() == S
    assert lib.fxb_meter_read(b._h, None, None, None, None, 1) == 0 and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
    # disabling then enabling gives zeros
    b.process_block(x)
    assert b.meter_samples() == S and b.meter_enable(False) == 0 and lib.fxb_meter_samples(b._h) == FX_E_ARG
    assert b.meter_enable() == 0 and b.meter_samples() == 0 and same_meters(b.meter_read(), meter_zero(2, N))
