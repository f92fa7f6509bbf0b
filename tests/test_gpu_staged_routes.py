"""STAGED code under the bus routes, the meters, instance-major blocks and the by-list state calls.  A batch of a few hundred
voices of a chain-like program runs as a pipeline of stages by default (the wavefronts of one workgroup, live rows handed over
through LDS, every state row stored at block end by the stage of its last write) - and the features those batches use were tested
on config3 / config4 only, which the planner cannot cut.  Here three programs it does cut (staged_route_programs.py; the cuts and
the stages that store the named registers are asserted without a GPU in test_staged_route_programs.py) go through those routes.

Every test builds three handles: S under FX_STAGES=4, D with the default policy (stage tuner on), U under FX_STAGES=1 - the knobs
are copied when a handle is created - and asserts after every block that S and D ran two or more wavefronts per workgroup
(FXB_INFO_WAVES_PER_WG) on translated code and U one.  References: one oracle object per instance, all 200, for every
per-instance word (outputs, every register, output latches, positions, delay memory, LFSR words, instruction counters); the numpy
models of the route tests, fed with the oracles' outputs, for mix, tap, aux and meter rows; and U, the tier those route tests pin
to the same models, for bit equality of every side row.  The by-list calls are modelled by tools/fuzz_voices.py's voice model.

N = 200: four workgroups of staged code, the last with 8 instances.  Blocks of a few dozen samples, 300 where a class of block
lengths needs it."""
import os
import sys

import numpy as np
import pytest

import fx8010_programs as progs
import meter_level_model as LV
import meter_list_model as ML
import meter_target_model as TG
import staged_route_programs as SP
from pyoracle import Oracle
from route_models import expand, feed_model, gain_mix_model, gains_for, meter_model, meter_zero, mix_model, same_meters, same_words, send_model
from test_bus_feed_stub import feed_structure
from test_gpu_bus import cutoffs, group_input

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

N = 200
ALL = np.arange(N, dtype=np.int64)
WATCH = (0, 63, 64, 127, 128, 191, 192, 199)      # both sides of every wavefront and shard boundary
SHARDS = [(0, 128), (128, 64), (192, 8)]
STATE_TYPES = (0, 1, 2, 3, 4, 11)                 # fx_model.hpp RegType: static, temp, control, input, output, ccr


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and bool((got.view(np.uint32) == want.view(np.uint32)).all())


def first_bad(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return bad[:4].tolist(), len(bad)


@pytest.fixture
def make(gpu, monkeypatch):
    """make(name, devices=None, builder=True, only=None) -> {"S": ..., "D": ..., "U": ...}: handles of one program, created under
    FX_STAGES=4, unset and 1"""
    def build(name, devices=None, builder=True, only=("S", "D", "U")):
        for k in [k for k in os.environ if k.startswith("FX_")]:
            monkeypatch.delenv(k, raising=False)
        if not builder:
            monkeypatch.setenv("FX_BUILDER", "0")
        channels, text = SP.PROGRAMS[name][:2]
        out = Trio()
        out.name = name
        for tag, stages in (("S", "4"), ("D", None), ("U", "1")):
            if tag not in only:
                continue
            if stages is None:
                monkeypatch.delenv("FX_STAGES", raising=False)
            else:
                monkeypatch.setenv("FX_STAGES", stages)
            b = gpu.Batch(N, channels, 0) if devices is None else gpu.Batch(N, channels, devices=devices)
            assert b.load_text(text), b.errors()
            out[tag] = b
        monkeypatch.delenv("FX_STAGES", raising=False)
        return out
    return build


class Trio(dict):
    """{"S": ..., "D": ..., "U": ...} and the name of their program"""
    name = None


def ran(hs, what, scheduled=False):
    """FXB_INFO_WAVES_PER_WG and FXB_INFO_KERNEL behind the block that just ran: staged translated code on S and D (one wavefront
    per workgroup where the block armed a schedule: planStages refuses tracks), plain code on U; -> {tag: wavefronts}.
    D runs what the default policy chooses: staged code for the programs of SP.DEFAULT_POLICY_STAGES; for the others it stays
    in the comparison as the library's own choice (translated code, whatever its stage count)"""
    waves = {tag: b.info("waves_per_wg") for tag, b in hs.items()}
    kernels = {tag: b.info("kernel") for tag, b in hs.items()}
    for tag in hs:
        if tag == "U" or scheduled:
            assert waves[tag] == 1, (what, waves, kernels)
        elif tag == "D" and hs.name not in SP.DEFAULT_POLICY_STAGES:
            assert kernels[tag] >= 9, (what, waves, kernels)
        else:
            assert waves[tag] >= 2 and kernels[tag] >= 9, (what, waves, kernels)
    return waves


class Voices:
    """the reference: one oracle object per instance.  Mono programs keep them in the voice model of tools/fuzz_voices.py (its
    model_copy / model_reset / model_load / model_set_registers are what the by-list calls are held to)"""

    def __init__(self, name):
        self.channels, self.text, self.named, self.control = SP.PROGRAMS[name]
        import fx8010_amd as A
        fe = A.FrontEnd(self.channels)
        assert fe.load_text(self.text) and fe.lower() == 0
        self.names = [r[0] for r in fe.registers() if r[1] in STATE_TYPES and r[0] != "noise"]
        self.A = [fe.lower_info("itram_slots"), fe.lower_info("xtram_slots")]
        self.h = None
        if self.channels == 1:
            import fuzz_voices
            self.h = fuzz_voices.Handle(fuzz_voices.Program(self.text, 0), N, list(range(N)), False, 1)
            self.o = self.h.o
        else:
            self.o = {}
            for n in range(N):
                self.o[n] = Oracle(self.channels)
                assert self.o[n].load_text(self.text)

    def block(self, x, before=None):
        """x [S, channels, N] -> the oracles' outputs [S, channels, N]; before(t, n, oracle) runs in front of sample t (then the
        oracles are stepped sample by sample)"""
        S = x.shape[0]
        y = np.empty_like(x)
        for n in range(N):
            o = self.o[n]
            xn = np.ascontiguousarray(x[:, :, n])
            if before is None:
                y[:, :, n] = o.process_block(xn).reshape(S, self.channels)
            else:
                for t in range(S):
                    before(t, n, o)
                    y[t, :, n] = o.process_block(xn[t:t + 1]).reshape(self.channels)
            assert o.ood_flags() == 0, "instance %d left the parity domain: the test's own inputs are wrong" % n
        return y

    def set_all(self, key, v):
        for o in self.o.values():
            o.set_register(key, float(v))
        if self.h is not None:
            self.h.broadcast[key] = float(v)

    def set_array(self, key, values):
        for n in range(N):
            self.o[n].set_register(key, float(values[n]))

    def check(self, b, what):
        """every register, output latch, position, LFSR word and instruction counter of all instances (one image read), the
        delay memory of all instances, and FXB_OOD - against the oracles"""
        got = bits(b.get_registers_list(self.names, ALL))
        want = np.array([[self.o[n].get_register_word(r) for n in range(N)] for r in self.names], dtype=np.uint32)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, "registers", [(self.names[k], int(n), "%08x" % got[k, n], "%08x" % want[k, n]) for k, n in bad[:6]], len(bad))
        img = b.save_state()
        hdr = np.frombuffer(img[:64].tobytes(), dtype=np.int32)
        nregs, nrows = int(hdr[5]), int(hdr[6])
        rows = img[64:64 + nrows * N * 4].view(np.uint32).reshape(nrows, N)
        base = nregs + self.channels                      # fx_decode.cpp makeLayout: registers, output latches, 4 positions, 2 LFSR words, flags, counter
        cursors = np.array([self.o[n].cursors() for n in range(N)], dtype=np.int32).T
        assert np.array_equal(rows[base:base + 4].view(np.int32), cursors), (what, "positions", np.argwhere(rows[base:base + 4].view(np.int32) != cursors)[:4].tolist())
        lfsr = np.array([self.o[n].lfsr() for n in range(N)], dtype=np.int32).T
        assert np.array_equal(rows[base + 4:base + 6].view(np.int32), lfsr), (what, "LFSR words", np.argwhere(rows[base + 4:base + 6].view(np.int32) != lfsr)[:4].tolist())
        count = rows[base + 7].astype(np.uint64) | (rows[base + 8].astype(np.uint64) << np.uint64(32))
        want_count = np.array([self.o[n].instruction_counter() for n in range(N)], dtype=np.uint64)
        assert np.array_equal(count, want_count), (what, "instruction counters", np.argwhere(count != want_count)[:4].tolist())
        for n in WATCH:      # ... and through the calls a host would make
            assert b.instruction_counter_i(n) == self.o[n].instruction_counter(), (what, n)
            assert b.get_cursors_i(n) == self.o[n].cursors(), (what, n)
        assert b.instruction_counter() == int(want_count.sum()), what
        for w in (0, 1):
            if self.A[w] > 0:
                got = bits(b.get_tram_list(w, ALL, 0, self.A[w]))
                want = np.stack([bits(self.o[n].tram(w, self.A[w])) for n in range(N)])
                assert np.array_equal(got, want), (what, "delay line %d" % w, np.argwhere(got != want)[:4].tolist())
        assert b.ood_flags() == 0, what


def seed_noise(hs, v):
    for n in range(N):
        for b in hs.values():
            assert b.seed_noise_i(n, 1234 + n, -77 * n) == 0
        v.o[n].seed_noise(1234 + n, -77 * n)


def spread(hs, v):
    """one value per instance on the control every stage reads (a folded control becomes a row that every stage loads), and for the
    noise program a seed per instance: no two members of a bus group are alike"""
    per = cutoffs(N)
    for b in hs.values():
        assert b.set_register_array(v.control, per) == 0
    v.set_array(v.control, per)
    if "noise" in v.text:
        seed_noise(hs, v)


# ---- the entries of a bus block ---------------------------------------------------------------------------------------------------

def run_bus(gpu, b, entry, x, K, shared_in, mix_out, taps=0, aux=0):
    """one bus block through the pageable host entry, the pinned one (in place; on ONE buffer where input and output have one
    shape) or the device entry -> (out, tap rows or None, aux rows or None) as numpy arrays"""
    S, ch = x.shape[0], b.channels
    width = b.bus_groups(K) if mix_out else N
    if entry == "pageable":
        res = b.process_block_bus(x, K, shared_in, mix_out, taps=bool(taps), aux=bool(aux))
        res = res if isinstance(res, tuple) else (res,)
        return res[0], (res[1] if taps else None), (res[-1] if aux else None)
    if entry == "pinned":
        held = [gpu.HostBuffer(x.shape)]
        held[0].array[...] = x
        if x.shape[2] == width:
            out = held[0].array
        else:
            held.append(gpu.HostBuffer((S, ch, width)))
            out = held[-1].array
        side = {}
        for key, count in (("tap_out", taps), ("aux_out", aux)):
            if count:
                held.append(gpu.HostBuffer((S, ch, count)))
                side[key] = held[-1].array
        before = b.info("host_inplace_blocks")
        b.process_block_bus(held[0].array, K, shared_in, mix_out, out=out, **side)
        assert b.info("host_inplace_blocks") > before, "pinned buffers are processed in place"
        res = (out.copy(), side["tap_out"].copy() if taps else None, side["aux_out"].copy() if aux else None)
        for h in held:
            h.close()
        return res
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    d_out = torch.full((S, ch, width), -7.0, dtype=torch.float32, device="cuda")
    d_tap = torch.full((S, ch, taps), -7.0, dtype=torch.float32, device="cuda") if taps else None
    d_aux = torch.full((S, ch, aux), -7.0, dtype=torch.float32, device="cuda") if aux else None
    torch.cuda.synchronize()
    assert b.process_block_bus_dev(d_in, d_out, S, K, shared_in, mix_out, d_tap_out=d_tap, d_aux_out=d_aux) == 0
    assert b.sync() == 0
    return d_out.cpu().numpy(), (d_tap.cpu().numpy() if taps else None), (d_aux.cpu().numpy() if aux else None)


def run_feed(gpu, b, entry, src, K, mix_out):
    S, ch = src.shape[0], b.channels
    width = b.bus_groups(K) if mix_out else N
    if entry == "pageable":
        return b.process_block_bus_feed(src, K, mix_out)
    if entry == "pinned":
        held = [gpu.HostBuffer(src.shape), gpu.HostBuffer((S, ch, width))]
        held[0].array[...] = src
        out = b.process_block_bus_feed(held[0].array, K, mix_out, out=held[1].array).copy()
        for h in held:
            h.close()
        return out
    import torch
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to("cuda")
    d_out = torch.full((S, ch, width), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert b.process_block_bus_feed_dev(d_src, d_out, S, K, mix_out) == 0
    assert b.sync() == 0
    return d_out.cpu().numpy()


def bus_case(gpu, make, name, entry, devices=None, full=True):
    """groups of 8: the unmixed route against the oracles; a plain mix, taps on {0, 63, 64, 199} and two sends, a feed block, gains
    static and ramping (config2: with a voice that has gone NaN and is muted) against the models and against U.  -> the handles"""
    hs = make(name, devices=devices)
    v = Voices(name)
    ch, K, S = v.channels, 8, 33
    spread(hs, v)
    G = hs["S"].bus_groups(K)
    assert G == 25
    rng = np.random.default_rng(5)
    clock = [0]

    def shared(S):
        xg = group_input(G, S, ch, clock[0])
        clock[0] += S
        return xg, expand(xg, K, N)

    def every(what, call, scheduled=False):
        got = {tag: call(b) for tag, b in hs.items()}
        ran(hs, "%s %s: %s" % (name, entry, what), scheduled)
        return got

    # the unmixed route: shared input, per-instance output
    xg, x = shared(S)
    y = v.block(x)
    for tag, got in every("unmixed", lambda b: run_bus(gpu, b, entry, xg, K, True, False)[0]).items():
        assert same_bits(got, y), (tag, "unmixed", first_bad(got, y))
    # ... once more, now that every stage has state to load
    xg, x = shared(S)
    y = v.block(x)
    for tag, got in every("unmixed again", lambda b: run_bus(gpu, b, entry, xg, K, True, False)[0]).items():
        assert same_bits(got, y), (tag, "unmixed again", first_bad(got, y))
    # the plain mix
    xg, x = shared(S)
    y = v.block(x)
    got = every("mix", lambda b: run_bus(gpu, b, entry, xg, K, True, True)[0])
    for tag in hs:
        assert same_words(got[tag], mix_model(y, K)) and same_bits(got[tag], got["U"]), (tag, "mix")
    for tag, b in hs.items():
        v.check(b, "%s %s %s after the mix" % (name, entry, tag))
    if not full:
        return hs, v
    # taps and two sends beside the mix
    taps = np.array([0, 63, 64, 199], dtype=np.int64)
    # (every bus inside one shard of the three-shard run: three entries of [192, 200) with a repeat, 70 of [0, 128) - more than a
    # wavefront of entries, unsorted, both ends and repeats among them)
    off = np.array([0, 3, 73], dtype=np.int64)
    mem = np.concatenate([[199, 192, 199], [127, 0, 127], rng.integers(0, 128, 67)]).astype(np.int64)
    sg = gains_for(rng, ch, int(off[-1]))
    for b in hs.values():
        assert b.bus_set_taps(taps) == 0 and b.bus_set_sends(off, mem, sg) == 0
    xg, x = shared(S)
    y = v.block(x)
    got = every("taps and sends", lambda b: run_bus(gpu, b, entry, xg, K, True, True, taps=4, aux=2))
    for tag in hs:
        out, tap, aux = got[tag]
        assert same_words(out, mix_model(y, K)), (tag, "mix beside taps and sends")
        assert same_bits(tap, y[:, :, taps]), (tag, "taps", first_bad(tap, y[:, :, taps]))
        assert same_words(aux, send_model(y, off, mem, sg, sg, False, S)), (tag, "sends")
        assert all(same_bits(a, u) for a, u in zip(got[tag], got["U"])), (tag, "side rows against U")
    # a feed block: every instance's input summed on the device from 7 source rows, per-instance output
    foff, fsrc = feed_structure(rng, N, 7)
    for b in hs.values():
        assert b.bus_set_feeds(7, foff, fsrc) == 0
    src = group_input(7, S, ch, clock[0])
    clock[0] += S
    y = v.block(feed_model(src, foff, fsrc, None, None, False, S))
    for tag, got in every("feeds", lambda b: run_feed(gpu, b, entry, src, 1, False)).items():
        assert same_bits(got, y), (tag, "feeds", first_bad(got, y))
    # gains: a static set, then a ramp; per-instance input, mixed output.  config2: voice 9 hears a NaN, goes NaN for good and is muted
    g0, g1 = gains_for(rng, ch, N), gains_for(rng, ch, N)
    g0[:, 9] = g1[:, 9] = 0.0
    for block, (a, b_, ramp) in enumerate(((g0, g0, False), (g0, g1, True))):
        for b in hs.values():
            assert b.bus_set_gains(b_, ramp=ramp) == 0
        x = group_input(N, S, ch, clock[0])
        clock[0] += S
        if name == "config2" and block == 0:
            x[5, 0, 9] = np.nan
        y = v.block(x)
        want = gain_mix_model(y, a, b_, ramp, S, K)
        if name == "config2":
            assert np.isnan(y[-1, 0, 9]) and np.isfinite(want).all(), "the muted voice is NaN and its bus is finite"
        got = every("gains, ramp %d" % ramp, lambda b: run_bus(gpu, b, entry, x, K, False, True)[0])
        for tag in hs:
            assert same_words(got[tag], want) and same_bits(got[tag], got["U"]), (tag, "gains", ramp)
    for tag, b in hs.items():
        v.check(b, "%s %s %s at the end" % (name, entry, tag))
    return hs, v


@pytest.mark.parametrize("entry", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("name", ["config2", "mixed"])
def test_bus_blocks_on_staged_code(gpu, make, name, entry):
    """Measured on an MI355X, seconds per case: config2-pageable 0.34 (the first case of the file also loads the library and the first code: 1.5 s of setup), config2-pinned 0.08, config2-device 0.10, mixed-pageable 0.10, mixed-pinned 0.11, mixed-device 0.10."""
    bus_case(gpu, make, name, entry)


def test_bus_blocks_of_the_three_channel_program(gpu, make):
    """the 3-channel chain (cut 4 under FX_STAGES=4), once: unmixed and mixed, pageable entry.  Measured: 0.06 s."""
    bus_case(gpu, make, "chain3", "pageable", full=False)


# ---- meters -----------------------------------------------------------------------------------------------------------------------

def test_meters_on_staged_blocks(gpu, make):
    """output, target and level meters of staged blocks: every row against the numpy models fed with the oracles' outputs; then
    select / read_list / reset_list queued behind a staged device-entry block that nobody waited for.  Measured: 0.07 s."""
    import torch
    hs = make("config2")
    v = Voices("config2")
    spread(hs, v)
    rng = np.random.default_rng(12)
    tw = (rng.standard_normal((40, 1, -(-N // 3))) * 0.3).astype(np.float32)
    for b in hs.values():
        assert b.meter_enable() == 0 and b.meter_set_target(tw, 3, True) == 0 and b.meter_set_level(0.5, 0.25) == 0
    four, match, level, pos, clock = meter_zero(1, N), TG.match_zero(1, N), LV.level_zero(1, N), 0, 0

    def took(y):
        nonlocal four, match, level, pos
        four = meter_model(y, four)
        match, pos = TG.match_model(y, tw, 3, pos, True, match)
        level = LV.level_model(y, np.float32(0.5), np.float32(0.25), level)

    def compare(what):
        for tag, b in hs.items():
            assert same_meters(b.meter_read(), four), (tag, what, "output meters")
            assert TG.same_match(b.meter_read_match(), match) and b.meter_target_pos() == pos, (tag, what, "target meters")
            assert LV.same_level(b.meter_read_level(), level), (tag, what, "level meters")

    for S in (16, 17, 33):
        x = group_input(N, S, 1, clock)
        clock += S
        y = v.block(x)
        for tag, b in hs.items():
            assert same_bits(b.process_block(x), y), (tag, S)
        ran(hs, "metered block of %d" % S)
        took(y)
        compare("block of %d" % S)
    # queries behind a queued block: the device entry returns at once, reset_list is stream-ordered behind it, select and
    # read_list are synchronous and cover it
    L = np.array([199, 0, 64, 63, 130], dtype=np.int64)
    S = 48
    x = group_input(N, S, 1, clock)
    clock += S
    y = v.block(x)
    took(y)
    thr = float(np.median(ML.value(four, 0)))
    d_in = torch.from_numpy(x).to("cuda")
    torch.cuda.synchronize()
    for tag, b in hs.items():
        d_out = torch.full((S, 1, N), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert b.process_block_dev(d_in.data_ptr(), d_out.data_ptr(), S) == 0
        lst, m = b.meter_select(0, thr)
        want = ML.model(four, 0, thr, False)
        assert m == want.size and np.array_equal(lst, want), (tag, "select behind a queued staged block")
        assert ML.same_rows(b.meter_read_list(L), ML.columns(four, L)), (tag, "read_list")
        assert b.meter_reset_list(L) == 0
        assert b.sync() == 0
        assert same_bits(d_out.cpu().numpy(), y), tag
    ran(hs, "the queued block")
    four, match, level = ML.zeroed(four, L), TG.zeroed(match, L), LV.zeroed(level, L)
    compare("after reset_list")
    x = group_input(N, 33, 1, clock)
    y = v.block(x)
    for tag, b in hs.items():
        assert same_bits(b.process_block(x), y), tag
    ran(hs, "the block behind the list reset")
    took(y)
    compare("a block on the reset columns")
    for tag, b in hs.items():
        v.check(b, "meters " + tag)


# ---- instance-major blocks -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["config2", "chain3"])
def test_instance_major_blocks_on_staged_code(gpu, make, name):
    """per-instance streams, transposed on the GPU into a scratch block on which the program runs IN PLACE (stage 0 reads input a
    burst ahead of the stage that stores output into the same rows): strided views of a longer pageable and of a pinned array, then
    the device entry on views of a longer tensor and on ONE packed tensor both ways.  Measured: config2 0.04 s, chain3 0.07 s."""
    import torch
    hs = make(name)
    v = Voices(name)
    ch = v.channels
    spread(hs, v)
    frames, S = 90, 33
    wide = np.stack([progs.stimulus(N, frames, seed=7 + 1000 * c) for c in range(ch)], axis=1)      # [frames, channels, N]
    whole = np.ascontiguousarray(wide.transpose(2, 0, 1))                                            # [N, frames, channels]
    pin_in, pin_out = gpu.HostBuffer(whole.shape), gpu.HostBuffer(whole.shape)
    pin_in.array[...] = whole
    d_whole = torch.from_numpy(whole).to("cuda")
    torch.cuda.synchronize()
    for block, (f0, S, how) in enumerate(((3, 33, "pageable"), (36, 31, "pinned"), (5, 33, "device"), (40, 40, "device, one tensor"))):
        y = v.block(np.ascontiguousarray(wide[f0:f0 + S]))
        want = np.ascontiguousarray(y.transpose(2, 0, 1))
        for tag, b in hs.items():
            if how == "pageable":
                out = np.zeros_like(whole)
                b.process_block_imajor(whole[:, f0:f0 + S, :], out=out[:, f0:f0 + S, :])
                assert not out[:, :f0].any() and not out[:, f0 + S:].any(), (tag, "words outside the runs were written")
                got = out[:, f0:f0 + S, :]
            elif how == "pinned":
                pin_out.array[...] = 0
                before = b.info("host_inplace_blocks")
                b.process_block_imajor(pin_in.array[:, f0:f0 + S, :], out=pin_out.array[:, f0:f0 + S, :])
                assert b.info("host_inplace_blocks") > before
                assert not pin_out.array[:, :f0].any() and not pin_out.array[:, f0 + S:].any(), (tag, "words outside the runs were written")
                got = pin_out.array[:, f0:f0 + S, :].copy()
            elif how == "device":
                d_out = torch.full((N, frames, ch), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                assert b.process_block_imajor_dev(d_whole[:, f0:f0 + S, :], d_out[:, f0:f0 + S, :], S) == 0 and b.sync() == 0
                got = d_out.cpu().numpy()
                assert (got[:, :f0] == -7.0).all() and (got[:, f0 + S:] == -7.0).all(), (tag, "frames outside the block were written")
                got = got[:, f0:f0 + S, :]
            else:
                d = torch.from_numpy(np.ascontiguousarray(whole[:, f0:f0 + S, :])).to("cuda")
                torch.cuda.synchronize()
                assert b.process_block_imajor_dev(d.data_ptr(), d.data_ptr(), S) == 0 and b.sync() == 0
                got = d.cpu().numpy()
            assert same_bits(got, want), (tag, how, first_bad(got, want))
        ran(hs, "%s instance-major block %d (%s)" % (name, block, how))
    for tag, b in hs.items():
        assert b.info("imajor_blocks") == 4
        v.check(b, "instance-major " + tag)
    pin_in.close()
    pin_out.close()


# ---- block lengths and by-list calls ---------------------------------------------------------------------------------------------

def test_block_lengths_change_with_by_list_calls_between(gpu, make):
    """blocks of 8, 300, 8, 60 and 1 samples - the three classes of block length staged code is generated for - with a register
    list set, a copy and a reset between them: rows written between two blocks are loaded by whichever stages the next block's
    code has.  The code of each class is generated ahead (fxb_prepare), so every block runs its own class's; at least two
    different stage counts must have run on D.  Measured: 0.13 s; wavefronts per workgroup block by block S 4, 4, 4, 4, 4; D 4, 8, 4, 8, 4; U 1, 1, 1, 1, 1."""
    hs = make("config2")
    v = Voices("config2")
    h = v.h
    rng = np.random.default_rng(21)
    for b in hs.values():
        for S in (8, 300, 60):
            assert b.prepare(S, True) == 0
    keys = ["s0", "s7", "s15", "s22", "s30", "t"]
    clock, seen = 0, {tag: [] for tag in hs}

    def block(S):
        nonlocal clock
        x = group_input(N, S, 1, clock)
        clock += S
        y = v.block(x)
        for tag, b in hs.items():
            got = b.process_block(x)
            assert same_bits(got, y), (tag, S, first_bad(got, y))
        waves = ran(hs, "block of %d" % S)
        for tag in hs:
            seen[tag].append(waves[tag])
            v.check(hs[tag], "%s after the block of %d" % (tag, S))

    block(8)
    L = np.array([199, 0, 63, 64, 65, 128, 191, 192, 5], dtype=np.int64)
    vals = rng.uniform(-0.9, 0.9, (len(keys), L.size)).astype(np.float32)
    for b in hs.values():
        assert b.set_registers_list(keys, L, vals) == 0
    h.model_set_registers(keys, [int(n) for n in L], vals)
    block(300)
    src, dst = [0, 199, 64, 64], [63, 1, 192, 130]
    for b in hs.values():
        assert b.copy_instances(src, dst) == 0
    h.model_copy(src, dst)
    block(8)
    R = [199, 64, 7, 128]
    for b in hs.values():
        assert b.reset_instances(R) == 0
    h.model_reset(R)
    block(60)
    L2 = np.array([192, 193, 63], dtype=np.int64)
    vals2 = rng.uniform(-0.9, 0.9, (len(keys), L2.size)).astype(np.float32)
    for b in hs.values():
        assert b.set_registers_list(keys, L2, vals2) == 0
    h.model_set_registers(keys, [int(n) for n in L2], vals2)
    block(1)
    print("wavefronts per workgroup, block by block:", seen)
    assert len(set(seen["D"])) >= 2, seen


# ---- schedules: the fall back to plain code and the way back ------------------------------------------------------------------

def test_scheduled_blocks_fall_back_and_staged_code_takes_the_state_back(gpu, make):
    """staged block, a block with a broadcast track, one with a per-instance track, one with a list schedule: planStages refuses
    tracks, so the scheduled blocks run one wavefront per workgroup on another code object, which takes over what the stages
    stored.  The oracles are stepped sample by sample; registers, positions, delay memory, LFSR words and counters are compared
    after every block.  A register that has had a schedule stays trackable for the life of its handle (DESIGN.md sections 4.5 and
    4.6: arming never re-translates), so on THESE handles staged code does not come back - two more blocks on them run the code
    with the trackable register, compared like the others.  Staged code takes the state back the way a host gets it back: the
    state image goes into three fresh handles, which run two blocks staged.  Measured: 0.31 s; behind the schedules S, D and U ran one wavefront per workgroup."""
    hs = make("mixed")
    v = Voices("mixed")
    seed_noise(hs, v)
    S, clock = 33, 0
    steps = np.linspace(0.05, 0.9, 5).astype(np.float32)
    per = (steps[:, None] * (0.5 + 0.5 * cutoffs(N))[None, :]).astype(np.float32)          # [steps, N]
    L = np.array([199, 0, 64, 63, 192, 100], dtype=np.int64)
    lv = np.random.default_rng(3).uniform(0.05, 0.9, (4, L.size)).astype(np.float32)      # [steps, len(L)]
    where = {int(n): i for i, n in enumerate(L)}

    def broadcast(t, n, o):
        if t % 8 == 0 and t // 8 < steps.size:
            o.set_register("k", float(steps[t // 8]))

    def per_instance(t, n, o):
        if t % 8 == 0 and t // 8 < per.shape[0]:
            o.set_register("k", float(per[t // 8, n]))

    def listed(t, n, o):
        if n in where and t >= 2 and (t - 2) % 3 == 0 and (t - 2) // 3 < lv.shape[0]:
            o.set_register("k", float(lv[(t - 2) // 3, where[n]]))

    def block(hs, what, arm=None, before=None, count=True):
        nonlocal clock
        x = group_input(N, S, 1, clock)
        clock += S
        y = v.block(x, before)
        for tag, b in hs.items():
            if arm:
                assert arm(b) == 0, (tag, what, b.last_error())
            got = b.process_block(x)
            assert same_bits(got, y), (tag, what, first_bad(got, y))
        waves = ran(hs, what, scheduled=arm is not None) if count else {tag: b.info("waves_per_wg") for tag, b in hs.items()}
        for tag, b in hs.items():
            v.check(b, "%s after %s" % (tag, what))
        return waves

    block(hs, "a staged block")
    block(hs, "a second staged block")
    block(hs, "a broadcast track", lambda b: b.set_register_track("k", steps, 8), broadcast)
    block(hs, "a per-instance track", lambda b: b.set_register_track("k", per, 8), per_instance)
    block(hs, "a list schedule", lambda b: b.set_register_tracks_list("k", L, lv, first=2, period=3), listed)
    after = [block(hs, "a block behind the schedules", count=False), block(hs, "a second block behind the schedules", count=False)]
    print("wavefronts per workgroup behind the schedules:", after)
    assert all(w["U"] == 1 for w in after)
    image = hs["S"].save_state()
    for tag, b in hs.items():
        assert np.array_equal(b.save_state(), image), (tag, "one state image whatever code ran")
    fresh = make("mixed")
    for tag, b in fresh.items():
        assert b.load_state(image) == 0, (tag, b.last_error())
    block(fresh, "a staged block on the loaded image")
    block(fresh, "a second staged block on the loaded image")


# ---- the by-list state calls ------------------------------------------------------------------------------------------------------

def state_calls_case(gpu, make, devices=None, extra=()):
    """register list set / get over names stored by different stages and `k` (folded at first: the list set turns it into a row that
    every stage reads), copy, reset, save / load, a rotated load at another position - between staged blocks of the delay-line and
    noise program, everything against the oracles, the instruction counter of every instance included"""
    hs = make("mixed", devices=devices)
    for tag in extra:      # (a single-shard twin of S for the sharded run: staged like S)
        hs[tag] = make("mixed", only=("S",))["S"]
    v = Voices("mixed")
    h = v.h
    seed_noise(hs, v)
    rng = np.random.default_rng(31)
    clock = 0

    def block(S, what):
        nonlocal clock
        x = group_input(N, S, 1, clock)
        clock += S
        y = v.block(x)
        for tag, b in hs.items():
            got = b.process_block(x)
            assert same_bits(got, y), (tag, what, first_bad(got, y))
        ran(hs, what)
        for tag, b in hs.items():
            v.check(b, "%s after %s" % (tag, what))

    block(33, "the first block")
    # register list set and get: names of stage 0, of the middle and of the last stage, and k
    keys = ["a", "s0", "s3", "s14", "s29", "u", "k"]
    L = np.array([199, 0, 63, 64, 127, 128, 191, 192, 77], dtype=np.int64)
    vals = rng.uniform(-0.9, 0.9, (len(keys), L.size)).astype(np.float32)
    vals[-1] = rng.uniform(0.05, 0.9, L.size).astype(np.float32)
    for tag, b in hs.items():
        assert b.info("control_rows") == 0, (tag, "k starts folded into the code")
        assert b.set_registers_list(keys, L, vals) == 0
        assert same_bits(b.get_registers_list(keys, L), vals), tag
    h.model_set_registers(keys, [int(n) for n in L], vals)
    block(33, "a register list set")
    for tag, b in hs.items():
        got = bits(b.get_registers_list(keys, ALL))
        want = np.array([[v.o[n].get_register_word(r) for n in range(N)] for r in keys], dtype=np.uint32)
        assert np.array_equal(got, want), (tag, "get_registers_list")
    # copy (sources and destinations in different workgroups and shards), then reset
    src, dst = [0, 199, 64, 64, 130], [63, 1, 192, 129, 198]
    for b in hs.values():
        assert b.copy_instances(src, dst) == 0
    h.model_copy(src, dst)
    block(20, "a copy")
    R = [199, 64, 7, 128, 192]
    for b in hs.values():
        assert b.reset_instances(R) == 0
    h.model_reset(R)
    block(33, "a reset")
    # save, disturb the saved voices by list, load back: the records' positions are their destinations'
    saved = [5, 63, 64, 191, 199]
    images = {tag: b.save_instances(saved) for tag, b in hs.items()}
    records = [v.o[n].clone() for n in saved]
    upset = rng.uniform(-0.9, 0.9, (3, len(saved))).astype(np.float32)
    for tag, b in hs.items():
        assert b.set_registers_list(["a", "s14", "s29"], saved, upset) == 0
        assert b.load_instances(saved, images[tag]) == 0, b.last_error()
    new, why, _ = h.model_load(records, saved, False)
    assert why is None and len(new) == len(saved)
    for d, (c, moved) in new.items():
        v.o[d] = c
    block(20, "a save and a load")          # 20 samples: the ring of 11 words stands 9 further
    # ... the same records once more, now behind 20 samples: a plain load is refused, a rotated one turns the ring by 9
    into = [6, 62, 65, 190, 198]
    new, why, _ = h.model_load(records, into, False)
    assert why is not None
    for tag, b in hs.items():
        with pytest.raises(RuntimeError):
            b.load_instances(into, images[tag])
        assert b.load_instances_rotated(into, images[tag]) == 0, b.last_error()
    new, why, _ = h.model_load(records, into, True)
    assert why is None and all(moved for c, moved in new.values()), "the shift is not zero"
    for d, (c, moved) in new.items():
        v.o[d] = c
    block(33, "a rotated load")
    block(1, "a block of one sample")
    return hs, v


def test_by_list_state_calls_between_staged_blocks(gpu, make):
    """Measured: 0.18 s."""
    state_calls_case(gpu, make)


# ---- a moving control ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", [True, False], ids=["builder_thread", "callers_thread_only"])
@pytest.mark.parametrize("name, key, values", [("config2", "cutoff", (0.2, 0.35, 0.5, 0.15, 0.6, 0.25)), ("mixed_e", "e", (5.0, 4.0, 6.0))], ids=["config2-cutoff", "mixed_e-e"])
def test_a_moving_control(gpu, make, name, key, values, builder):
    """Broadcast writes to a control between blocks, then ten blocks of rest, then one set_register_i on the control every stage
    reads.  config2's cutoff is read by the INTERP of every stage: the first write takes the code from the folded value to the
    control-row variant, staged like the first (with the builder thread the tuner then tries other stage counts: 4, 2, 8 were
    seen).  mixed_e's `e` is the table number of its LOGs, which no row can hold: the library interprets while it moves (the
    translation is deferred: FXB_INFO_KERNEL 1 .. 8) and returns to staged code when it has rested - the way back from plain to
    staged code.  Every word against the oracles after every block; which code ran is recorded block by block.
    Measured: 0.30 to 0.39 s per case; config2 with the builder thread: S 4 stages throughout, D 4, 4, 4, 2, 2, 2, then 8; mixed_e: kernel 1 .. 8 on the blocks behind the writes, 2 stages again afterwards."""
    hs = make(name, builder=builder)
    v = Voices(name)
    if "noise" in v.text:
        seed_noise(hs, v)
    S, clock = 33, 0
    seen = {tag: [] for tag in hs}

    def block(what):
        nonlocal clock
        x = group_input(N, S, 1, clock)
        clock += S
        y = v.block(x)
        for tag, b in hs.items():
            got = b.process_block(x)
            assert same_bits(got, y), (tag, what, first_bad(got, y))
            seen[tag].append((b.info("kernel"), b.info("waves_per_wg"), b.info("control_rows")))
            v.check(b, "%s after %s" % (tag, what))

    block("the first block")
    block("the second block")
    for k, value in enumerate(values):
        for b in hs.values():
            assert b.set_register(key, value) == 0
        v.set_all(key, value)
        block("broadcast write %d" % k)
    for k in range(10):      # the control rests: a deferred translation comes due, the code settles
        block("rest %d" % k)
    for b in hs.values():
        assert b.set_register_i(v.control, 77, 0.4) == 0
    v.o[77].set_register(v.control, 0.4)
    block("a per-instance write")
    block("the last block")
    print("(kernel, wavefronts per workgroup, control rows), block by block:", seen)
    for tag in ("S", "D") if name in SP.DEFAULT_POLICY_STAGES else ("S",):
        assert seen[tag][0][1] >= 2 and seen[tag][1][1] >= 2, (tag, "staged before the control moves", seen[tag])
        if key == "e":
            assert any(1 <= k <= 8 for k, _, _ in seen[tag][2:2 + len(values)]), (tag, "the interpreter ran while the control moved", seen[tag])
        else:
            assert all(rows > 0 for _, _, rows in seen[tag][2:]), (tag, "the control-row variant ran", seen[tag])
        assert all(w >= 2 for k, w, _ in seen[tag] if k >= 9), (tag, "translated code is staged code on every block", seen[tag])
        assert all(k >= 9 and w >= 2 for k, w, _ in seen[tag][-4:]), (tag, "staged code returns", seen[tag])
    assert all(w == 1 for _, w, _ in seen["U"]), seen["U"]


def test_the_default_policy_in_long_blocks(gpu, make):
    """the delay-line and noise program under the DEFAULT policy: blocks of a few dozen samples run plain (the planner's costs),
    blocks of 300 start in two stages, and the stage tuner then times its other options on the caller's launches - three stages
    and the plain program (2, 2, 2, 2, 2, 2, 3, 3 and 2, 2, 2, 2, 2, 2, 1, ... were seen; which is kept is a matter of time, not
    of words).  Twelve blocks of 300 with register list sets and a copy between them: every block is the oracles' whatever code
    ran it, the first ones run staged, and more than one code object ran.  Measured: 0.26 s with eight blocks; under 1.1 s with twelve (the whole
    suite's slowest-60 list starts there)."""
    hs = make("mixed", only=("D", "U"))
    v = Voices("mixed")
    seed_noise(hs, v)
    rng = np.random.default_rng(41)
    keys = ["a", "s0", "s14", "s29", "k"]
    L = np.array([199, 0, 63, 64, 128, 192], dtype=np.int64)
    S, seen = 300, []
    for k in range(12):
        x = group_input(N, S, 1, k * S)
        y = v.block(x)
        for tag, b in hs.items():
            got = b.process_block(x)
            assert same_bits(got, y), (tag, k, first_bad(got, y))
        waves = {tag: b.info("waves_per_wg") for tag, b in hs.items()}
        seen.append(waves["D"])
        assert hs["D"].info("kernel") >= 9 and waves["U"] == 1 and (waves["D"] >= 2 or k >= 3), (k, waves)
        for tag, b in hs.items():
            v.check(b, "%s after block %d" % (tag, k))
        if k in (1, 5, 8):
            vals = rng.uniform(0.05, 0.9, (len(keys), L.size)).astype(np.float32)
            for b in hs.values():
                assert b.set_registers_list(keys, L, vals) == 0
            v.h.model_set_registers(keys, [int(n) for n in L], vals)
        if k == 3:
            for b in hs.values():
                assert b.copy_instances([0, 199], [100, 1]) == 0
            v.h.model_copy([0, 199], [100, 1])
    print("wavefronts per workgroup on D, block by block:", seen)
    assert sum(w >= 2 for w in seen) >= 3, seen


# ---- three shards on one GPU ---------------------------------------------------------------------------------------------------------

def test_three_shards_bus_blocks(gpu, make):
    """[0, 128), [128, 192), [192, 200) on one GPU: the bus case once (pageable entry; groups of 8 divide every shard), and the
    whole state image equal to a single handle's.  Measured: 0.17 s."""
    assert gpu.shard_plan(N, 3) == SHARDS
    hs, v = bus_case(gpu, make, "config2", "pageable", devices=[0, 0, 0])
    assert hs["S"].shards() == [(0, first, count) for first, count in SHARDS]
    one, _ = bus_case(gpu, make, "config2", "pageable")
    for tag in hs:
        assert np.array_equal(hs[tag].save_state(), one[tag].save_state()), tag


def test_three_shards_by_list_state_calls(gpu, make):
    """the by-list calls once on three shards (copies across shard borders, a list that names all three), beside a single-shard
    twin that makes the same calls: save_state equal at the end.  Measured: 0.32 s."""
    hs, v = state_calls_case(gpu, make, devices=[0, 0, 0], extra=("one",))
    assert hs["S"].shards() == [(0, first, count) for first, count in SHARDS]
    assert np.array_equal(hs["S"].save_state(), hs["one"].save_state())
