"""Level meters on the GPU (fxb_meter_set_level ... fxb_meter_select_level): the two level rows against
meter_level_model.level_model - the definition of include/fx8010_amd.h "Level meters" in numpy float32 / uint32, one operation per
line - of the per-instance output block y.  y is what a twin handle with meters off returns for the same block.  Every figure is
compared word for word, fp32 as uint32; the four existing accumulators must equal meter_model(y) and, with a target set, the two
match rows match_model - they are taken by the same code as with the mode off.

Shapes: S = 33 is four rounds of eight loads plus one sample; 16 + 17, 1 and 8 cut the stream elsewhere; N = 1, 63, 64, 65, 130, 257
put the end of the batch at every lane phase and in a second workgroup.  Parameter pairs: (0.5, 0.25) a plain fall, (1.0, 0.0) the
running peak with the counter off, (0.0, 1.0) the last magnitude with everything below the rail quiet, (0.999, 1e-4) a slow fall.
The `quiet` counter's saturation at 0xFFFFFFFF is not reached here - it would take 2^32 samples; the model test of
tests/test_meter_level_stub.py covers it."""
import numpy as np
import pytest

import fx8010_programs as progs
import meter_level_model as L
import meter_target_model as T
from test_bus_stub import expand, mix_model
from test_gpu_meter import NONFINITE, PASS_THROUGH, bits, cutoffs, on_tier, pcm, same_bits, same_words, stereo, tier  # noqa: F401
from test_meter_stub import meter_model, meter_zero, same_meters

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
PARAMS = ((0.5, 0.25), (1.0, 0.0), (0.0, 1.0), (0.999, 1e-4))
# MACS adds +0 to its A operand, which turns -0.0 into +0.0 (PASS_THROUGH); here the product in * 0 carries the sign of `in`, so a
# -0.0 on the input is a -0.0 on the output, and every other word passes as it does through PASS_THROUGH
SIGNED_THROUGH = "input in 0\noutput out 0\nmacs out, in, in, 0\nend"


def handles(gpu, text, N, channels, control="cutoff", values=None, devices=None):
    """(the handle with meters on, its twin with meters off)"""
    out = []
    for first in (True, False):
        b = gpu.Batch(N, channels, 0) if devices is None or not first else gpu.Batch(N, channels, devices=devices)
        assert b.load_text(text), b.errors()
        if control:
            assert b.set_register_array(control, cutoffs(N) if values is None else values) == 0
        if first:
            assert b.meter_enable() == 0
        out.append(b)
    return out


class Follow:
    """the model of everything the handle m has been through since its meters were zero"""

    def __init__(self, m, N, channels, release, floor, shards=1):
        self.m, self.N, self.ch, self.shards = m, N, channels, shards
        self.four = meter_zero(channels, N)
        self.acc = L.level_zero(channels, N)
        self.launches = m.info("meter_level_launches")
        self.plain = m.info("meter_launches")
        self.set(release, floor)

    def set(self, release, floor):
        assert self.m.meter_set_level(release, floor) == 0
        self.release, self.floor = np.float32(release), np.float32(floor)

    def took(self, what, y, launches=1):
        self.acc = L.level_model(y, self.release, self.floor, self.acc)
        self.four = meter_model(y, self.four)
        self.launches += launches * self.shards
        self.plain += launches * self.shards
        got = self.m.meter_read_level()
        tag = (what, self.N, float(self.release), float(self.floor))
        assert L.same_level(got, self.acc), tag + (np.argwhere(bits(got["level"]) != bits(self.acc["level"]))[:4].tolist(), np.argwhere(got["quiet"] != self.acc["quiet"])[:4].tolist())
        assert same_meters(self.m.meter_read(), self.four), tag + ("the four",)
        assert self.m.info("meter_level_launches") == self.launches and self.m.info("meter_launches") == self.plain, tag


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 257])
def test_sizes_cuts_and_parameter_pairs(gpu, N, channels):
    text = progs.config3() if channels == 1 else stereo(progs.config3())
    m, t = handles(gpu, text, N, channels)
    clock = 0
    for release, floor in PARAMS:
        m.meter_read(reset=True)
        f = Follow(m, N, channels, release, floor)
        for S in (33, 16, 17, 1, 8):
            x = pcm(N, S, channels, clock)
            clock += S
            y = t.process_block(x)
            assert same_bits(m.process_block(x), y)
            f.took("block of %d" % S, y)
        if floor == 1.0:
            assert f.acc["quiet"].any(), "some voice is below the rail"
    assert m.info("meter_target_launches") == 0
    m.close()
    t.close()


def test_release_one_is_the_peak_and_release_zero_the_last_magnitude(gpu):
    N, S = 130, 33
    m, t = handles(gpu, NONFINITE, N, 1, control="vol")
    x = pcm(N, S, 1, 0)
    for (s, n), v in {(5, 0): 3.0, (9, 63): np.nan, (S - 1, 64): -np.inf, (S - 1, 65): np.nan, (S - 1, N - 1): 3.0, (0, 129): -np.inf}.items():
        x[s, 0, n] = v
    y = t.process_block(x)
    assert not np.isfinite(y[S - 1, 0, [64, 65, N - 1]]).any() and np.isfinite(y[S - 1, 0, :64]).all()
    assert m.meter_set_level(1.0, 0.0) == 0
    assert same_words(m.process_block(x), y)
    got = m.meter_read_level()
    assert np.array_equal(bits(got["level"]), bits(m.meter_read()["peak"])) and not got["quiet"].any(), "release = 1: the running peak, bit for bit"
    assert m.meter_set_level(0.0, 1.0) == 0
    assert same_words(m.process_block(x), y)
    last = np.where(np.isfinite(y[S - 1]), np.abs(y[S - 1]), np.float32(0.0))
    got = m.meter_read_level()
    assert np.array_equal(bits(got["level"]), bits(last)) and (bits(got["level"])[0, [64, 65, N - 1]] == 0).all(), "release = 0: the last magnitude, +0 where it is not finite"
    assert m.info("meter_level_launches") == 2 == m.info("meter_launches")


def edge_input(N, S, floor, program):
    """column n is loud for its first n mod 11 samples and silent afterwards, but for one word at sample 20 + n mod 7 taken by turns
    from the eight kinds.  For PASS_THROUGH and SIGNED_THROUGH the words are 0.5, 0 and the kind itself; NONFINITE (with vol = 0.001)
    puts about 1.0 out for an input of 0, -0.001 for -1, NaN for NaN, +Inf for 3 and -Inf for -Inf"""
    f = np.float32(floor)
    kinds = [f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1)), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), np.float32(1e-42)]
    through = program != NONFINITE
    x = np.full((S, 1, N), 0.0 if through else -1.0, dtype=np.float32)
    for n in range(N):
        x[:n % 11, 0, n] = 0.5 if through else 0.0
        kind = kinds[n % 8]
        if not through:
            kind = {3: np.float32(np.nan), 4: np.float32(3.0), 5: np.float32(-np.inf)}.get(n % 8, np.float32(-1.0))
        x[20 + n % 7, 0, n] = kind
    return x, kinds


def test_the_edges_of_the_definition(gpu):
    """the floor itself and its two neighbours, NaN, +-Inf, -0.0 and a denormal, each on the output of some column, breaking a
    quiet run at every phase of a round of eight loads"""
    N, S, release, floor = 130, 40, 0.5, 0.25
    ys = {}
    pairs = {}
    for name, text in (("through", PASS_THROUGH), ("nonfinite", NONFINITE), ("signed", SIGNED_THROUGH)):
        m, t = handles(gpu, text, N, 1, control="vol" if text == NONFINITE else None, values=np.full(N, 0.001, dtype=np.float32))
        x, kinds = edge_input(N, S, floor, text)
        ys[name] = (x, t.process_block(x))
        pairs[name] = m
    # the test is not vacuous: asserted on y itself, before any device figure is compared
    everything = np.concatenate([bits(y).reshape(-1) for _, y in ys.values()])
    for kind in kinds:
        assert (everything == bits(kind)).any() or (np.isnan(kind) and np.isnan(np.concatenate([y.reshape(-1) for _, y in ys.values()])).any()), ("a kind of word is missing on every output", kind)
    assert (bits(ys["through"][1]) == bits(kinds[0])).any() and (bits(ys["signed"][1]) == 0x80000000).any() and np.isinf(ys["nonfinite"][1]).any() and np.isnan(ys["nonfinite"][1]).any()
    for name, (x, y) in ys.items():
        want = L.level_model(y, release, floor)
        assert (want["quiet"] >= 9).any(), (name, "some column ends with a quiet run longer than a round of loads")
        inside = [n for n in range(N) if (20 + n % 7) % 8 not in (0, 7) and want["quiet"][0, n] == S - 1 - (20 + n % 7)]
        assert inside, (name, "some column's run is reset inside a round")
        m = pairs[name]
        f = Follow(m, N, 1, release, floor)
        assert same_words(m.process_block(x), y)
        f.took("edges, " + name, y)


def test_the_fall_through_the_denormals(gpu):
    N = 130
    m, t = handles(gpu, PASS_THROUGH, N, 1, control=None)
    assert m.meter_set_level(0.5, 0.0) == 0
    x = np.zeros((151, 1, N), dtype=np.float32)
    x[0] = 1.0
    assert same_bits(m.process_block(x[:150]), x[:150])
    assert (bits(m.meter_read_level()["level"]) == 0x00000001).all(), "150 samples after an impulse of 1.0: the smallest denormal"
    assert same_bits(m.process_block(x[150:]), x[150:])
    assert (bits(m.meter_read_level()["level"]) == 0x00000000).all(), "one more: +0"


def test_a_plain_case_on_every_tier(gpu, tier):
    N, S = 197, 33
    m, t = handles(gpu, progs.config3(), N, 1)
    f = Follow(m, N, 1, 0.999, 1e-4)
    for k in range(2):
        x = pcm(N, S, 1, k * S)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y)
        f.took("block %d" % k, y)
    assert on_tier(m, tier) and m.meter_samples() == 2 * S


def test_an_armed_control_track_cuts_the_block_and_not_the_figures(gpu, tier):
    """a 33-sample block with a period-8 track at N = 197: the interpreter and HIP tiers cut it into five segments - five level
    launches; the translated tier reads the schedule by itself: one.  The figures are those of the uncut y."""
    N, S = 197, 33
    m, t = handles(gpu, progs.config3(), N, 1, control=None)
    steps = np.linspace(0.05, 0.9, 5).astype(np.float32)
    f = Follow(m, N, 1, 0.5, 0.25)
    for b in (m, t):
        assert b.set_register_track("cutoff", steps, 8) == 0
    x = pcm(N, S, 1, 0)
    y = t.process_block(x)
    assert same_bits(m.process_block(x), y)
    f.took("armed", y, launches=1 if tier == "default" else 5)
    assert on_tier(m, tier)


def test_target_and_level_together(gpu):
    N, S = 130, 33
    m, t = handles(gpu, progs.config3(), N, 1)
    rng = np.random.default_rng(12)
    tw = (rng.standard_normal((40, 1, -(-N // 3))) * 0.3).astype(np.float32)
    assert m.meter_set_target(tw, 3, True) == 0 and m.meter_set_level(0.5, 0.25) == 0
    four, match, level, pos = meter_zero(1, N), T.match_zero(1, N), L.level_zero(1, N), 0
    for k, S in enumerate((16, 17, 33)):
        x = pcm(N, S, 1, 100 * k)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y)
        four = meter_model(y, four)
        match, pos = T.match_model(y, tw, 3, pos, True, match)
        level = L.level_model(y, 0.5, 0.25, level)
        assert same_meters(m.meter_read(), four) and T.same_match(m.meter_read_match(), match) and L.same_level(m.meter_read_level(), level), k
        assert m.meter_target_pos() == pos
    assert m.info("meter_target_launches") == 3 == m.info("meter_level_launches") and m.info("meter_launches") == 0
    # a list reset zeroes all eight columns of the listed voices
    lst = np.array([0, 63, 64, 129], dtype=np.int64)
    assert m.meter_reset_list(lst) == 0
    for k in four:
        four[k][:, lst] = 0
    assert same_meters(m.meter_read(), four) and T.same_match(m.meter_read_match(), T.zeroed(match, lst)) and L.same_level(m.meter_read_level(), L.zeroed(level, lst))


def test_bus_instance_major_and_device_entry_blocks(gpu):
    import torch

    N, S, K, channels = 257, 33, 64, 2
    m, t = handles(gpu, stereo(progs.config3()), N, channels)
    f = Follow(m, N, channels, 0.999, 1e-4)
    # a bus block with MIX_OUT
    x = pcm(N, S, channels, 0)
    y = t.process_block(x)
    assert same_words(m.process_block_bus(x, K, False, True), mix_model(y, K))
    f.took("bus", y)
    # an instance-major block
    x = pcm(N, S, channels, S)
    y = t.process_block(x)
    got = m.process_block_imajor(np.ascontiguousarray(x.transpose(2, 0, 1)))
    assert same_bits(np.ascontiguousarray(got.transpose(1, 2, 0)), y)
    f.took("instance-major", y)
    # a device-entry block at a pitch above N
    P = N + 59
    x = pcm(N, S, channels, 2 * S)
    y = t.process_block(x)
    d_in = torch.zeros((S, channels, P), dtype=torch.float32, device="cuda")
    d_out = torch.full((S, channels, P), -7.0, dtype=torch.float32, device="cuda")
    d_in[:, :, :N] = torch.from_numpy(x).to("cuda")
    torch.cuda.synchronize()
    assert m.process_block_dev_pitched(d_in[:, :, :N], d_out[:, :, :N], S) == 0
    assert m.sync() == 0
    got = d_out.cpu().numpy()
    assert same_bits(got[:, :, :N], y) and (got[:, :, N:] == -7.0).all()
    f.took("device entry at pitch %d" % P, y)


def test_two_shards_on_one_gpu_equal_the_single_handle(gpu):
    N, S, channels = 130, 33, 2
    text = stereo(progs.config3())
    m, t = handles(gpu, text, N, channels, devices=[0, 0])
    one, _ = handles(gpu, text, N, channels)
    _.close()
    assert len(m.shards()) == 2 and 0 < m.shards()[1][1] < N and m.shards()[1][1] % 256 != 0, m.shards()   # (no multiple of a workgroup)
    f = Follow(m, N, channels, 0.5, 0.25, shards=2)
    assert one.meter_set_level(0.5, 0.25) == 0
    for k, S in enumerate((16, 17, 33)):
        x = pcm(N, S, channels, 100 * k)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y) and same_bits(one.process_block(x), y)
        f.took("block %d" % k, y)
        assert L.same_level(m.meter_read_level(), one.meter_read_level())
    rows = one.meter_read_level()
    for stat, thr in ((0, float(np.median(L.V(rows, 0)))), (1, 1.0)):
        for below in (False, True):
            assert np.array_equal(m.meter_select_level(stat, thr, below=below)[0], one.meter_select_level(stat, thr, below=below)[0])
    lst = [129, 0, m.shards()[1][1], m.shards()[1][1] - 1, 0]
    assert L.same_level(m.meter_read_level_list(lst), one.meter_read_level_list(lst))


def falling_voices(N, S, channels=1):
    """voice n sounds (0.5, and a level of its own on the last sounding sample) and falls silent after S - (5 n mod (S + 1)) samples:
    many distinct quiet runs and envelopes"""
    n = np.arange(N)
    stop = S - (5 * n) % (S + 1)   # sounding samples: 0 .. S
    sounding = np.arange(S)[:, None] < stop[None, :]
    x = np.array(np.broadcast_to(np.where(sounding, np.float32(0.5), np.float32(0.0))[:, None, :], (S, channels, N)), dtype=np.float32, order="C")
    own = (0.3 + 0.6 * ((n * 37) % 101) / 101.0).astype(np.float32)
    some = n[stop > 0]
    x[stop[some] - 1, :, some] = own[some, None]
    if channels > 1:
        x[:, 0, 7] = 0.5   # one channel goes on sounding: the voice is not quiet
    return x


def level_rows(gpu, N, channels):
    m, t = handles(gpu, PASS_THROUGH if channels == 1 else PASS_THROUGH.replace("output out 0", "output out 0\ninput in1 1\noutput out1 1").replace("\nend", "\nmacs out1, in1, 0, 0\nend"), N, channels, control=None)
    t.close()
    assert m.meter_set_level(0.5, 0.25) == 0
    x = falling_voices(N, 33, channels)
    m.process_block(x)
    rows = m.meter_read_level()
    assert L.same_level(rows, L.level_model(x, 0.5, 0.25)), "every word of x lies in 0..0.9 and passes as it is"
    return m, rows


def test_select_level_thresholds_caps_and_ranges(gpu):
    N = 257
    m, rows = level_rows(gpu, N, 2)
    assert rows["quiet"][0, 7] == 0 and rows["quiet"][1, 7] > 0 and L.V(rows, 1)[7] == 0, "the minimum over the channels"
    before = m.info("meter_level_selects")
    assert L.check_selects(m._lib, m, rows, N) >= 6
    assert m.info("meter_level_selects") > before + 50 and m.info("meter_selects") == 0 and m.info("meter_match_selects") == 0
    assert m._lib.fxb_meter_select_level(m._h, 2, L.C_DOUBLE(0.0), 0, N, None, 0, 0) == FX_E_ARG
    assert m._lib.fxb_meter_select(m._h, 4, L.C_DOUBLE(0.0), 0, N, None, 0, 0) == FX_E_ARG, "fxb_meter_select keeps refusing stat = 4"


def test_select_level_where_a_scan_lane_owns_two_counts(gpu):
    N = 66000
    m, rows = level_rows(gpu, N, 1)
    for stat, thr in ((0, float(np.median(L.V(rows, 0)))), (1, 8.0), (1, 0.5), (0, np.inf), (1, -np.inf)):
        for below in (False, True):
            want = L.select(rows, stat, thr, below)
            got, n = m.meter_select_level(stat, thr, below=below)
            assert n == want.size and np.array_equal(got, want), (stat, thr, below)
    thr = float(np.median(L.V(rows, 0)))
    M = L.select(rows, 0, thr, False).size
    assert 0 < M < N
    for cap in (0, 1, M - 1, M, M + 7):
        L.check_one(m._lib, m, rows, 0, thr, False, 0, N, cap)
    L.check_one(m._lib, m, rows, 1, 8.0, False, 77, N - 77, 40000)


def test_read_level_list_and_reset_list(gpu):
    N = 257
    m, rows = level_rows(gpu, N, 2)
    lst = np.array([256, 0, 64, 63, 0, 130, 256], dtype=np.int64)
    assert L.same_level(m.meter_read_level_list(lst), {k: v[:, lst] for k, v in rows.items()}), "repeats are fine without reset"
    assert m._lib.fxb_meter_read_level_list(m._h, lst.ctypes.data, lst.size, None, None, 1) == FX_E_ARG and L.same_level(m.meter_read_level(), rows), "a repeated instance under reset is refused"
    lst = np.array([256, 0, 64, 63, 130], dtype=np.int64)
    assert L.same_level(m.meter_read_level_list(lst, reset=True), {k: v[:, lst] for k, v in rows.items()})
    rows = L.zeroed(rows, lst)
    assert L.same_level(m.meter_read_level(), rows), "the listed columns and no others"
    four = m.meter_read()
    lst = np.array([1, 65, 255], dtype=np.int64)
    assert m.meter_reset_list(lst) == 0
    rows = L.zeroed(rows, lst)
    for k in four:
        four[k][:, lst] = 0
    assert L.same_level(m.meter_read_level(), rows) and same_meters(m.meter_read(), four), "reset_list zeroes the listed level columns and no others"
    assert m.info("meter_level_list_reads") == 2


def test_the_loop_closed_once(gpu):
    """256 voices, voice n silent from sample 8 n on; after every block of 32 the device names exactly the voices that have been
    silent for at least 64 samples; a voice whose meters were reset by list leaves the next answer"""
    N, S, hold = 256, 32, 64.0
    m, t = handles(gpu, PASS_THROUGH, N, 1, control=None)
    t.close()
    assert m.meter_set_level(0.999, 0.01) == 0
    acc = L.level_zero(1, N)
    n = np.arange(N)
    dropped = None
    for block in range(8 * N // S + 3):
        s = block * S + np.arange(S)
        x = np.where(s[:, None] < 8 * n[None, :], np.float32(0.5), np.float32(0.0)).astype(np.float32).reshape(S, 1, N)
        m.process_block(x)
        acc = L.level_model(x, 0.999, 0.01, acc)
        want = L.select(acc, L.QUIET, hold, False)
        got, count = m.meter_select_level(L.QUIET, hold)
        assert count == want.size and np.array_equal(got, want), (block, got[:8], want[:8])
        if dropped is not None:
            assert dropped not in got.tolist(), "a reused slot's quiet run starts again"
            dropped = None
        if block in (10, 40) and want.size:
            dropped = int(want[-1])
            assert m.meter_reset_list([dropped]) == 0
            acc = L.zeroed(acc, [dropped])
    assert L.same_level(m.meter_read_level(), acc) and want.size == N
