"""Tone meters on the GPU (fxb_meter_set_tones ... fxb_meter_rank_tone): the tone rows against meter_tone_model.tone_model - the
definition of include/fx8010_amd.h "Tone meters" in numpy float64, one operation per line - of the per-instance output block y.  y
is what a twin handle with meters off returns for the same block.  Every figure is compared word for word, fp64 as uint64; the four
existing accumulators must equal meter_model(y) and, with a target and level meters set, the other four their models - they are
taken by the same kernels as with the mode off.

Shapes: S = 33 is four rounds of eight loads plus one sample; 16 + 17, 1 and 8 cut the stream elsewhere; N = 1, 63, 64, 65, 130, 257
put the end of the batch at every lane phase and in a second workgroup.  Coefficient sets: K = 1, 3 and 8 from 2.0, -2.0, 0.0 and
2 cos(2 pi k / 64); every K from 1 to 8 runs once at N = 65, since each is a kernel of its own."""
import numpy as np
import pytest

import fx8010_programs as progs
import meter_level_model as L
import meter_target_model as TG
import meter_tone_model as T
from test_bus_stub import mix_model
from test_gpu_meter import NONFINITE, PASS_THROUGH, bits, cutoffs, on_tier, pcm, same_bits, same_words, stereo, tier  # noqa: F401
from test_gpu_meter_level import SIGNED_THROUGH, edge_input
from test_meter_stub import meter_model, meter_zero, same_meters

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SETS = ([T.coeff(5, 64)], [2.0, -2.0, 0.0], [2.0, -2.0, 0.0] + [T.coeff(k, 64) for k in (1, 7, 16, 31, 32)])
STEREO_THROUGH = PASS_THROUGH.replace("output out 0", "output out 0\ninput in1 1\noutput out1 1").replace("\nend", "\nmacs out1, in1, 0, 0\nend")


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

    def __init__(self, m, N, channels, coeffs, shards=1):
        self.m, self.N, self.ch, self.shards = m, N, channels, shards
        self.four = meter_zero(channels, N)
        self.launches = m.info("meter_tone_launches")
        self.plain = m.info("meter_launches")
        self.set(coeffs)

    def set(self, coeffs):
        assert self.m.meter_set_tones(coeffs) == 0
        self.coeffs = [float(c) + 0.0 for c in coeffs]
        assert np.array_equal(self.m.meter_get_tones().view(np.uint64), np.array(self.coeffs).view(np.uint64))
        self.acc = T.tone_zero(len(coeffs), self.ch, self.N)

    def rows(self):
        return T.rows_of(self.acc, self.coeffs)

    def took(self, what, y, launches=1, plain=True):
        self.acc = T.tone_model(y, self.coeffs, self.acc)
        self.four = meter_model(y, self.four)
        self.launches += launches * self.shards
        self.plain += launches * self.shards if plain else 0
        got = self.m.meter_read_tones()
        tag = (what, self.N, len(self.coeffs))
        assert T.same_tones(got, self.rows()), tag + (T.differing(got, self.rows()),)
        assert same_meters(self.m.meter_read(), self.four), tag + ("the four",)
        assert self.m.info("meter_tone_launches") == self.launches and self.m.info("meter_launches") == self.plain, tag


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 257])
def test_sizes_cuts_and_coefficient_sets(gpu, N, channels):
    text = progs.config3() if channels == 1 else stereo(progs.config3())
    m, t = handles(gpu, text, N, channels)
    clock = 0
    for coeffs in SETS:
        m.meter_read(reset=True)
        f = Follow(m, N, channels, coeffs)
        for S in (33, 16, 17, 1, 8):
            x = pcm(N, S, channels, clock)
            clock += S
            y = t.process_block(x)
            assert same_bits(m.process_block(x), y)
            f.took("block of %d" % S, y)
        assert np.isfinite(f.rows()["power"]).all() and f.acc["s1"].any()
    assert m.info("meter_target_launches") == 0 and m.info("meter_level_launches") == 0
    m.close()
    t.close()


def test_every_tone_count_is_a_kernel_of_its_own(gpu):
    N = 65
    m, t = handles(gpu, progs.config3(), N, 1)
    every = [2.0, T.coeff(3, 64), -2.0, T.coeff(9, 64), 0.0, T.coeff(21, 64), T.coeff(30, 64), -1.0]
    clock = 0
    f = None
    for K in range(1, 9):
        if f is None:
            f = Follow(m, N, 1, every[:K])
        else:
            f.set(every[:K])
        for S in (17, 16):
            x = pcm(N, S, 1, clock)
            clock += S
            y = t.process_block(x)
            assert same_bits(m.process_block(x), y)
            f.took("K = %d, block of %d" % (K, S), y)
    # 33 = 17 + 16, on the device as in the model
    x = pcm(N, 33, 1, 7)
    y = t.process_block(x)
    f.set(every)
    assert same_bits(m.process_block(x), y)
    f.took("33 at once", y)
    # (the program has a state of its own, so the twin says what the next 33 samples are; they are cut as 16 + 17)
    f.set(every)
    x = pcm(N, 33, 1, 40)
    y = np.concatenate([t.process_block(x[:16]), t.process_block(x[16:])])
    assert same_bits(m.process_block(x[:16]), y[:16]) and same_bits(m.process_block(x[16:]), y[16:])
    f.took("16 + 17", y, launches=2)
    assert T.same_tones(f.acc, T.tone_model(y, every), ("s1", "s2")), "16 + 17 samples leave the words of 33"


def test_the_edges_of_the_input_words(gpu):
    """NaN, +-Inf, -0.0 and a denormal on the output, through the programs test_gpu_meter_level.py uses for them"""
    N, S = 130, 40
    coeffs = [2.0, T.coeff(5, 40), 0.0]
    ys = {}
    for name, text in (("through", PASS_THROUGH), ("nonfinite", NONFINITE), ("signed", SIGNED_THROUGH)):
        m, t = handles(gpu, text, N, 1, control="vol" if text == NONFINITE else None, values=np.full(N, 0.001, dtype=np.float32))
        x, kinds = edge_input(N, S, 0.25, text)
        ys[name] = (m, x, t.process_block(x))
        t.close()
    # the test is not vacuous: asserted on y itself, before any device figure is compared
    everything = np.concatenate([bits(y).reshape(-1) for _, _, y in ys.values()])
    assert np.isnan(ys["nonfinite"][2]).any() and (everything == 0x7f800000).any() and (everything == 0xff800000).any(), "NaN, +Inf and -Inf"
    assert (everything == 0x80000000).any() and (((everything & 0x7f800000) == 0) & ((everything & 0x007fffff) != 0)).any(), "-0.0 and a denormal"
    for name, (m, x, y) in ys.items():
        f = Follow(m, N, 1, coeffs)
        assert same_words(m.process_block(x), y)
        f.took("edges, " + name, y)
        assert np.isfinite(f.rows()["power"]).all() and f.acc["s1"].any()
        m.close()


def test_a_plain_case_on_every_tier(gpu, tier):
    N, S = 197, 33
    m, t = handles(gpu, progs.config3(), N, 1)
    f = Follow(m, N, 1, SETS[1])
    for k in range(2):
        x = pcm(N, S, 1, k * S)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y)
        f.took("block %d" % k, y)
    assert on_tier(m, tier) and m.meter_samples() == 2 * S


def test_an_armed_control_track_cuts_the_block_and_not_the_figures(gpu, tier):
    """a 33-sample block with a period-8 track at N = 197: the interpreter and HIP tiers cut it into five segments - five tone
    launches; the translated tier reads the schedule by itself: one.  The figures are those of the uncut y."""
    N, S = 197, 33
    m, t = handles(gpu, progs.config3(), N, 1, control=None)
    steps = np.linspace(0.05, 0.9, 5).astype(np.float32)
    f = Follow(m, N, 1, SETS[1])
    for b in (m, t):
        assert b.set_register_track("cutoff", steps, 8) == 0
    x = pcm(N, S, 1, 0)
    y = t.process_block(x)
    assert same_bits(m.process_block(x), y)
    f.took("armed", y, launches=1 if tier == "default" else 5)
    assert on_tier(m, tier)


def test_target_level_and_tones_together(gpu):
    N = 130
    m, t = handles(gpu, progs.config3(), N, 1)
    rng = np.random.default_rng(12)
    tw = (rng.standard_normal((40, 1, -(-N // 3))) * 0.3).astype(np.float32)
    coeffs = SETS[1]
    assert m.meter_set_target(tw, 3, True) == 0 and m.meter_set_level(0.5, 0.25) == 0 and m.meter_set_tones(coeffs) == 0
    four, match, level, tones, pos = meter_zero(1, N), TG.match_zero(1, N), L.level_zero(1, N), T.tone_zero(3, 1, N), 0
    for k, S in enumerate((16, 17, 33)):
        x = pcm(N, S, 1, 100 * k)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y)
        four = meter_model(y, four)
        match, pos = TG.match_model(y, tw, 3, pos, True, match)
        level = L.level_model(y, 0.5, 0.25, level)
        tones = T.tone_model(y, coeffs, tones)
        assert same_meters(m.meter_read(), four) and TG.same_match(m.meter_read_match(), match) and L.same_level(m.meter_read_level(), level), k
        assert T.same_tones(m.meter_read_tones(), T.rows_of(tones, coeffs)), k
        assert m.meter_target_pos() == pos
    assert m.info("meter_target_launches") == 3 == m.info("meter_level_launches") == m.info("meter_tone_launches") and m.info("meter_launches") == 0
    # a list reset zeroes all ten kinds of column of the listed voices
    lst = np.array([0, 63, 64, 129], dtype=np.int64)
    assert m.meter_reset_list(lst) == 0
    for k in four:
        four[k][:, lst] = 0
    assert same_meters(m.meter_read(), four) and TG.same_match(m.meter_read_match(), TG.zeroed(match, lst)) and L.same_level(m.meter_read_level(), L.zeroed(level, lst))
    assert T.same_tones(m.meter_read_tones(), T.rows_of(T.zeroed(tones, lst), coeffs))


def test_bus_instance_major_and_device_entry_blocks(gpu):
    import torch

    N, S, K, channels = 257, 33, 64, 2
    m, t = handles(gpu, stereo(progs.config3()), N, channels)
    f = Follow(m, N, channels, SETS[2])
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
    N, channels = 130, 2
    text = stereo(progs.config3())
    m, t = handles(gpu, text, N, channels, devices=[0, 0])
    one, _ = handles(gpu, text, N, channels)
    _.close()
    assert len(m.shards()) == 2 and 0 < m.shards()[1][1] < N and m.shards()[1][1] % 256 != 0, m.shards()   # (no multiple of a workgroup)
    f = Follow(m, N, channels, SETS[1], shards=2)
    assert one.meter_set_tones(SETS[1]) == 0
    for k, S in enumerate((16, 17, 33)):
        x = pcm(N, S, channels, 100 * k)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y) and same_bits(one.process_block(x), y)
        f.took("block %d" % k, y)
        assert T.same_tones(m.meter_read_tones(), one.meter_read_tones())
    rows = one.meter_read_tones()
    for tone in range(3):
        thr = float(np.median(T.V(rows, tone)))
        for below in (False, True):
            assert np.array_equal(m.meter_select_tone(tone, thr, below=below)[0], one.meter_select_tone(tone, thr, below=below)[0])
            for largest in (False, True):
                a, b = m.meter_rank_tone(tone, 9, thr, below=below, largest=largest), one.meter_rank_tone(tone, 9, thr, below=below, largest=largest)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
                T.check_rank(m._lib, m, rows, tone, 9, thr, below, largest, what="two shards")
    lst = [129, 0, m.shards()[1][1], m.shards()[1][1] - 1, 0]
    assert T.same_tones(m.meter_read_tones_list(lst), one.meter_read_tones_list(lst))


def tied_voices(N, S, channels, group=5):
    """groups of `group` neighbouring voices get identical input, so that P ties bit for bit and the instance number decides; the
    groups differ in level and in frequency.  One channel of voice 7 carries a louder signal of its own."""
    g = np.arange(N) // group
    t = np.arange(S, dtype=np.float64)[:, None]
    x = ((0.05 + 0.9 * ((g * 37) % 101) / 101.0)[None, :] * np.sin(2 * np.pi * (1 + g % 15)[None, :] * t / 32.0 + 0.4)).astype(np.float32)
    x = np.array(np.broadcast_to(x[:, None, :], (S, channels, N)), dtype=np.float32, order="C")
    if channels > 1:
        x[:, 1, 7] = 0.95
    return x


def tone_rows(gpu, N, channels, coeffs):
    m, t = handles(gpu, PASS_THROUGH if channels == 1 else STEREO_THROUGH, N, channels, control=None)
    t.close()
    assert m.meter_set_tones(coeffs) == 0
    x = tied_voices(N, 32, channels)
    m.process_block(x)
    rows = m.meter_read_tones()
    assert T.same_tones(rows, T.rows_of(T.tone_model(x, coeffs), coeffs)), "every word of x lies inside +-1 and passes as it is"
    return m, rows


def test_select_tone_thresholds_caps_and_ranges(gpu):
    N = 257
    coeffs = [T.coeff(3, 32), T.coeff(8, 32)]
    m, rows = tone_rows(gpu, N, 2, coeffs)
    assert T.V(rows, 0)[7] == rows["power"][0, 1, 7] > rows["power"][0, 0, 7], "the maximum over the channels"
    before = m.info("meter_tone_selects")
    assert T.check_selects(m._lib, m, rows, N, 2) >= 6
    assert m.info("meter_tone_selects") > before + 50 and m.info("meter_selects") == 0 and m.info("meter_level_selects") == 0
    assert m._lib.fxb_meter_select_tone(m._h, 2, T.C.c_double(0.0), 0, N, None, 0, 0) == FX_E_ARG, "tone = K"
    assert m._lib.fxb_meter_select(m._h, 4, T.C.c_double(0.0), 0, N, None, 0, 0) == FX_E_ARG, "fxb_meter_select keeps refusing stat = 4"


def test_select_tone_where_a_scan_lane_owns_two_counts(gpu):
    N = 66000
    coeffs = [T.coeff(3, 32)]
    m, rows = tone_rows(gpu, N, 1, coeffs)
    thr = float(np.median(T.V(rows, 0)))
    for t in (thr, 0.0, np.inf, -np.inf):
        for below in (False, True):
            want = T.select(rows, 0, t, below)
            got, n = m.meter_select_tone(0, t, below=below)
            assert n == want.size and np.array_equal(got, want), (t, below)
    M = T.select(rows, 0, thr, False).size
    assert 0 < M < N
    for cap in (0, 1, M - 1, M, M + 7):
        T.check_select(m._lib, m, rows, 0, thr, False, 0, N, cap)
    T.check_select(m._lib, m, rows, 0, thr, True, 77, N - 77, 40000)


def test_rank_tone_with_ties_decided_by_the_instance_number(gpu):
    N = 257
    coeffs = [T.coeff(3, 32), T.coeff(8, 32)]
    m, rows = tone_rows(gpu, N, 2, coeffs)
    v = T.V(rows, 0)
    assert np.unique(v.view(np.uint64)).size <= -(-N // 5) + 1 and (v[10:15].view(np.uint64) == v[10:11].view(np.uint64)).all(), "P ties bit for bit inside a group"
    before = m.info("meter_tone_ranks")
    calls = T.check_ranks(m._lib, m, rows, 2)
    # (a call over an empty range launches nothing)
    assert 50 < m.info("meter_tone_ranks") - before <= calls and m.info("meter_ranks") == 0 and m.info("meter_level_ranks") == 0
    # a k that ends inside a group of equals: the smaller numbers win, in both directions
    for largest in (False, True):
        full = T.rank(rows, 0, N, largest=largest)[1]
        for k in (1, 2, 3, 4, 6, 7, 64, 66):
            got = m.meter_rank_tone(0, k, largest=largest)
            assert np.array_equal(got[1], full[:k]), (largest, k)
    assert m._lib.fxb_meter_rank_tone(m._h, 2, 3, T.C.c_double(0.0), 0, N, None, None, 0) == FX_E_ARG


def test_read_tones_list_reset_and_reset_list(gpu):
    N = 257
    coeffs = [T.coeff(3, 32), 2.0, -2.0]
    m, rows = tone_rows(gpu, N, 2, coeffs)
    x = tied_voices(N, 32, 2)
    acc = T.tone_model(x, coeffs)
    lst = np.array([256, 0, 64, 63, 0, 130, 256], dtype=np.int64)
    assert T.same_tones(m.meter_read_tones_list(lst), {k: v[:, :, lst] for k, v in rows.items()}), "repeats are fine without reset"
    assert m._lib.fxb_meter_read_tones_list(m._h, lst.ctypes.data, lst.size, None, None, None, 1) == FX_E_ARG and T.same_tones(m.meter_read_tones(), rows), "a repeated instance under reset is refused"
    lst = np.array([256, 0, 64, 63, 130], dtype=np.int64)
    assert T.same_tones(m.meter_read_tones_list(lst, reset=True), {k: v[:, :, lst] for k, v in rows.items()})
    acc = T.zeroed(acc, lst)
    assert T.same_tones(m.meter_read_tones(), T.rows_of(acc, coeffs)), "the listed columns and no others"
    four = m.meter_read()
    lst = np.array([1, 65, 255], dtype=np.int64)
    assert m.meter_reset_list(lst) == 0
    acc = T.zeroed(acc, lst)
    for k in four:
        four[k][:, lst] = 0
    assert T.same_tones(m.meter_read_tones(), T.rows_of(acc, coeffs)) and same_meters(m.meter_read(), four), "reset_list zeroes the listed tone columns and no others"
    assert m.info("meter_tone_list_reads") == 2
    # a list reset between two host blocks (nothing is in flight here; the queued case is the test below)
    lst = np.array([2, 66, 256], dtype=np.int64)
    m.process_block(x)
    assert m.meter_reset_list(lst) == 0
    m.process_block(x)
    acc = T.tone_model(x, coeffs, T.zeroed(T.tone_model(x, coeffs, acc), lst))
    assert T.same_tones(m.meter_read_tones(), T.rows_of(acc, coeffs))
    # a full read with reset zeroes the tone rows alone; fxb_meter_read(reset) zeroes them with the others
    four = m.meter_read()
    assert T.same_tones(m.meter_read_tones(reset=True), T.rows_of(acc, coeffs)) and not m.meter_read_tones()["s1"].any() and same_meters(m.meter_read(), four)
    m.process_block(x)
    m.meter_read(reset=True)
    got = m.meter_read_tones()
    assert not got["s1"].any() and not got["s2"].any() and not got["power"].any() and m.meter_get_tones().size == 3


def test_reset_list_behind_a_queued_block_on_caller_streams(gpu):
    """a device-entry block on stream A, reset_list with no sync, a block on stream B, then the synchronous read: block 1 zeroed on
    the list, plus block 2.  S = 2048 at N = 777: the first block is still running when the reset is queued, so fx_tone_zero has to
    sit behind it inside the event frame.  The staging is reserved by an earlier call of the same length; nothing is allocated
    between the two blocks."""
    import torch

    N, S, channels = 777, 2048, 1
    coeffs = [T.coeff(3, 32), 2.0, -2.0, 0.0]
    rng = np.random.default_rng(13)
    m, t = handles(gpu, progs.config3(), N, channels)   # (a filter with a state: y is what the device wrote, read back below)
    t.close()
    assert m.meter_set_tones(coeffs) == 0
    m.process_block(tied_voices(N, 8, channels))
    assert m.meter_reset_list(np.arange(257, dtype=np.int64)) == 0   # (the staging of a list this long exists from here)
    m.meter_read(reset=True)
    assert not m.meter_read_tones()["s1"].any()
    blocks = [np.tile(tied_voices(N, 32, channels, group=g), (S // 32, 1, 1)) * np.float32(a) for g, a in ((5, 1.0), (3, 0.5))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda") for x in blocks]
    d_out = [torch.full((S, channels, N), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    lst = np.concatenate([[0, N - 1], rng.permutation(np.arange(1, N - 1))[:255]]).astype(np.int64)
    zeros, launches = m.info("meter_list_resets"), m.info("meter_tone_launches")
    assert m.process_block_dev_pitched(d_in[0], d_out[0], S, stream=streams[0].cuda_stream) == 0
    assert m.meter_reset_list(lst) == 0
    assert m.process_block_dev_pitched(d_in[1], d_out[1], S, stream=streams[1].cuda_stream) == 0
    got = m.meter_read_tones()   # (synchronous: it covers everything queued)
    y = [d.cpu().numpy() for d in d_out]
    assert not (y[0] == -7.0).any() and not (y[1] == -7.0).any() and np.isfinite(y[0]).all() and y[0].any() and y[1].any()
    one = T.tone_model(y[0], coeffs)
    want = T.tone_model(y[1], coeffs, T.zeroed(one, lst))
    assert T.same_tones(got, T.rows_of(want, coeffs)), T.differing(got, T.rows_of(want, coeffs))
    # the order matters to the words compared: neither "never zeroed" nor "zeroed behind block 2" gives them
    assert not T.same_tones(got, T.rows_of(T.tone_model(y[1], coeffs, one), coeffs)) and not T.same_tones(got, T.rows_of(T.zeroed(want, lst), coeffs))
    others = np.setdiff1d(np.arange(N), lst)
    assert np.array_equal(got["s1"][:, :, others].view(np.uint64), T.tone_model(y[1], coeffs, one)["s1"][:, :, others].view(np.uint64)), "the unlisted voices carry both blocks"
    assert m.info("meter_list_resets") == zeros + 1 and m.info("meter_tone_launches") == launches + 2 and m.meter_samples() == 2 * S
    assert T.same_tones(m.meter_read_tones_list(lst[:9]), {k: v[:, :, lst[:9]] for k, v in got.items()})
    m.close()


def test_the_loop_closed_once(gpu):
    """256 pass-through voices, each fed one of four on-bin sines over 64 samples: fxb_meter_select_tone(t, 1.0) names exactly the
    voices of tone t"""
    N, S, bins, A = 256, 64, (4, 8, 12, 16), 0.5
    x = T.sines(S, bins, A, N)
    coeffs = [T.coeff(k, S) for k in bins]
    # the model's own separation first: on-bin above 255, off-bin below 1e-9
    P = T.power(T.tone_model(x, coeffs), coeffs)[:, 0, :]
    own = (np.arange(N) % 4)[None, :] == np.arange(4)[:, None]
    assert (P[own] > 255.0).all() and (np.abs(P[~own]) < 1e-9).all()
    m, t = handles(gpu, PASS_THROUGH, N, 1, control=None)
    t.close()
    assert m.meter_set_tones(coeffs) == 0
    assert same_bits(m.process_block(x[:40]), x[:40]) and same_bits(m.process_block(x[40:]), x[40:])
    assert T.same_tones(m.meter_read_tones(), T.rows_of(T.tone_model(x, coeffs), coeffs))
    for tone in range(4):
        got, count = m.meter_select_tone(tone, 1.0)
        assert count == N // 4 and np.array_equal(got, np.arange(tone, N, 4)), tone
        ranked = m.meter_rank_tone(tone, 3, largest=True)
        assert ranked[0] == N and (ranked[1] % 4 == tone).all()
