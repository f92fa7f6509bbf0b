"""Target meters on the GPU (fxb_meter_set_target ... fxb_meter_best): the two match rows against meter_target_model.match_model -
the definition of include/fx8010_amd.h "Target meters" in numpy float64, one operation per line - of the per-instance output block
y and the target the test set.  y is what a twin handle with meters off returns for the same block.  Every figure is compared bit
for bit, fp64 words as integers; the four existing accumulators must equal meter_model(y) - they are taken by the same code as
without a target - and, in one test, those of a metered twin without a target.

Shapes: S = 33 is four rounds of eight loads plus one sample; N = 63, 64, 65, 130, 257 put the end of the batch at every lane phase
and in a second workgroup; group 3 puts target-column boundaries at every lane phase, 65 straddles wavefronts.  Target lengths:
T = 5 with LOOP wraps several times inside one round of eight; T = 40 with blocks of 16 + 17 + 16 carries the position over and
wraps in the third block; T = 20 without LOOP ends inside a round and the later samples change only the four.  The target carries
NaN, +-Inf, +-0, denormals, +-1.0 and words 2^100 away from y in lanes of their own; y carries NaN and +-Inf through a program that
does not saturate."""
import numpy as np
import pytest

import fx8010_programs as progs
import meter_target_model as T
from test_bus_stub import expand, mix_model
from test_gpu_meter import NONFINITE, bits, cutoffs, on_tier, pcm, same_bits, same_words, stereo, tier  # noqa: F401
from test_meter_stub import meter_model, meter_zero, same_meters

pytestmark = pytest.mark.gpu

FX_E_ARG = -3


def handles(gpu, text, N, channels, control="cutoff", values=None, devices=None, twin_metered=False):
    """(the handle with meters on, its twin with meters off - or on, without a target)"""
    out = []
    for first in (True, False):
        b = gpu.Batch(N, channels, 0) if devices is None or not first else gpu.Batch(N, channels, devices=devices)
        assert b.load_text(text), b.errors()
        if control:
            assert b.set_register_array(control, cutoffs(N) if values is None else values) == 0
        if first or twin_metered:
            assert b.meter_enable() == 0
        out.append(b)
    return out


def target_words(rng, shape):
    """levels like an output's, and in lanes of their own NaN, +-Inf, +-0, denormals, +-1.0, +-2^100 and 2^-100"""
    t = (rng.standard_normal(shape) * 0.3).astype(np.float32)
    flat = t.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, -1e-44, 1.0, -1.0, 2.0 ** 100, -2.0 ** 100, 2.0 ** -100):
        flat[rng.integers(0, flat.size, max(flat.size // 40, 1))] = np.float32(v)
    return t


class Follow:
    """the model of everything the handle m has been through since its meters were zero"""

    def __init__(self, m, N, channels):
        self.m, self.N, self.ch = m, N, channels
        self.four = meter_zero(channels, N)
        self.launches = m.info("meter_target_launches")

    def target(self, t, group, loop):
        assert self.m.meter_set_target(t, group, loop) == 0 and self.m.meter_target_pos() == 0
        self.t, self.group, self.loop, self.pos, self.acc = t, group, loop, 0, T.match_zero(self.ch, self.N)

    def took(self, what, y, launches=1):
        self.acc, self.pos = T.match_model(y, self.t, self.group, self.pos, self.loop, self.acc)
        self.four = meter_model(y, self.four)
        self.launches += launches
        got = self.m.meter_read_match()
        assert T.same_match(got, self.acc), (what, self.N, self.group, self.t.shape[0], self.loop, np.argwhere(got["err"].view(np.uint64) != self.acc["err"].view(np.uint64))[:4].tolist())
        assert same_meters(self.m.meter_read(), self.four), (what, "the four")
        assert self.m.meter_target_pos() == self.pos and self.m.info("meter_target_launches") == self.launches, what


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 257])
def test_sizes_groups_and_target_lengths(gpu, N, channels):
    text = progs.config3() if channels == 1 else stereo(progs.config3())
    m, t = handles(gpu, text, N, channels)
    f = Follow(m, N, channels)
    rng = np.random.default_rng(100 * N + channels)
    clock = 0
    for group in sorted({1, 3, 64, 65, N}):
        G = -(-N // min(group, N))
        for tlen, loop, cuts in ((5, True, (33,)), (33, False, (33,)), (40, True, (16, 17, 16)), (20, False, (33,))):
            f.target(target_words(rng, (tlen, channels, G)), group, loop)
            for S in cuts:
                x = pcm(N, S, channels, clock)
                clock += S
                y = t.process_block(x)
                assert same_bits(m.process_block(x), y)
                f.took("block of %d" % S, y)
            if (tlen, loop) == (20, False):
                assert f.pos == 33 and (T.V(f.acc, 0) > 0).any()
    assert m.info("meter_launches") == 0, "fx_meter_target in place of fx_meter"
    m.close()
    t.close()


def test_a_plain_case_on_every_tier_and_the_four_against_a_metered_twin(gpu, tier):
    N, S = 197, 33
    m, p = handles(gpu, progs.config3(), N, 1, twin_metered=True)
    rng = np.random.default_rng(5)
    f = Follow(m, N, 1)
    f.target(target_words(rng, (40, 1, 66)), 3, True)
    for k in range(2):
        x = pcm(N, S, 1, k * S)
        y = p.process_block(x)
        assert same_bits(m.process_block(x), y)
        f.took("block %d" % k, y)
        assert same_meters(m.meter_read(), p.meter_read()), "the four with a target set are those of a twin without one"
    assert on_tier(m, tier) and p.info("meter_launches") == 2 and m.info("meter_launches") == 0 and m.meter_samples() == p.meter_samples() == 2 * S


def test_an_armed_control_track_carries_the_position_through_its_segments(gpu, tier):
    """a 33-sample block with a period-8 track at N = 197: the interpreter and HIP tiers cut it into five segments - five target
    launches, the position carried through them; the translated tier reads the schedule by itself: one launch"""
    N, S = 197, 33
    m, t = handles(gpu, progs.config3(), N, 1, control=None)
    steps = np.linspace(0.05, 0.9, 5).astype(np.float32)
    rng = np.random.default_rng(6)
    f = Follow(m, N, 1)
    f.target(target_words(rng, (40, 1, 66)), 3, True)
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
        f.took("armed, bus %d" % bus, y, launches=1 if tier == "default" else 5)
        assert on_tier(m, tier)


def test_nonfinite_output_words_change_neither_figure(gpu):
    """MACW does not saturate: an input of 3 puts +Inf on the output, a NaN input a NaN, -Inf itself"""
    N, S = 197, 33
    m, t = handles(gpu, NONFINITE, N, 1, control="vol")
    x = pcm(N, S, 1, 0)
    for (s, n), v in {(5, 0): 3.0, (9, 63): np.nan, (11, 64): -np.inf, (12, 64): np.nan, (32, N - 1): 3.0, (0, 130): -np.inf}.items():
        x[s, 0, n] = v
    f = Follow(m, N, 1)
    f.target(target_words(np.random.default_rng(7), (33, 1, N)), 1, False)
    y = t.process_block(x)
    assert same_words(m.process_block(x), y) and not np.isfinite(y).all()
    f.took("poisoned", y)
    got = m.meter_read_match()
    assert np.isfinite(got["err"]).all() and np.isfinite(got["cross"]).all() and m.meter_read()["nonfinite"].sum() == 6


def test_bus_instance_major_and_device_entry_blocks(gpu):
    import torch

    N, S, K, channels = 257, 33, 64, 2
    m, t = handles(gpu, stereo(progs.config3()), N, channels)
    rng = np.random.default_rng(8)
    f = Follow(m, N, channels)
    f.target(target_words(rng, (40, channels, 86)), 3, True)
    # a bus block with SHARED_IN | MIX_OUT
    xg = pcm(m.bus_groups(K), S, channels, 0)
    y = t.process_block(expand(xg, K, N))
    assert same_words(m.process_block_bus(xg, K, True, True), mix_model(y, K))
    f.took("bus", y)
    # an instance-major block
    x = pcm(N, S, channels, S)
    y = t.process_block(x)
    got = m.process_block_imajor(np.ascontiguousarray(x.transpose(2, 0, 1)))
    assert same_bits(np.ascontiguousarray(got.transpose(1, 2, 0)), y)
    f.took("instance-major", y)
    # a device-entry block on a caller stream
    x = pcm(N, S, channels, 2 * S)
    y = t.process_block(x)
    stream = torch.cuda.Stream()
    d_in = torch.from_numpy(x).to("cuda")
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    assert m.process_block_dev_pitched(d_in, d_out, S, stream=stream.cuda_stream) == 0
    assert m.sync() == 0
    assert same_bits(d_out.cpu().numpy(), y)
    f.took("device entry on a caller stream", y)
    # a list reset zeroes all six columns of the listed voices
    L = np.array([0, 63, 64, 256], dtype=np.int64)
    assert m.meter_reset_list(L) == 0
    f.acc = T.zeroed(f.acc, L)
    for k in f.four:
        f.four[k][:, L] = 0
    f.took("a list reset", np.zeros((0, channels, N), dtype=np.float32), launches=0)


def test_two_shards_on_one_gpu_with_group_3(gpu):
    N, S, channels = 64 * 7 + 17, 33, 2   # (the second shard starts at 256: no multiple of 3)
    m, t = handles(gpu, stereo(progs.config3()), N, channels, devices=[0, 0])
    assert len(m.shards()) == 2 and m.shards()[1][1] % 3 != 0, m.shards()
    rng = np.random.default_rng(9)
    f = Follow(m, N, channels)
    f.target(target_words(rng, (40, channels, -(-N // 3))), 3, True)
    for k, S in enumerate((16, 17, 16)):
        x = pcm(N, S, channels, 100 * k)
        y = t.process_block(x)
        assert same_bits(m.process_block(x), y)
        f.took("block %d" % k, y, launches=2)
    rows = m.meter_read_match()
    first = m.shards()[1][1]
    for group in (1, 3, 64, first - 1, first + 1, N):
        for stat in (0, 1):
            for largest in (False, True):
                assert T.same_best(m.meter_best(stat, group, largest), T.best(rows, stat, group, largest)), (group, stat, largest)
    for stat, thr in ((0, float(np.median(T.V(rows, 0)))), (1, 0.0)):
        for below in (False, True):
            want = T.select(rows, stat, thr, below)
            got, n = m.meter_select_match(stat, thr, below=below)
            assert n == want.size and np.array_equal(got, want)
            got, n = m.meter_select_match(stat, thr, below=below, first=first - 5, n_range=11, cap=3)
            want = T.select(rows, stat, thr, below, first - 5, 11)
            assert n == want.size and np.array_equal(got, want[:3])


def test_seek_and_the_resets(gpu):
    N, S = 130, 33
    m, t = handles(gpu, progs.config3(), N, 1)
    rng = np.random.default_rng(10)
    f = Follow(m, N, 1)
    f.target(target_words(rng, (50, 1, N)), 1, False)
    x = pcm(N, S, 1, 0)
    y = t.process_block(x)
    m.process_block(x)
    f.took("from 0", y)
    # a seek in mid-stream
    assert m.meter_target_seek(7) == 0
    f.pos = 7
    x = pcm(N, S, 1, S)
    y = t.process_block(x)
    m.process_block(x)
    f.took("from 7", y)
    assert m.meter_target_seek(50) == 0 and m.meter_target_pos() == 50 and m._lib.fxb_meter_target_seek(m._h, 51) == FX_E_ARG
    f.pos = 50
    x = pcm(N, S, 1, 2 * S)
    y = t.process_block(x)
    m.process_block(x)
    f.took("from the end: only the four move", y)
    # read_match with reset leaves the four existing accumulators alone
    assert T.same_match(m.meter_read_match(reset=True), f.acc)
    f.acc = T.match_zero(1, N)
    assert T.same_match(m.meter_read_match(), f.acc) and same_meters(m.meter_read(), f.four) and m.meter_samples() == 3 * S and m.meter_target_pos() == 50 + S
    assert m.meter_target_seek(0) == 0
    f.pos = 0
    x = pcm(N, S, 1, 3 * S)
    y = t.process_block(x)
    m.process_block(x)
    f.took("after the reset of the two", y)
    # fxb_meter_read(reset) zeroes all six
    m.meter_read(reset=True)
    assert T.same_match(m.meter_read_match(), T.match_zero(1, N)) and same_meters(m.meter_read(), meter_zero(1, N)) and m.meter_target_pos() == S
    # the target dropped: the queries are refused, fx_meter again
    assert m.meter_clear_target() == 0 and m._lib.fxb_meter_read_match(m._h, None, None, 0) == FX_E_ARG and m._lib.fxb_meter_best(m._h, 0, 1, None, None, 0) == FX_E_ARG
    m.process_block(x)
    assert m.info("meter_launches") == 1 and same_meters(m.meter_read(), meter_model(t.process_block(x)))


def sweep(gpu, N, channels=1):
    """one signal through N settings (cutoffs with equal ones in places), a target of both signs: (m, rows)"""
    text = progs.config3() if channels == 1 else stereo(progs.config3())
    values = cutoffs(N)
    values[9:12] = values[9]          # equal settings: ties inside a group of 3 and of 64
    values[64:70] = values[64]
    m, t = handles(gpu, text, N, channels, values=values)
    rng = np.random.default_rng(11)
    S, K = 33, 64
    tw = (rng.standard_normal((S, channels, -(-N // K))) * 0.2).astype(np.float32)
    assert m.meter_set_target(tw, K) == 0
    xg = pcm(1, S, channels, 0)
    y = t.process_block(expand(xg, N, N))
    m.process_block_bus(xg, N, True, True)
    rows = m.meter_read_match()
    assert T.same_match(rows, T.match_model(y, tw, K, 0, False)[0])
    t.close()
    return m, rows


def test_select_match_thresholds_and_caps(gpu):
    N = 257
    m, rows = sweep(gpu, N, 2)
    assert (T.V(rows, 1) < 0).any() and (T.V(rows, 1) > 0).any(), "cross values of both signs"
    before = m.info("meter_match_selects")
    assert T.check_selects(m._lib, m, rows, N) >= 6
    assert m.info("meter_match_selects") > before + 50 and m.info("meter_selects") == 0
    assert m._lib.fxb_meter_select(m._h, 4, T.C_DOUBLE(0.0), 0, N, None, 0, 0) == FX_E_ARG, "fxb_meter_select keeps refusing stat = 4"


def test_select_match_where_a_scan_lane_owns_two_counts(gpu):
    N = 66000
    m, rows = sweep(gpu, N)
    for stat, thr in ((0, float(np.median(T.V(rows, 0)))), (1, 0.0)):
        for below in (False, True):
            want = T.select(rows, stat, thr, below)
            got, n = m.meter_select_match(stat, thr, below=below)
            assert n == want.size and 0 < n < N and np.array_equal(got, want), (stat, below)
    T.check_one(m._lib, m, rows, 0, float(np.median(T.V(rows, 0))), False, 65, N - 65, 40000)


def test_best_groups_ties_and_largest(gpu):
    N = 257
    m, rows = sweep(gpu, N)
    v = T.V(rows, 0)
    assert v[9] == v[10] == v[11] and v[64] == v[69], "equal settings give equal figures"
    before = m.info("meter_match_bests")
    for group in (1, 3, 64, 65, N):
        for stat in (0, 1):
            for largest in (False, True):
                assert T.same_best(m.meter_best(stat, group, largest), T.best(rows, stat, group, largest)), (group, stat, largest)
    assert m.info("meter_match_bests") == before + 20
    w, val = m.meter_best(T.ERROR, 64)
    assert w.size == 5 and w[4] == 256 and val[4] == v[256], "a last group of one instance"
    # a tie decides: make the tied instances the best of their groups by comparing on the negated order too
    for group in (3, 64, N):
        for largest in (False, True):
            w, _ = m.meter_best(T.ERROR, group, largest)
            for g, n in enumerate(w):
                part = v[g * group:(g + 1) * group]
                assert n == g * group + int(np.nonzero(part == (part.max() if largest else part.min()))[0][0]), "the smallest number of equal ones"
    w, _ = m.meter_best(T.CROSS, N, largest=True)
    assert w[0] == int(np.argmax(T.V(rows, 1)))


def test_the_loop_closed_once(gpu):
    """config3 with `cutoff` swept over 256 instances; the target is the output of instance 100 taken from a twin; bus blocks with
    shared input; fxb_meter_best(ERROR, N) returns 100 with value +0.0"""
    N, S = 256, 33
    values = np.linspace(0.05, 0.95, N).astype(np.float32)
    m, t = handles(gpu, progs.config3(), N, 1, values=values)
    blocks = [pcm(1, S, 1, k * S) for k in range(3)]
    wanted = np.concatenate([t.process_block(expand(xg, N, N))[:, :, 100:101] for xg in blocks])   # [3 S, 1, 1]
    assert m.meter_set_target(wanted, N) == 0
    for xg in blocks:
        m.process_block_bus(xg, N, True, True)
    w, v = m.meter_best(T.ERROR, N)
    assert w.tolist() == [100] and v.view(np.uint64).tolist() == [0], (w, v)
    rows = m.meter_read_match()
    assert (np.delete(T.V(rows, 0), 100) > 0).all() and m.meter_target_pos() == 3 * S and m.info("meter_target_launches") == 3
    got, n = m.meter_select_match(T.ERROR, 0.0, below=False, cap=0)
    assert n == N and m.meter_select_match(T.ERROR, np.nextafter(0.0, 1.0), below=True)[0].tolist() == [100]
