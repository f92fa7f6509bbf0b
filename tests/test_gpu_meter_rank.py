"""Meter ranks on the GPU (fxb_meter_rank, fxb_meter_rank_match, fxb_meter_rank_level): the kernels of csrc/fx_meter_rank.hip against
the numpy model of tests/meter_rank_model.py over the arrays the read calls return.  Bar: equality everywhere - the list word for
word, the values as integer words, the return value, the marks behind min(M, k) untouched, every accumulator unchanged by the
call.  No tolerance.

The program is the one-gain MACW program of tests/test_gpu_meter_list.py (out = 0 + in * volume, one instruction per channel), the
meters are accumulated over blocks of 16 + 17 samples.  Three kinds of handle: the four accumulators alone; a target set (err and
cross, a negative cross included: meter_rank_model.target_for); level meters on (envelope and quiet run).  The k values come from
the model (k_values: 0, 1, 2, 63, 64, 65, 257, M - 1, M, M + 1), the thresholds too; what the data and the k reach - every digit
of the radix select, ties at the k-th key across a wavefront and a chunk boundary, the corner counts - is asserted without a GPU
in tests/test_meter_rank_model.py.

Sizes.  A chunk is 256 instances (kMeterSelectChunk) FROM `first`; the scan is one workgroup of 256 lanes in which a lane owns
ceil(chunks / 256) consecutive chunks.  N = 1, 63, 64, 65 around a wavefront, 130 (two wavefronts and a tail of two), 257 (a second
chunk of one instance), 300 (the directed ladder) and 66 000: 258 chunks, lanes 0 .. 128 of the scan own two chunks each, the last
chunk is 208 instances wide - run once per family with 8-sample blocks."""
import numpy as np
import pytest

import meter_level_model as L
import meter_list_model as M
import meter_rank_model as R
import meter_target_model as T
from pyoracle import Oracle
from test_gpu_meter_list import program
from test_meter_stub import meter_model

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SCAN_LOOPS = 66000   # > kMeterSelectChunk * kMeterScanWidth: a lane of the scan owns two chunks


@pytest.fixture(scope="module")
def lib(gpu):
    return gpu.load()


def handle(gpu, N, channels, kind, x=None, devices=None, cut=16):
    """kind: "meter" (the four accumulators alone), "match" (a target set), "level" (level meters on), "all"; x goes through in two
    blocks cut at `cut`"""
    b = gpu.Batch(N, channels, 0) if devices is None else gpu.Batch(N, channels, devices=devices)
    assert b.load_text(program(channels)), b.errors()
    assert b.meter_enable() == 0
    if kind in ("match", "all"):
        assert b.meter_set_target(R.target_for(x), group=1) == 0
    if kind in ("level", "all"):
        assert b.meter_set_level(R.LEVEL_RELEASE, R.LEVEL_FLOOR) == 0
    if x is not None:
        b.process_block(x[:cut])
        b.process_block(x[cut:])
    return b


def rows_of(b, kind):
    out = {"meter": b.meter_read()}
    if kind in ("match", "all"):
        out["match"] = b.meter_read_match()
    if kind in ("level", "all"):
        out["level"] = b.meter_read_level()
    return out


def same_all(got, want):
    same = {"meter": M.same_rows, "match": T.same_match, "level": L.same_level}
    return got.keys() == want.keys() and all(same[k](got[k], want[k]) for k in got)


CHANNELS = {1: 1, 63: 2, 64: 4, 65: 1, 130: 2, 257: 4}


@pytest.mark.parametrize("kind", R.FAMILIES)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 257])
def test_ranks_equal_the_numpy_model(gpu, lib, N, kind):
    """every stat of the family, the four flag combinations (BELOW with LARGEST among them), the model's thresholds and k values,
    ranges with an unaligned `first`; the counter; nothing changed"""
    channels = CHANNELS[N]
    x = M.voices(N, channels, 33, seed=N)
    b = handle(gpu, N, channels, kind, x)
    rows = rows_of(b, kind)
    before = b.info(R.COUNTER[kind])
    calls = R.check_ranks(lib, b, kind, rows[kind], "N=%d" % N, starts=(0, 1, 63, 65))
    assert 0 < b.info(R.COUNTER[kind]) - before < calls and b.info(R.COUNTER[kind]) == lib.fxb_info(b._h, R.INFO[kind])
    assert [b.info(R.COUNTER[f]) for f in R.FAMILIES if f != kind] == [0, 0]
    if kind == "match" and N >= 63:
        cross = R.value("match", rows["match"], T.CROSS)
        assert (cross < 0).any() and (cross > 0).any() and R.check_digits(lib, b, "match", cross, T.CROSS) >= {0}
    assert same_all(rows_of(b, kind), rows) and b.meter_samples() == 33, "a rank changes nothing"
    b.close()


@pytest.mark.parametrize("channels", [1, 2, 4])
def test_every_channel_count_on_one_handle_of_all_three_kinds(gpu, lib, channels):
    N = 130
    x = M.voices(N, channels, 33, seed=7)
    b = handle(gpu, N, channels, "all", x)
    rows = rows_of(b, "all")
    for family in R.FAMILIES:
        R.check_ranks(lib, b, family, rows[family], "channels=%d" % channels, ks=(0, 1, 64, 65, N), starts=(0, 77))
    assert same_all(rows_of(b, "all"), rows)
    b.close()


def test_the_directed_ladder(gpu, lib):
    """meter_rank_model.ladder_voices: the k-th and (k + 1)-th keys first differ in every digit below the top one; ties at the k-th
    key across instance 63 | 64 and 255 | 256 of which fewer win than exist; M < k, M == k, M == 0, k == 0; every V equal; LARGEST
    with ties; two calls in a row give identical words"""
    x = R.ladder_voices()
    b = handle(gpu, R.LADDER_N, 1, "meter", x)
    rows = b.meter_read()
    assert M.same_rows(rows, meter_model(x)), "out = in: the sums are the model's, exact"
    energy, peak, nonfinite = (R.value("meter", rows, s) for s in (0, 1, 3))
    assert R.check_digits(lib, b, "meter", energy, 0) >= set(range(1, R.PASSES))
    for k in (99, 100, 101, 269, 270, 271, 288 + 5, 288 + 6):
        for largest in (False, True):
            R.check_one(lib, b, "meter", energy, 0, k, largest=largest, what="ladder tie")
            R.check_one(lib, b, "meter", peak, 1, k, largest=largest, what="ladder peak tie")
    t = 1.0 + 2.0 ** -30
    for k in R.k_values(4):
        assert R.check_one(lib, b, "meter", energy, 0, k, t, what="inside the ladder") == 4
        assert R.check_one(lib, b, "meter", energy, 0, k, np.inf) == 0
        R.check_one(lib, b, "meter", nonfinite, 3, k, largest=bool(k & 1), what="every V equal")
    for first, n_range in ((1, 299), (63, 200), (200, 100), (255, 2), (257, 43)):
        for k in (1, 64, n_range):
            R.check_one(lib, b, "meter", energy, 0, k, 1.0, first=first, n_range=n_range, what="ladder range")
            R.check_one(lib, b, "meter", energy, 0, k, 1.5, True, True, first, n_range, what="ladder range, BELOW with LARGEST")
    for k, flags in ((100, 0), (270, R.LARGEST), (7, R.BELOW | R.LARGEST)):
        one, two = R.raw_rank(lib, b, "meter", 0, k, 2.0 if flags & R.BELOW else -np.inf, flags, 0, R.LADDER_N), R.raw_rank(lib, b, "meter", 0, k, 2.0 if flags & R.BELOW else -np.inf, flags, 0, R.LADDER_N)
        assert one[2] == two[2] == R.LADDER_N and np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and (one[0][:k] != R.MARK).all()
    assert M.same_rows(b.meter_read(), rows)
    b.close()


@pytest.mark.parametrize("kind", R.FAMILIES)
def test_ranks_where_the_chunk_scan_loops(gpu, lib, kind):
    """N = 66 000 (module docstring), 8-sample blocks, one channel"""
    N = SCAN_LOOPS
    x = M.voices(N, 1, 8, seed=5)
    b = handle(gpu, N, 1, kind, x, cut=4)
    rows = rows_of(b, kind)[kind]
    for stat in R.STATS[kind]:
        V = R.value(kind, rows, stat)
        for largest in (False, True):
            for k in (0, 1, 257, 4096, 4097, 65537, N, N + 1):
                R.check_one(lib, b, kind, V, stat, k, largest=largest, what="N=66000")
        t = R.thresholds(V)[1]
        for below, largest in ((False, False), (True, True)):
            for k in R.k_values(R.rank(V, 0, t, below)[0]):
                R.check_one(lib, b, kind, V, stat, k, t, below, largest, what="N=66000")
        for first, n_range in ((65535, 3), (65536, N - 65536), (255, 65300), (N - 1, 1), (1, N - 1)):
            R.check_one(lib, b, kind, V, stat, 300, t, True, False, first, n_range, "N=66000 range")
    b.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_shards_on_one_gpu_against_the_single_handle(gpu, lib, devices):
    """fxb_create_on_devices with the ordinal two and three times, N no multiple of the shard count: ranges across the borders, k
    inside and beyond every part, the merge under (V, n); a shard whose part is empty launches nothing"""
    N, channels = 335, 2
    x = M.voices(N, channels, 33, seed=8)
    b, one = handle(gpu, N, channels, "all", x, devices=devices), handle(gpu, N, channels, "all", x)
    borders = [f for _, f, _ in b.shards()][1:]
    assert len(borders) == len(devices) - 1 and N % len(devices) != 0
    rows = rows_of(one, "all")
    assert same_all(rows_of(b, "all"), rows)
    ranges = [(0, N), (1, N - 1)] + [(f - 1, 2) for f in borders] + [(borders[0] - 30, 100), (borders[-1], N - borders[-1]), (borders[0] + 3, 20)]
    for family in R.FAMILIES:
        for stat in R.STATS[family]:
            V = R.value(family, rows[family], stat)
            for first, n_range in ranges:
                for flags in range(4):
                    for k in (0, 1, 64, n_range - 1, n_range + 3):
                        args = (stat, k, R.thresholds(V)[1], flags, first, n_range)
                        got, want = R.raw_rank(lib, b, family, *args), R.raw_rank(lib, one, family, *args)
                        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("the single handle's words", family) + args
                        R.check_one(lib, b, family, V, stat, k, args[2], bool(flags & 1), bool(flags & 2), first, n_range, "shards")
    for (first, n_range), launches in (((0, N), len(devices)), ((borders[0] - 1, 2), 2), ((borders[0] + 3, 20), 1), ((5, 0), 0)):
        before = b.info("meter_ranks")
        b.meter_rank(1, 4, first=first, n_range=n_range)
        assert b.info("meter_ranks") - before == launches, "a shard whose part is empty launches nothing"
    for h in (b, one):
        h.close()


def test_refusals_launch_nothing_and_write_nothing(gpu, lib):
    N, channels = 130, 2
    x = M.voices(N, channels, 33, seed=3)
    b = handle(gpu, N, channels, "all", x)
    rows = rows_of(b, "all")
    lst, val = np.full(N + 8, R.MARK, dtype=np.int64), np.full(N + 8, R.VMARK, dtype=np.uint64)
    for family in R.FAMILIES:
        top = R.STATS[family][-1]
        for stat, k, t, first, n_range, null, flags in ((top + 1, 3, 0.0, 0, N, False, 0), (-1, 3, 0.0, 0, N, False, 0), (0, 3, np.nan, 0, N, False, 0), (0, 3, 0.0, 0, N, False, 4),
                                                       (0, 3, 0.0, -1, 4, False, 0), (0, 3, 0.0, 0, -1, False, 0), (0, 3, 0.0, 1, N, False, 0), (0, -1, 0.0, 0, N, False, 0), (0, 1, 0.0, 0, N, True, 0)):
            got = getattr(lib, R.CALL[family])(b._h, stat, k, t, first, n_range, None if null else lst.ctypes.data, val.ctypes.data, flags)
            assert got == FX_E_ARG and b.last_error() and (lst == R.MARK).all() and (val == R.VMARK).all(), (family, stat, k, t, first, n_range, null, flags)
        assert getattr(lib, R.CALL[family])(b._h, 0, 3, 0.0, 5, 0, lst.ctypes.data, val.ctypes.data, 0) == 0, "n_range == 0 returns 0 without a launch"
    assert [b.info(R.COUNTER[f]) for f in R.FAMILIES] == [0, 0, 0] and same_all(rows_of(b, "all"), rows)
    b.close()
    off = handle(gpu, N, channels, "meter", x)
    for family, word in (("match", "no target is set"), ("level", "the mode is off")):
        assert getattr(lib, R.CALL[family])(off._h, 0, 3, 0.0, 0, N, lst.ctypes.data, val.ctypes.data, 0) == FX_E_ARG and word in off.last_error()
    assert off.meter_enable(False) == 0
    assert lib.fxb_meter_rank(off._h, 0, 3, 0.0, 0, N, lst.ctypes.data, val.ctypes.data, 0) == FX_E_ARG and "metering is off" in off.last_error()
    assert (lst == R.MARK).all() and (val == R.VMARK).all()
    off.close()


def test_a_rank_behind_a_queued_block_and_a_list_reset_sees_both(gpu, lib):
    """a device-entry block on a stream of the caller's, fxb_meter_reset_list with no sync, then the rank: the reset voices are the
    quietest - zero energy -, in instance order, and every other voice has the block's energy"""
    import torch

    N, S = 777, 2048
    rng = np.random.default_rng(13)
    warm = M.pattern_voices(N, 1, 8, [])
    b = handle(gpu, N, 1, "meter", warm, cut=4)
    b.meter_rank(0, 300)   # (the staging exists before anything is queued)
    assert b.meter_read(reset=True) is not None
    x = np.tile(M.pattern_voices(N, 1, 32, np.arange(0, N, 5)), (S // 32, 1, 1))
    stream = torch.cuda.Stream()
    d_in, d_out = torch.from_numpy(x).to("cuda"), torch.full((S, 1, N), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    Lz = np.sort(rng.permutation(N)[:257]).astype(np.int64)
    assert b.process_block_dev_pitched(d_in, d_out, S, stream=stream.cuda_stream) == 0
    assert b.meter_reset_list(Lz) == 0
    lst, val, m = R.raw_rank(lib, b, "meter", 0, 300, -np.inf, 0, 0, N)
    want = M.zeroed(meter_model(d_out.cpu().numpy()), Lz)
    rows = b.meter_read()
    assert M.same_rows(rows, want) and rows["energy"].max() > 0
    V = R.value("meter", rows, 0)
    assert m == N and np.array_equal(lst[:257], Lz) and (val[:257] == 0).all(), "the reset voices first, in instance order"
    assert np.array_equal(lst[:300], R.rank(V, 300)[1]) and np.array_equal(val[:300], R.rank(V, 300)[2].view(np.uint64)) and (val[257:300] != 0).all()
    b.close()


def test_the_voice_stealing_loop_closed_once(gpu, lib):
    """rank the K quietest voices by envelope, reset their meters, recall a preset into them, process a
    block - the stolen voices play the preset (against the oracle) with fresh meters, every other voice plays on (against a twin)"""
    N, K, S = 130, 8, 16
    text = program(1)
    vol = np.ones(N, dtype=np.float32)
    vol[5] = 0.25   # the preset lives in voice 5
    b, twin = handle(gpu, N, 1, "level"), handle(gpu, N, 1, "meter")
    x1, x2 = M.pattern_voices(N, 1, S, np.arange(0, N, 3)), M.pattern_voices(N, 1, S, np.arange(1, N, 2))
    x1[:, 0, 40:48] *= np.float32(0.0625)   # eight voices quieter than the rest, one of them quieter still
    x1[:, 0, 44] *= np.float32(0.5)
    for h in (b, twin):
        assert h.set_register_array("volume", vol) == 0
        h.process_block(x1)
    assert b.bank_create(1) == 0 and b.bank_store([0], [5]) == 0
    level = b.meter_read_level()
    m, steal, env = b.meter_rank_level(gpu.LEVEL_ENVELOPE, K)
    want = R.rank(R.value("level", level, L.ENVELOPE), K)
    assert m == N and np.array_equal(steal, want[1]) and np.array_equal(env.view(np.uint64), want[2].view(np.uint64))
    assert steal[0] == 44 and sorted(steal.tolist()) == list(range(40, 48)), "the eight quiet voices, the quietest first"
    assert b.meter_reset_list(steal) == 0 and b.bank_recall([0] * K, steal) == 0
    y, yt = b.process_block(x2).reshape(S, N), twin.process_block(x2).reshape(S, N)
    assert b.bank_status() == (0, -1, 0)
    others = np.setdiff1d(np.arange(N), steal)
    assert np.array_equal(y[:, others].view(np.uint32), yt[:, others].view(np.uint32)), "every other voice plays on"
    for n in steal:
        o = Oracle(1)
        assert o.load_text(text)
        o.set_register("volume", 0.25)
        assert np.array_equal(o.process_block(x2[:, 0, n].copy()).view(np.uint32), y[:, n].view(np.uint32)), "a stolen voice plays the preset"
    after = b.meter_read_level()
    fresh = L.level_model(y[:, None, :], R.LEVEL_RELEASE, R.LEVEL_FLOOR)
    carried = L.level_model(y[:, None, :], R.LEVEL_RELEASE, R.LEVEL_FLOOR, level)
    for key in ("level", "quiet"):
        carried[key][:, steal] = fresh[key][:, steal]
    assert L.same_level(after, carried), "fresh meters for the stolen voices, the others' carried on"
    for h in (b, twin):
        h.close()
