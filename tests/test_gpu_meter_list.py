"""Meter queries by list on the GPU (fxb_meter_select, fxb_meter_read_list, fxb_meter_reset_list): the kernels of
csrc/fx_meter_list.hip against the numpy model of tests/meter_list_model.py over the arrays fxb_meter_read returns.  Bar: equality
everywhere - the list word for word, the count, the words behind min(M, cap) untouched, accumulators bit for bit (fp64 and fp32
words as integers).  No tolerance.

The program is the one-gain program of fx8010_programs (config1_shipped: out = 0 + in * volume, volume = 1.0) with MACW in place
of MACS, so that a non-finite input word is a non-finite output word, and with one such instruction per channel: the per-instance
input (meter_list_model.voices: +-1.0, the float below 1, denormals, NaN, +-Inf, silence, the loud channel moving from instance
to instance) decides the meters.  What a channel's output is of its input is the emulation's business (the reference's input-refresh
rule lets a later channel hear an earlier one's word): the model is numpy over what fxb_meter_read returns, and the named match
patterns (meter_list_model.pattern_voices) give every channel the same level.

Sizes.  A chunk of the select is 256 instances (kMeterSelectChunk), and the scan is one workgroup of 256 lanes (kMeterScanWidth)
in which a lane owns ceil(chunks / 256) consecutive chunk counts: up to 256 x 256 = 65 536 instances a lane has at most one count,
and 65 537 is the smallest batch at which a lane loops over several.  N = 66 000 is such a batch whose shape is ragged as well: 258
chunks, lanes 0 .. 128 own two counts each and the others none, the last chunk 208 instances wide.  Below that: 1, 63, 64, 65 around a wavefront, 130 (two wavefronts
and a tail of two), 257 (a second chunk of one instance)."""
import numpy as np
import pytest

import fx8010_programs as progs
import meter_list_model as M
from test_meter_stub import meter_model, meter_zero

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SCAN_LOOPS = 66000   # > kMeterSelectChunk * kMeterScanWidth: a lane of the scan owns two counts


def program(channels):
    text = progs.config1_shipped().replace("macs out_l, 0, in_l, volume", "macw out_l, 0, in_l, volume")
    assert "macw" in text and text.endswith("\nend")
    more = "".join("input in%d %d\noutput out%d %d\n" % (c, c, c, c) for c in range(1, channels))
    code = "".join("macw out%d, 0, in%d, volume\n" % (c, c) for c in range(1, channels))
    return text[:-3].replace("macw out_l", more + "macw out_l", 1) + code + "end"


def handle(gpu, N, channels, devices=None, meters=True):
    b = gpu.Batch(N, channels, 0) if devices is None else gpu.Batch(N, channels, devices=devices)
    assert b.load_text(program(channels)), b.errors()
    if meters:
        assert b.meter_enable() == 0
    return b


@pytest.fixture(scope="module")
def lib(gpu):
    return gpu.load()


@pytest.mark.parametrize("channels", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 257])
def test_select_equals_the_numpy_model(gpu, lib, N, channels):
    """meters accumulated over two blocks of 16 + 17 samples; every stat, both directions, the thresholds, caps and ranges of
    meter_list_model.check_selects"""
    b = handle(gpu, N, channels)
    x = M.voices(N, channels, 33, seed=N)
    y = np.concatenate([b.process_block(x[:16]), b.process_block(x[16:])]).reshape(33, channels, N)
    rows = b.meter_read()
    assert M.same_rows(rows, meter_model(y)), "the meters are those of the output block"
    before = b.info("meter_selects")
    kinds = M.check_selects(lib, b, rows, N, "N=%d" % N)
    assert kinds >= (3 if N >= 63 else 2), "the thresholds gave match counts of several kinds"
    assert b.info("meter_selects") > before and M.same_rows(b.meter_read(), rows), "a select changes nothing"
    if N >= 63:
        assert rows["nonfinite"].max() >= 1 and rows["full_scale"].max() >= 1 and (rows["peak"].max(axis=0) == 0).any()
    b.close()


@pytest.mark.parametrize("channels", [1, 2])
def test_select_where_the_chunk_scan_loops(gpu, lib, channels):
    """N = 66 000 (module docstring), 8-sample blocks of the smallest program"""
    N = SCAN_LOOPS
    b = handle(gpu, N, channels)
    b.process_block(M.voices(N, channels, 8, seed=5))
    rows = b.meter_read()
    for stat in range(4):
        for t in M.thresholds(rows, stat):
            for below in (False, True):
                M.check_one(lib, b, rows, stat, t, below, 0, N, N)
    peak = M.value(rows, 1)
    for t, below in ((0.95, False), (0.2, True)):
        got, m = b.meter_select(gpu.METER_PEAK, t, below=below)
        assert np.array_equal(got, M.model(rows, 1, t, below)) and m == got.size and 0 < m < N // 2
    every64 = M.model(rows, 1, 0.85, False)
    assert every64.size >= N // 64 and np.isin(np.arange(0, N, 64)[(peak[::64] > 0)], every64).all()
    # caps that end in the first chunk, behind the 256th chunk, and in the last chunk; ranges that start and end there
    t = 0.5
    total = M.model(rows, 1, t, False).size
    for cap in (0, 1, 100, total - 1, total, total + 1, N + 5):
        M.check_one(lib, b, rows, 1, t, False, 0, N, cap)
    for first, n_range in ((65535, 3), (65536, N - 65536), (65537, 400), (255, 65300), (N - 1, 1), (N, 0), (1, N - 1)):
        M.check_one(lib, b, rows, 1, t, True, first, n_range, n_range)
        M.check_one(lib, b, rows, 3, 1.0, False, first, n_range, 5)
    b.close()


@pytest.mark.parametrize("channels", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 64, 257, SCAN_LOOPS])
def test_named_match_patterns_over_the_whole_batch(gpu, lib, N, channels):
    """none, all, only instance 0, only instance N - 1 (at 257 and 66 000 the single match sits in the last chunk and every chunk
    count in front of it is zero: the scan carries nothing, the emit of the last chunk starts at offset 0; BELOW, every count in
    front is full), every 64th: each ONE select over the whole batch, list and M asserted against the written-out list"""
    b = handle(gpu, N, channels)
    assert M.check_patterns(lib, b, N, channels) == 7
    b.close()


def test_read_list_and_its_reset(gpu, lib):
    N, channels = 257, 2
    rng = np.random.default_rng(7)
    b = handle(gpu, N, channels)
    b.process_block(M.voices(N, channels, 33, seed=1))
    rows = b.meter_read()
    for L in M.lists_of(rng, N) + [np.array([5, 5, 256, 0, 5], dtype=np.int64)]:
        assert M.same_rows(b.meter_read_list(L), M.columns(rows, L)), L[:8]
    # null arrays: only what is asked for is written
    L = np.array([256, 0, 130], dtype=np.int64)
    peak = np.full((channels, 3), -5.0, dtype=np.float32)
    assert lib.fxb_meter_read_list(b._h, L.ctypes.data, 3, None, peak.ctypes.data, None, None, 0) == 0
    assert np.array_equal(peak.view(np.uint32), rows["peak"][:, L].view(np.uint32))
    assert b.meter_read_list([])["energy"].shape == (channels, 0)
    # reset: exactly the listed columns, the values read are those in front of the zeroing
    samples, reads = b.meter_samples(), b.info("meter_list_reads")
    for L in M.lists_of(rng, N)[:5]:
        b.meter_reset_list(np.arange(N))
        b.sync()
        assert M.same_rows(b.meter_read(), meter_zero(channels, N))
        b.process_block(M.voices(N, channels, 17, seed=2))
        rows = b.meter_read()
        assert M.same_rows(b.meter_read_list(L, reset=True), M.columns(rows, L))
        assert M.same_rows(b.meter_read(), M.zeroed(rows, L)), "the listed columns are zero, no other has changed"
    assert b.info("meter_list_reads") == reads + 5 and b.meter_samples() == samples + 5 * 17, "the list calls leave the sample count alone"
    # refusals change nothing
    rows, seen = b.meter_read(), (b.info("meter_selects"), b.info("meter_list_reads"), b.info("meter_list_resets"))
    out = np.zeros((channels, 3), dtype=np.float64)
    for L, count, reset in ((np.array([1, 2, 1]), 3, 1), (np.array([0, N, 1]), 3, 0), (np.array([0, -1, 1]), 3, 0), (np.array([0, 1, 2]), -1, 0), (None, 2, 0)):
        held = None if L is None else np.ascontiguousarray(L, dtype=np.int64)
        p = None if held is None else held.ctypes.data
        assert lib.fxb_meter_read_list(b._h, p, count, out.ctypes.data, None, None, None, reset) == FX_E_ARG, (L, count)
        assert lib.fxb_meter_reset_list(b._h, p, count) == (0 if reset else FX_E_ARG), (L, count)   # (repeats are fine for a reset)
        b.sync()
    for stat, t, first, n_range, cap, flags, null in ((4, 0.0, 0, N, N, 0, False), (-1, 0.0, 0, N, N, 0, False), (1, np.nan, 0, N, N, 0, False), (1, 0.0, -1, 5, 5, 0, False),
                                                    (1, 0.0, 0, -1, 5, 0, False), (1, 0.0, 1, N, N, 0, False), (1, 0.0, 0, N, -1, 0, False), (1, 0.0, 0, N, N, 2, False), (1, 0.0, 0, N, 4, 0, True)):
        buf = np.full(N + 8, M.MARK, dtype=np.int64)
        got = lib.fxb_meter_select(b._h, stat, t, first, n_range, None if null else buf.ctypes.data, cap, flags)
        assert got == FX_E_ARG and b.last_error() and (buf == M.MARK).all(), (stat, t, first, n_range, cap, flags, null)
    assert lib.fxb_meter_select(b._h, 1, 0.0, 0, N, None, 0, 0) == N, "a count query takes a null list"
    want = M.zeroed(rows, [1, 2])
    assert M.same_rows(b.meter_read(), want) and (b.info("meter_selects"), b.info("meter_list_reads"), b.info("meter_list_resets")) == (seen[0] + 1, seen[1], seen[2] + 1)
    off = handle(gpu, N, channels, meters=False)
    assert lib.fxb_meter_select(off._h, 1, 0.0, 0, N, None, 0, 0) == FX_E_ARG and lib.fxb_meter_reset_list(off._h, L0.ctypes.data, 1) == FX_E_ARG
    assert lib.fxb_meter_read_list(off._h, L0.ctypes.data, 1, out.ctypes.data, None, None, None, 0) == FX_E_ARG and "metering is off" in off.last_error()
    off.close()
    b.close()


L0 = np.zeros(1, dtype=np.int64)


def test_reset_list_against_twins(gpu):
    """after the reset and one more block the listed columns equal the meters of a fresh handle that saw only that block, the
    others those of a handle that saw everything"""
    N, channels = 130, 2
    rng = np.random.default_rng(11)
    x1, x2 = M.voices(N, channels, 16, seed=3), M.voices(N, channels, 17, seed=4)[:, :, ::-1].copy()
    for L in M.lists_of(rng, N) + [np.array([7, 7, 129, 7], dtype=np.int64)]:
        b, everything, fresh = handle(gpu, N, channels), handle(gpu, N, channels), handle(gpu, N, channels)
        b.process_block(x1)
        assert b.meter_reset_list(L) == 0
        b.process_block(x2)
        everything.process_block(x1)
        everything.process_block(x2)
        fresh.process_block(x2)
        want, part = everything.meter_read(), fresh.meter_read()
        for k in M.FIELDS:
            want[k][:, L] = part[k][:, L]
        assert M.same_rows(b.meter_read(), want), L[:8]
        assert b.meter_samples() == 33 and b.info("meter_list_resets") == 1
        for h in (b, everything, fresh):
            h.close()


def test_reset_list_between_blocks_on_caller_streams(gpu, lib):
    """a device-entry block on stream A, reset_list with no sync, a block on stream B, then select and the reads: block 1 zeroed on
    L, plus block 2.  S = 2048 at N = 777: the first block is still running when the reset is queued"""
    import torch

    N, S, channels = 777, 2048, 1
    rng = np.random.default_rng(13)
    b = handle(gpu, N, channels)
    b.process_block(M.voices(N, channels, 8, seed=9))
    assert b.meter_read(reset=True) is not None
    blocks = [np.tile(M.voices(N, channels, 32, seed=20 + k), (S // 32, 1, 1)) for k in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = [torch.from_numpy(x).to("cuda") for x in blocks]
    d_out = [torch.full((S, channels, N), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    L = np.concatenate([[0, N - 1], rng.permutation(np.arange(1, N - 1))[:255]]).astype(np.int64)
    assert b.process_block_dev_pitched(d_in[0], d_out[0], S, stream=streams[0].cuda_stream) == 0
    assert b.meter_reset_list(L) == 0
    assert b.process_block_dev_pitched(d_in[1], d_out[1], S, stream=streams[1].cuda_stream) == 0
    got, m = b.meter_select(gpu.METER_ENERGY, 0.0, below=False, cap=0)   # (synchronous: it covers everything queued)
    y = [t.cpu().numpy() for t in d_out]
    want = meter_model(y[1], M.zeroed(meter_model(y[0]), L))
    rows = b.meter_read()
    assert M.same_rows(rows, want) and m == N and b.meter_samples() == 2 * S + 0
    assert not M.same_rows(rows, meter_model(y[1], meter_model(y[0]))) and not M.same_rows(rows, M.zeroed(want, L)), "the order matters to the words compared"
    M.check_selects(lib, b, rows, N, "streams")
    assert M.same_rows(b.meter_read_list(L), M.columns(want, L))
    b.close()


def test_bus_block_meters_selected_and_reset_and_the_loop_closed(gpu, lib):
    """meters produced by a bus block with a mixed output; then the loop the calls are for, once: select the voices that went
    non-finite, set their bus gains to zero by list, and the next mixed block has a finite bus"""
    N, K, S = 256, 64, 16
    b, twin = handle(gpu, N, 1), handle(gpu, N, 1, meters=False)
    x = M.voices(N, 1, S, seed=6)
    assert b.bus_set_gains(np.ones((1, N), dtype=np.float32)) == 0
    mix = b.process_block_bus(x, K, shared_in=False, mix_out=True)
    rows = b.meter_read()
    assert M.same_rows(rows, meter_model(twin.process_block(x))), "the per-instance block never left the device, and every voice has its figures"
    assert not np.isfinite(mix).all()
    M.check_selects(lib, b, rows, N, "bus")
    bad, m = b.meter_select(gpu.METER_NONFINITE, 1.0)
    assert m == bad.size > 0 and np.array_equal(bad, np.nonzero(rows["nonfinite"][0] >= 1)[0])
    assert b.bus_set_gains_list(bad, np.zeros((1, bad.size), dtype=np.float32)) == 0
    assert b.meter_reset_list(bad) == 0
    clean = x.copy()
    clean[:, :, bad] = np.where(np.isfinite(clean[:, :, bad]), clean[:, :, bad], np.float32(0.25))   # (0 x NaN is NaN: what a muted voice plays must be finite words, its level does not matter)
    mix = b.process_block_bus(clean, K, shared_in=False, mix_out=True)
    assert np.isfinite(mix).all(), "the muted voices are off the bus"
    after = b.meter_read()
    y = twin.process_block(clean)
    part = meter_model(y)
    want = meter_model(y, rows)
    for k in M.FIELDS:
        want[k][:, bad] = part[k][:, bad]
    assert M.same_rows(after, want) and b.meter_select(gpu.METER_NONFINITE, 1.0)[1] == 0
    b.close()
    twin.close()


def test_two_shards_on_one_gpu(gpu, lib):
    """fxb_create_on_devices with the ordinal twice, N = 130 + 130 instances - which the partition cuts at a multiple of 64,
    192 + 68: ranges across the border, caps inside shard 1, lists on both"""
    N, channels = 260, 2
    rng = np.random.default_rng(17)
    b, one = handle(gpu, N, channels, devices=[0, 0]), handle(gpu, N, channels)
    assert [(f, c) for _, f, c in b.shards()] == [(0, 192), (192, 68)]
    x = M.voices(N, channels, 33, seed=8)
    for h in (b, one):
        h.process_block(x[:16])
        h.process_block(x[16:])
    rows = one.meter_read()
    assert M.same_rows(b.meter_read(), rows)
    M.check_selects(lib, b, rows, N, "two shards")
    for first, n_range in ((100, 160), (191, 2), (192, 68), (0, 192), (191, 1), (193, 60)):
        for stat, t, below in ((1, 0.5, False), (1, 0.5, True), (0, 0.0, False), (3, 1.0, False)):
            want = M.check_one(lib, b, rows, stat, t, below, first, n_range, n_range)
            inside0 = int((want < 192).sum())
            for cap in {0, 1, inside0, inside0 + 1, max(want.size - 1, 0), want.size + 3}:   # a cap that ends inside shard 1
                M.check_one(lib, b, rows, stat, t, below, first, n_range, cap)
    before = b.info("meter_selects")
    b.meter_select(1, 0.5, first=200, n_range=20)
    assert b.info("meter_selects") == before + 1, "a shard whose part is empty launches nothing"
    for L in M.lists_of(rng, N) + [np.array([191, 192, 191, 259, 0], dtype=np.int64)]:
        assert M.same_rows(b.meter_read_list(L), M.columns(rows, L))
    L = np.array([200, 191, 192, 3], dtype=np.int64)
    assert M.same_rows(b.meter_read_list(L, reset=True), M.columns(rows, L)) and M.same_rows(b.meter_read(), M.zeroed(rows, L))
    rows = M.zeroed(rows, L)
    before = b.info("meter_list_resets")
    assert b.meter_reset_list([5, 6, 5]) == 0 and b.info("meter_list_resets") == before + 1, "a shard without an entry launches nothing"
    assert b.meter_reset_list([128, 258, 192]) == 0 and b.info("meter_list_resets") == before + 3
    assert M.same_rows(b.meter_read(), M.zeroed(rows, [5, 6, 128, 258, 192])) and b.meter_samples() == 33
    for h in (b, one):
        h.close()
