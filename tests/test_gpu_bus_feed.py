"""Bus feeds on the GPU: fxb_process_block_bus_feed* against a second handle that runs the existing calls on the [S][C][N] block
feed_model builds - the definition of include/fx8010_amd.h "Bus feeds" as numpy, which tests/test_bus_feed_stub.py pins against
the sum written out one add at a time.  Words are compared as uint32: no tolerance anywhere; all instance state afterwards equal
to the plain handle's."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_bus_feed_stub import COUNTS, feed_model, feed_structure
from test_bus_gain_stub import gains_for
from test_bus_send_stub import structure
from test_bus_stub import mix_model, same_words
from test_bus_tap_stub import same_bits, signal
from test_gpu_bus import NONFINITE, cutoffs, group_input, handles, program, register_names, same_state
from test_gpu_bus_tap import kernel_tier, right_tier  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SHARED_IN, MIX_OUT = 1, 2


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def feeds_are(b, M, offsets, sources, gains):
    m, off, src, g = b.bus_get_feeds()
    return m == M and np.array_equal(off, offsets) and np.array_equal(src, sources) and same_bits(g, gains)


def channels_of(text, channels):
    """the mono configuration programs with further channels that go through their state"""
    if channels <= 2:
        return program_text(text, channels)
    assert text.endswith("\nend") and "static t" in text
    more = "".join("\ninput in%d %d\noutput out%d %d" % (c, c, c, c) for c in range(1, channels))
    return text[:-3].replace("output out 0", "output out 0" + more, 1) + "".join("macs out%d, in%d, t, 0.5\n" % (c, c) for c in range(1, channels)) + "end"


def program_text(text, channels):
    if channels == 1:
        return text
    return text[:-3].replace("output out 0", "output out 0\ninput in1 1\noutput out1 1", 1) + "macs out1, in1, t, 0.5\nend"


def source_rows(M, S, channels, clock):
    """the stimulus of the bus tests, with denormals and both zeros among its words: finite"""
    x = group_input(M, S, channels, clock)
    flat = x.reshape(-1).view(np.uint32)
    for k, word in enumerate((0x80000000, 0x00000001, 0x80000003, 0x00000000, 0x007fffff)):
        flat[(k * 5 + clock) % flat.size] = word
    return x


def first_difference(got, want, where):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: [sample, channel, column] %s of %d words, got %r want %r" % (where, bad[:4].tolist(), want.size, got[tuple(bad[0])], want[tuple(bad[0])])


GRID = [("default", 777, 1), ("default", 777, 2), ("default", 200, 3), ("hip", 200, 1), ("asm", 200, 1)]


@pytest.mark.parametrize("kernel_tier,N,channels", GRID, indirect=["kernel_tier"], ids=["%s-N%d-C%d" % g for g in GRID])
def test_feeds_bit_exact(gpu, kernel_tier, N, channels):
    """M = 1, 3 and 70 source columns; per-instance lists of 0, 1, 2, 5 and 65 entries, unsorted with repeats, instances 0 and
    N - 1 always fed; blocks of 33, 1 and 33 samples with state carried (rows in whole groups of the kernel's eight and a ragged
    rest; N = 777 and 200 leave the last wavefront ragged, and an odd N moves the 16-byte boundary from row to row), unweighted,
    with static gains (+-0.0 and a denormal among them), a ramp block and the block after it.  `out` unmixed and with
    FXB_BUS_MIX_OUT (K = 130) against a plain handle fed feed_model's block; then all instance state"""
    K = 130
    rng = np.random.default_rng(5000 * N + channels)
    text = channels_of(progs.config3(), channels)
    names = register_names(gpu, text, channels)
    plain, b, bm = handles(gpu, text, N, channels, 3)
    clock, blocks = 0, 0

    def block(S, M, off, src, a, bb, ramp):
        nonlocal clock, blocks
        x = source_rows(M, S, channels, clock)
        clock += S
        blocks += 1
        want_in = feed_model(x, off, src, a, bb, ramp, S)
        y = plain.process_block(want_in)
        where = "N %d C %d M %d S %d ramp %d weighted %d" % (N, channels, M, S, ramp, bb is not None)
        first_difference(b.process_block_bus_feed(x), y, where + ": out")
        assert same_words(bm.process_block_bus_feed(x, K, True), mix_model(y, K)), where + ": the mix"

    for M in (1, 3, 70):
        off, src = feed_structure(rng, N, M)
        count = np.diff(off)
        assert count[0] > 0 and count[N - 1] > 0 and set(count.tolist()) == set(COUNTS)
        E = int(off[-1])
        g0, g1 = gains_for(rng, channels, E), gains_for(rng, channels, E)
        assert (g0 == 0.0).any() and np.signbit(g0[g0 == 0.0]).any() and (np.abs(g0[g0 != 0.0]) < 2.0 ** -126).any()
        for h in (b, bm):
            assert h.bus_set_feeds(M, off, src) == 0 and feeds_are(h, M, off, src, np.ones((channels, E), dtype=np.float32)), h.last_error()
        block(33, M, off, src, None, None, False)
        block(1, M, off, src, None, None, False)
        block(33, M, off, src, None, None, False)
        for h in (b, bm):
            assert h.bus_set_feed_gains(g0) == 0 and feeds_are(h, M, off, src, g0)
        block(33, M, off, src, g0, g0, False)
        for h in (b, bm):
            assert h.bus_set_feed_gains(g1, True) == 0 and feeds_are(h, M, off, src, g0)
        block(33, M, off, src, g0, g1, True)
        assert feeds_are(b, M, off, src, g1)
        block(1, M, off, src, g1, g1, False)
    for h in (b, bm):
        same_state(gpu, h, plain, names, sorted({0, min(63, N - 1), min(64, N - 1), N - 1}), tram=1000)
        assert h.info("bus_feed_blocks") == blocks and h.info("bus_blocks") == blocks and right_tier(h, kernel_tier)
    for h in (plain, b, bm):
        h.close()


@pytest.mark.parametrize("K", [63, 64])
def test_the_map_n_over_k_is_the_shared_input(gpu, K):
    """M = G, sources[n] = n / K, unweighted - the map variant of the kernel - on words of every kind: NaNs of both signs with
    payloads, a signalling NaN, +-Inf.  `out` and state are those of FXB_BUS_SHARED_IN on every word"""
    N, S = 777, 33
    text = program("config3", 2)
    names = register_names(gpu, text, 2)
    rng = np.random.default_rng(7 + K)
    shared, b = handles(gpu, text, N, 2, 2)
    G = b.bus_groups(K)
    assert b.bus_set_feeds(G, np.arange(N + 1), np.arange(N) // K) == 0, b.last_error()
    for step, S_ in enumerate((S, 1, S)):
        x = signal(rng, (S_, 2, G))
        words = x.reshape(-1).view(np.uint32)
        for k, word in enumerate((0x7fc12345, 0xffc00001, 0x7f812345, 0xff800001, 0x7f800000, 0xff800000, 0x80000000)):
            words[(k * 11 + step) % words.size] = word
        mix = step == 2
        want = shared.process_block_bus(x, K, True, mix)
        got = b.process_block_bus_feed(x, K, mix)
        assert same_bits(got, want) if not mix else same_words(got, want), (K, step)
    same_state(gpu, b, shared, names, (0, 63, 64, N - 1), tram=1000)
    # the input words themselves, through a program that moves them: MACW does not saturate
    vol = cutoffs(N)
    shared, b = handles(gpu, NONFINITE, N, 1, 2, control="vol", values=vol)
    assert b.bus_set_feeds(G, np.arange(N + 1), np.arange(N) // K) == 0
    x = group_input(G, S, 1, 0)
    x[5, 0, 1 % G], x[9, 0, 2 % G], x[11, 0, G - 1] = 3.0, np.nan, -np.inf
    want = shared.process_block_bus(x, K, True, False)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert same_bits(b.process_block_bus_feed(x), want)


def test_a_zero_gain_keeps_a_nan_column_out_of_an_instance(gpu):
    """source column 1 is NaN throughout; instance 70 lists it with a gain of 0.0, instance 131 with -0.0: their input word is
    +0.0f + the rest, every other instance that lists it hears the NaN, and nobody else changes"""
    N, S, M = 300, 9, 3
    text = progs.config3()
    plain, b = handles(gpu, text, N, 1, 2)
    offsets = np.arange(0, 2 * N + 1, 2).astype(np.int64)
    sources = np.tile(np.array([0, 2], dtype=np.int64), N)
    for n in (70, 131, 200):
        sources[2 * n] = 1
    g = np.ones((1, 2 * N), dtype=np.float32)
    g[0, 2 * 70], g[0, 2 * 131] = 0.0, -0.0
    assert b.bus_set_feeds(M, offsets, sources, g) == 0
    x = group_input(M, S, 1, 0)
    x[:, 0, 1] = np.nan
    block = feed_model(x, offsets, sources, g, g, False, S)
    assert np.isnan(block[:, 0, 200]).all() and np.isfinite(np.delete(block, 200, axis=2)).all()
    assert same_bits(block[:, 0, 70], (np.float32(0.0) + x[:, 0, 2]).astype(np.float32)) and same_bits(block[:, 0, 131], block[:, 0, 70])
    assert same_words(b.process_block_bus_feed(x), plain.process_block(block))
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 70, 131, 200, N - 1), tram=1000)


def test_source_rows_pinned_pageable_device_and_on_a_second_stream(gpu):
    import torch

    text = progs.config3()
    N, S, K, M = 4133, 33, 64, 70
    rng = np.random.default_rng(31)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    off, src = feed_structure(rng, N, M)
    g = gains_for(rng, 1, int(off[-1]))
    assert b.bus_set_feeds(M, off, src, g) == 0
    xs = [source_rows(M, S, 1, k * S) for k in range(5)]
    ys = [plain.process_block(feed_model(x, off, src, g, g, False, S)) for x in xs[:3]]
    # pinned src and out: the mix stored in place, the source rows copied to the device all the same
    pin_src, pin_out = gpu.HostBuffer((S, 1, M)), gpu.HostBuffer((S, 1, G))
    pin_src.array[...] = xs[0]
    before = (b.info("host_staged_blocks"), b.info("host_inplace_blocks"))
    assert b.process_block_bus_feed(pin_src.array, K, True, out=pin_out.array) is pin_out.array
    assert (b.info("host_staged_blocks"), b.info("host_inplace_blocks")) == (before[0], before[1] + 1)
    assert same_words(pin_out.array, mix_model(ys[0], K)), "pinned"
    # pageable
    assert same_words(b.process_block_bus_feed(xs[1], K, True), mix_model(ys[1], K)), "pageable"
    # the device entry with a pinned src (copied on the stream)
    pin_src.array[...] = xs[2]
    pin_out.array[...] = -7.0
    assert b.process_block_bus_feed_dev(pin_src.array.ctypes.data, pin_out.array.ctypes.data, S, K, True) == 0 and b.sync() == 0, b.last_error()
    assert same_words(pin_out.array, mix_model(ys[2], K)), "device entry, pinned src"
    # device tensors on a second stream: two blocks back to back, then fxb_sync only
    plain2, b2 = handles(gpu, text, N, 1, 2)
    assert b2.bus_set_feeds(M, off, src, g) == 0
    ys2 = [plain2.process_block(feed_model(x, off, src, g, g, False, S)) for x in xs[3:5]]
    stream = torch.cuda.Stream()
    d_src = [torch.from_numpy(xs[k]).to("cuda") for k in (3, 4)]
    d_out = [torch.full((S, 1, G), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        assert b2.process_block_bus_feed_dev(d_src[k], d_out[k], S, K, True, stream=stream.cuda_stream) == 0, b2.last_error()
    assert b2.sync() == 0
    for k in range(2):
        assert same_words(d_out[k].cpu().numpy(), mix_model(ys2[k], K)), k
    assert b2.info("bus_feed_blocks") == 2 and b.info("bus_feed_blocks") == 3
    same_state(gpu, b2, plain2, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)


def test_feed_rows_of_the_two_pieces_of_a_block(gpu):
    """262 144 instances x 96 samples, mono, a short program: a per-instance block of 96 MiB, run in two pieces on the 64 MiB
    scratch, with a ramp of the feed gains pending: t goes by the sample of the call"""
    text = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
    N, S, M = 262144, 96, 70
    rng = np.random.default_rng(37)
    plain, b = handles(gpu, text, N, 1, 2, control="vol")
    off, src = feed_structure(rng, N, M, counts=(0, 1, 2))
    E = int(off[-1])
    g0, g1 = gains_for(rng, 1, E), gains_for(rng, 1, E)
    assert b.bus_set_feeds(M, off, src, g0) == 0 and b.bus_set_feed_gains(g1, True) == 0
    x = source_rows(M, S, 1, 0)
    y = plain.process_block(feed_model(x, off, src, g0, g1, True, S))
    first_difference(b.process_block_bus_feed(x), y, "two pieces, ramping")
    assert b.info("bus_feed_blocks") == 1 and b.info("bus_blocks") == 1 and feeds_are(b, M, off, src, g1)


def test_refusals_and_a_sharded_handle_equals_the_single_one(gpu):
    lib = gpu.load()
    text = program("config3", 2)
    N, S, K, M = 64 * 16 + 17, 9, 64, 7
    rng = np.random.default_rng(41)
    plain, b = handles(gpu, text, N, 2, 2)
    many = gpu.Batch(N, 2, devices=[0, 0, 0])
    G = b.bus_groups(K)
    off, src = feed_structure(rng, N, M)
    E = int(off[-1])
    g, g1 = gains_for(rng, 2, E), gains_for(rng, 2, E)
    ps, po, pn = gpu.HostBuffer((S, 2, M)), gpu.HostBuffer((S, 2, G)), gpu.HostBuffer((S, 2, N))
    both = gpu.HostBuffer((4 * S, 2, N))
    ps.array[...] = source_rows(M, S, 2, 0)
    pn.array[...] = -7.0
    at = lambda h, o: C.c_void_p(h.array.ctypes.data + o * 4)
    host = lambda x, y, n, k, flags: lib.fxb_process_block_bus_feed(b._h, ptr(x), ptr(y), None, None, n, k, flags)
    dev = lambda x, y, n, k, flags: lib.fxb_process_block_bus_feed_dev(b._h, ptr(x), ptr(y), None, None, n, k, flags, None)
    assert host(ps.array, pn.array, S, K, 0) == FX_E_ARG and "feeds are off" in b.last_error()
    assert lib.fxb_bus_set_feed_gains(b._h, ptr(g), 0) == FX_E_ARG
    bad_source, bad_gain, down = src.copy(), g.copy(), off.copy()
    bad_source[E - 1], bad_gain[0, 7], down[3] = M, np.nan, off[4] + 1
    sets = [lib.fxb_bus_set_feeds(b._h, M, ptr(off), ptr(bad_source), ptr(g)), lib.fxb_bus_set_feeds(b._h, M, ptr(off), ptr(src), ptr(bad_gain)),
            lib.fxb_bus_set_feeds(b._h, M, ptr(down), ptr(src), None), lib.fxb_bus_set_feeds(b._h, -1, ptr(off), ptr(src), None),
            lib.fxb_bus_set_feeds(b._h, M, None, ptr(src), None), lib.fxb_bus_set_feeds(b._h, 1 << 29, ptr(off), ptr(src), None)]
    assert sets == [FX_E_ARG] * len(sets) and b.bus_get_feeds()[0] == 0, sets
    assert many.bus_set_feeds(M, off, src, g) == 0   # (before the program is loaded)
    assert many.load_text(text) and many.set_register_array("cutoff", cutoffs(N)) == 0, many.errors()
    assert b.bus_set_feeds(M, off, src, g) == 0
    rows = S * 2 * M
    refused = [
        host(ps.array, pn.array, S, K, SHARED_IN), dev(ps.array, po.array, S, K, 3), host(ps.array, pn.array, S, K, 4), host(None, pn.array, S, K, 0),
        host(ps.array, None, S, K, 0), host(ps.array, pn.array, -1, K, 0), host(ps.array, po.array, S, 0, MIX_OUT),
        lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, 0), None, None, S, K, 0),
        lib.fxb_process_block_bus_feed(b._h, at(both, 0), at(both, rows - 1), None, None, S, K, 0),
        lib.fxb_process_block_bus_feed(b._h, ptr(ps.array), ptr(po.array), ptr(pn.array), None, S, K, MIX_OUT),   # (taps are off)
        dev(np.zeros((S, 2, M), dtype=np.float32), po.array, S, K, MIX_OUT),   # (a pageable d_src: the device cannot address it)
        lib.fxb_process_block_bus_feed_dev(many._h, ptr(ps.array), ptr(po.array), None, None, S, K, MIX_OUT, None),   # (several shards)
        lib.fxb_bus_set_feed_gains(b._h, ptr(bad_gain), 1),
    ]
    assert refused == [FX_E_ARG] * len(refused), refused
    assert (pn.array == -7.0).all() and feeds_are(b, M, off, src, g) and b.info("bus_blocks") == 0 and b.info("bus_feed_blocks") == 0
    # the next blocks are right, on the single handle and on three shards: host entry in place and staged, then with a ramp
    for step, route in enumerate(("pinned", "pageable", "ramp")):
        x = source_rows(M, S, 2, step * S)
        if route == "ramp":
            assert b.bus_set_feed_gains(g1, True) == 0 and many.bus_set_feed_gains(g1, True) == 0
        y = plain.process_block(feed_model(x, off, src, g, g1 if route == "ramp" else g, route == "ramp", S))
        if route == "pinned":
            ps.array[...] = x
            assert host(ps.array, po.array, S, K, MIX_OUT) == 0 and same_words(po.array, mix_model(y, K)), b.last_error()
            assert lib.fxb_process_block_bus_feed(many._h, ptr(ps.array), ptr(po.array), None, None, S, K, MIX_OUT) == 0 and same_words(po.array, mix_model(y, K)), many.last_error()
        else:
            first_difference(b.process_block_bus_feed(x), y, route)
            first_difference(many.process_block_bus_feed(x), y, route + ", three shards")
    assert feeds_are(many, M, off, src, g1) and many.info("bus_feed_blocks") == 3 * 3
    names = register_names(gpu, text, 2)
    same_state(gpu, b, plain, names, (0, 63, 64, N - 1), tram=1000)
    same_state(gpu, many, plain, names, (0, 63, 64, N - 1), tram=1000)


def test_a_send_effect_return_chain_stays_on_the_device(gpu):
    """handle A's aux rows in device memory are handle B's source rows, in the same stream, without a host copy: the result is
    the two-step host version's"""
    import torch

    text = progs.config3()
    NA, NB, S, K, A = 777, 200, 33, 64, 5
    rng = np.random.default_rng(43)
    a_host, a_dev = handles(gpu, text, NA, 1, 2)
    b_host, b_dev = handles(gpu, text, NB, 1, 2)
    soff, smem = structure(rng, NA, (65, 3, 0, 130, 1))
    sg = gains_for(rng, 1, int(soff[-1]), special=False)
    foff, fsrc = feed_structure(rng, NB, A, counts=(1, 2))
    fg = gains_for(rng, 1, int(foff[-1]))
    for h in (a_host, a_dev):
        assert h.bus_set_sends(soff, smem, sg) == 0
    for h in (b_host, b_dev):
        assert h.bus_set_feeds(A, foff, fsrc, fg) == 0
    stream = torch.cuda.Stream()
    GA, GB = a_dev.bus_groups(K), b_dev.bus_groups(K)
    for step in range(2):
        xa = group_input(GA, S, 1, step * S)
        # two steps on the host
        mix_a, aux = a_host.process_block_bus(xa, K, True, True, aux=True)
        want = b_host.process_block_bus_feed(aux, K, True)
        # one stream on the device
        d_in = torch.from_numpy(xa).to("cuda")
        d_mix = torch.empty((S, 1, GA), dtype=torch.float32, device="cuda")
        d_aux = torch.full((S, 1, A), -7.0, dtype=torch.float32, device="cuda")
        d_out = torch.full((S, 1, GB), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert a_dev.process_block_bus_dev(d_in, d_mix, S, K, stream=stream.cuda_stream, d_aux_out=d_aux) == 0, a_dev.last_error()
        assert b_dev.process_block_bus_feed_dev(d_aux, d_out, S, K, True, stream=stream.cuda_stream) == 0, b_dev.last_error()
        assert b_dev.sync() == 0 and a_dev.sync() == 0
        assert same_words(d_mix.cpu().numpy(), mix_a) and same_words(d_aux.cpu().numpy(), aux) and same_words(d_out.cpu().numpy(), want), step
    same_state(gpu, b_dev, b_host, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, NB - 1), tram=1000)
