"""Gain sets by list on the GPU: fxb_bus_set_gains_list / _send_gains_list / _feed_gains_list - the kernel fx_gain_scatter - against
the state model of tests/test_bus_gain_list_stub.py (a, b and pending as include/fx8010_amd.h "Gain sets by list" defines them)
feeding the models of the bus gains, the sends and the feeds, on the output of a plain handle.  Bar: every word equal (where the
model is NaN the result is NaN), no tolerance anywhere, and all instance state afterwards equal to the plain handle's.  The shapes
are the smallest at which the kernel's indexing can go wrong: lists of 1, 64, 65 and all N entries (one lane, a whole wavefront,
one lane of a second workgroup, many workgroups), indices 0 and N - 1 always among them, one and two channels, and the three row
pitches - N, E, and the quad-padded pitch of feeds whose E is no multiple of 4."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_bus_feed_stub import feed_model, feed_structure
from test_bus_gain_list_stub import GainState
from test_bus_gain_stub import gain_mix_model, gains_for
from test_bus_send_stub import send_model
from test_bus_stub import expand, mix_model, same_words
from test_bus_tap_stub import same_bits
from test_gpu_bus import cutoffs, group_input, handles, program, register_names, same_state
from test_gpu_bus_feed import source_rows
from test_gpu_bus_gain import kernel_tier, right_tier  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FX_E_ARG = -3


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def a_list(rng, W, n):
    """n distinct indices of 0..W-1 in a shuffled order, 0 and W - 1 among them (n == 1: 0; n == W: all of them)"""
    if n >= W:
        return rng.permutation(W).astype(np.int64)
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    return rng.permutation(np.concatenate([[0, W - 1], rng.permutation(np.arange(1, W - 1))[:n - 2]])).astype(np.int64)


def values(rng, channels, W, n):
    return np.ascontiguousarray(gains_for(rng, channels, max(W, 19))[:, :n])   # (the specials of gains_for sit in the first 19 columns: +-0, denormals, +-1e30)


GRID = [("default", 5, 2, 1), ("default", 65, 64, 2), ("default", 200, 63, 1), ("default", 777, 130, 2), ("hip", 777, 130, 2), ("asm", 777, 130, 2)]


@pytest.mark.parametrize("kernel_tier,N,K,channels", GRID, indirect=["kernel_tier"], ids=["%s-N%d-K%d-C%d" % g for g in GRID])
def test_bus_gains_by_list_bit_exact(gpu, kernel_tier, N, K, channels):
    """a static full set, then blocks of 33, 1 and 2 samples with a list set in front of each - lists of 1, 64, 65 and N entries,
    the ramp sequence 1, 1 (pending twice with no block between), 0 while pending, 0, 1 - get after every set and every block"""
    rng = np.random.default_rng(7000 * N + K)
    text = program("config3", channels)
    names = register_names(gpu, text, channels)
    plain, b = handles(gpu, text, N, channels, 2)
    G = plain.bus_groups(K)
    g0 = gains_for(rng, channels, N)
    assert b.bus_set_gains(g0) == 0
    m = GainState(g0)
    clock, blocks, sets = 0, 0, 0

    def listed(n, ramp):
        nonlocal sets
        L = a_list(rng, N, min(n, N))
        g = values(rng, channels, N, L.size)
        assert b.bus_set_gains_list(L, g, ramp=bool(ramp)) == 0, b.last_error()
        m.listed(L, g, ramp)
        sets += 1
        assert same_bits(b.bus_get_gains(), m.in_force()), ("get after a list set", n, ramp)
        assert b.info("gain_list_sets") == sets

    def block(S):
        nonlocal clock, blocks
        xg = group_input(G, S, channels, clock)
        clock += S
        blocks += 1
        y = plain.process_block(expand(xg, K, N))
        a, bb, ramp = m.consume()
        assert same_words(b.process_block_bus(xg, K), gain_mix_model(y, a, bb, ramp, S, K)), "N %d K %d C %d S %d ramp %d block %d" % (N, K, channels, S, ramp, blocks)
        assert same_bits(b.bus_get_gains(), m.in_force()), "get after a block"

    block(33)   # the static full set
    sizes = (1, 64, 65, N)
    for round_, S in enumerate((33, 1, 2)):
        n = lambda k: sizes[(round_ + k) % 4]
        listed(n(0), 1)
        listed(n(1), 1)   # pending twice with no block between: a stays
        block(S)
        listed(n(2), 1)
        listed(n(3), 0)   # ramp = 0 while pending: the ramp stays pending for the others
        assert m.pending
        block(S)
        listed(n(1), 0)   # ramp = 0, none pending
        block(S)
        listed(n(3), 1)
        block(S)
    assert b.bus_set_gains_list([], np.zeros((channels, 0), dtype=np.float32), ramp=True) == 0 and b.info("gain_list_sets") == sets, "count 0 changes nothing"
    block(33)
    same_state(gpu, b, plain, names, sorted({0, min(63, N - 1), min(64, N - 1), N - 1}), tram=1000)
    assert b.info("bus_gain_blocks") == blocks and b.info("bus_blocks") == blocks and right_tier(b, kernel_tier)
    # refused, and nothing changes: a repeated index, an index of N, a value that is not finite
    lib = gpu.load()
    g = values(rng, channels, N, 2)
    for L in (np.array([0, 0], dtype=np.int64), np.array([0, N], dtype=np.int64)):
        assert lib.fxb_bus_set_gains_list(b._h, ptr(L), 2, ptr(g), 1) == FX_E_ARG
    bad = g.copy()
    bad[channels - 1, 1] = np.inf
    assert lib.fxb_bus_set_gains_list(b._h, ptr(np.array([0, N - 1], dtype=np.int64)), 2, ptr(bad), 0) == FX_E_ARG
    assert b.info("gain_list_sets") == sets and same_bits(b.bus_get_gains(), m.in_force())
    block(2)
    for h in (plain, b):
        h.close()


def test_send_gains_by_list_bit_exact(gpu):
    """N = 200, C = 2, three buses of 1, 64 and 1 030 entries (the last crosses the 1 024 chunk boundary); list sets that touch the
    entries at 0, 1 023, 1 024, 1 029 and E - 1 of the long bus and of the structure: ramp 1, ramp 1 again, ramp 0 while pending"""
    N, K, ch = 200, 63, 2
    rng = np.random.default_rng(71)
    text = program("config3", ch)
    names = register_names(gpu, text, ch)
    plain, b = handles(gpu, text, N, ch, 2)
    G = plain.bus_groups(K)
    off = np.array([0, 1, 65, 1095], dtype=np.int64)
    E = int(off[-1])
    mem = rng.integers(0, N, E).astype(np.int64)
    mem[[0, 1, 64, 65, E - 1]] = (N - 1, 0, N - 1, 0, N - 1)
    g0 = gains_for(rng, ch, E)
    assert b.bus_set_sends(off, mem, g0) == 0
    m = GainState(g0)
    long_bus = 65
    # (the entries 0, 1 023, 1 024, 1 029 and E - 1 counted from the head of the structure and from the head of the long bus)
    touched = np.unique(np.array([0, 1023, 1024, 1029, long_bus + 0, long_bus + 1023, long_bus + 1024, long_bus + 1029, E - 1], dtype=np.int64))
    clock = 0

    def listed(L, ramp):
        g = values(rng, ch, E, L.size)
        assert b.bus_set_send_gains_list(L, g, ramp=bool(ramp)) == 0, b.last_error()
        m.listed(L, g, ramp)
        assert same_bits(b.bus_get_sends()[2], m.in_force())

    def block(S):
        nonlocal clock
        xg = group_input(G, S, ch, clock)
        clock += S
        y = plain.process_block(expand(xg, K, N))
        a, bb, ramp = m.consume()
        out, aux = b.process_block_bus(xg, K, aux=True)
        assert same_words(out, mix_model(y, K)), "the group mix is unchanged"
        assert same_words(aux, send_model(y, off, mem, a, bb, ramp, S)), (S, ramp)
        assert same_bits(b.bus_get_sends()[2], m.in_force())

    block(33)
    listed(rng.permutation(touched), 1)
    listed(rng.permutation(np.unique(np.concatenate([touched, a_list(rng, E, 65)]))), 1)   # ramp 1 again: a stays (more than 64 entries: two workgroups)
    block(33)
    listed(a_list(rng, E, 64), 1)
    listed(touched, 0)       # ramp 0 while pending
    assert m.pending
    block(2)
    listed(touched[:1], 0)   # one entry, none pending
    block(1)
    listed(a_list(rng, E, E), 1)
    block(33)
    assert b.info("gain_list_sets") == 6 and b.info("bus_send_blocks") == 5
    same_state(gpu, b, plain, names, (0, 63, 64, N - 1), tram=1000)
    for h in (plain, b):
        h.close()


@pytest.mark.parametrize("form", ["lists", "map"])
def test_feed_gains_by_list_bit_exact(gpu, form):
    """N = 65, C = 2, 0 / 1 / 3 entries per instance, and the map form (one entry each): the feeds go from unweighted, so the gain
    rows have the quad-padded pitch, and E is no multiple of 4; lists hold the first and the last entry and an entry of the last
    instance"""
    N, M, ch = 65, 7, 2
    rng = np.random.default_rng(75 if form == "lists" else 79)   # (lists: E = 111)
    text = program("config3", ch)
    names = register_names(gpu, text, ch)
    plain, b = handles(gpu, text, N, ch, 2)
    off, src = feed_structure(rng, N, M, counts=(1,) if form == "map" else (0, 1, 3))
    E = int(off[-1])
    assert E % 4 != 0 and E >= 65, E
    assert b.bus_set_feeds(M, off, src) == 0
    ones = np.ones((ch, E), dtype=np.float32)
    m = GainState(ones)
    weighted = False
    clock = 0
    last = np.array([0, E - 1, int(off[N - 1])], dtype=np.int64)   # the first entry, the last one, the first of the last instance
    last = np.unique(last)

    def listed(L, ramp):
        nonlocal weighted
        g = values(rng, ch, E, L.size)
        assert b.bus_set_feed_gains_list(L, g, ramp=bool(ramp)) == 0, b.last_error()
        m.listed(L, g, ramp)
        weighted = True
        assert same_bits(b.bus_get_feeds()[3], m.in_force())

    def block(S):
        nonlocal clock
        x = source_rows(M, S, ch, clock)
        clock += S
        a, bb, ramp = m.consume()
        want = plain.process_block(feed_model(x, off, src, a, bb, ramp, S) if weighted else feed_model(x, off, src, None, None, False, S))
        assert same_words(b.process_block_bus_feed(x), want), (form, S, ramp)
        assert same_bits(b.bus_get_feeds()[3], m.in_force())

    block(33)                # unweighted
    assert b.bus_set_feed_gains_list([], np.zeros((ch, 0), dtype=np.float32)) == 0 and b.info("gain_list_sets") == 0
    block(2)                 # ... still
    listed(last, 1)          # from unweighted: weighted with a = b = 1.0f everywhere, then the ramp
    assert same_bits(b.bus_get_feeds()[3], ones)
    block(33)
    listed(a_list(rng, E, 64), 1)
    listed(a_list(rng, E, 65), 1)
    block(1)
    listed(a_list(rng, E, E), 1)
    listed(last, 0)          # ramp 0 while pending
    block(33)
    listed(last[-1:], 0)
    block(2)
    # ... and from unweighted without a ramp
    assert b.bus_set_feed_gains(None) == 0
    weighted, m = False, GainState(ones)
    block(2)
    listed(last, 0)
    block(33)
    assert b.info("gain_list_sets") == 7
    same_state(gpu, b, plain, names, (0, 63, 64), tram=1000)
    for h in (plain, b):
        h.close()


def test_list_sets_between_blocks_on_a_callers_stream(gpu):
    """a block on the caller's stream, a list set, a second block on the caller's stream, fxb_sync once: the first block has the old
    weights, the second the new ones - for the bus gains and for the send gains"""
    import torch

    text = progs.config3()
    N, S, K = 65536, 96, 64   # (a mix over 24 MiB behind a long emulation launch: the sets below overtake the blocks on the host)
    rng = np.random.default_rng(83)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    off = np.array([0, 1, 65, 1095], dtype=np.int64)
    E = int(off[-1])
    mem = rng.integers(0, N, E).astype(np.int64)
    g0, s0 = gains_for(rng, 1, N), gains_for(rng, 1, E)
    assert b.bus_set_gains(g0) == 0 and b.bus_set_sends(off, mem, s0) == 0
    mg, ms = GainState(g0), GainState(s0)
    stream = torch.cuda.Stream()
    blocks = [group_input(G, S, 1, k * S) for k in range(3)]
    ys = [plain.process_block(expand(xg, K, N)) for xg in blocks]
    d_in = [torch.from_numpy(xg).to("cuda") for xg in blocks]
    d_out = [torch.full((S, 1, G), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    d_aux = [torch.full((S, 1, 3), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    want = []

    def queue(k):
        assert b.process_block_bus_dev(d_in[k], d_out[k], S, K, stream=stream.cuda_stream, d_aux_out=d_aux[k]) == 0
        want.append((gain_mix_model(ys[k], *mg.consume(), S, K), send_model(ys[k], off, mem, *ms.consume(), S)))

    def listed(state, fn, W, n, ramp):
        L = a_list(rng, W, n)
        g = values(rng, 1, W, L.size)
        assert fn(L, g, ramp=bool(ramp)) == 0
        state.listed(L, g, ramp)

    queue(0)
    listed(mg, b.bus_set_gains_list, N, 1024, 0)
    listed(ms, b.bus_set_send_gains_list, E, 65, 0)
    queue(1)
    listed(mg, b.bus_set_gains_list, N, 65, 1)   # ... and a ramp by list behind them
    listed(ms, b.bus_set_send_gains_list, E, 64, 1)
    queue(2)
    assert b.sync() == 0
    for k in range(3):
        assert same_words(d_out[k].cpu().numpy(), want[k][0]), "block %d: the mix with the gains it was queued with" % k
        assert same_words(d_aux[k].cpu().numpy(), want[k][1]), "block %d: the aux rows with the send gains it was queued with" % k
    assert same_bits(b.bus_get_gains(), mg.in_force()) and same_bits(b.bus_get_sends()[2], ms.in_force()) and b.info("gain_list_sets") == 4
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)


@pytest.mark.parametrize("shards,N", [(2, 64 * 10 + 17), (3, 64 * 16 + 17)])
def test_sharded_handles_equal_the_single_one(gpu, shards, N):
    """shard starts at multiples of K, as tests/test_gpu_bus_gain.py chooses them; a list inside one shard starts a ramp"""
    text = program("config3", 2)
    names = register_names(gpu, text, 2)
    plan = gpu.shard_plan(N, shards)
    assert all(first % 192 == 0 for first, _ in plan), plan
    rng = np.random.default_rng(N + 1)
    S, K = 33, 64
    plain, one = handles(gpu, text, N, 2, 2)
    many = gpu.Batch(N, 2, devices=[0] * shards)
    g0 = gains_for(rng, 2, N)
    assert many.bus_set_gains(g0) == 0 and one.bus_set_gains(g0) == 0
    assert many.load_text(text), many.errors()
    assert many.set_register_array("cutoff", cutoffs(N)) == 0
    m = GainState(g0)
    G = many.bus_groups(K)
    first, count = plan[-1]
    inside = (first + rng.permutation(count)[:65]).astype(np.int64)   # wholly inside the last shard
    sets = 0
    for block, (L, ramp) in enumerate(((inside, 1), (a_list(rng, N, 130), 1), (inside, 0), (a_list(rng, N, N), 1))):
        g = values(rng, 2, N, L.size)
        if block == 2:   # ramp = 0 by a list inside one shard while a ramp of all shards is pending
            g2 = gains_for(rng, 2, N)
            for h in (many, one):
                assert h.bus_set_gains(g2, ramp=True) == 0
            m.full(g2, 1)
        for h in (many, one):
            assert h.bus_set_gains_list(L, g, ramp=bool(ramp)) == 0, h.last_error()
        m.listed(L, g, ramp)
        sets += 1
        assert same_bits(many.bus_get_gains(), m.in_force()) and same_bits(one.bus_get_gains(), m.in_force()), "get sees one state on all shards"
        xg = group_input(G, S, 2, block * S)
        y = plain.process_block(expand(xg, K, N))
        a, bb, pending = m.consume()
        want = one.process_block_bus(xg, K)
        assert same_words(want, gain_mix_model(y, a, bb, pending, S, K)), block
        assert same_words(many.process_block_bus(xg, K), want), block
        assert same_bits(many.bus_get_gains(), m.in_force())
    assert one.info("gain_list_sets") == sets and many.info("gain_list_sets") == 2 + 2 * shards, "a shard without an entry launches nothing"
    same_state(gpu, many, plain, names, (0, 63, 64, plan[1][0], N - 1), tram=1000)
    for h in (plain, one, many):
        h.close()
