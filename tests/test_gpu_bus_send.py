"""Bus sends on the GPU: fxb_process_block_bus_aux* against a second handle that runs fxb_process_block on the expanded input (y;
tests/test_gpu_bus.py pins that against the oracle).  The aux rows must be send_model of y - the definition of
include/fx8010_amd.h "Bus sends" as numpy, which tests/test_bus_send_stub.py pins against the group mix - the mix what mix_model /
gain_mix_model of y give and the taps y[:, :, list].  Words are compared as uint32: no tolerance anywhere; all instance state
afterwards equal to the plain handle's."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_bus_gain_stub import gain_mix_model, gains_for
from test_bus_send_stub import send_model, structure
from test_bus_stub import expand, mix_model, same_words
from test_bus_tap_stub import same_bits, tap_list
from test_gpu_bus import NONFINITE, cutoffs, group_input, handles, program, register_names, same_state
from test_gpu_bus_feed import channels_of
from test_gpu_bus_tap import kernel_tier, right_tier  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SHARED_IN, MIX_OUT = 1, 2
# the lane boundary, the chunk boundary, Q = 2 and Q = 3 with a one-entry last chunk, and Q = 65: the fold's second 64-lane step
SIZES = (0, 1, 63, 64, 65, 1024, 1025, 2049, 65537)


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def sends_are(b, offsets, members, gains):
    off, mem, g = b.bus_get_sends()
    return np.array_equal(off, offsets) and np.array_equal(mem, members) and same_bits(g, gains)


GRID = [("default", 777, 130, 1), ("default", 777, 130, 2), ("hip", 200, 63, 1), ("asm", 200, 63, 1)]


@pytest.mark.parametrize("kernel_tier,N,K,channels", GRID, indirect=["kernel_tier"], ids=["%s-N%d-K%d-C%d" % g for g in GRID])
def test_sends_bit_exact(gpu, kernel_tier, N, K, channels):
    """blocks of 33, 1 and 33 samples with state carried (rows in whole groups of the kernel's eight and a ragged rest) on one
    structure of buses of 0 .. 65 537 entries - unsorted lists with repeats, the first and the last instance in every non-empty
    one - with static gains (+-0.0 and a denormal among them), a ramp block with taps beside it and the block after it; then a
    structure of 65 short buses, across the fold's 64-bus block boundary"""
    rng = np.random.default_rng(3000 * N + K + channels)
    text = program("config3", channels)
    names = register_names(gpu, text, channels)
    plain, b = handles(gpu, text, N, channels, 2)
    G = plain.bus_groups(K)
    offsets, members = structure(rng, N, SIZES)
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        assert hi == lo or (N - 1 in members[lo:hi] and (hi - lo < 2 or 0 in members[lo:hi]))
    E = int(offsets[-1])
    g0, g1, g2 = gains_for(rng, channels, E), gains_for(rng, channels, E), gains_for(rng, channels, E)
    assert (g0 == 0.0).any() and np.signbit(g0[g0 == 0.0]).any() and (np.abs(g0[g0 != 0.0]) < 2.0 ** -126).any()
    taps = tap_list(rng, N, 65)
    assert b.bus_set_sends(offsets, members, g0) == 0 and sends_are(b, offsets, members, g0) and b.bus_set_taps(taps) == 0
    clock = 0

    def block(S, off, mem, a, bb, ramp, tapped=False):
        nonlocal clock
        xg = group_input(G, S, channels, clock)
        clock += S
        y = plain.process_block(expand(xg, K, N))
        got = b.process_block_bus(xg, K, True, True, taps=tapped, aux=True)
        where = "N %d K %d C %d S %d ramp %d" % (N, K, channels, S, ramp)
        assert same_words(got[0], mix_model(y, K)), where + ": the mix"
        if tapped:
            assert same_bits(got[1], y[:, :, taps]), where + ": the taps"
        want = send_model(y, off, mem, a, bb, ramp, S)
        bad = np.argwhere(got[-1].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, where + ": aux [sample, channel, bus] %s of %d words, got %r want %r" % (bad[:4].tolist(), want.size, got[-1][tuple(bad[0])], want[tuple(bad[0])])

    block(33, offsets, members, g0, g0, False)
    block(1, offsets, members, g0, g0, False)
    assert b.bus_set_send_gains(g1, True) == 0 and sends_are(b, offsets, members, g0)
    block(33, offsets, members, g0, g1, True, tapped=True)
    assert sends_are(b, offsets, members, g1)
    block(33, offsets, members, g1, g1, False)
    assert b.bus_set_send_gains(g2, True) == 0
    block(1, offsets, members, g1, g2, True)   # a ramp of one sample is its target
    off2, mem2 = structure(rng, N, (3, 1, 2, 70, 5) * 13)
    h0, h1 = gains_for(rng, channels, int(off2[-1])), gains_for(rng, channels, int(off2[-1]))
    assert b.bus_set_sends(off2, mem2, h0) == 0
    block(33, off2, mem2, h0, h0, False, tapped=True)
    assert b.bus_set_send_gains(h1, True) == 0
    block(33, off2, mem2, h0, h1, True)
    block(1, off2, mem2, h1, h1, False)
    same_state(gpu, b, plain, names, sorted({0, min(63, N - 1), min(64, N - 1), N - 1}), tram=1000)
    assert b.info("bus_send_blocks") == 8 and b.info("bus_blocks") == 8 and b.info("bus_tap_blocks") == 2 and right_tier(b, kernel_tier)
    for h in (plain, b):
        h.close()


def test_sends_at_three_channels_and_a_bus_of_257_chunks(gpu):
    """N = 200, K = 63, three channels - the send kernel's frame of one gain row per row, for channel counts other than 1 and 2 -
    and buses of 0, 1, 1 025 and 262 145 entries: 262 145 = 256 * 1 024 + 1 is 257 chunks, the second 256-chunk step of the fold's
    walk, with a one-entry last chunk.  A block of 3 samples is nine rows: one full group of the kernel's eight and a ragged one.
    Static gains, then a ramp"""
    N, K, channels, S = 200, 63, 3, 3
    rng = np.random.default_rng(47)
    text = channels_of(progs.config3(), channels)
    plain, b = handles(gpu, text, N, channels, 2)
    G = plain.bus_groups(K)
    offsets, members = structure(rng, N, (0, 1, 1025, 262145))
    E = int(offsets[-1])
    g0, g1 = gains_for(rng, channels, E), gains_for(rng, channels, E)
    assert b.bus_set_sends(offsets, members, g0) == 0 and sends_are(b, offsets, members, g0)
    for step, ramp in enumerate((False, True)):
        if ramp:
            assert b.bus_set_send_gains(g1, True) == 0
        xg = group_input(G, S, channels, step * S)
        y = plain.process_block(expand(xg, K, N))
        out, aux = b.process_block_bus(xg, K, True, True, aux=True)
        assert same_words(out, mix_model(y, K)), "ramp %d: the mix" % ramp
        want = send_model(y, offsets, members, g0, g1 if ramp else g0, ramp, S)
        bad = np.argwhere(aux.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, "ramp %d: aux [sample, channel, bus] %s of %d words, got %r want %r" % (ramp, bad[:4].tolist(), want.size, aux[tuple(bad[0])], want[tuple(bad[0])])
    assert sends_are(b, offsets, members, g1) and b.info("bus_send_blocks") == 2 and b.info("bus_blocks") == 2
    same_state(gpu, b, plain, register_names(gpu, text, channels), (0, 63, 64, N - 1), tram=1000)
    for h in (plain, b):
        h.close()


def test_sends_are_pre_fader_and_a_zero_send_mutes(gpu):
    """MACW does not saturate: an instance fed NaN and one fed Inf put non-finite words on their outputs.  A bus gain of 0 keeps
    them off `out` while an aux bus with send gain 1 carries non-finite words; with send gains of 0.0 / -0.0 the aux bus is finite
    and is the model's"""
    N, S, K = 1000, 33, 64
    vol = cutoffs(N)
    plain, b = handles(gpu, NONFINITE, N, 1, 2, control="vol", values=vol)
    nan_fed, inf_fed = 70, 131
    rng = np.random.default_rng(29)
    g = gains_for(rng, 1, N, special=False)
    g[0, nan_fed], g[0, inf_fed] = 0.0, -0.0
    offsets = np.array([0, N, N + 4], dtype=np.int64)
    members = np.concatenate([rng.permutation(N), [inf_fed, 0, nan_fed, N - 1]]).astype(np.int64)
    ones = np.ones((1, N + 4), dtype=np.float32)
    assert b.bus_set_gains(g) == 0 and b.bus_set_sends(offsets, members) == 0
    for step in range(2):
        x = expand(group_input(plain.bus_groups(K), S, 1, step * S), K, N)
        x[:, 0, nan_fed] = np.nan
        x[:, 0, inf_fed] = np.inf
        y = plain.process_block(x)
        bad = ~np.isfinite(y[:, 0, :])
        assert bad[:, nan_fed].any() and bad[:, inf_fed].any() and not np.delete(bad, (nan_fed, inf_fed), axis=1).any()
        out, aux = b.process_block_bus(x, K, False, True, aux=True)
        assert np.isfinite(out).all() and same_words(out, gain_mix_model(y, g, g, False, S, K)), "a muted voice reached the bus"
        if step == 0:
            assert not np.isfinite(aux[:, 0, 0]).all() and not np.isfinite(aux[:, 0, 1]).all(), "pre-fader: the bus gains do not act on the sends"
            assert same_words(aux, send_model(y, offsets, members, ones, ones, False, S))
            sg = gains_for(rng, 1, N + 4, special=False)
            sg[0, members == nan_fed], sg[0, members == inf_fed] = 0.0, -0.0
            assert b.bus_set_send_gains(sg) == 0
        else:
            assert np.isfinite(aux).all(), "a send gain of zero keeps a voice off the aux bus"
            assert same_words(aux, send_model(y, offsets, members, sg, sg, False, S)) and (aux != 0.0).any()
    same_state(gpu, b, plain, ["a", "t", "out", "ccr"], (0, 63, 64, nan_fed, inf_fed, N - 1))


def test_aux_rows_pinned_pageable_and_on_a_second_stream(gpu):
    import torch

    text = progs.config3()
    N, S, K = 4133, 33, 64
    rng = np.random.default_rng(31)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    offsets, members = structure(rng, N, (65, 2049, 0, 1))
    A = offsets.size - 1
    g = gains_for(rng, 1, int(offsets[-1]))
    taps = tap_list(rng, N, 5)
    assert b.bus_set_sends(offsets, members, g) == 0 and b.bus_set_taps(taps) == 0
    blocks = [group_input(G, S, 1, k * S) for k in range(4)]
    ys = [plain.process_block(expand(xg, K, N)) for xg in blocks]
    want = [send_model(y, offsets, members, g, g, False, S) for y in ys]
    # pinned: everything in place, the aux rows stored over PCIe
    pin_in, pin_out, pin_aux = gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, A))
    pin_in.array[...] = blocks[0]
    pin_aux.array[...] = -7.0
    before = (b.info("host_staged_blocks"), b.info("host_inplace_blocks"))
    out, aux = b.process_block_bus(pin_in.array, K, out=pin_out.array, aux_out=pin_aux.array)
    assert out is pin_out.array and aux is pin_aux.array
    assert (b.info("host_staged_blocks"), b.info("host_inplace_blocks")) == (before[0], before[1] + 1)
    assert same_words(out, mix_model(ys[0], K)) and same_words(aux, want[0]), "pinned"
    # pageable: staged
    out, tp, aux = b.process_block_bus(blocks[1], K, taps=True, aux=True)
    assert (b.info("host_staged_blocks"), b.info("host_inplace_blocks")) == (before[0] + 1, before[1] + 1)
    assert same_words(out, mix_model(ys[1], K)) and same_bits(tp, ys[1][:, :, taps]) and same_words(aux, want[1]), "pageable"
    # device tensors on a second stream: two blocks back to back, then fxb_sync only
    stream = torch.cuda.Stream()
    d_in = [torch.from_numpy(blocks[k]).to("cuda") for k in (2, 3)]
    d_out = [torch.full((S, 1, G), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    d_aux = [torch.full((S, 1, A), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        assert b.process_block_bus_dev(d_in[k], d_out[k], S, K, stream=stream.cuda_stream, d_aux_out=d_aux[k]) == 0
    assert b.sync() == 0
    for k in range(2):
        assert same_words(d_out[k].cpu().numpy(), mix_model(ys[2 + k], K)), k
        assert same_words(d_aux[k].cpu().numpy(), want[2 + k]), k
    assert b.info("bus_send_blocks") == 4 and b.info("bus_blocks") == 4 and b.info("bus_tap_blocks") == 1
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)


def test_aux_rows_of_the_two_pieces_of_a_block(gpu):
    """262 144 instances x 96 samples, mono, a short program: a per-instance block of 96 MiB, run in two pieces on the 64 MiB
    scratch; each piece delivers its rows - of one bus of all instances (Q = 256) and one of 65"""
    text = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
    N, S, K = 262144, 96, 64
    rng = np.random.default_rng(37)
    plain, b = handles(gpu, text, N, 1, 2, control="vol")
    G = b.bus_groups(K)
    offsets = np.array([0, N, N + 65], dtype=np.int64)
    members = np.concatenate([np.arange(N), tap_list(rng, N, 65)]).astype(np.int64)
    g = gains_for(rng, 1, N + 65)
    assert b.bus_set_sends(offsets, members, g) == 0
    xg = group_input(G, S, 1, 0)
    y = plain.process_block(expand(xg, K, N))
    out, aux = b.process_block_bus(xg, K, aux=True)
    assert same_words(aux, send_model(y, offsets, members, g, g, False, S)) and same_words(out, mix_model(y, K))
    assert b.info("bus_send_blocks") == 1 and b.info("bus_blocks") == 1


def test_refusals_and_the_block_behind_them(gpu):
    lib = gpu.load()
    text = progs.config3()
    N, S, K = 300, 8, 64
    rng = np.random.default_rng(41)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    offsets, members = structure(rng, N, (65, 0, 1025))
    A, E = offsets.size - 1, int(offsets[-1])
    g = gains_for(rng, 1, E)
    xg = gpu.HostBuffer((S, 1, G))
    yg, yn, pa = gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, N)), gpu.HostBuffer((S, 1, A))
    both = gpu.HostBuffer((4 * S, 1, N))
    xg.array[...] = group_input(G, S, 1, 0)
    pa.array[...] = -7.0
    page = np.full((S, 1, A), -7.0, dtype=np.float32)
    at = lambda h, off: C.c_void_p(h.array.ctypes.data + off * 4)
    host = lambda x, y, a, n, k, flags: lib.fxb_process_block_bus_aux(b._h, ptr(x), ptr(y), None, ptr(a), n, k, flags)
    dev = lambda x, y, a, n, k, flags: lib.fxb_process_block_bus_aux_dev(b._h, ptr(x), ptr(y), None, ptr(a), n, k, flags, None)
    assert host(xg.array, yg.array, pa.array, S, K, 3) == FX_E_ARG and "sends are off" in b.last_error()
    assert lib.fxb_bus_set_send_gains(b._h, ptr(g), 0) == FX_E_ARG
    bad_member, bad_gain = members.copy(), g.copy()
    bad_member[E - 1], bad_gain[0, 7] = N, np.nan
    down = np.array([0, 5, 4, 6], dtype=np.int64)
    assert lib.fxb_bus_set_sends(b._h, A, ptr(offsets), ptr(bad_member), ptr(g)) == FX_E_ARG and lib.fxb_bus_set_sends(b._h, A, ptr(offsets), ptr(members), ptr(bad_gain)) == FX_E_ARG
    assert lib.fxb_bus_set_sends(b._h, 3, ptr(down), ptr(members), None) == FX_E_ARG and lib.fxb_bus_set_sends(b._h, 65537, ptr(offsets), ptr(members), None) == FX_E_ARG
    assert lib.fxb_bus_set_sends(b._h, A, None, ptr(members), None) == FX_E_ARG and lib.fxb_bus_set_sends(b._h, -1, ptr(offsets), ptr(members), None) == FX_E_ARG
    assert b.bus_get_sends()[1].size == 0
    assert b.bus_set_sends(offsets, members, g) == 0
    rows = S * A
    refused = [
        host(xg.array, yn.array, pa.array, S, K, SHARED_IN), dev(xg.array, yn.array, pa.array, S, K, SHARED_IN), host(yn.array, yn.array, pa.array, S, K, 0),
        lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, S * N - 1), S, K, MIX_OUT),
        lib.fxb_process_block_bus_aux(b._h, at(both, rows - 1), at(both, 2 * S * N), None, at(both, 0), S, K, MIX_OUT),
        lib.fxb_process_block_bus_aux(b._h, at(both, 0), at(both, 2 * S * N), None, at(both, 2 * S * N + S * G - 1), S, K, MIX_OUT),
        host(xg.array, yg.array, pa.array, S, 0, 3), host(xg.array, yg.array, pa.array, S, K, 7), host(None, yg.array, pa.array, S, K, 3),
        host(xg.array, yg.array, pa.array, -1, K, 3),
        dev(xg.array, yg.array, page, S, K, 3),   # (pageable rows: the device cannot address them)
        lib.fxb_bus_set_send_gains(b._h, ptr(bad_gain), 1),
    ]
    assert refused == [FX_E_ARG] * len(refused), refused
    many = gpu.Batch(N, 1, devices=[0, 0])
    assert many.load_text(text) and many.bus_set_sends([0, 2], [1, 2]) == 0
    assert lib.fxb_process_block_bus_aux_dev(many._h, ptr(xg.array), ptr(yg.array), None, ptr(pa.array), S, K, 3, None) == FX_E_ARG
    assert (pa.array == -7.0).all() and (page == -7.0).all() and sends_are(b, offsets, members, g)
    assert b.info("bus_blocks") == 0 and b.info("bus_send_blocks") == 0
    # the next block with aux rows is right: host entry, then the device entry on the handle's stream
    for call in (host, dev):
        y = plain.process_block(expand(xg.array, K, N))
        assert call(xg.array, yg.array, pa.array, S, K, 3) == 0 and b.sync() == 0, b.last_error()
        assert same_words(yg.array, mix_model(y, K)) and same_words(pa.array, send_model(y, offsets, members, g, g, False, S))
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)


def test_sharded_handle_equals_the_single_one(gpu):
    """three shards on one device: buses on every shard, interleaved, then a structure that leaves the middle shard without one,
    on pinned rows (every shard stores its columns in place) and on pageable ones; a bus across two shards is refused"""
    text = program("config3", 2)
    N, S, K = 64 * 16 + 17, 9, 64
    plan = gpu.shard_plan(N, 3)
    rng = np.random.default_rng(43)
    plain = handles(gpu, text, N, 2, 1)[0]
    many = gpu.Batch(N, 2, devices=[0, 0, 0])
    bounds = [(plan[k][0], plan[k + 1][0] if k < 2 else N) for k in range(3)]

    def build(spec):
        lists = []
        for shard, M in spec:
            lo, hi = bounds[shard]
            lst = rng.integers(lo, hi, M)
            lst[:2] = (hi - 1, lo)[:M]
            lists.append(lst.astype(np.int64))
        return np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.int64), np.concatenate(lists).astype(np.int64)

    structures = (build([(2, 65), (0, 1025), (1, 3), (0, 0), (2, 2049), (1, 64)]), build([(2, 5), (0, 70), (2, 1)]))
    assert many.bus_set_sends(*structures[0]) == 0   # (before the program is loaded)
    assert many.load_text(text), many.errors()
    assert many.set_register_array("cutoff", cutoffs(N)) == 0
    G = many.bus_groups(K)
    for block, (offsets, members) in enumerate(structures):
        E = int(offsets[-1])
        g, g1 = gains_for(rng, 2, E), gains_for(rng, 2, E)
        assert many.bus_set_sends(offsets, members, g) == 0 and sends_are(many, offsets, members, g)
        for route in ("pinned", "pageable"):
            xg = group_input(G, S, 2, (2 * block + (route == "pageable")) * S)
            y = plain.process_block(expand(xg, K, N))
            pin = gpu.HostBuffer((S, 2, offsets.size - 1))
            aux_rows = pin.array if route == "pinned" else np.empty((S, 2, offsets.size - 1), dtype=np.float32)
            aux_rows[...] = -7.0
            ramp = route == "pageable"
            if ramp:
                assert many.bus_set_send_gains(g1, True) == 0
            out, aux = many.process_block_bus(xg, K, aux_out=aux_rows)
            assert same_words(out, mix_model(y, K)) and same_words(aux, send_model(y, offsets, members, g, g1 if ramp else g, ramp, S)), (block, route)
    straddling = members.copy()
    straddling[offsets[2] - 1] = bounds[1][0]
    assert many._lib.fxb_bus_set_sends(many._h, 3, ptr(offsets), ptr(straddling), None) == FX_E_ARG and "aux bus 1 " in many.last_error()
    assert sends_are(many, offsets, members, g1)
    assert many.info("bus_send_blocks") == 4 * 3
    same_state(gpu, many, plain, register_names(gpu, text, 2), (0, 63, 64, bounds[1][0], N - 1), tram=1000)
