"""Bus taps on the GPU: fxb_process_block_bus_tap* against a second handle that runs fxb_process_block on the expanded input (y;
tests/test_gpu_bus.py pins that against the oracle).  The taps must be y[:, :, list] as 32-bit patterns, NaNs included, and the
mix what mix_model / gain_mix_model of y give.  No tolerance anywhere; all instance state afterwards equal to the plain handle's."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_bus_gain_stub import SHAPES, gain_mix_model, gains_for
from test_bus_stub import expand, mix_model, same_words
from test_bus_tap_stub import same_bits, tap_list
from test_gpu_bus import NONFINITE, cutoffs, group_input, handles, program, register_names, same_state

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SHARED_IN, MIX_OUT = 1, 2


@pytest.fixture
def kernel_tier(request, monkeypatch):
    for name in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(name, raising=False)
    if request.param != "default":
        monkeypatch.setenv("FX_KERNEL", request.param)
    return request.param


def right_tier(b, tier):
    k = b.info("kernel")
    return k >= 9 if tier == "default" else (1 <= k < 9 if tier == "asm" else k == 0)


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


# the whole (N, K) list with one and two channels on the translated tier, two shapes on the others
GRID = [("default", N, K, ch) for N, K in SHAPES for ch in (1, 2)] + [(t, 777, 130, 2) for t in ("hip", "asm")] + [(t, 200, 63, 1) for t in ("hip", "asm")]


@pytest.mark.parametrize("kernel_tier,N,K,channels", GRID, indirect=["kernel_tier"], ids=["%s-N%d-K%d-C%d" % g for g in GRID])
def test_taps_and_mix_bit_exact(gpu, kernel_tier, N, K, channels):
    """blocks of 33, 1 and 33 samples (rows in whole chunks of the kernel's eight and a ragged rest) on two handles whose state
    carries - one with a shared input, one fed per instance - each block with lists of two of the sizes 1, 65 and 130, so that every
    size meets a long block on either handle; every list has the first and the last instance, a repeat and an unsorted stretch"""
    rng = np.random.default_rng(1000 * N + K)
    text = program("config3", channels)
    names = register_names(gpu, text, channels)
    plain, both, only_mix = handles(gpu, text, N, channels, 3)
    G = plain.bus_groups(K)
    clock = 0
    for S, T_both, T_mix in ((33, 1, 65), (1, 130, 1), (33, 65, 130)):
        lists = tap_list(rng, N, T_both), tap_list(rng, N, T_mix)
        for b, lst in zip((both, only_mix), lists):
            assert b.bus_set_taps(lst) == 0 and np.array_equal(b.bus_get_taps(), lst)
        xg = group_input(G, S, channels, clock)
        clock += S
        x = expand(xg, K, N)
        y = plain.process_block(x)
        want_mix = mix_model(y, K)
        where = "N %d K %d C %d S %d T %d / %d" % (N, K, channels, S, T_both, T_mix)
        out, taps = both.process_block_bus(xg, K, True, True, taps=True)
        assert same_words(out, want_mix) and same_bits(taps, y[:, :, lists[0]]), where + ": both"
        out, taps = only_mix.process_block_bus(x, K, False, True, taps=True)
        assert same_words(out, want_mix) and same_bits(taps, y[:, :, lists[1]]), where + ": mix out"
    watched = sorted({0, min(63, N - 1), min(64, N - 1), N - 1})
    for b in (both, only_mix):
        same_state(gpu, b, plain, names, watched, tram=1000)
        assert b.info("bus_tap_blocks") == 3 and b.info("bus_blocks") == 3 and right_tier(b, kernel_tier)
    for b in (plain, both, only_mix):
        b.close()


@pytest.mark.parametrize("K", [64, 65])
def test_taps_are_pre_fader(gpu, K):
    """MACW does not saturate: an instance fed NaN and one fed Inf put non-finite words on their outputs.  Muted, they stay off the
    bus, the meters count them, and their taps carry exactly the words the plain handle wrote"""
    N, S = 1000, 33
    vol = cutoffs(N)
    plain, b = handles(gpu, NONFINITE, N, 1, 2, control="vol", values=vol)
    assert b.meter_enable() == 0
    nan_fed, inf_fed = 70, 131
    x = expand(group_input(plain.bus_groups(K), S, 1, 0), K, N)
    x[:, 0, nan_fed] = np.nan
    x[:, 0, inf_fed] = np.inf
    y = plain.process_block(x)
    bad = ~np.isfinite(y[:, 0, :])
    assert bad[:, nan_fed].any() and bad[:, inf_fed].any() and not np.delete(bad, (nan_fed, inf_fed), axis=1).any()
    g = gains_for(np.random.default_rng(K), 1, N, special=False)
    g[0, nan_fed], g[0, inf_fed] = 0.0, -0.0
    lst = np.array([inf_fed, 0, nan_fed, N - 1, nan_fed], dtype=np.int64)
    assert b.bus_set_gains(g) == 0 and b.bus_set_taps(lst) == 0
    got, taps = b.process_block_bus(x, K, False, True, taps=True)
    assert np.isfinite(got).all(), "a muted voice reached the bus"
    assert same_words(got, gain_mix_model(y, g, g, False, S, K))
    assert same_bits(taps, y[:, :, lst]), "the taps of the muted voices carry the plain handle's non-finite words"
    assert not np.isfinite(taps[:, 0, 0]).all() and np.isnan(taps[:, 0, 2]).any()
    meters = b.meter_read()
    assert meters["nonfinite"][0, nan_fed] == bad[:, nan_fed].sum() > 0 and meters["nonfinite"][0, inf_fed] == bad[:, inf_fed].sum() > 0
    assert meters["nonfinite"].sum() == bad.sum()
    same_state(gpu, b, plain, ["a", "t", "out", "ccr"], (0, 63, 64, nan_fed, inf_fed, N - 1))


def test_tap_rows_pinned_pageable_and_on_a_second_stream(gpu):
    import torch

    text = progs.config3()
    N, S, K, T = 4133, 33, 64, 65
    rng = np.random.default_rng(13)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    lst = tap_list(rng, N, T)
    assert b.bus_set_taps(lst) == 0
    blocks = [group_input(G, S, 1, k * S) for k in range(4)]
    ys = [plain.process_block(expand(xg, K, N)) for xg in blocks]
    # pinned: everything in place, the tap rows stored over PCIe
    pin_in, pin_out, pin_tap = gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, T))
    pin_in.array[...] = blocks[0]
    pin_tap.array[...] = -7.0
    before = (b.info("host_staged_blocks"), b.info("host_inplace_blocks"))
    out, taps = b.process_block_bus(pin_in.array, K, out=pin_out.array, tap_out=pin_tap.array)
    assert out is pin_out.array and taps is pin_tap.array
    assert (b.info("host_staged_blocks"), b.info("host_inplace_blocks")) == (before[0], before[1] + 1)
    assert same_words(out, mix_model(ys[0], K)) and same_bits(taps, ys[0][:, :, lst]), "pinned"
    # pageable: staged
    out, taps = b.process_block_bus(blocks[1], K, taps=True)
    assert (b.info("host_staged_blocks"), b.info("host_inplace_blocks")) == (before[0] + 1, before[1] + 1)
    assert same_words(out, mix_model(ys[1], K)) and same_bits(taps, ys[1][:, :, lst]), "pageable"
    # device tensors on a second stream: two blocks back to back, then fxb_sync only
    stream = torch.cuda.Stream()
    d_in = [torch.from_numpy(blocks[k]).to("cuda") for k in (2, 3)]
    d_out = [torch.full((S, 1, G), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    d_tap = [torch.full((S, 1, T), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        assert b.process_block_bus_dev(d_in[k], d_out[k], S, K, stream=stream.cuda_stream, d_tap_out=d_tap[k]) == 0
    assert b.sync() == 0
    for k in range(2):
        assert same_words(d_out[k].cpu().numpy(), mix_model(ys[2 + k], K)), k
        assert same_bits(d_tap[k].cpu().numpy(), ys[2 + k][:, :, lst]), k
    assert b.info("bus_tap_blocks") == 4 and b.info("bus_blocks") == 4
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)


def test_tap_rows_of_the_two_pieces_of_a_block(gpu):
    """262 144 instances x 96 samples, mono, a short program: a per-instance block of 96 MiB, run in two pieces on the 64 MiB
    scratch; each piece delivers its rows"""
    text = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
    N, S, K, T = 262144, 96, 64, 65
    rng = np.random.default_rng(17)
    plain, b = handles(gpu, text, N, 1, 2, control="vol")
    G = b.bus_groups(K)
    lst = tap_list(rng, N, T)
    assert b.bus_set_taps(lst) == 0
    xg = group_input(G, S, 1, 0)
    y = plain.process_block(expand(xg, K, N))
    out, taps = b.process_block_bus(xg, K, taps=True)
    assert same_bits(taps, y[:, :, lst]) and same_words(out, mix_model(y, K))
    assert b.info("bus_tap_blocks") == 1 and b.info("bus_blocks") == 1


def test_refusals_and_the_block_behind_them(gpu):
    lib = gpu.load()
    text = progs.config3()
    N, S, K, T = 300, 8, 64, 65
    rng = np.random.default_rng(19)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    xg = gpu.HostBuffer((S, 1, G))
    yg, yn, pt = gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, N)), gpu.HostBuffer((S, 1, T))
    both = gpu.HostBuffer((4 * S, 1, N))
    xg.array[...] = group_input(G, S, 1, 0)
    pt.array[...] = -7.0
    page = np.full((S, 1, T), -7.0, dtype=np.float32)
    at = lambda h, off: C.c_void_p(h.array.ctypes.data + off * 4)
    host = lambda x, y, t, n, k, flags: lib.fxb_process_block_bus_tap(b._h, ptr(x), ptr(y), ptr(t), n, k, flags)
    dev = lambda x, y, t, n, k, flags: lib.fxb_process_block_bus_tap_dev(b._h, ptr(x), ptr(y), ptr(t), n, k, flags, None)
    assert host(xg.array, yg.array, pt.array, S, K, 3) == FX_E_ARG and "taps are off" in b.last_error()
    lst = tap_list(rng, N, T)
    bad = lst.copy()
    bad[T - 1] = N
    assert lib.fxb_bus_set_taps(b._h, ptr(bad), T) == FX_E_ARG and lib.fxb_bus_set_taps(b._h, ptr(lst), 65537) == FX_E_ARG
    assert lib.fxb_bus_set_taps(b._h, None, 2) == FX_E_ARG and lib.fxb_bus_set_taps(b._h, ptr(lst), -1) == FX_E_ARG
    assert b.bus_get_taps().size == 0
    assert b.bus_set_taps(lst) == 0
    rows = S * T
    refused = [
        host(xg.array, yn.array, pt.array, S, K, SHARED_IN), dev(xg.array, yn.array, pt.array, S, K, SHARED_IN), host(yn.array, yn.array, pt.array, S, K, 0),
        lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, S * N - 1), S, K, MIX_OUT),
        lib.fxb_process_block_bus_tap(b._h, at(both, rows - 1), at(both, 2 * S * N), at(both, 0), S, K, MIX_OUT),
        lib.fxb_process_block_bus_tap(b._h, at(both, 0), at(both, 2 * S * N), at(both, 2 * S * N + S * G - 1), S, K, MIX_OUT),
        host(xg.array, yg.array, pt.array, S, 0, 3), host(xg.array, yg.array, pt.array, S, K, 7), host(None, yg.array, pt.array, S, K, 3),
        host(xg.array, yg.array, pt.array, -1, K, 3),
        dev(xg.array, yg.array, page, S, K, 3),   # (pageable rows: the device cannot address them; rows that run past the end of a
                                                  # pinned allocation are refused in tests/test_bus_tap_stub.py, where its size is exact)
    ]
    assert refused == [FX_E_ARG] * len(refused), refused
    many = gpu.Batch(N, 1, devices=[0, 0])
    assert many.load_text(text) and many.bus_set_taps(lst) == 0
    assert lib.fxb_process_block_bus_tap_dev(many._h, ptr(xg.array), ptr(yg.array), ptr(pt.array), S, K, 3, None) == FX_E_ARG
    assert (pt.array == -7.0).all() and (page == -7.0).all() and np.array_equal(b.bus_get_taps(), lst)
    assert b.info("bus_blocks") == 0 and b.info("bus_tap_blocks") == 0
    # the next tapped block is right: host entry, then the device entry on the handle's stream
    y = plain.process_block(expand(xg.array, K, N))
    assert host(xg.array, yg.array, pt.array, S, K, 3) == 0, b.last_error()
    assert same_words(yg.array, mix_model(y, K)) and same_bits(pt.array, y[:, :, lst])
    y = plain.process_block(expand(xg.array, K, N))
    assert dev(xg.array, yg.array, pt.array, S, K, 3) == 0 and b.sync() == 0, b.last_error()
    assert same_words(yg.array, mix_model(y, K)) and same_bits(pt.array, y[:, :, lst])
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)


def test_sharded_handle_equals_the_single_one(gpu):
    """three shards on one device: a list that hits every shard with repeats across them and one that skips the middle shard, on
    pinned rows (every shard stores its columns in place) and on pageable ones"""
    text = program("config3", 2)
    N, S, K = 64 * 16 + 17, 9, 64
    plan = gpu.shard_plan(N, 3)
    rng = np.random.default_rng(23)
    plain = handles(gpu, text, N, 2, 1)[0]
    many = gpu.Batch(N, 2, devices=[0, 0, 0])
    first, second = plan[1][0], plan[2][0]
    lists = (np.concatenate([tap_list(rng, N, 65), [first - 1, first, second - 1, second, first]]).astype(np.int64),
             np.array([N - 1, 0, second, first - 1, 0, N - 1], dtype=np.int64))
    assert many.bus_set_taps(lists[0]) == 0   # (before the program is loaded)
    assert many.load_text(text), many.errors()
    assert many.set_register_array("cutoff", cutoffs(N)) == 0
    G = many.bus_groups(K)
    for block, lst in enumerate(lists):
        assert many.bus_set_taps(lst) == 0 and np.array_equal(many.bus_get_taps(), lst)
        for route in ("pinned", "pageable"):
            xg = group_input(G, S, 2, (2 * block + (route == "pageable")) * S)
            y = plain.process_block(expand(xg, K, N))
            pin = gpu.HostBuffer((S, 2, lst.size))
            tap_rows = pin.array if route == "pinned" else np.empty((S, 2, lst.size), dtype=np.float32)
            tap_rows[...] = -7.0
            out, taps = many.process_block_bus(xg, K, tap_out=tap_rows)
            assert same_words(out, mix_model(y, K)) and same_bits(taps, y[:, :, lst]), (block, route)
    assert many.info("bus_tap_blocks") == 4 * 3
    same_state(gpu, many, plain, register_names(gpu, text, 2), (0, 63, 64, first, N - 1), tram=1000)
