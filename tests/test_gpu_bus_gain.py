"""Bus gains on the GPU: fxb_process_block_bus* with fxb_bus_set_gains against a second handle that runs fxb_process_block on the
expanded input (y; tests/test_gpu_bus.py pins that against the oracle) and gain_mix_model(y, a, b, ramp, S, K) - the numpy fp32
restatement of the definition in include/fx8010_amd.h "Bus gains" that tests/test_bus_gain_stub.py checks against the definition
written out one operation at a time.  Bar: every word equal (where the model is NaN the result is NaN), no tolerance anywhere,
and all instance state afterwards equal to the plain handle's."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_bus_gain_stub import SHAPES, gain_mix_model, gains_for
from test_bus_stub import expand, mix_model, same_words
from test_gpu_bus import NONFINITE, cutoffs, group_input, handles, program, register_names, same_state

pytestmark = pytest.mark.gpu

FX_E_ARG = -3


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


# the whole (N, K) list with one and two channels on the translated tier, one shape with both K regimes' neighbours on the others
GRID = [("default", N, K, ch) for N, K in SHAPES for ch in (1, 2)] + [(t, 777, 130, 2) for t in ("hip", "asm")] + [(t, 200, 63, 1) for t in ("hip", "asm")]


@pytest.mark.parametrize("kernel_tier,N,K,channels", GRID, indirect=["kernel_tier"], ids=["%s-N%d-K%d-C%d" % g for g in GRID])
def test_static_gains_and_ramps_bit_exact(gpu, kernel_tier, N, K, channels):
    """static gains, a ramp over 33 samples, a ramp over one sample (w = b), a static block again - on handles whose state carries"""
    rng = np.random.default_rng(1000 * N + K)
    text = program("config3", channels)
    names = register_names(gpu, text, channels)
    plain, both, only_mix = handles(gpu, text, N, channels, 3)
    G = plain.bus_groups(K)
    a = gains_for(rng, channels, N)
    for b in (both, only_mix):
        assert b.bus_set_gains(a) == 0
    clock = 0
    for S, ramp in ((33, False), (33, True), (1, True), (33, False), (2, True)):
        g = gains_for(rng, channels, N) if ramp else a
        if ramp:
            for b in (both, only_mix):
                assert b.bus_set_gains(g, ramp=True) == 0
                assert same_words(b.bus_get_gains(), a)
        xg = group_input(G, S, channels, clock)
        clock += S
        x = expand(xg, K, N)
        y = plain.process_block(x)
        want = gain_mix_model(y, a, g, ramp, S, K)
        where = "N %d K %d C %d S %d ramp %d" % (N, K, channels, S, ramp)
        assert same_words(both.process_block_bus(xg, K, True, True), want), where + ": both"
        assert same_words(only_mix.process_block_bus(x, K, False, True), want), where + ": mix out"
        a = g
        for b in (both, only_mix):
            assert same_words(b.bus_get_gains(), a)
    watched = sorted({0, min(63, N - 1), min(64, N - 1), N - 1})
    for b in (both, only_mix):
        same_state(gpu, b, plain, names, watched, tram=1000)
        assert b.info("bus_gain_blocks") == 5 and b.info("bus_blocks") == 5 and right_tier(b, kernel_tier)
    # gains of 1.0f give the words of the unweighted sum; NULL turns the gains off
    xg = group_input(G, 33, channels, clock)
    y = plain.process_block(expand(xg, K, N))
    assert both.bus_set_gains(np.ones((channels, N), dtype=np.float32)) == 0 and only_mix.bus_set_gains(None) == 0
    assert same_words(both.process_block_bus(xg, K), mix_model(y, K)) and same_words(only_mix.process_block_bus(expand(xg, K, N), K, False, True), mix_model(y, K))
    assert both.info("bus_gain_blocks") == 6 and only_mix.info("bus_gain_blocks") == 5
    assert gpu.load().fxb_bus_get_gains(only_mix._h, C.c_void_p(a.ctypes.data)) == FX_E_ARG
    for b in (plain, both, only_mix):
        b.close()


@pytest.mark.parametrize("K", [64, 65])
def test_a_gain_of_zero_mutes_whatever_the_voice_holds(gpu, K):
    """MACW does not saturate: an instance fed NaN and one fed Inf put non-finite words on their outputs.  A gain of +0 or -0
    keeps them off the bus; any other gain does not; the meters, which look in front of the mix, still count them"""
    N, S = 1000, 33
    vol = cutoffs(N)
    plain, b = handles(gpu, NONFINITE, N, 1, 2, control="vol", values=vol)
    assert b.meter_enable() == 0
    nan_fed, inf_fed = 70, 131   # (both in group 1 for K = 64; in groups 1 and 2 for K = 65)
    x = expand(group_input(plain.bus_groups(K), S, 1, 0), K, N)
    x[:, 0, nan_fed] = np.nan
    x[:, 0, inf_fed] = np.inf
    y = plain.process_block(x)
    bad = ~np.isfinite(y[:, 0, :])
    assert bad[:, nan_fed].any() and bad[:, inf_fed].any() and not np.delete(bad, (nan_fed, inf_fed), axis=1).any()
    rng = np.random.default_rng(K)
    g = gains_for(rng, 1, N, special=False)
    g[0, nan_fed], g[0, inf_fed] = 0.0, -0.0
    assert b.bus_set_gains(g) == 0
    got = b.process_block_bus(x, K, False, True)
    assert np.isfinite(got).all(), "a muted voice reached the bus"
    assert same_words(got, gain_mix_model(y, g, g, False, S, K))
    meters = b.meter_read()
    assert meters["nonfinite"][0, nan_fed] == bad[:, nan_fed].sum() > 0 and meters["nonfinite"][0, inf_fed] == bad[:, inf_fed].sum() > 0, "the meters are pre-fader"
    assert meters["nonfinite"].sum() == bad.sum()
    # un-muting with a ramp: the first sample already carries a non-zero weight
    y = plain.process_block(x)
    g2 = g.copy()
    g2[0, nan_fed], g2[0, inf_fed] = 0.5, -0.25
    assert b.bus_set_gains(g2, ramp=True) == 0
    got = b.process_block_bus(x, K, False, True)
    want = gain_mix_model(y, g, g2, True, S, K)
    assert same_words(got, want)
    assert np.isnan(got[:, 0, nan_fed // K]).any() and not np.isfinite(got[:, 0, inf_fed // K]).all(), "a non-zero gain lets the voice through"
    # ... and muting with one: zero exactly on the last sample
    y = plain.process_block(x)
    assert b.bus_set_gains(g, ramp=True) == 0
    got = b.process_block_bus(x, K, False, True)
    assert same_words(got, gain_mix_model(y, g2, g, True, S, K)) and np.isfinite(got[S - 1]).all()
    same_state(gpu, b, plain, ["a", "t", "out", "ccr"], (0, 63, 64, nan_fed, inf_fed, N - 1))


def test_a_ramp_across_the_pieces_of_a_block(gpu):
    """262 107 instances x 96 samples: a per-instance block of 96 MiB, run in two pieces on the 64 MiB scratch, with one S"""
    text = progs.config3()
    N, S, K = 262107, 96, 64
    rng = np.random.default_rng(7)
    plain, both = handles(gpu, text, N, 1, 2)
    a, g = gains_for(rng, 1, N), gains_for(rng, 1, N)
    assert both.bus_set_gains(a) == 0 and both.bus_set_gains(g, ramp=True) == 0
    xg = group_input(plain.bus_groups(K), S, 1, 0)
    y = plain.process_block(expand(xg, K, N))
    got = both.process_block_bus(xg, K)
    assert same_words(got, gain_mix_model(y, a, g, True, S, K))
    assert same_words(got[S - 1:], gain_mix_model(y[S - 1:], g, g, False, 1, K)), "the last row equals a static block at b"
    assert same_words(both.bus_get_gains(), g)
    same_state(gpu, both, plain, ["rd", "a", "t", "s31", "out", "ccr"], (0, 63, 64, 131072, N - 1), tram=1000)
    # the next block is static
    y = plain.process_block(expand(xg, K, N))
    assert same_words(both.process_block_bus(xg, K), gain_mix_model(y, g, g, False, S, K))
    assert both.info("bus_gain_blocks") == 2


@pytest.mark.parametrize("shards,N", [(2, 64 * 10 + 17), (3, 64 * 16 + 17)])
def test_sharded_handles_equal_the_single_one(gpu, shards, N):
    text = program("config3", 2)
    names = register_names(gpu, text, 2)
    plan = gpu.shard_plan(N, shards)
    assert all(first % 192 == 0 for first, _ in plan), plan
    rng = np.random.default_rng(N)
    S = 33
    for K in (64, 192):
        plain, one = handles(gpu, text, N, 2, 2)
        many = gpu.Batch(N, 2, devices=[0] * shards)
        a = gains_for(rng, 2, N)
        assert many.bus_set_gains(a) == 0 and one.bus_set_gains(a) == 0   # (before the program is loaded)
        assert many.load_text(text), many.errors()
        assert many.set_register_array("cutoff", cutoffs(N)) == 0
        G = many.bus_groups(K)
        for block, ramp in enumerate((False, True, False)):
            g = gains_for(rng, 2, N) if ramp else a
            if ramp:
                assert many.bus_set_gains(g, ramp=True) == 0 and one.bus_set_gains(g, ramp=True) == 0
            xg = group_input(G, S, 2, block * S)
            y = plain.process_block(expand(xg, K, N))
            want = one.process_block_bus(xg, K)
            assert same_words(want, gain_mix_model(y, a, g, ramp, S, K)), (K, ramp)
            assert same_words(many.process_block_bus(xg, K), want), (K, ramp)
            a = g
            assert same_words(many.bus_get_gains(), a), "get assembles by global instance"
        same_state(gpu, many, plain, names, (0, 63, 64, plan[1][0], N - 1), tram=1000)
        assert many.info("bus_gain_blocks") == 3 * shards and one.info("bus_gain_blocks") == 3
        bad = a.copy()
        bad[1, N - 1] = np.inf
        assert gpu.load().fxb_bus_set_gains(many._h, C.c_void_p(bad.ctypes.data), 0) == FX_E_ARG and same_words(many.bus_get_gains(), a)
        for b in (plain, one, many):
            b.close()


def test_a_set_between_two_blocks_on_a_callers_stream(gpu):
    """device-entry blocks on a stream that is not the handle's own, the gains set between them, fxb_sync only at the end: the first
    block keeps the gains it was queued with, the second has the new ones, a ramp queued behind them starts from those"""
    import torch

    text = progs.config3()
    N, S, K = 65536, 96, 64   # (a mix over 24 MiB behind a long emulation launch: the sets below overtake the blocks on the host)
    rng = np.random.default_rng(11)
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    stream = torch.cuda.Stream()
    blocks = [group_input(G, S, 1, k * S) for k in range(3)]
    ys = [plain.process_block(expand(xg, K, N)) for xg in blocks]
    g = [gains_for(rng, 1, N) for _ in range(3)]
    d_in = [torch.from_numpy(xg).to("cuda") for xg in blocks]
    d_out = [torch.full((S, 1, G), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    assert b.bus_set_gains(g[0]) == 0
    assert b.process_block_bus_dev(d_in[0], d_out[0], S, K, stream=stream.cuda_stream) == 0
    assert b.bus_set_gains(g[1]) == 0
    assert b.process_block_bus_dev(d_in[1], d_out[1], S, K, stream=stream.cuda_stream) == 0
    assert b.bus_set_gains(g[2], ramp=True) == 0
    assert b.process_block_bus_dev(d_in[2], d_out[2], S, K, stream=stream.cuda_stream) == 0
    assert b.sync() == 0
    fetch = lambda t: t.cpu().numpy()
    assert same_words(fetch(d_out[0]), gain_mix_model(ys[0], g[0], g[0], False, S, K)), "the first block lost the gains it was queued with"
    assert same_words(fetch(d_out[1]), gain_mix_model(ys[1], g[1], g[1], False, S, K)), "the second block did not see the new gains"
    assert same_words(fetch(d_out[2]), gain_mix_model(ys[2], g[1], g[2], True, S, K)), "the ramp"
    assert same_words(b.bus_get_gains(), g[2]) and b.info("bus_gain_blocks") == 3
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)
