"""Group buses on the GPU: fxb_process_block_bus* against a second handle that runs fxb_process_block on the expanded input (y;
existing tests pin that against the oracle, and instances 0, 63, 64 and N - 1 are checked against it here as well) and, for mixed
outputs, against mix_model(y, K) - a numpy fp32 restatement of the summation order include/fx8010_amd.h fixes.  Bar: every word
equal (where the model is NaN the result is NaN), and all instance state afterwards equal to the plain handle's."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
SHARED_IN, MIX_OUT = 1, 2
MODES = ((True, False), (False, True), (True, True))


@pytest.fixture(params=["default", "asm", "hip"], ids=["xlate", "asm", "hip"])
def tier(request, monkeypatch):
    """the three kernel tiers: the program translated to gfx950 code (the default), the hand-written interpreter, the HIP C++
    kernel - selected through FX_KERNEL like tests/test_gpu_parity.py does"""
    for name in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(name, raising=False)
    if request.param != "default":
        monkeypatch.setenv("FX_KERNEL", request.param)
    return request.param


def mix_model(y, K):
    """[..., N] -> [..., G]: every group's sum in the order include/fx8010_amd.h fixes, in fp32 (numpy adds float32 arrays in
    float32, round to nearest, one rounding per add): 64 partial sums start at +0.0; member m = j * 64 + l of a group, where it
    exists, is added to p[l] for j ascending; then p[l] = p[l] + p[l + step] for l < step, step = 32 ... 1; the sum is p[0].
    Only the lanes below W = min(64, K) are held: no member is ever added to a lane at or above K, so those lanes are +0.0 when
    the tree starts, a tree step can only give them +0.0 + +0.0, and where a step reads one of them it adds that +0.0.
    (tests/test_bus_stub.py checks this function against the order written out one add at a time.)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    N = y.shape[-1]
    K = min(int(K), N)
    G, J, W = -(-N // K), -(-K // 64), min(64, K)
    lead = y.shape[:-1]
    members = np.zeros(lead + (G * K,), dtype=np.float32)
    members[..., :N] = y
    exists = np.arange(G * K) < N
    members, exists = members.reshape(lead + (G, K)), exists.reshape(G, K)
    p = np.zeros(lead + (G, W), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(J):
            w = min(64, K - j * 64)
            p[..., :w] = np.where(exists[:, j * 64:j * 64 + w], p[..., :w] + members[..., j * 64:j * 64 + w], p[..., :w])
        for step in (32, 16, 8, 4, 2, 1):
            held = min(step, W)                      # lanes l < step that are held
            paired = max(0, min(W - step, step))     # ... whose partner l + step is held as well
            other = np.zeros(lead + (G, held), dtype=np.float32)
            other[..., :paired] = p[..., step:step + paired]
            p[..., :held] = p[..., :held] + other
    return np.ascontiguousarray(p[..., 0])


def expand(x, K, N):
    """[..., G] -> [..., N]: instance n hears column n // K"""
    return np.ascontiguousarray(x[..., np.arange(N) // min(int(K), N)])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def same_words(got, want):
    """where the model is NaN the result is NaN; everywhere else the bit patterns are equal"""
    nan = np.isnan(want)
    return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and bool((bits(got)[~nan] == bits(want)[~nan]).all())


def stereo(text):
    """the mono configuration programs with a second channel that goes through their state"""
    assert text.endswith("\nend") and "static t" in text
    return text[:-3].replace("output out 0", "output out 0\ninput in1 1\noutput out1 1", 1) + "macs out1, in1, t, 0.5\nend"


def program(name, channels):
    text = progs.CONFIGS[name]()
    return text if channels == 1 else stereo(text)


def register_names(gpu, text, channels):
    f = gpu.FrontEnd(channels)
    assert f.load_text(text), f.errors()
    return [r[0] for r in f.registers()]


def cutoffs(N):
    """one setting per instance: what makes the members of a group differ"""
    return (0.05 + 0.9 * (progs.stimulus(N, 1, seed=4242)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32)


def group_input(G, S, channels, clock, seed=7):
    return np.ascontiguousarray(np.stack([progs.stimulus(G, S, first_sample=clock, seed=seed + 1000 * c) for c in range(channels)], axis=1))   # [S, channels, G]


def handles(gpu, text, N, channels, count, control="cutoff", values=None):
    out = []
    values = cutoffs(N) if values is None else values
    for _ in range(count):
        b = gpu.Batch(N, channels, 0)
        assert b.load_text(text), b.errors()
        if control:
            assert b.set_register_array(control, values) == 0
        out.append(b)
    return out


def same_state(gpu, a, b, names, instances, tram=0):
    for r in names:
        assert np.array_equal(bits(a.get_register_array(r)), bits(b.get_register_array(r))), "register %s" % r
    assert a.instruction_counter() == b.instruction_counter()
    for n in instances:
        assert a.instruction_counter_i(n) == b.instruction_counter_i(n), n
        assert a.get_cursors_i(n) == b.get_cursors_i(n), n
        if tram:
            assert np.array_equal(bits(a.get_tram_i(0, n, tram)), bits(b.get_tram_i(0, n, tram))), n
    assert a.ood_flags() == b.ood_flags()


SHAPES_N = (1, 63, 64, 65, 200, 4133, 65499)
SHAPES_S = (1, 33, 96)


def shapes_k(N):
    return (1, 2, 63, 64, 65, 128, 1000, N, N + 5)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", ["config3", "config4", "config2"])
def test_bus_blocks_bit_exact(gpu, tier, name, channels):
    """the whole shape grid - every N, every K, every block length - in each of the three modes, on one set of handles per N whose
    state carries from block to block (the plain handle and the three bus handles hear the same signal in every block)"""
    text = program(name, channels)
    names = register_names(gpu, text, channels)
    for N in SHAPES_N:
        plain, only_in, only_mix, both = handles(gpu, text, N, channels, 4)
        watched = sorted({0, min(63, N - 1), min(64, N - 1), N - 1})
        oracles = []
        for n in watched:
            o = Oracle(channels)
            assert o.load_text(text), o.errors()
            o.set_register("cutoff", float(cutoffs(N)[n]))
            oracles.append(o)
        clock = 0
        for K in shapes_k(N):
            G = plain.bus_groups(K)
            assert G == -(-N // K)
            for S in SHAPES_S:
                xg = group_input(G, S, channels, clock)
                clock += S
                x = expand(xg, K, N)
                y = plain.process_block(x)
                for n, o in zip(watched, oracles):
                    ref = o.process_block(np.ascontiguousarray(x[:, :, n]))
                    assert same_bits(ref.reshape(S, channels), y[:, :, n]), "N %d K %d S %d: instance %d differs from the oracle" % (N, K, S, n)
                where = "N %d K %d S %d" % (N, K, S)
                assert same_bits(only_in.process_block_bus(xg, K, True, False), y), where + ": shared in"
                model = mix_model(y, K)
                assert same_words(only_mix.process_block_bus(x, K, False, True), model), where + ": mix out"
                assert same_words(both.process_block_bus(xg, K, True, True), model), where + ": both"
        for b in (only_in, only_mix, both):
            same_state(gpu, b, plain, names, watched, tram=1000 if name == "config3" else 0)
            assert b.info("bus_blocks") == len(shapes_k(N)) * len(SHAPES_S)
            assert b.info("kernel") >= 9 if tier == "default" else (1 <= b.info("kernel") < 9 if tier == "asm" else b.info("kernel") == 0)
        for b in (plain, only_in, only_mix, both):
            b.close()


NONFINITE = ("static a\ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic big = 100000000000000000000000000000000000000.0\n"
             "static tiny = 0.00000000000000000000000000000000000001\nstatic t\n"
             "macs a, 0, vol, in\nmacw t, big, in, big\nmacw out, a, t, tiny\nend")


def test_nan_and_inf_pass_through(gpu, tier):
    """MACW does not saturate: an input of 3 puts +Inf on the output, a NaN input a NaN, -Inf itself - in some groups, not in others"""
    N, S = 4133, 33
    vol = cutoffs(N)
    for K in (64, 65, 1000):
        plain, only_in, only_mix, both = handles(gpu, NONFINITE, N, 1, 4, control="vol", values=vol)
        G = plain.bus_groups(K)
        xg = group_input(G, S, 1, 0)
        xg[5, 0, 1 % G] = 3.0
        xg[9, 0, 2 % G] = np.nan
        xg[11, 0, G - 1] = -np.inf
        x = expand(xg, K, N)
        y = plain.process_block(x)
        assert np.isnan(y).any() and np.isinf(y).any() and np.isfinite(y).any()
        model = mix_model(y, K)
        assert np.isnan(model).any() and np.isinf(model).any() and np.isfinite(model).any()
        assert same_bits(only_in.process_block_bus(xg, K, True, False), y)
        assert same_words(only_mix.process_block_bus(x, K, False, True), model)
        assert same_words(both.process_block_bus(xg, K, True, True), model)
        for b in (only_in, only_mix, both):
            same_state(gpu, b, plain, ["a", "t", "out", "ccr"], (0, 63, 64, N - 1))


def test_two_bus_blocks_are_one_of_twice_the_length(gpu, tier):
    text = progs.config3()
    names = register_names(gpu, text, 1)
    N, S, K = 1000, 48, 65
    twice, once = handles(gpu, text, N, 1, 2)
    xg = group_input(twice.bus_groups(K), 2 * S, 1, 0)
    got = np.concatenate([twice.process_block_bus(xg[:S], K), twice.process_block_bus(xg[S:], K)], axis=0)
    assert same_bits(got, once.process_block_bus(xg, K))
    same_state(gpu, twice, once, names, (0, 63, 64, N - 1), tram=1000)


def test_a_block_above_the_scratch_limit_equals_the_uncut_result(gpu):
    """262 107 instances x 96 samples: a per-instance block of 96 MiB, run in two pieces on the 64 MiB scratch"""
    text = progs.config3()
    N, S, K = 262107, 96, 64
    plain, both = handles(gpu, text, N, 1, 2)
    xg = group_input(plain.bus_groups(K), S, 1, 0)
    y = plain.process_block(expand(xg, K, N))
    assert same_words(both.process_block_bus(xg, K), mix_model(y, K))
    same_state(gpu, both, plain, ["rd", "a", "t", "s31", "out", "ccr"], (0, 63, 64, 131072, N - 1), tram=1000)
    # ... and once more, now that both have state
    y = plain.process_block(expand(xg, K, N))
    assert same_words(both.process_block_bus(xg, K), mix_model(y, K))


def test_an_armed_control_track_applies(gpu, tier):
    text = progs.config3()
    names = register_names(gpu, text, 1)
    N, S, K = 1000, 64, 64
    plain, both, only_in = handles(gpu, text, N, 1, 3, control=None)
    G = plain.bus_groups(K)
    steps = np.linspace(0.05, 0.9, 8).astype(np.float32)
    per = (steps[:, None] * (0.5 + 0.5 * cutoffs(N))[None, :]).astype(np.float32)   # [steps, N]
    for block, (key, values) in enumerate((("cutoff", steps), ("fb", per), ("cutoff", per))):
        xg = group_input(G, S, 1, block * S)
        for b in (plain, both, only_in):
            assert b.set_register_track(key, values, 8) == 0
        y = plain.process_block(expand(xg, K, N))
        assert same_words(both.process_block_bus(xg, K), mix_model(y, K)), key
        assert same_bits(only_in.process_block_bus(xg, K, True, False), y), key
    for b in (both, only_in):
        same_state(gpu, b, plain, names, (0, 63, 64, N - 1), tram=1000)


def test_routes_and_counters(gpu):
    import torch

    text = progs.config4()
    N, S, K = 4133, 32, 64
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    look = lambda: (b.info("host_staged_blocks"), b.info("host_inplace_blocks"), b.info("bus_blocks"))
    blocks = []

    def reference():
        xg = group_input(G, S, 1, len(blocks) * S)
        blocks.append(xg)
        return xg, mix_model(plain.process_block(expand(xg, K, N)), K)

    # pinned buffers: in place
    pin_in, pin_out = gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, G))
    xg, want = reference()
    pin_in.array[...] = xg
    before = look()
    assert b.process_block_bus(pin_in.array, K, out=pin_out.array) is pin_out.array
    assert look() == (before[0], before[1] + 1, before[2] + 1) and same_words(pin_out.array, want)
    # ... on one buffer
    xg, want = reference()
    pin_in.array[...] = xg
    assert b.process_block_bus(pin_in.array, K, out=pin_in.array) is pin_in.array and same_words(pin_in.array, want)
    assert look() == (before[0], before[1] + 2, before[2] + 2)
    # pageable buffers: staged
    xg, want = reference()
    before = look()
    assert same_words(b.process_block_bus(xg, K), want)
    assert look() == (before[0] + 1, before[1], before[2] + 1)
    # the device entry: torch tensors, a stream that is not the default one
    xg, want = reference()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_in = torch.from_numpy(xg).to("cuda", non_blocking=False)
        d_out = torch.zeros((S, 1, G), dtype=torch.float32, device="cuda")
        stream.synchronize()
        before = look()
        assert b.process_block_bus_dev(d_in, d_out, S, K, stream=stream.cuda_stream) == 0
        stream.synchronize()
    assert b.sync() == 0
    assert look() == (before[0], before[1], before[2] + 1) and same_words(d_out.cpu().numpy(), want)
    # ... mixed output only, from a per-instance tensor on the device
    xg, want = reference()
    d_wide = torch.from_numpy(expand(xg, K, N)).to("cuda")
    torch.cuda.synchronize()
    assert b.process_block_bus_dev(d_wide, d_out, S, K, shared_in=False, stream=stream.cuda_stream) == 0
    stream.synchronize()
    assert same_words(d_out.cpu().numpy(), want)
    # a pageable pointer handed to the device entry
    ms, before = b.last_kernel_ms(), look()
    page = np.zeros((S, 1, G), dtype=np.float32)
    rc = gpu.load().fxb_process_block_bus_dev(b._h, C.c_void_p(page.ctypes.data), C.c_void_p(d_out.data_ptr()), S, K, 3, None)
    assert rc == FX_E_ARG and "not memory of this handle's device" in b.last_error()
    assert look() == before and b.last_kernel_ms() == ms
    same_state(gpu, b, plain, ["x", "a", "b", "o", "ccr"], (0, 63, 64, N - 1))
    pin_in.close()
    pin_out.close()


def test_sync_alone_covers_a_block_on_another_stream(gpu):
    """fxb_sync is the documented partner of the device entry: after a bus block on a stream that is not the handle's own (and
    does not synchronise with the default stream) it must not return before the mix kernel has written the output.  The one
    scratch block must not be refilled - by a block on a second stream, by a host-entry block - while the previous bus block
    still reads it."""
    import torch

    text = progs.config3()
    N, S, K = 262144, 96, 64   # a mix kernel over 96 MiB behind a long emulation launch: two pieces
    plain, b = handles(gpu, text, N, 1, 2)
    G = b.bus_groups(K)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    blocks = [group_input(G, S, 1, k * S) for k in range(4)]
    wants = [mix_model(plain.process_block(expand(xg, K, N)), K) for xg in blocks]
    d_in = [torch.from_numpy(xg).to("cuda") for xg in blocks]
    d_out = [torch.full((S, 1, G), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    host_out = gpu.HostBuffer((S, 1, G))
    torch.cuda.synchronize()
    fetch = lambda t: t.cpu().numpy()   # (torch's copy on its default stream, which does not wait for streams made by torch.cuda.Stream)

    # 1. one block on streams[0], then fxb_sync ONLY
    assert b.process_block_bus_dev(d_in[0], d_out[0], S, K, stream=streams[0].cuda_stream) == 0
    assert b.sync() == 0
    assert same_words(fetch(d_out[0]), wants[0]), "fxb_sync returned before the last kernel of a bus block"
    # 2. a block on streams[0], at once one on streams[1], at once a host-entry block: three fillings of the one scratch
    assert b.process_block_bus_dev(d_in[1], d_out[1], S, K, stream=streams[0].cuda_stream) == 0
    assert b.process_block_bus_dev(d_in[2], d_out[2], S, K, stream=streams[1].cuda_stream) == 0
    pin_in = gpu.HostBuffer((S, 1, G))
    pin_in.array[...] = blocks[3]
    assert b.process_block_bus(pin_in.array, K, out=host_out.array) is host_out.array
    assert same_words(host_out.array, wants[3]), "host entry behind two device-entry blocks"
    assert b.sync() == 0
    assert same_words(fetch(d_out[1]), wants[1]) and same_words(fetch(d_out[2]), wants[2])
    same_state(gpu, b, plain, ["rd", "a", "t", "out", "ccr"], (0, 63, 64, N - 1), tram=1000)
    pin_in.close()
    host_out.close()


def test_refusals_change_nothing(gpu):
    lib = gpu.load()
    N, S, K = 300, 8, 64
    (b,) = handles(gpu, progs.config3(), N, 1, 1)
    G = b.bus_groups(K)
    narrow_in, narrow_out, wide = gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((S, 1, G)), gpu.HostBuffer((2 * S, 1, N))
    narrow_in.array[...] = 0.25
    wide.array[...] = 0.125
    assert b.process_block_bus(narrow_in.array, K, out=narrow_out.array) is not None
    first = narrow_out.array.copy()
    ms = b.last_kernel_ms()
    seen = (b.info("host_staged_blocks"), b.info("host_inplace_blocks"), b.info("bus_blocks"), b.instruction_counter())
    p = lambda h, off=0: C.c_void_p(h.array.ctypes.data + 4 * off)
    host, dev = lib.fxb_process_block_bus, lib.fxb_process_block_bus_dev
    refused = {
        "group 0": lambda: host(b._h, p(narrow_in), p(narrow_out), S, 0, 3),
        "group below 0": lambda: host(b._h, p(narrow_in), p(narrow_out), S, -64, 3),
        "group 0 without flags": lambda: host(b._h, p(wide), p(wide), S, 0, 0),
        "unknown flag bit": lambda: host(b._h, p(narrow_in), p(narrow_out), S, K, 4),
        "unknown flag bits": lambda: host(b._h, p(narrow_in), p(narrow_out), S, K, 0x80000003),
        "null in": lambda: host(b._h, None, p(narrow_out), S, K, 3),
        "null out": lambda: host(b._h, p(narrow_in), None, S, K, 3),
        "one buffer, two layouts (shared in)": lambda: host(b._h, p(wide), p(wide), S, K, SHARED_IN),
        "one buffer, two layouts (mix out)": lambda: host(b._h, p(wide), p(wide), S, K, MIX_OUT),
        "one layout, shifted": lambda: host(b._h, p(wide), p(wide, 3), S, K, 3),
        "out inside in": lambda: host(b._h, p(wide), p(wide, S * N - 1), S, K, MIX_OUT),
        "in inside out": lambda: host(b._h, p(wide, S * N - 1), p(wide), S, K, SHARED_IN),
        "device entry: group 0": lambda: dev(b._h, p(narrow_in), p(narrow_out), S, 0, 3, None),
        "device entry: unknown flag bit": lambda: dev(b._h, p(narrow_in), p(narrow_out), S, K, 8, None),
        "device entry: null": lambda: dev(b._h, p(narrow_in), None, S, K, 3, None),
        "device entry: overlap": lambda: dev(b._h, p(wide), p(wide, 1), S, K, 3, None),
    }
    for what, call in refused.items():
        assert call() == FX_E_ARG and b.last_error(), what
        assert b.last_kernel_ms() == ms, what
        assert (b.info("host_staged_blocks"), b.info("host_inplace_blocks"), b.info("bus_blocks"), b.instruction_counter()) == seen, what
    assert lib.fxb_bus_groups(b._h, 0) == FX_E_ARG and lib.fxb_bus_groups(None, 4) == FX_E_ARG
    # the 2^32 stride limit, applied to every layout: 4 channels x 2^28 columns x 4 bytes (refused in front of everything else)
    big = gpu.Batch(1 << 28, 4, 0)
    for flags in (1, 2, 3):
        for group in (1, 64, 1 << 28):
            assert host(big._h, p(narrow_in), p(narrow_out), 1, group, flags) == FX_E_ARG and "2^32" in big.last_error(), (flags, group)
    assert big.info("bus_blocks") == 0
    big.close()
    # zero samples: lowers the program, returns 0; the handle goes on as one that was never refused anything
    assert host(b._h, None, None, 0, K, 3) == 0 and host(b._h, p(narrow_in), p(narrow_out), 0, K, 3) == 0
    (again,) = handles(gpu, progs.config3(), N, 1, 1)
    assert same_bits(again.process_block_bus(narrow_in.array.copy(), K), first)
    assert same_bits(again.process_block_bus(narrow_in.array.copy(), K), b.process_block_bus(narrow_in.array.copy(), K))
    # ... and footprints that touch without overlapping are fine
    assert host(b._h, p(wide), p(wide, S * N), S, K, MIX_OUT) == 0, b.last_error()
    for h in (narrow_in, narrow_out, wide):
        h.close()


@pytest.mark.parametrize("shards,N", [(2, 64 * 10 + 17), (3, 64 * 16 + 17)])
def test_sharded_handles_equal_the_single_one(gpu, shards, N):
    text = progs.config3()
    names = register_names(gpu, text, 1)
    plan = gpu.shard_plan(N, shards)
    assert all(first % 192 == 0 for first, _ in plan), plan
    S = 33
    for K in (64, 192):
        for pinned in (False, True):
            single = handles(gpu, text, N, 1, 3)
            split = []
            for _ in range(3):
                b = gpu.Batch(N, 1, devices=[0] * shards)
                assert b.load_text(text), b.errors()
                assert b.set_register_array("cutoff", cutoffs(N)) == 0
                split.append(b)
            G = split[0].bus_groups(K)
            for block in range(2):
                xg = group_input(G, S, 1, block * S)
                x = expand(xg, K, N)
                for (shared_in, mix_out), one, many in zip(MODES, single, split):
                    want = one.process_block_bus(xg if shared_in else x, K, shared_in, mix_out)
                    if pinned:
                        src, dst = gpu.HostBuffer((S, 1, G if shared_in else N)), gpu.HostBuffer((S, 1, G if mix_out else N))
                        src.array[...] = xg if shared_in else x
                        before = many.info("host_inplace_blocks")
                        got = many.process_block_bus(src.array, K, shared_in, mix_out, out=dst.array).copy()
                        assert many.info("host_inplace_blocks") == before + shards and many.info("host_staged_blocks") == 0
                        src.close()
                        dst.close()
                    else:
                        got = many.process_block_bus(xg if shared_in else x, K, shared_in, mix_out)
                    assert same_bits(got, want), (K, pinned, shared_in, mix_out)
            for one, many in zip(single, split):
                same_state(gpu, many, one, names, (0, 63, 64, plan[1][0], N - 1), tram=1000)
                assert many.info("bus_blocks") == 2 * shards
    # a group size the plan does not divide
    many = gpu.Batch(N, 1, devices=[0] * shards)
    assert many.load_text(text)
    xg = np.zeros((S, 1, many.bus_groups(100)), dtype=np.float32)
    out = np.zeros_like(xg)
    rc = gpu.load().fxb_process_block_bus(many._h, C.c_void_p(xg.ctypes.data), C.c_void_p(out.ctypes.data), S, 100, 3)
    assert rc == FX_E_ARG and "straddles" in many.last_error(), many.last_error()
    assert many.info("bus_blocks") == 0
