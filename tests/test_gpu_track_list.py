"""Register tracks by list on the GPU: fxb_set_register_tracks_list (kernels fx_track_hold / fx_track_scatter in csrc/fx_tracks.hip;
the generated loop re-loads the expanded rows by itself).  The bar everywhere is equality of 32-bit patterns with the TWIN of the
definition in include/fx8010_amd.h "Register tracks by list": a second handle whose blocks the test cuts at every sample where a
step falls due, with fxb_set_registers_list in front of each piece - PCM, every register row and save_state() - on the translated
tier and with FX_KERNEL=asm / hip; and with oracle objects that get setRegisterValue for the listed voices in front of the due
process() call.  N = 200 (three full wavefronts and a ragged one), S = 32 and 45.  The host's bookkeeping without a GPU is
tests/test_track_list_stub.py."""
import re

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle
from quiet_programs import GENERATED
from test_gpu_bus import bits, register_names
from test_gpu_bus_gain import kernel_tier, right_tier  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

N = 200
# +0, -0, the smallest denormal, the largest (negative), +-1e30, a quiet NaN with a payload
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7149f2ca, 0xf149f2ca, 0x7fc12345], dtype=np.uint32).view(np.float32)
# (first, period, steps) for S = 32: (3, 5, 9) runs past the block, (32, 1, 1) has nothing due, (31, 7, 2) one step inside
SHAPES = ((0, 8, 4), (0, 1, 32), (13, 1, 1), (3, 5, 9), (32, 1, 1), (31, 7, 2))

# a one-pole filter whose coefficient and whose output gain are controls read as plain operands
SMALL = ("input in 0\noutput out 0\ncontrol coef = 0.5\ncontrol gain = 0.25\ncontrol trim = 0.75\nstatic a\nstatic b\n"
         "interp a, a, coef, in\nmacs b, a, trim, 0.5\nmacs out, 0, b, gain\nend")
# a quiet-loop program that reads its control `k` as an operand and has a delay line
QUIET = next(text for _, text in GENERATED if re.search(r", k\b", text) and "xdelay" in text)
PROGRAMS = {
    "small": (SMALL, ["coef", "gain"], "trim", 0.9),
    "config3": (progs.config3(), ["cutoff", "fb"], None, 0.9),   # the committed delay-line program: events meet the hoisted TRAM reads
    "quiet": (QUIET, ["k"], None, 0.2),                          # a quiet-loop program: the twin runs its quiet loop between the cuts
}


def stimulus(S, first, level, n=N):
    return np.ascontiguousarray(progs.stimulus(n, S, first_sample=first) * np.float32(level / 0.9), dtype=np.float32)


def a_list(rng, n, count):
    if count >= n:
        return rng.permutation(n).astype(np.int64)
    if count == 1:
        return np.array([n - 1], dtype=np.int64)
    return rng.permutation(np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:count - 2]])).astype(np.int64)


def step_values(rng, steps, n_keys, count, special=True):
    """[steps, n_keys, count] settings in (0, 1) with the specials walking through the columns from one step to the next: a
    wavefront leaves the fast stream at an event"""
    v = rng.uniform(0.02, 0.98, (steps, n_keys, count)).astype(np.float32)
    if special:
        for q in range(steps):
            for k in range(n_keys):
                for j, s in enumerate(SPECIALS):
                    if (q + j) % 3 == 0:
                        v[q, k, (q + k + j * 3) % count] = s
    return v


class Schedule:
    def __init__(self, keys, L, v, first, period):
        self.keys, self.L, self.v, self.first, self.period = list(keys), np.ascontiguousarray(L, dtype=np.int64), np.ascontiguousarray(v, dtype=np.float32), first, period

    def due(self, S):
        return [self.first + q * self.period for q in range(self.v.shape[0]) if self.first + q * self.period < S]


def cut_block(t, x, schedules, dense=None, broadcast=None):
    """the twin of the definition: the block cut at every due sample, fxb_set_registers_list in front of each piece in arming
    order (a dense / broadcast track (key, values, period) is written through set_register_array / set_register there)"""
    S = x.shape[0]
    cuts = {0, S}
    for s in schedules:
        cuts |= set(s.due(S))
    for tr in (dense, broadcast):
        if tr:
            cuts |= {q * tr[2] for q in range(len(tr[1])) if q * tr[2] < S}
    cuts = sorted(cuts)
    y = np.zeros_like(x)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if dense and lo % dense[2] == 0 and lo // dense[2] < len(dense[1]):
            assert t.set_register_array(dense[0], dense[1][lo // dense[2]]) == 0
        if broadcast and lo % broadcast[2] == 0 and lo // broadcast[2] < len(broadcast[1]):
            assert t.set_register(broadcast[0], float(broadcast[1][lo // broadcast[2]])) == 0
        for s in schedules:
            if lo in s.due(S):
                assert t.set_registers_list(s.keys, s.L, s.v[(lo - s.first) // s.period]) == 0
        y[lo:hi] = t.process_block(x[lo:hi])
    return y


def same_handles(b, t, names, what):
    for r in names:
        assert np.array_equal(bits(b.get_register_array(r)), bits(t.get_register_array(r))), (what, "register " + r)
    assert np.array_equal(b.save_state(), t.save_state()), (what, "save_state")


def pair(gpu, text, n=N, devices=None, spread=None):
    ch = 1
    b = gpu.Batch(n, ch, 0) if devices is None else gpu.Batch(n, ch, devices=devices)
    t = gpu.Batch(n, ch, 0)
    for h in (b, t):
        assert h.load_text(text), h.errors()
        if spread:   # the voices differ before anything is armed: the held rows are not constants
            for k, key in enumerate(spread):
                assert h.set_register_array(key, np.linspace(0.1 + 0.05 * k, 0.9 - 0.05 * k, n).astype(np.float32)) == 0
    return b, t


GRID = [(tier, name) for tier in ("default", "asm", "hip") for name in PROGRAMS]


@pytest.mark.parametrize("kernel_tier,name", GRID, indirect=["kernel_tier"], ids=["%s-%s" % g for g in GRID])
def test_list_schedules_equal_the_cut_block_twin_bit_for_bit(gpu, kernel_tier, name):
    """every schedule shape for S = 32 and 45 with lists of 1, 2, 63, 64, 65 and all N voices, one and two keys, NaN with payload, -0
    and denormals among the step values; two schedules on one register with disjoint lists and interleaved events; a list
    schedule beside a dense per-instance and a broadcast track due at the same samples; FXB_INFO_TRACK_LIST_EXPANDS"""
    text, keys, third, level = PROGRAMS[name]
    rng = np.random.default_rng(sum(map(ord, kernel_tier + name)))
    names = register_names(gpu, text, 1)
    b, t = pair(gpu, text, spread=keys)
    clock, expands = 0, 0
    sizes = (1, 2, 63, 64, 65, N)

    def block(S, schedules, what, **tracks):
        nonlocal clock, expands
        for tr in tracks.values():
            assert b.set_register_track(tr[0], tr[1], tr[2]) == 0
        for s in schedules:
            assert b.set_register_tracks_list(s.keys, s.L, s.v, first=s.first, period=s.period) == 0, (what, b.last_error())
        x = stimulus(S, clock, level)
        clock += S
        got = b.process_block(x)
        want = cut_block(t, x, schedules, **tracks)
        assert np.array_equal(bits(got), bits(want)), (what, "PCM")
        same_handles(b, t, names, what)
        if kernel_tier == "default" and any(s.due(S) for s in schedules):
            expands += 1
        assert b.info("track_list_expands") == expands, what

    step = 0
    for S in (32, 45):
        for first, period, steps in SHAPES:
            L = a_list(rng, N, sizes[step % 6])
            k = keys[:1 + step % len(keys)] if step % 2 else keys[-1:]
            step += 1
            block(S, [Schedule(k, L, step_values(rng, steps, len(k), L.size), first, period)], (S, L.size, first, period, steps))
        perm = rng.permutation(N).astype(np.int64)
        block(S, [Schedule(keys[:1], perm[:65], step_values(rng, 4, 1, 65), 0, 8), Schedule(keys[::-1], perm[65:130], step_values(rng, 9, len(keys), 65), 3, 5),
                  Schedule(keys[:1], perm[130:131], step_values(rng, 1, 1, 1), 13, 1)], ("interleaved", S))
    if third:
        dense = (keys[1], rng.uniform(0.1, 0.9, (4, N)).astype(np.float32), 8)
        broadcast = (third, np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32), 8)
        block(32, [Schedule(keys[:1], a_list(rng, N, 64), step_values(rng, 4, 1, 64), 0, 8)], "three kinds", dense=dense, broadcast=broadcast)
    assert right_tier(b, kernel_tier) and right_tier(t, kernel_tier), b.tier_note()
    if name == "quiet" and kernel_tier == "default":
        # (the translator plans no quiet loop for code with a trackable register - fxp_quiet_plan: "a control track is armed" - so
        # the handle runs the steady loop here while the twin, which has no trackable register, is free to run its quiet loop)
        assert b.info("xlate_quiet") in (0, 1)
    assert b.ood_flags() == t.ood_flags()
    for h in (b, t):
        h.close()


@pytest.mark.parametrize("name", ["small", "config3"])
def test_list_schedules_against_the_oracle(gpu, monkeypatch, name):
    """the translated tier against oracle objects, one per instance, that get setRegisterValue for the listed voices in front of
    the due process() call: every instance, every sample, for blocks of 32 and 45 samples with two schedules each"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    text, keys, _, level = PROGRAMS[name]
    rng = np.random.default_rng(77)
    b = gpu.Batch(N, 1, 0)
    assert b.load_text(text), b.errors()
    oracles = []
    for _ in range(N):
        o = Oracle(1)
        assert o.load_text(text), o.errors()
        oracles.append(o)
    clock = 0
    for S in (32, 45, 32):
        perm = rng.permutation(N).astype(np.int64)
        schedules = [Schedule(keys, np.concatenate([[0, 63, 64, 127, 128, N - 1], perm[(perm > 128) & (perm < N - 1)][:14]]).astype(np.int64), None, 0, 8),
                     Schedule(keys[:1], perm[(perm > 0) & (perm < 63)][:30], None, 13, 7)]
        for s, steps in zip(schedules, (4, 3)):
            s.v = step_values(rng, steps, len(s.keys), s.L.size, special=False)
            assert b.set_register_tracks_list(s.keys, s.L, s.v, first=s.first, period=s.period) == 0, b.last_error()
        x = stimulus(S, clock, level)
        clock += S
        y = b.process_block(x)
        cuts = sorted({0, S} | {d for s in schedules for d in s.due(S)})
        for inst, o in enumerate(oracles):
            ref = np.zeros(S, dtype=np.float32)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                for s in schedules:
                    at = np.flatnonzero(s.L == inst)
                    if lo in s.due(S) and at.size:
                        for k, key in enumerate(s.keys):
                            o.set_register(key, float(s.v[(lo - s.first) // s.period, k, at[0]]))
                ref[lo:hi] = o.process_block(np.ascontiguousarray(x[lo:hi, inst]))
            assert np.array_equal(bits(y[:, inst]), bits(ref)), "instance %d, S %d" % (inst, S)
            for key in keys:
                assert b.get_register_bits_i(key, inst) == o.get_register_bits(key), (inst, key)
    assert b.info("kernel") >= 9 and b.info("track_list_expands") == 3, b.tier_note()
    b.close()


def test_list_schedule_between_blocks_on_two_caller_streams(gpu, monkeypatch):
    """a block queued on stream A, a schedule armed, the next block on stream B, another schedule, a block on the handle's own
    stream: the first block keeps what it was queued with, the others have their steps"""
    import torch

    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    text, keys, _, level = PROGRAMS["small"]
    S = 32
    rng = np.random.default_rng(5)
    names = register_names(gpu, text, 1)
    b, t = pair(gpu, text, spread=keys)
    warm = Schedule(keys, a_list(rng, N, 3), step_values(rng, 1, 2, 3), 0, 1)   # (rows, code and staging exist before anything is queued)
    assert b.set_register_tracks_list(warm.keys, warm.L, warm.v) == 0
    x0 = stimulus(8, 0, level)
    assert np.array_equal(bits(b.process_block(x0)), bits(cut_block(t, x0, [warm])))
    blocks = [stimulus(S, 8 + k * S, level) for k in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = [torch.from_numpy(x.reshape(S, 1, N)).to("cuda") for x in blocks]
    d_out = [torch.full((S, 1, N), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    one = Schedule(keys, a_list(rng, N, 65), step_values(rng, 4, 2, 65), 0, 8)
    two = Schedule(keys[:1], a_list(rng, N, 64), step_values(rng, 9, 1, 64), 3, 5)
    assert b.process_block_dev_pitched(d_in[0], d_out[0], S, stream=streams[0].cuda_stream) == 0
    assert b.set_register_tracks_list(one.keys, one.L, one.v, first=one.first, period=one.period) == 0
    assert b.process_block_dev_pitched(d_in[1], d_out[1], S, stream=streams[1].cuda_stream) == 0
    assert b.set_register_tracks_list(two.keys, two.L, two.v, first=two.first, period=two.period) == 0
    assert b.process_block_dev_pitched(d_in[2], d_out[2], S) == 0
    assert b.sync() == 0
    want = [cut_block(t, blocks[0], []), cut_block(t, blocks[1], [one]), cut_block(t, blocks[2], [two])]
    for k in range(3):
        assert np.array_equal(bits(d_out[k].cpu().numpy().reshape(S, N)), bits(want[k])), "block %d: the values it was queued with" % k
    same_handles(b, t, names, "after the streams")
    assert b.info("track_list_expands") == 3
    for h in (b, t):
        h.close()


def test_list_schedule_through_the_bus_and_the_instance_major_entries(gpu, monkeypatch):
    """fxb_process_block_bus (a shared input per group of 8, the mixed output) and fxb_process_block_imajor, once each, against the
    same entry of the twin cut at the due samples"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    text, keys, _, level = PROGRAMS["small"]
    S, K = 32, 8
    rng = np.random.default_rng(6)
    names = register_names(gpu, text, 1)
    b, t = pair(gpu, text, spread=keys)
    s = Schedule(keys, a_list(rng, N, 65), step_values(rng, 4, 2, 65, special=False), 3, 8)
    cuts = sorted({0, S} | set(s.due(S)))

    def twin(x, entry, axis):
        pieces = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if lo in s.due(S):
                assert t.set_registers_list(s.keys, s.L, s.v[(lo - s.first) // s.period]) == 0
            pieces.append(entry(t, np.ascontiguousarray(np.take(x, np.arange(lo, hi), axis=axis))))
        return np.concatenate(pieces, axis=axis)

    G = -(-N // K)
    xg = stimulus(S, 0, level, n=G)
    assert b.set_register_tracks_list(s.keys, s.L, s.v, first=s.first, period=s.period) == 0
    got = b.process_block_bus(xg, K)
    assert np.array_equal(bits(got), bits(twin(xg, lambda h, x: h.process_block_bus(x, K), 0))), "bus block"
    same_handles(b, t, names, "bus block")
    xi = np.ascontiguousarray(stimulus(S, S, level).T.reshape(N, S, 1))
    assert b.set_register_tracks_list(s.keys, s.L, s.v, first=s.first, period=s.period) == 0
    got = b.process_block_imajor(xi)
    assert np.array_equal(bits(got), bits(twin(xi, lambda h, x: h.process_block_imajor(x), 1))), "instance-major block"
    same_handles(b, t, names, "instance-major block")
    assert b.info("track_list_expands") == 2
    for h in (b, t):
        h.close()


def test_two_shards_on_one_gpu_equal_the_cut_block_twin(gpu, monkeypatch):
    """devices = [0, 0]: a list wholly inside the last shard (the other launches nothing), lists on both shards"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    text, keys, _, level = PROGRAMS["small"]
    n, S = 64 * 10 + 17, 45
    rng = np.random.default_rng(n)
    names = register_names(gpu, text, 1)
    many, t = pair(gpu, text, n=n, devices=[0, 0], spread=keys)
    (_, _, _), (_, first, count) = many.shards()
    inside = (first + rng.permutation(count)[:65]).astype(np.int64)
    clock = 0
    for L, launches in ((inside, 1), (a_list(rng, n, 130), 2), (a_list(rng, n, n), 2)):
        for f, p, steps in SHAPES[:4]:
            s = Schedule(keys, L, step_values(rng, steps, 2, L.size), f, p)
            before = many.info("track_list_expands")
            assert many.set_register_tracks_list(s.keys, s.L, s.v, first=f, period=p) == 0, many.last_error()
            x = stimulus(S, clock, level, n=n)
            clock += S
            assert np.array_equal(bits(many.process_block(x)), bits(cut_block(t, x, [s]))), (L.size, f, p, steps)
            same_handles(many, t, names, (L.size, f, p, steps))
            assert many.info("track_list_expands") == before + launches, "a shard without entries launches nothing"
    for h in (many, t):
        h.close()
