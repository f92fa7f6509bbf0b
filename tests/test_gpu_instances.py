"""Per-instance state calls on the GPU: fxb_copy_instances, fxb_reset_instances, fxb_save_instances and fxb_load_instances against
the oracle and against twin handles.  The two kernels move words, so the bar everywhere is equality of 32-bit patterns: a copied
instance must continue exactly like an oracle object that replayed the SOURCE's history, a reset one like a fresh object, a loaded
one like the instance it was saved from - outputs, every register, instruction counter, delay-line positions, delay memory and
LFSR words - and every instance a call did not name must equal a twin handle that made no such call, word for word.  N = 200 is
three wavefronts plus 8 lanes; instances 0, 63, 64, 127, 128, 199 sit on both sides of every wavefront boundary."""
import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
S1, S2 = 1037, 1100   # samples before and after the call under test: delay words written before it are read back after it
NOISE = "input in 0\noutput out 0\nstatic noise\nstatic a\nmacs a, in, noise, 0.5\nmacs out, 0, a, 1.0\nend"


def use_tier(monkeypatch, name):
    """the three kernel tiers, selected through FX_KERNEL as tests/test_gpu_imajor.py does; hip2 / hip4: the HIP C++ kernel with two
    and four instances per lane (delay memory tiled in 128 and 256 columns)"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    if name.startswith("hip") and name != "hip":
        monkeypatch.setenv("FX_KERNEL", "hip")
        monkeypatch.setenv("FX_INST_PER_LANE", name[3:])
    elif name != "xlate":
        monkeypatch.setenv("FX_KERNEL", name)


@pytest.fixture(params=["xlate", "asm", "hip"])
def tier(request, monkeypatch):
    use_tier(monkeypatch, request.param)
    return request.param


def right_tier(b, tier):
    k = b.info("kernel")
    if tier.startswith("hip"):
        return k == 0 and (tier == "hip" or b.info("inst_per_lane") == int(tier[3:]))
    return k >= 9 if tier == "xlate" else 1 <= k < 9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cutoffs(N):
    """one setting per instance: no two instances go through the same filter"""
    return (0.05 + 0.9 * (progs.stimulus(N, 1, seed=4242)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32)


def state_registers(text):
    """every register the program declares as state or control, its output latch and the condition register"""
    names = ["out", "ccr"]
    for line in text.split("\n"):
        w = line.split()
        if len(w) >= 2 and w[0] in ("static", "control") and w[1] != "noise":
            names.append(w[1])
    return names


def run(b, x, clock=0):
    """x [S, N] through b in uneven blocks; returns [S, N]"""
    out, at, k = [], 0, 0
    sizes = (1, 33, 300, 7, 64, 500)
    while at < x.shape[0]:
        n = min(sizes[k % len(sizes)], x.shape[0] - at)
        out.append(b.process_block(np.ascontiguousarray(x[at:at + n])))
        at += n
        k += 1
    return np.concatenate(out, axis=0)


def handle(gpu, text, N, control=None, values=None, devices=None):
    b = gpu.Batch(N, 1, 0) if devices is None else gpu.Batch(N, 1, devices=devices)
    assert b.load_text(text), b.errors()
    if control:
        assert b.set_register_array(control, values) == 0
    return b


def replay(text, parts, control=None, value=None, writes=()):
    """an oracle object through the concatenated `parts` ([S] each); returns it and its outputs over the LAST part"""
    o = Oracle(1)
    assert o.load_text(text), o.errors()
    for key, v in writes:
        o.set_register(key, float(v))
    if control:
        o.set_register(control, float(value))
    y = None
    for p in parts:
        y = o.process_block(np.ascontiguousarray(p, dtype=np.float32))
    return o, y


def record_of(b, inst):
    """the record of one instance as uint32 words"""
    return b.save_instances([inst])[64:].view(np.uint32)


def lfsr_of(b, inst):
    at = b.info("num_registers") + b.channels + 4   # state rows: registers, latches, four positions, two LFSR words
    return [int(v) for v in record_of(b, inst)[at:at + 2].view(np.int32)]


def equals_oracle(b, inst, o, names, y_gpu, y_ref, tram):
    assert np.array_equal(bits(y_gpu), bits(y_ref)), "instance %d: outputs" % inst
    for r in names:
        assert b.get_register_bits_i(r, inst) == o.get_register_bits(r), "instance %d register %s" % (inst, r)
    assert b.instruction_counter_i(inst) == o.instruction_counter(), inst
    assert b.get_cursors_i(inst) == o.cursors(), inst
    assert lfsr_of(b, inst) == o.lfsr(), inst
    for which, n in tram:
        assert np.array_equal(bits(b.get_tram_i(which, inst, n)), bits(o.tram(which, n))), "instance %d delay memory %d" % (inst, which)


PROGRAMS = {
    # name: (text, per-instance control, delay memory to compare [(which, words)])
    "config3": (progs.config3, "cutoff", [(0, 1000)]),
    "config5": (progs.config5, "damp", [(1, 8192)]),
}


def copy_against_the_oracle(gpu, tier, name, N, pairs, devices=None):
    make, control, tram = PROGRAMS[name]
    text = make()
    cut = cutoffs(N)
    b, twin = handle(gpu, text, N, control, cut, devices), handle(gpu, text, N, control, cut)
    x1, x2 = progs.stimulus(N, S1), progs.stimulus(N, S2, first_sample=S1, seed=99)
    y1 = run(b, x1)
    assert np.array_equal(bits(y1), bits(run(twin, x1))) and right_tier(twin, tier), twin.tier_note()
    gathers, scatters = b.info("instance_gathers"), b.info("instance_scatters")
    src, dst = [s for s, _ in pairs], [d for _, d in pairs]
    assert b.copy_instances(src, dst) == 0
    y2, t2 = run(b, x2), run(twin, x2)
    assert b.info("instance_gathers") > gathers and b.info("instance_scatters") > scatters
    names = state_registers(text)
    for s, d in pairs:
        o, ref = replay(text, [x1[:, s], x2[:, d]], control, cut[s])
        equals_oracle(b, d, o, names + [control], y2[:, d], ref, tram)
    # every instance the copy did not name: the twin's words - outputs, registers, counters, positions, delay memory
    rest = np.setdiff1d(np.arange(N), dst)
    assert np.array_equal(bits(y2[:, rest]), bits(t2[:, rest]))
    for r in names + [control]:
        assert np.array_equal(bits(b.get_register_array(r))[rest], bits(twin.get_register_array(r))[rest]), r
    image, timage = b.save_instances(rest), twin.save_instances(rest)
    assert np.array_equal(image, timage), "an instance outside the destination list changed"
    return b, twin


def pairs_for(N):
    return [(0, 64), (63, N - 1), (128, 1), (128, 2), (128, 127)]


@pytest.mark.parametrize("name,N", [("config3", 200), ("config5", 130)])
def test_copy_continues_like_the_source(gpu, tier, name, N):
    """1. copy 0 -> 64, 63 -> N - 1 and 128 -> {1, 2, 127} after 1 037 samples in uneven blocks, then 1 100 samples of fresh input"""
    copy_against_the_oracle(gpu, tier, name, N, pairs_for(N))


@pytest.mark.parametrize("lanes", ["hip2", "hip4"])
def test_copy_on_the_hip_tier_with_several_instances_per_lane(gpu, monkeypatch, lanes):
    """4. delay memory tiled in 128 / 256 columns: sources and destinations on both sides of a column-tile boundary"""
    use_tier(monkeypatch, lanes)
    # (no destination is a source: 127 / 129 and 255 / 257 stand on the two sides of the boundaries as sources, 126 / 128 and 254 / 256 as destinations)
    copy_against_the_oracle(gpu, lanes, "config3", 300, [(127, 128), (255, 256), (0, 299), (129, 126), (257, 254), (129, 63)])


def test_copy_across_three_shards_equals_the_single_handle(gpu, tier):
    """5. three shards on the one GPU ([0, 128), [128, 192), [192, 200)): pairs inside a shard and across shards"""
    b, twin = copy_against_the_oracle(gpu, tier, "config3", 200, pairs_for(200), devices=[0, 0, 0])
    assert [f for _, f, _ in b.shards()] == [0, 128, 192]
    one = handle(gpu, progs.config3(), 200, "cutoff", cutoffs(200))
    x1, x2 = progs.stimulus(200, S1), progs.stimulus(200, S2, first_sample=S1, seed=99)
    run(one, x1)
    assert one.copy_instances(*zip(*pairs_for(200))) == 0
    run(one, x2)
    assert np.array_equal(one.save_state(), b.save_state())


def test_reset_without_delay_lines_equals_a_fresh_object(gpu, tier):
    """2a. config2: a broadcast write, a per-instance write and 300 samples, then reset {0, 64, 199}"""
    text, N, group = progs.config2(), 200, [0, 64, 199]
    b = handle(gpu, text, N)
    assert b.set_register("cutoff", 0.3) == 0 and b.set_register_i("cutoff", 64, 0.7) == 0
    x1, x2 = progs.stimulus(N, 300), progs.stimulus(N, 500, first_sample=300, seed=5)
    run(b, x1)
    assert b.reset_instances(group) == 0
    y2 = run(b, x2)
    assert right_tier(b, tier), b.tier_note()
    names = state_registers(text)
    for i in group:
        o, ref = replay(text, [x2[:, i]], writes=[("cutoff", 0.3)])
        equals_oracle(b, i, o, names, y2[:, i], ref, [])
    for i, v in ((1, 0.3), (63, 0.3)):   # an untouched neighbour keeps its history
        o, ref = replay(text, [x1[:, i], x2[:, i]], writes=[("cutoff", v)])
        equals_oracle(b, i, o, names, y2[:, i], ref, [])


def test_reset_with_a_delay_line_keeps_the_positions(gpu, tier):
    """2b. config3 reads and writes its delay line once per sample at offset 0: only the distance between the positions matters,
    so a reset instance sounds like a fresh object although its positions are the neighbours' - and its delay memory is the fresh
    object's, rotated by the kept position"""
    text, N, group = progs.config3(), 200, [0, 64, 199]
    b = handle(gpu, text, N)
    x1, x2 = progs.stimulus(N, S1), progs.stimulus(N, S2, first_sample=S1, seed=5)
    run(b, x1)
    assert b.reset_instances(group) == 0
    y2 = run(b, x2)
    assert right_tier(b, tier), b.tier_note()
    names = state_registers(text)
    for i in group:
        o, ref = replay(text, [x2[:, i]])
        assert np.array_equal(bits(y2[:, i]), bits(ref)), i
        for r in names:
            assert b.get_register_bits_i(r, i) == o.get_register_bits(r), (i, r)
        assert b.instruction_counter_i(i) == o.instruction_counter()
        assert b.get_cursors_i(i) == b.get_cursors_i(i + 1 if i + 1 < N else i - 1), "the positions are the neighbours'"
        shift = (b.get_cursors_i(i)[0] - o.cursors()[0]) % 1000
        assert (b.get_cursors_i(i)[1] - o.cursors()[1]) % 1000 == shift
        assert np.array_equal(bits(b.get_tram_i(0, i, 1000)), np.roll(bits(o.tram(0, 1000)), shift)), i
    o, ref = replay(text, [x1[:, 1], x2[:, 1]])
    equals_oracle(b, 1, o, names, y2[:, 1], ref, [(0, 1000)])


def test_reset_restarts_the_noise_generator(gpu, tier):
    """2c. the LFSR of a reset instance starts again from the reference's seeds"""
    N, group = 200, [0, 64, 199]
    b = handle(gpu, NOISE, N)
    x1, x2 = progs.stimulus(N, 100), progs.stimulus(N, 100, first_sample=100, seed=5)
    run(b, x1)
    assert b.reset_instances(group) == 0
    y2 = run(b, x2)
    for i in group:
        o, ref = replay(NOISE, [x2[:, i]])
        assert np.array_equal(bits(y2[:, i]), bits(ref)) and lfsr_of(b, i) == o.lfsr(), i
    o, ref = replay(NOISE, [x1[:, 63], x2[:, 63]])
    assert np.array_equal(bits(y2[:, 63]), bits(ref)) and lfsr_of(b, 63) == o.lfsr()


def test_save_and_load_between_handles(gpu, tier):
    """3. records of {0, 63, 130} of handle A into {5, 64, 199} of handle B, which ran the same number of samples on other input"""
    text, N = progs.config3(), 200
    cut = cutoffs(N)
    A, B, T = (handle(gpu, text, N, "cutoff", cut) for _ in range(3))
    xa, xb = progs.stimulus(N, S1), progs.stimulus(N, S1, seed=31)
    run(A, xa)
    run(B, xb)
    run(T, xb)
    src, dst = [0, 63, 130], [5, 64, 199]
    image = A.save_instances(src)
    assert image.size == A.instance_image_size(3) and B.load_instances(dst, image) == 0 and T.load_instances(dst, image) == 0
    x2 = progs.stimulus(N, S2, first_sample=S1, seed=99)
    run(A, x2)
    y2 = run(B, x2[:, ::-1])
    run(T, x2[:, ::-1])
    assert right_tier(B, tier), B.tier_note()
    names = state_registers(text)
    for s, d in zip(src, dst):
        o, ref = replay(text, [xa[:, s], x2[:, N - 1 - d]], "cutoff", cut[s])
        equals_oracle(B, d, o, names, y2[:, d], ref, [(0, 1000)])
    o, ref = replay(text, [xb[:, 6], x2[:, N - 1 - 6]], "cutoff", cut[6])
    equals_oracle(B, 6, o, names, y2[:, 6], ref, [(0, 1000)])
    # B one block ahead of A: the positions differ, the load is refused and changes nothing
    x3 = progs.stimulus(N, 32, first_sample=S1 + S2, seed=7)
    run(B, x3)
    run(T, x3)
    with pytest.raises(RuntimeError, match="positions"):
        B.load_instances(dst, A.save_instances(src))
    x4 = progs.stimulus(N, 64, first_sample=S1 + S2 + 32, seed=8)
    assert np.array_equal(bits(run(B, x4)), bits(run(T, x4))) and np.array_equal(B.save_state(), T.save_state())


def test_load_without_delay_lines_at_any_time(gpu, tier):
    """3. config2 executes no delay-line instruction: its records load into a handle that has run another number of samples"""
    text, N = progs.config2(), 200
    cut = cutoffs(N)
    A, B = handle(gpu, text, N, "cutoff", cut), handle(gpu, text, N, "cutoff", cut)
    xa, xb = progs.stimulus(N, 300), progs.stimulus(N, 411, seed=31)
    run(A, xa)
    run(B, xb)
    assert B.load_instances([5, 64, 199], A.save_instances([0, 63, 130])) == 0
    x2 = progs.stimulus(N, 200, first_sample=500, seed=99)
    y2 = run(B, x2)
    names = state_registers(text)
    for s, d in zip([0, 63, 130], [5, 64, 199]):
        o, ref = replay(text, [xa[:, s], x2[:, d]], "cutoff", cut[s])
        equals_oracle(B, d, o, names, y2[:, d], ref, [])


def test_meters_are_left_alone(gpu, tier):
    """6. copy and reset change no meter: every instance reads as on a twin that made neither call"""
    text, N = progs.config3(), 200
    b, twin = handle(gpu, text, N), handle(gpu, text, N)
    x = progs.stimulus(N, 333)
    for h in (b, twin):
        assert h.meter_enable(True) == 0
        run(h, x)
    assert b.copy_instances([0, 63], [64, 199]) == 0 and b.reset_instances([1, 128]) == 0
    got, want = b.meter_read(), twin.meter_read()
    for k in want:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert b.meter_samples() == twin.meter_samples() == 333


def test_copy_in_front_of_a_block_with_a_control_track(gpu, tier):
    """6. a copy followed directly by a block with a schedule armed: the destination follows the oracle through the changes"""
    text, N = progs.config3(), 200
    b = handle(gpu, text, N)
    x1, x2 = progs.stimulus(N, S1), progs.stimulus(N, 48, first_sample=S1, seed=99)
    run(b, x1)
    assert b.copy_instances([0, 63], [64, 199]) == 0
    steps = [0.2, 0.4, 0.6]
    assert b.set_register_track("cutoff", steps, 16) == 0
    y2 = b.process_block(x2)
    for s, d in ((0, 64), (63, 199), (5, 5)):
        o = Oracle(1)
        assert o.load_text(text)
        o.process_block(x1[:, s].copy())
        ref = []
        for k, v in enumerate(steps):
            o.set_register("cutoff", v)
            ref.append(o.process_block(x2[16 * k:16 * k + 16, d].copy()))
        assert np.array_equal(bits(y2[:, d]), bits(np.concatenate(ref))), (s, d)
        assert b.instruction_counter_i(d) == o.instruction_counter()


def test_nan_payloads_survive_as_patterns(gpu):
    """7. words no float operation would preserve (quiet and signalling NaNs with payloads) in registers and delay memory, put there
    through fxb_load_state, come out of copy and save / load bit for bit"""
    text, N = progs.config3(), 200
    b = handle(gpu, text, N)
    run(b, progs.stimulus(N, 64))
    raw = b.save_state()
    n = int(raw[8:16].view(np.int64)[0])
    regs, rows, islots = (int(raw[o:o + 4].view(np.int32)[0]) for o in (20, 24, 28))
    assert n == N and islots >= 1000
    body = raw[64:].view(np.uint32)
    state, tram = body[:rows * N].reshape(rows, N), body[rows * N:rows * N + N * islots].reshape(N, islots)
    f = gpu.FrontEnd(1)
    assert f.load_text(text)
    row = [r[0] for r in f.registers()].index("s5")
    assert row < regs
    for i, inst in enumerate((0, 63, 128)):
        state[row, inst] = 0x7FC0DEAD + i
        tram[inst, 3::97] = 0x7F800001 + i       # signalling
        tram[inst, 5::89] = 0xFFC12345 + i       # quiet, negative, with a payload
    assert b.load_state(raw) == 0

    def records():
        img = b.save_state()[64:].view(np.uint32)
        return np.concatenate([img[:rows * N].reshape(rows, N).T, img[rows * N:].reshape(N, -1)], axis=1)

    before = records()
    assert before[0, row] == 0x7FC0DEAD and before[63, rows + 3] == 0x7F800002
    assert b.copy_instances([0, 63, 128, 128], [64, 199, 1, 127]) == 0
    image = b.save_instances([0, 63, 128])
    assert np.array_equal(image[64:].view(np.uint32).reshape(3, -1), before[[0, 63, 128]])
    assert b.load_instances([2, 3, 4], image) == 0
    after = records()
    want = before.copy()
    want[[64, 199, 1, 127, 2, 3, 4]] = before[[0, 63, 128, 128, 0, 63, 128]]
    assert np.array_equal(after, want)
