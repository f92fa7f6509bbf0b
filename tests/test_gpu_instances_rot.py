"""fxb_load_instances_rotated on the GPU: records saved at one delay-line position load at any other, their delay memory rotated by
the kernel fx_inst_scatter_rot.  The bar is that of tests/test_gpu_instances.py (whose helpers these are): equality of 32-bit
patterns.  From the call on the destination must continue exactly like an oracle object that replayed the SAVED instance's history
and then the destination's input - outputs, every register, instruction counter and LFSR words - while its positions stay those of
its neighbours and its delay memory is the oracle's, rolled by the difference of the positions; every instance the call did not
name must equal a twin handle that made no call, word for word."""
import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle
from test_gpu_instances import (S1, S2, bits, cutoffs, handle, lfsr_of, right_tier, run, state_registers, tier,  # noqa: F401 (tier: a fixture)
                                use_tier)

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
HDR = "static a\nstatic b\ninput in 0\noutput out 0\nstatic noise\nstatic rd\ncontrol vol = 0.5\n"
# both lines, tiny and of different size: reads, then writes, every sample (the sizes of test_gpu_parity's delay programs)
TINY = "itramsize 7 \nxtramsize 11 \n" + HDR + "idelay read, rd, at, 0\nxdelay read, b, at, 0\nidelay write, in, at, 0\nxdelay write, rd, at, 0\nmacs out, rd, b, 0.5\nend"
# the read and the write of one line together in a SKIP shadow taken by the sign of the input: both positions move together, and
# differ from instance to instance
SHADOW_BOTH = ("itramsize 7 \n" + HDR + "static t\nmacs t, in, 0, 0\nskip ccr, ccr, 6, 2\nidelay read, rd, at, 0\nidelay write, in, at, 0\n"
               "macs out, rd, a, 0.5\nmacs a, in, 0, 0\nend")
# ... only the read: the two positions drift apart, differently in every instance
SHADOW_READ = ("itramsize 7 \n" + HDR + "static t\nidelay write, in, at, 0\nmacs t, in, 0, 0\nskip ccr, ccr, 6, 1\nidelay read, rd, at, 0\n"
               "macs out, rd, a, 0.5\nmacs a, in, 0, 0\nend")
OFFSET3 = "itramsize 8 \n" + HDR + "idelay read, rd, at, 0\nidelay write, in, at, 3\nmacs out, 0, rd, 1.0\nend"
TWO_READS = "itramsize 8 \n" + HDR + "idelay read, rd, at, 0\nidelay read, b, at, 0\nidelay write, in, at, 0\nmacs out, rd, b, 0.5\nend"
WRITE_IN = "itramsize 16 \ninput in 0\noutput out 0\nstatic rd\nidelay read, rd, at, 0\nidelay write, in, at, 0\nmacs out, rd, 0, 0\nend"
# the DANE vocabulary of tests/test_dane_tram.py: one write tap and read taps at positions of their own, on both lines
TWO_TAPS = ("itramsize 64 \nxtramsize 500 \ninput in 0\noutput out 0\nstatic w\nstatic r1\nstatic r2\nstatic xr\nidelay write, w, at, 0\nidelay read, r1, at, 7\n"
            "idelay read, r2, at, 19\nxdelay write, in, at, 3\nxdelay read, xr, at, 403\nmacs w, in, 0, 0\nmacs out, r1, r2, 0.5\nend")
OPT_DANE = 1


def replay(text, parts, control=None, value=None, dane=False):
    """an oracle object through the concatenated `parts` ([S] each); returns it and its outputs over the LAST part"""
    o = Oracle(1)
    if dane:
        o.set_option(OPT_DANE)
    assert o.load_text(text), o.errors()
    if control:
        o.set_register(control, float(value))
    y = None
    for p in parts:
        y = o.process_block(np.ascontiguousarray(p, dtype=np.float32))
    return o, y


def shifts_between(saved, held, sizes, dane=False):
    """the rotation per line from the positions a record was saved at and those its destination held at the load; both kinds agree"""
    out = []
    for line, z in enumerate(sizes):
        if not z:
            out.append(0)
            continue
        d = (held[2 * line] - saved[2 * line]) % z
        assert dane or (held[2 * line + 1] - saved[2 * line + 1]) % z == d
        out.append(d)
    return out


def continues_like(b, inst, o, names, y_gpu, y_ref, tram, shifts):
    """the comparison of test_gpu_instances.equals_oracle, with the delay memory rolled by `shifts` and without the positions"""
    assert np.array_equal(bits(y_gpu), bits(y_ref)), "instance %d: outputs" % inst
    for r in names:
        assert b.get_register_bits_i(r, inst) == o.get_register_bits(r), "instance %d register %s" % (inst, r)
    assert b.instruction_counter_i(inst) == o.instruction_counter(), inst
    assert lfsr_of(b, inst) == o.lfsr(), inst
    for which, n in tram:
        assert np.array_equal(bits(b.get_tram_i(which, inst, n)), np.roll(bits(o.tram(which, n)), shifts[which])), "instance %d delay memory %d" % (inst, which)


def unlisted_equal_the_twin(b, twin, N, dst, y, t, names):
    rest = np.setdiff1d(np.arange(N), dst)
    assert np.array_equal(bits(y[:, rest]), bits(t[:, rest]))
    for r in names:
        assert np.array_equal(bits(b.get_register_array(r))[rest], bits(twin.get_register_array(r))[rest]), r
    assert np.array_equal(b.save_instances(rest), twin.save_instances(rest)), "an instance outside the destination list changed"


def undo(gpu, tier, name, N, src, dst, first=S1, later=S2, devices=None):
    """save `src` after `first` samples, run `later` more, load into `dst` of the same handle, continue on fresh input"""
    make, control, tram = {"config3": (progs.config3, "cutoff", [(0, 1000)]), "config5": (progs.config5, "damp", [(1, 8192)])}[name]
    sizes = (1000, 0) if name == "config3" else (0, 8192)
    text = make()
    cut = cutoffs(N)
    b, twin = handle(gpu, text, N, control, cut, devices), handle(gpu, text, N, control, cut)
    x1, x2, x3 = progs.stimulus(N, first), progs.stimulus(N, later, first_sample=first, seed=99), progs.stimulus(N, 300, first_sample=first + later, seed=7)
    assert np.array_equal(bits(run(b, x1)), bits(run(twin, x1))) and right_tier(twin, tier), twin.tier_note()
    image = b.save_instances(src)
    saved = [b.get_cursors_i(s) for s in src]
    run(b, x2)
    run(twin, x2)
    with pytest.raises(RuntimeError, match="positions"):
        b.load_instances(dst, image)
    held = [b.get_cursors_i(d) for d in dst]
    rotations, scatters = b.info("instance_rotations"), b.info("instance_scatters")
    assert b.load_instances_rotated(dst, image) == 0
    assert b.info("instance_rotations") > rotations and b.info("instance_scatters") == scatters
    y3, t3 = run(b, x3), run(twin, x3)
    names = state_registers(text) + [control]
    neighbour = next(i for i in range(N) if i not in dst)
    for k, (s, d) in enumerate(zip(src, dst)):
        o, ref = replay(text, [x1[:, s], x3[:, d]], control, cut[s])
        shifts = shifts_between(saved[k], held[k], sizes)
        assert any(shifts), "the test is about records that stand elsewhere"
        continues_like(b, d, o, names, y3[:, d], ref, tram, shifts)
        assert b.get_cursors_i(d) == b.get_cursors_i(neighbour), "the positions are those of an untouched neighbour"
        for line, z in enumerate(sizes):
            if z:
                assert (b.get_cursors_i(d)[2 * line] - o.cursors()[2 * line]) % z == shifts[line]
    unlisted_equal_the_twin(b, twin, N, dst, y3, t3, names)
    return b, (x1, x2, x3), image


def test_undo_on_one_handle(gpu, tier):
    """1. config3: records of {0, 63, 130} saved after 1 037 samples go into {5, 64, 199} 1 100 samples later (rotation 100)"""
    undo(gpu, tier, "config3", 200, [0, 63, 130], [5, 64, 199])


def test_undo_with_a_wrap_inside_a_word_tile(gpu, tier):
    """2. config5: 8 192 xTRAM words, four reads and four writes per sample; 700 samples later the rotation is 2 800, no multiple
    of 64: the wrap falls inside a tile of 64 record words"""
    b, _, _ = undo(gpu, tier, "config5", 130, [0, 63, 129], [5, 64, 128], later=700)
    assert b.info("instance_rings") == 2


def test_two_tiny_lines_at_once(gpu, tier):
    """3. lines of 7 and 11 slots: saves at ages 3, 5 and 10 loaded at age 23 (three calls, another rotation on each line), then 66
    records in one call: two entry tiles"""
    N = 70
    b, twin = handle(gpu, TINY, N), handle(gpu, TINY, N)
    assert b.info("instance_rings") == 3
    x = progs.stimulus(N, 60)
    ages, images = (3, 5, 10), {}
    at = 0
    for age in ages + (23,):
        for h in (b, twin):
            run(h, x[at:age])
        at = age
        if age != 23:
            images[age] = b.save_instances([age]), b.save_instances(np.arange(66))
    dst = {3: 0, 5: 64, 10: 69}
    for age in ages:
        assert (23 - age) % 7 != (23 - age) % 11
        assert b.load_instances_rotated([dst[age]], images[age][0]) == 0
    y, t = run(b, x[23:30]), run(twin, x[23:30])
    assert right_tier(b, tier) and right_tier(twin, tier), b.tier_note()
    names = state_registers(TINY)
    for age in ages:
        o, ref = replay(TINY, [x[:age, age], x[23:30, dst[age]]])
        continues_like(b, dst[age], o, names, y[:, dst[age]], ref, [(0, 7), (1, 11)], [(23 - age) % 7, (23 - age) % 11])
        assert b.get_cursors_i(dst[age]) == b.get_cursors_i(1)
    unlisted_equal_the_twin(b, twin, N, list(dst.values()), y, t, names)
    into = np.arange(4, 70)
    assert b.load_instances_rotated(into, images[10][1]) == 0
    y = run(b, x[30:45])
    for s, d in zip(range(66), into):
        o, ref = replay(TINY, [x[:10, s], x[30:45, d]])
        continues_like(b, d, o, names, y[:, d], ref, [(0, 7), (1, 11)], [20 % 7, 20 % 11])


def test_positions_that_differ_per_instance(gpu, tier):
    """4. delay instructions in a SKIP shadow: every instance has positions of its own.  Read and write in one shadow move together
    and a record loads anywhere; with only the read in the shadow a pair whose two shifts disagree is refused, nothing changed"""
    N = 130
    x = progs.stimulus(N, 140)
    b = handle(gpu, SHADOW_BOTH, N)
    run(b, x[:40])
    src, dst = [0, 63, 64, 129], [65, 1, 128, 62]
    image = b.save_instances(src)
    saved = [b.get_cursors_i(s) for s in src]
    run(b, x[40:90])
    held = [b.get_cursors_i(d) for d in dst]
    assert len({tuple(c) for c in held}) > 1, "the positions differ from instance to instance"
    assert b.load_instances_rotated(dst, image) == 0
    y = run(b, x[90:])
    assert right_tier(b, tier), b.tier_note()
    names = state_registers(SHADOW_BOTH)
    some = False
    for k, (s, d) in enumerate(zip(src, dst)):
        o, ref = replay(SHADOW_BOTH, [x[:40, s], x[90:, d]])
        shifts = shifts_between(saved[k], held[k], (7, 0))
        some = some or shifts[0] != 0
        continues_like(b, d, o, names, y[:, d], ref, [(0, 7)], shifts)
    assert some
    o, ref = replay(SHADOW_BOTH, [x[:, 2]])
    assert np.array_equal(bits(y[:, 2]), bits(ref[90:]))
    # only the read in the shadow
    c, twin = handle(gpu, SHADOW_READ, N), handle(gpu, SHADOW_READ, N)
    for h in (c, twin):
        run(h, x[:90])
    assert right_tier(c, tier) and right_tier(twin, tier), c.tier_note()
    cur = [c.get_cursors_i(i) for i in range(N)]
    s, d = next((s, d) for s in range(N) for d in range(N) if s != d and (cur[d][0] - cur[s][0]) % 7 != (cur[d][1] - cur[s][1]) % 7)
    one, image = np.array([d], dtype=np.int64), c.save_instances([s])
    rc = c._lib.fxb_load_instances_rotated(c._h, one.ctypes.data, 1, image.ctypes.data, image.size)
    assert rc == FX_E_ARG and "iTRAM" in c.last_error() and "entry 0" in c.last_error(), c.last_error()
    assert np.array_equal(c.save_state(), twin.save_state()) and c.info("instance_rotations") == 0
    # (the write is unconditional: every instance writes at one place, so a pair loads only where the read positions agree too)
    s, d = next((s, d) for s in range(N) for d in range(N) if s != d and cur[d] == cur[s])
    assert c.load_instances_rotated([d], c.save_instances([s])) == 0
    y = run(c, x[90:])
    o, ref = replay(SHADOW_READ, [x[:90, s], x[90:, d]])
    continues_like(c, d, o, state_registers(SHADOW_READ), y[:, d], ref, [(0, 7)], shifts_between(cur[s], cur[d], (7, 0)))


@pytest.mark.parametrize("lanes", ["hip2", "hip4"])
def test_undo_on_the_hip_tier_with_several_instances_per_lane(gpu, monkeypatch, lanes):
    """5. delay memory tiled in 128 / 256 columns: sources and destinations on both sides of the column-tile boundaries"""
    use_tier(monkeypatch, lanes)
    undo(gpu, lanes, "config3", 300, [126, 129, 254, 257], [127, 128, 255, 256])


def test_undo_across_three_shards_equals_the_single_handle(gpu, tier):
    """6. three shards on the one GPU ([0, 128), [128, 192), [192, 200)): the same calls leave the single handle's image"""
    src, dst = [0, 63, 130, 199], [5, 64, 192, 129]
    b, (x1, x2, x3), _ = undo(gpu, tier, "config3", 200, src, dst, devices=[0, 0, 0])
    assert [f for _, f, _ in b.shards()] == [0, 128, 192]
    one = handle(gpu, progs.config3(), 200, "cutoff", cutoffs(200))
    run(one, x1)
    image = one.save_instances(src)
    run(one, x2)
    assert one.load_instances_rotated(dst, image) == 0
    run(one, x3)
    assert np.array_equal(one.save_state(), b.save_state())


def test_between_two_handles_of_different_age(gpu, tier):
    """7. records of {0, 63, 130} of handle A after 1 037 samples into {5, 64, 199} of handle B, which has run 1 500 samples of
    other input"""
    text, N = progs.config3(), 200
    cut = cutoffs(N)
    A, B, T = (handle(gpu, text, N, "cutoff", cut) for _ in range(3))
    xa, xb = progs.stimulus(N, S1), progs.stimulus(N, 1500, seed=31)
    run(A, xa)
    run(B, xb)
    run(T, xb)
    src, dst = [0, 63, 130], [5, 64, 199]
    image = A.save_instances(src)
    assert B.load_instances_rotated(dst, image) == 0
    x2 = progs.stimulus(N, 300, first_sample=1500, seed=99)
    y2, t2 = run(B, x2), run(T, x2)
    assert right_tier(B, tier), B.tier_note()
    names = state_registers(text) + ["cutoff"]
    for s, d in zip(src, dst):
        o, ref = replay(text, [xa[:, s], x2[:, d]], "cutoff", cut[s])
        continues_like(B, d, o, names, y2[:, d], ref, [(0, 1000)], [(1500 - S1) % 1000, 0])
        assert B.get_cursors_i(d) == B.get_cursors_i(6)
    unlisted_equal_the_twin(B, T, N, dst, y2, t2, names)


def test_refusals_and_rings(gpu, tier):
    """8. a line written at offset 3 is no ring: refused at another age, naming the line, loaded at the same age; two reads and one
    write per sample drift apart: refused where the two shifts disagree.  Nothing changes: save_state equals a twin's"""
    N = 70
    x = progs.stimulus(N, 40)
    for text, ages in ((OFFSET3, (10, 13)), (TWO_READS, (10, 13))):
        A, B, T = (handle(gpu, text, N) for _ in range(3))
        run(A, x[:ages[0]])
        for h in (B, T):
            run(h, x[:ages[1]])
        for h in (A, B, T):
            assert right_tier(h, tier), h.tier_note()
        image = A.save_instances([0, 64])
        dst = np.array([69, 1], dtype=np.int64)
        rc = B._lib.fxb_load_instances_rotated(B._h, dst.ctypes.data, 2, image.ctypes.data, image.size)
        assert rc == FX_E_ARG and "iTRAM" in B.last_error() and "entry 0" in B.last_error(), B.last_error()
        with pytest.raises(RuntimeError, match="iTRAM"):
            B.load_instances_rotated(dst, image)
        assert np.array_equal(B.save_state(), T.save_state())
        assert B.info("instance_rotations") == 0 and B.info("instance_rings") == (0 if text is OFFSET3 else 1)
    # the line that is no ring, at equal age
    A, B = handle(gpu, OFFSET3, N), handle(gpu, OFFSET3, N)
    run(A, x[:13])
    run(B, x[:13, ::-1])
    assert B.load_instances_rotated([69, 1], A.save_instances([0, 64])) == 0 and B.info("instance_rotations") == 1
    y = run(B, x[13:])
    assert right_tier(A, tier) and right_tier(B, tier), B.tier_note()
    for s, d in ((0, 69), (64, 1)):
        o, ref = replay(OFFSET3, [x[:13, s], x[13:, d]])
        continues_like(B, d, o, state_registers(OFFSET3), y[:, d], ref, [(0, 8)], [0, 0])
    for text, want in ((progs.config3(), 1), (progs.config5(), 2), (TINY, 3), (progs.config2(), 0), (OFFSET3, 0)):
        h = handle(gpu, text, 64)
        assert h.info("instance_rings") == want and right_tier(h, tier), h.tier_note()


def test_rotation_zero_leaves_the_state_of_the_plain_load(gpu, tier):
    """9. two handles of equal age: one takes load_instances, the other load_instances_rotated"""
    text, N = progs.config3(), 200
    A, B, C = (handle(gpu, text, N, "cutoff", cutoffs(N)) for _ in range(3))
    run(A, progs.stimulus(N, 333))
    for h in (B, C):
        run(h, progs.stimulus(N, 333, seed=31))
    for h in (A, B, C):
        assert right_tier(h, tier), h.tier_note()
    image = A.save_instances([0, 63, 130])
    assert B.load_instances([5, 64, 199], image) == 0 and C.load_instances_rotated([5, 64, 199], image) == 0
    assert np.array_equal(B.save_state(), C.save_state())
    assert (B.info("instance_scatters"), B.info("instance_rotations"), C.info("instance_scatters"), C.info("instance_rotations")) == (1, 0, 0, 1)


def test_dane_model(gpu, tier):
    """10. FX_OPT_TRAM_DANE: one counter per line, every line a ring; ages 100 and 137 differ by no multiple of 64 or 500"""
    N = 130
    x = progs.stimulus(N, 200)
    b = gpu.Batch(N, 1, 0)
    b.set_option(gpu.OPT_TRAM_DANE)
    assert b.load_text(TWO_TAPS), b.errors()
    assert b.info("instance_rings") == 3
    run(b, x[:100])
    src, dst = [0, 63, 129], [64, 128, 1]
    image = b.save_instances(src)
    saved = [b.get_cursors_i(s) for s in src]
    run(b, x[100:137])
    held = [b.get_cursors_i(d) for d in dst]
    assert b.load_instances_rotated(dst, image) == 0
    y = run(b, x[137:])
    assert right_tier(b, tier), b.tier_note()
    names = ["out", "ccr", "w", "r1", "r2", "xr"]
    for k, (s, d) in enumerate(zip(src, dst)):
        o, ref = replay(TWO_TAPS, [x[:100, s], x[137:, d]], dane=True)
        shifts = shifts_between(saved[k], held[k], (64, 500), dane=True)
        assert shifts[0] == (-37) % 64 and shifts[1] == (-37) % 500, "the counters step down once per sample"
        continues_like(b, d, o, names, y[:, d], ref, [(0, 64), (1, 500)], shifts)
    o, ref = replay(TWO_TAPS, [x[:, 2]], dane=True)
    assert np.array_equal(bits(y[:, 2]), bits(ref[137:]))


def test_patterns_survive_the_rotation(gpu, tier):
    """11. NaNs with payloads, a signalling NaN and -0 written into a delay line: the rotated delay memory carries the exact words"""
    N = 70
    x = np.ascontiguousarray(progs.stimulus(N, 30), dtype=np.float32)
    words = np.array([0x7FC0DEAD, 0xFFC12345, 0x7F800001, 0x80000000, 0x7FFFFFFF], dtype=np.uint32)
    x.view(np.uint32)[4:9, :] = words[:, None]
    b = handle(gpu, WRITE_IN, N)
    run(b, x[:12])
    assert right_tier(b, tier), b.tier_note()
    before = bits(b.get_tram_i(0, 0, 16)).copy()
    assert np.array_equal(before[4:9], words), "the delay line holds the words it was fed"
    image = b.save_instances([0])
    run(b, x[12:17])
    assert b.load_instances_rotated([69], image) == 0
    assert np.array_equal(bits(b.get_tram_i(0, 69, 16)), np.roll(before, 5))
