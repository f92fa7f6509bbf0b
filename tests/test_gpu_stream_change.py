"""Leaving the fast stream at every record, in every sample phase, on the device: the spliced programs of
stream_change_programs.py - one trigger record in front of a chosen instruction - run as batches of six wavefronts, five of which
meet the trigger in a sample of their own (first sample of a launch, a steady one, the last of a block, the first of the next
launch, a steady one in a ragged wavefront) and leave the fast stream for the exact stream behind that record; the sixth never
does.  Up to four registers of the program start at small non-zero values, a different one in every lane, so that the first
sample of the first launch has a state to get wrong.  Bit for bit against one oracle per compared instance, NaN words included.

The quiet loop: the plan refuses a program with a MACW / MACINTW, a LOG or a delay-line read in its middle, so of the spliced gen2
and wide1 programs only those of the `loud` trigger (a channel-1 word of 1.5, checked at the head of the sample) run a quiet loop -
all 95 of them, asserted - and two of wide1 with a leading delay-line read.  The other kinds sweep the fast stream of those bases.
The stages: the default tier must run config2 as a pipeline (more than one wavefront per workgroup) at every position of every
kind but the delay trigger's (a program that ends in a delay-line write is not cut), and the FX_STAGES=1 tier must not.  test_stream_change.py shows, without a GPU, that these programs translate and that the triggers fire
where they are meant to."""
import numpy as np
import pytest

import stream_change_programs as SC
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

TIERS = {"default": {}, "unstaged": {"FX_STAGES": "1"}, "xlate_v256": {"FX_KERNEL": "xlate_v256"}}
CASES = {(c[0], c[1]): c for c in SC.sweep_cases()}
# config4 and config5 are never cut into stages: they run on the unstaged variant only
PARAMS = [(name, sweep, tier) for (name, sweep), c in CASES.items() for tier in TIERS if c[6] or tier == "unstaged"]
WAVE_LANES = {w: SC.compared_lanes(w) for w in range(SC.WAVES)}
LANES = [lane for w in range(SC.WAVES) for lane in WAVE_LANES[w]]
_STIMULUS, _REFERENCE = {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stimulus(kind):
    if kind not in _STIMULUS:
        _STIMULUS[kind] = SC.stimulus(kind)
    return _STIMULUS[kind]


def reference(name, sweep, j):
    """(text, watched registers, preset registers, {lane: LaneRun}) of one spliced program: computed once, shared by the tiers"""
    key = (name, sweep, j)
    if key not in _REFERENCE:
        _, _, base, kind, gap, _, _ = CASES[(name, sweep)]
        text = SC.with_trigger(base, j, kind, gap)
        regs, presets = SC.watched_registers(base, kind), SC.preset_registers(base, kind)
        x = stimulus(kind)
        _REFERENCE[key] = (text, regs, presets, {lane: SC.LaneRun(Oracle, text, kind, x[:, :, lane], regs, lane, presets) for lane in LANES})
    return _REFERENCE[key]


def ood_and_counters(b, n_registers):
    """per compared instance (out-of-domain flags, instruction counter) out of the instances' records: the state rows lead a
    record - one per register of the program, then per channel an output latch, four delay-line positions, two noise words, the
    flags and the 64-bit counter (fx_batch.cpp, first lines)"""
    words = b.instance_words
    image = b.save_instances(LANES)[64:].view(np.uint32).reshape(len(LANES), words)
    at = n_registers + 2 + 4 + 2
    return {lane: (int(image[k, at]), int(image[k, at + 1]) | (int(image[k, at + 2]) << 32)) for k, lane in enumerate(LANES)}


def run_position(gpu, name, sweep, j, tier):
    _, _, base, kind, gap, _, _ = CASES[(name, sweep)]
    text, regs, presets, ref = reference(name, sweep, j)
    x = stimulus(kind)
    where = "%s %s position %d tier %s" % (name, sweep, j, tier)
    b = gpu.Batch(SC.N, 2, 0)
    assert b.load_text(text), (where, b.errors())
    fe = gpu.FrontEnd(2)
    assert fe.load_text(text)
    n_registers = len(fe.registers())
    for k, r in enumerate(presets):
        assert b.set_register_array(r, np.array([SC.preset_value(k, lane, kind) for lane in range(SC.N)], dtype=np.float32)) == 0, (where, r)
    at = 0
    for blk, length in enumerate(SC.blocks_of(kind)):
        y = b.process_block(x[at:at + length])
        if blk == 0:
            assert b.tier_note().startswith("translated to gfx950 code"), (where, b.tier_note())
            if tier == "unstaged":
                assert b.info("waves_per_wg") == 1, (where, "FX_STAGES=1 must not cut the program")
            elif tier == "default" and name == "config2" and kind != "delay":   # (a program that ends in a delay-line write is not cut)
                assert b.info("waves_per_wg") >= 2, (where, "the default tier runs config2 as a pipeline of stages")
            assert kind != "loud" or b.info("xlate_quiet") == 1, (where, "the loud trigger keeps the quiet loop", b.tier_note())
        rows = {r: bits(b.get_register_array(r)) for r in regs}
        state = ood_and_counters(b, n_registers)
        assert state[LANES[-1]][1] == b.instruction_counter_i(LANES[-1]), (where, "the counter is not where the record's layout says")
        met = 0
        for w in range(SC.WAVES):
            s = SC.trigger_sample(kind, w)
            phase = "wavefront %d (trigger sample %s) block %d" % (w, s, blk)
            # (the quiet loop checks the heads of the samples 0 .. S - 2 of a block of S: test_gpu_quiet_states.py)
            if s is not None and at <= s <= at + length - 2 and any(ref[lane].fired(kind, s) for lane in SC.trigger_lanes(w)):
                met += 1
            for lane in WAVE_LANES[w]:
                r = ref[lane]
                want, got = bits(r.out[blk]), bits(y[:, :, lane])
                bad = np.argwhere(want != got)
                assert bad.size == 0, "%s %s instance %d: output [sample, channel] %s: ref %08x got %08x" % (
                    where, phase, lane, bad[0].tolist(), want[tuple(bad[0])], got[tuple(bad[0])])
                for reg in regs:
                    assert int(rows[reg][lane]) == r.regs[blk][reg], "%s %s instance %d: register %s: ref %08x got %08x" % (
                        where, phase, lane, reg, r.regs[blk][reg], int(rows[reg][lane]))
                assert state[lane][1] == r.count[blk], "%s %s instance %d: instruction counter: ref %d got %d" % (
                    where, phase, lane, r.count[blk], state[lane][1])
                assert state[lane][0] == r.ood_block[blk], "%s %s instance %d: out-of-domain flags: ref %d got %d" % (
                    where, phase, lane, r.ood_block[blk], state[lane][0])
        if b.info("xlate_quiet"):
            assert b.info("xlate_quiet_left") >= met, (where, blk, b.info("xlate_quiet_left"), met)
        at += length
    b.close()


@pytest.mark.parametrize("name,sweep,tier", PARAMS, ids=["%s-%s-%s" % p for p in PARAMS])
def test_leaving_the_fast_stream_at_every_record(gpu, monkeypatch, name, sweep, tier):
    """every swept position of one program with one kind of trigger on one tier: one batch per position (six wavefronts, the last
    ragged; two blocks), compared on lane 0, the last valid lane, the four trigger lanes and four others of every wavefront:
    both blocks' output words, the trigger's registers, ccr, up to four registers of the program, the instruction counter and the
    out-of-domain flags of the instance, after each block.  The batch must say that it runs translated code; where it runs a quiet
    loop (it must for the loud trigger), at least as many wavefronts leave it in a block as the oracle says met their trigger at
    a head that the loop checks."""
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(k, raising=False)
    for k, v in TIERS[tier].items():
        monkeypatch.setenv(k, v)
    for j in CASES[(name, sweep)][5]:
        run_position(gpu, name, sweep, j, tier)
