"""The quiet loop on the device (fx_xlate.hpp QuietPlan) where a wrong plan, a wrong head check or a wrong
launch path would show: states at which a dropped saturation's input is exactly +-1 (found by the search of test_xlate_quiet.py),
checked rows at and just above their bounds in every row, sign and kind of row, a tail wavefront, rows outside their class at
launch, code swaps at run time, every launch path and the instance operations - always against pyoracle.Oracle objects, bit for
bit on outputs, registers, instruction counters, cursors and delay memory.

FXB_INFO_XLATE_QUIET_LEFT is predicted from the oracle, never from the code under test (Watch.block): a wavefront leaves when, at
the head of a sample s in [0, S - 2] of a block of S samples, a lane of it holds |in[s]| above 1 (or not finite) or a checked row
above its bound; the head value of a row that a leading delay-line read fills is what the oracle shows in that register AFTER
sample s (a NaN there - written to the line in an earlier launch - counts as above the bound: test_gpu_zero_signs.py).  A
wavefront that holds a row of the bounded class above 1 or not finite at launch never enters the loop and counts 0; so does
every wavefront of a block of one sample."""
import re

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle
from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT
from test_bus_feed_stub import feed_model
from test_bus_gain_stub import gain_mix_model, gains_for
from test_bus_send_stub import send_model, structure
from test_bus_stub import expand, same_words
from test_bus_tap_stub import tap_list
from test_meter_stub import meter_model, same_meters
from test_xlate_quiet import model, tight_states

pytestmark = pytest.mark.gpu

CONFIG5 = progs.CONFIGS["config5"]()
PROGRAMS = dict(GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT])
STATE5 = (["u", "v", "m"] + ["d%d" % k for k in range(4)] + ["w%d" % k for k in range(4)] + ["lp%d" % k for k in range(4)] +
          ["y%d" % k for k in range(40)])   # config5's rows of the bounded class
ABOVE = float(np.nextafter(np.float32(0.25), np.float32(1.0)))
R_CONTROL, R_CONST = 2, 5


@pytest.fixture
def translated(monkeypatch):
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def channels_of(text):
    return max(1, len(re.findall(r"^input ", text, re.M)))


def noise(n, samples, channels, level, seed=0):
    """[S, channels, N]: uniform noise at +-level, one stream per instance and channel"""
    return np.ascontiguousarray(np.stack([progs.stimulus(n, samples, first_instance=1000 * (seed * 4 + c)) * np.float32(level / 0.9)
                                          for c in range(channels)], axis=1), dtype=np.float32)


def handle(gpu, text, n, devices=None):
    ch = channels_of(text)
    b = gpu.Batch(n, ch, 0) if devices is None else gpu.Batch(n, ch, devices=devices)
    assert b.load_text(text), b.errors()
    return b


class Watch:
    """one oracle per watched lane of a handle, stepped a sample at a time: the reference of every block, and the number of
    wavefronts that leave the quiet loop in it (the rule of this module's first lines)"""

    def __init__(self, gpu, text, lanes, n, bounded=None, shards=None, plan_text=None):
        self.text, self.n, self.ch = text, n, channels_of(text)
        self.o, self.was_reset = {}, set()
        for i in sorted(set(lanes)):
            self.o[i] = Oracle(self.ch)
            assert self.o[i].load_text(text)
        fe = gpu.FrontEnd(self.ch)
        assert fe.load_text(text), fe.errors()
        self.registers = [r[0] for r in fe.registers() if r[1] not in (R_CONTROL, R_CONST)]
        self.trams = fe.tram_sizes()
        self.plan_for(plan_text or text)
        self.bounded = [n_ for n_, _ in self.checked] if bounded is None else list(bounded)
        # wavefronts: 64 consecutive lanes of a shard
        shards = shards or [(0, 0, n)]
        self.wave = {}
        for k, (_, first, count) in enumerate(shards):
            for i in range(first, first + count):
                self.wave[i] = (k, (i - first) // 64)

    def plan_for(self, text):
        """the checked rows by name, from the plan of a FrontEnd that holds `text`"""
        m = model("watch:" + text, text)
        self.plan = m.plan
        self.checked = [(n, b) for r, n, b in m.plan["checked"] if n is not None and b < 1.0 and r not in m.read_rows]
        self.reads = [(n, b) for r, n, b in m.plan["checked"] if n is not None and b < 1.0 and r in m.read_rows]
        self.in_channels = [r - 1 for r in m.input_rows]
        assert all(0 <= c < self.ch for c in self.in_channels)
        assert len(self.checked) + len(self.reads) + len(self.in_channels) == len(m.plan["checked"]), "every checked row is the input or has a name"

    def set(self, lane, reg, value):
        if lane in self.o:
            self.o[lane].set_register(reg, value)

    def reset(self, lane):
        """reset_instances: a fresh object - but for the positions of the delay lines, which stay (tests/test_gpu_instances.py);
        config5 reads and writes its line at offset 0 only, so the lane sounds like the fresh object"""
        self.o[lane] = Oracle(self.ch)
        assert self.o[lane].load_text(self.text)
        self.was_reset.add(lane)

    def block(self, x, predict=True):
        """x [S, channels, N] -> ({lane: reference [S, channels]}, wavefronts predicted to leave - None when not asked for)"""
        S = x.shape[0]
        if not predict:
            return {i: o.process_block(np.ascontiguousarray(x[:, :, i]) if self.ch > 1 else x[:, 0, i].copy()).reshape(S, self.ch)
                    for i, o in self.o.items()}, None
        never, leaves = set(), set()
        for i, o in self.o.items():
            if any(not abs(o.get_register(r)) <= 1.0 for r in self.bounded):
                never.add(self.wave[i])
        ref = {i: np.empty((S, self.ch), dtype=np.float32) for i in self.o}
        for s in range(S):
            for i, o in self.o.items():
                head = s <= S - 2 and self.wave[i] not in leaves and self.wave[i] not in never
                out = head and (any(not abs(float(x[s, c, i])) <= 1.0 for c in self.in_channels) or
                                any(abs(o.get_register(r)) > b for r, b in self.checked))
                ref[i][s] = o.process_block(np.ascontiguousarray(x[s:s + 1, :, i]).reshape(1, self.ch) if self.ch > 1 else x[s:s + 1, 0, i].copy())
                if head and not out:
                    out = any(not abs(o.get_register(r)) <= b for r, b in self.reads)   # (a NaN that comes back out of a delay line leaves too)
                if out:
                    leaves.add(self.wave[i])
        return ref, len(leaves)

    def outputs(self, y, ref, what=""):
        for i, r in ref.items():
            bad = np.argwhere(bits(r) != bits(y[:, :, i]))
            assert bad.size == 0, "%s instance %d: first mismatch at [sample, channel] %s of a block of %d: ref %08x got %08x" % (
                what, i, bad[0].tolist(), y.shape[0], bits(r)[tuple(bad[0])], bits(y[:, :, i])[tuple(bad[0])])

    def state(self, b, what=""):
        for i, o in self.o.items():
            assert b.instruction_counter_i(i) == o.instruction_counter(), (what, i)
            for r in self.registers:
                assert b.get_register_bits_i(r, i) == o.get_register_bits(r), (what, i, r, "%08x" % b.get_register_bits_i(r, i), "%08x" % o.get_register_bits(r))
            if i in self.was_reset:   # the positions are the handle's, the delay memory is the fresh object's, rotated by them
                have, fresh = b.get_cursors_i(i), o.cursors()
                for which, size in enumerate(self.trams):
                    if size > 0:
                        shift = (have[2 * which] - fresh[2 * which]) % size
                        assert (have[2 * which + 1] - fresh[2 * which + 1]) % size == shift, (what, i, which, have, fresh)
                        assert np.array_equal(bits(b.get_tram_i(which, i, size)), np.roll(bits(o.tram(which, size)), shift)), (what, i, which)
                continue
            assert b.get_cursors_i(i) == o.cursors(), (what, i)
            for which, size in enumerate(self.trams):
                if size > 0:
                    assert np.array_equal(bits(b.get_tram_i(which, i, size)), bits(o.tram(which, size))), (what, i, which)
        assert b.ood_flags() == 0

    def run(self, b, x, what="", predict=True):
        """one launch of `b` on x [S, channels, N], compared; returns (y, predicted count)"""
        ref, left = self.block(x, predict)
        y = b.process_block(x)
        self.outputs(y, ref, what)
        return y, left


def quiet5(samples, seed=0, n=192, watched=(), level=0.9):
    """config5's quiet input [S, 1, N]: a lane outside `watched` hears what the first lane of its wavefront hears, so that what
    the oracles of the watched lanes say about leaving holds for every lane"""
    x = noise(n, samples, 1, level, seed)
    for i in range(n):
        if i not in watched:
            x[:, :, i] = x[:, :, i - i % 64]
    return x


WATCH5 = (0, 63, 64, 70, 127, 128, 191)


def config5_pair(gpu, n=192, lanes=WATCH5, devices=None, text=CONFIG5):
    b = handle(gpu, text, n, devices)
    w = Watch(gpu, text, lanes, n, bounded=STATE5, shards=b.shards() if devices else None)
    return b, w


# ------------------------------------------------------------------------------------------------ tight states
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_tight_states(gpu, translated, name):
    """N = 130: wavefront 0 starts every block from the states of the CPU search (the best ones, their negations, random vertices:
    checked rows at +-bound, the first input sample at +-1.0 exactly), wavefront 1 from random states at an eighth of the bounds,
    the tail's two lanes from one of each; blocks of 2, 3 and 40 samples on one handle, one oracle per lane.  A program without a
    loop runs the same blocks: its handle must say so."""
    text = PROGRAMS[name]
    N, ch = 130, channels_of(text)
    m = model(name, text)
    b = handle(gpu, text, N)
    w = Watch(gpu, text, range(N), N)
    states = tight_states(name, text, 3 * 65)
    rng = np.random.default_rng(11)
    tight = list(range(64)) + [128]
    calm = list(range(64, 128)) + [129]
    for k, S in enumerate((2, 3, 40)):
        x = noise(N, S, ch, 0.9, seed=k)
        x[:, :, calm] *= np.float32(0.125)
        for j, i in enumerate(tight):
            regs, inputs = states[k * 65 + j]
            for r, v in regs.items():
                b.set_register_i(r, i, v)
                w.set(i, r, v)
            for c, v in inputs.items():
                x[0, c, i] = v
        if k == 0:
            for i in calm:
                for r, bound in w.checked:
                    v = float(np.float32(rng.uniform(-1.0, 1.0) * bound / 8))
                    b.set_register_i(r, i, v)
                    w.set(i, r, v)
        _, left = w.run(b, x, "%s block %d" % (name, k))
        assert b.info("xlate_quiet_left") == (left if m.plan["in_force"] else 0), (name, k, S)
        assert k > 0 or left == 0, "the tight states of the first block sit inside the bounds: their sample runs in the loop"
        print(name, "block of", S, "wavefronts predicted to leave:", left)
    w.state(b, name)
    assert b.info("kernel") >= 9
    assert b.info("xlate_quiet") == (1 if m.plan["in_force"] else 0), b.tier_note()
    assert b.info("xlate_unsaturated") == (m.plan["quiet_dropped"] if m.plan["in_force"] else m.plan["fast_dropped"])
    b.close()


# ------------------------------------------------------------------------------------------------ the head check, row by row
ROWS5 = ["lp%d" % k for k in range(4)] + ["y%d" % k for k in range(40)]


@pytest.mark.parametrize("value", [ABOVE, 0.25], ids=["above", "at"])
def test_every_checked_row_is_checked_with_both_signs(gpu, translated, value):
    """one wavefront per checked row that a register write reaches (config5's lp* and y*: 44), one lane of it - never the same -
    with that row at the float above 0.25 in magnitude, signs alternating: all 44 leave at sample 0.  With exactly +-0.25 in the
    same places nobody leaves at sample 0; what happens from sample 1 on the oracle says"""
    rows = ROWS5
    N = 64 * len(rows)
    lanes = sorted({64 * k for k in range(len(rows))} | {64 * k + 63 for k in range(len(rows))} | {64 * k + (7 * k + 3) % 64 for k in range(len(rows))})
    b, w = config5_pair(gpu, N, lanes)
    assert {n for n, _ in w.checked} == set(rows) and [n for n, _ in w.reads] == ["d0", "d1", "d2", "d3"]
    for k, r in enumerate(rows):
        i = 64 * k + (7 * k + 3) % 64
        v = value if k % 2 == 0 else -value
        b.set_register_i(r, i, v)
        w.set(i, r, v)
    x = quiet5(8, n=N, watched=lanes, level=0.05)
    _, left = w.run(b, x)
    assert b.info("xlate_quiet") == 1
    assert b.info("xlate_quiet_left") == left
    if value == ABOVE:
        assert left == len(rows) == 44
    _, left = w.run(b, quiet5(2, seed=1, n=N, watched=lanes, level=0.05))
    assert b.info("xlate_quiet_left") == left
    w.state(b)
    b.close()


def test_exactly_the_bound_stays_in_a_block_of_two(gpu, translated):
    """+-0.25 in every one of the 44 rows, one wavefront each: the one head a block of two samples checks passes"""
    rows = ROWS5
    N = 64 * len(rows)
    lanes = sorted({64 * k for k in range(len(rows))} | {64 * k + 63 for k in range(len(rows))} | {64 * k + (5 * k + 1) % 64 for k in range(len(rows))})
    b, w = config5_pair(gpu, N, lanes)
    for k, r in enumerate(rows):
        i = 64 * k + (5 * k + 1) % 64
        v = 0.25 if k % 2 else -0.25
        b.set_register_i(r, i, v)
        w.set(i, r, v)
    _, left = w.run(b, quiet5(2, n=N, watched=lanes, level=0.05))
    assert left == 0 and b.info("xlate_quiet_left") == 0 and b.info("xlate_quiet") == 1
    w.state(b)
    b.close()


def test_rows_filled_by_delay_line_reads_at_their_bounds(gpu, translated):
    """gen3 with both delay lines carrying the input times +-0.5 (quiet_programs.DELAY_EDIT), so that the edges are driven through
    the input and the oracle follows: in = 0.5 at sample 3 is back as -0.25 in the iTRAM's read row after sample 14 and as +0.25
    in the xTRAM's after sample 40 - lane 5, wavefront 0: stays - and the next float above 0.5 (lanes 70 and 129: wavefront 1 and
    the tail) as the next floats beyond: they leave, in the first block of 20 samples for the iTRAM row alone (the xTRAM's value
    is still on its way), in the second for the xTRAM row alone.  Lane 3 does the same with the signs the other way round."""
    name, text = DELAY_EDIT
    N = 130
    m = model(name, text)
    assert m.plan["in_force"]
    b = handle(gpu, text, N)
    w = Watch(gpu, text, range(N), N)
    assert sorted(n for n, _ in w.reads) == ["rd", "xd"] and not {"p", "q"} & {n for n, _ in w.checked}
    above = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    x = noise(N, 60, 1, 0.05)
    x[3, 0, 5], x[3, 0, 3], x[3, 0, 70], x[3, 0, 129] = 0.5, -0.5, above, -above
    for lo, hi in ((0, 20), (20, 60)):
        ref, left = w.block(x[lo:hi])
        y = b.process_block(x[lo:hi])
        w.outputs(y, ref, name)
        assert left == 2 and b.info("xlate_quiet_left") == 2, (lo, left, b.info("xlate_quiet_left"))
    # the edges were the ones meant: replay the four lanes and look at their read rows
    seen = {i: {"rd": set(), "xd": set()} for i in (3, 5, 70, 129)}
    for i in seen:
        o = Oracle(1)
        assert o.load_text(text)
        for s in range(60):
            o.process_block(x[s:s + 1, 0, i].copy())
            for r in ("rd", "xd"):
                seen[i][r].add(o.get_register_bits(r))
    q, qa = int(np.float32(0.25).view(np.uint32)), int(np.float32(ABOVE).view(np.uint32))
    sign = 0x80000000
    assert q | sign in seen[5]["rd"] and q in seen[5]["xd"] and q in seen[3]["rd"] and q | sign in seen[3]["xd"]
    assert qa | sign in seen[70]["rd"] and qa in seen[70]["xd"] and qa in seen[129]["rd"] and qa | sign in seen[129]["xd"]
    w.state(b, name)
    assert b.info("xlate_quiet") == 1
    b.close()


@pytest.mark.parametrize("name", ["gen3", "wide5", "wide1"])
def test_the_input_at_one_stays_and_the_next_float_leaves(gpu, translated, name):
    """the PCM input's own bound, at the last head a block of six samples checks (sample 4: what the loud sample does to the state
    is nobody's business any more), one fresh handle a case: +-1.0 in three wavefronts stays, the next float above 1 in the last
    lane of the tail sends one wavefront away, and in the block's last sample nothing is checked.  Programs that sit still on a
    quiet input: gen3, wide5 (LIMIT records) and wide1 (two channels)"""
    text = PROGRAMS[name]
    N = 130
    above = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    cases = [({(4, 5): 1.0, (4, 70): -1.0, (4, 129): 1.0}, 0), ({(4, 129): -above}, 1), ({(4, 64): above, (5, 0): above}, 1), ({(5, 3): -above}, 0)]
    for k, (loud, count) in enumerate(cases):
        b = handle(gpu, text, N)
        w = Watch(gpu, text, range(N), N)
        x = noise(N, 6, w.ch, 0.02, seed=k)
        for (s, i), v in loud.items():
            x[s, w.in_channels[-1], i] = v      # (wide1 has two channels, both checked: the second)
        _, left = w.run(b, x, name)
        assert left == count and b.info("xlate_quiet_left") == count, (name, k, left, b.info("xlate_quiet_left"))
        w.state(b, name)
        assert b.info("xlate_quiet") == 1
        b.close()


# ------------------------------------------------------------------------------------------------ rows outside their class at launch
NAN, INF = float("nan"), float("inf")
OUTSIDE = [("w0", 5.0, 0), ("y3", 3.0, 0), ("lp1", NAN, 0), ("y7", -INF, 0), ("u", INF, 0), ("y3", -0.0, None), ("y3", 0.5, 1)]


@pytest.mark.parametrize("reg,value,count", OUTSIDE, ids=["%s=%r" % (r, v) for r, v, _ in OUTSIDE])
def test_rows_outside_their_class_at_launch(gpu, translated, reg, value, count):
    """config5, lane 70: a row of the bounded class above 1 or not finite at launch - checked by the loop or not - keeps its
    wavefront out of the loop for that launch (the run-once code sends it to the exact stream: the count stays 0); -0.0 is inside
    every bound; 0.5 in a checked row enters and leaves at sample 0.  The launch after a reset of that lane is quiet again."""
    b, w = config5_pair(gpu)
    b.set_register_i(reg, 70, value)
    w.set(70, reg, value)
    _, left = w.run(b, quiet5(24, watched=WATCH5, level=0.2), reg)
    assert b.info("xlate_quiet") == 1
    assert left == (count if count is not None else left) and b.info("xlate_quiet_left") == left, (reg, value, left, b.info("xlate_quiet_left"))
    w.state(b, reg)
    b.reset_instances([70])
    w.reset(70)
    _, left = w.run(b, quiet5(24, seed=1, watched=WATCH5, level=0.2), reg + " after the reset")
    assert left == 0 and b.info("xlate_quiet_left") == 0
    w.state(b, reg + " after the reset")
    b.close()


# ------------------------------------------------------------------------------------------------ plan changes at run time
def with_control(text, name, value):
    out, n = re.subn(r"^control %s = \S+$" % name, "control %s = %r" % (name, value), text, flags=re.M)
    assert n == 1
    return out


@pytest.mark.parametrize("decay", [0.9, 1.0, 0.0])
def test_a_control_written_before_the_first_block_is_compiled_in(gpu, translated, decay):
    """decay is compiled in: the handle's loop is the plan of a FrontEnd that loaded the text with that value written in"""
    twin = with_control(CONFIG5, "decay", decay)
    m = model("config5 decay %r" % decay, twin)
    assert m.plan["in_force"] and m.plan["quiet_dropped"] == {0.9: 379, 1.0: 379, 0.0: 403}[decay]
    b = handle(gpu, CONFIG5, 192)
    b.set_register("decay", decay)
    w = Watch(gpu, CONFIG5, WATCH5, 192, bounded=STATE5, plan_text=twin)
    for o in w.o.values():
        o.set_register("decay", decay)
    x = quiet5(40, watched=WATCH5)
    x[5, 0, 70] = 1.5
    for k, (lo, hi) in enumerate(((0, 2), (2, 5), (5, 40))):
        _, left = w.run(b, x[lo:hi])
        assert b.info("xlate_quiet_left") == left and left == (1 if k == 2 else 0)
    assert b.info("xlate_quiet") == 1 and b.info("xlate_unsaturated") == m.plan["quiet_dropped"] and b.info("control_rows") == 0
    w.state(b)
    b.close()


FULL_IDLE, LEAN_IDLE = 249, 395   # config5's idle saturations with damp, decay and diff in rows / with decay alone in a row


def test_plan_changes_at_run_time(gpu, translated):
    """decay moves on a handle that has run: 0.45, 0.9, 1.0, 0.0 and back to 0.45; after every write blocks of 2, 3 and 40
    samples, then a rest, prepare() and the same blocks again; parity throughout.  A write to a control that has run translates
    nothing (fx_batch.cpp Batch::setRegister): the three declared controls get rows - the "full" code, in the cache since the
    first block - and a block or more later, when the builder thread has delivered it, the "lean" code in which decay alone has
    a row.  Both have a loop, which checks the control rows like any row of the bounded class: diff = 0.6 in the full code, a
    decay above 0.25 in the lean one send every wavefront to the fast loop at sample 0.  Which of the two a launch ran
    `control_rows` says; their counts of idle saturations are fixed.  Once decay has rested for its cooling time (8192 sample
    periods, twice as many after every further cooling: Batch::controlWritten) and prepare() has waited for the builder thread,
    every control is folded in: the handle runs the code of the text with that value written in, and its loop is that
    FrontEnd's plan - newly built for 0.9, 1.0 and 0.0, out of the cache without a build for both 0.45.
    Then a per-instance write (decay gets its row back) and an armed track on damp: no loop, FrontEnd.quiet_plan says why - and
    none after the track's end either, since a register that has had a track keeps the code that can re-load it."""
    lanes = (0, 70, 191)
    b, w = config5_pair(gpu, 192, lanes)
    rng = np.random.default_rng(23)
    clock = [0]
    counters = lambda: (b.info("code_cache_hits"), b.info("xlate_builds"), b.info("xlate_background_builds"))   # noqa: E731

    def blocks(what, decay, folded=None):
        """blocks of 2, 3 and 40 samples; folded: the plan the code in force must be (no control rows), None: controls in rows"""
        for S in (2, 3, 40):
            x = quiet5(S, seed=clock[0] % 7, watched=lanes, level=0.2)
            clock[0] += 1
            if folded is not None and S == 40:
                x[5, 0, 70] = 1.5      # one wavefront leaves the loop of the folded code mid-block
            _, left = w.run(b, x, what)
            assert folded is None or left == (1 if S == 40 else 0), (what, S, left)
            got, rows, idle = b.info("xlate_quiet_left"), b.info("control_rows"), b.info("xlate_unsaturated")
            print(what, "block of", S, "left", got, "predicted", left, "control rows", rows, "idle", idle)
            assert b.info("kernel") >= 9 and b.info("xlate_quiet") == 1, (what, b.tier_note())
            if folded is not None:
                assert rows == 0 and idle == folded["quiet_dropped"] and got == left, (what, S, rows, idle, got, left)
            elif rows == 3:
                assert idle == FULL_IDLE and got == 3, (what, S, idle, got)
            else:
                assert rows == 1 and idle == LEAN_IDLE and got == (3 if abs(decay) > 0.25 else left), (what, S, rows, idle, got, left)

    def rest(samples):
        """every lane hears the same quiet stream"""
        while samples > 0:
            x = np.ascontiguousarray(np.broadcast_to(rng.uniform(-0.2, 0.2, (4096, 1, 1)).astype(np.float32), (4096, 1, 192)))
            w.run(b, x, "at rest", predict=False)
            samples -= 4096

    plan = model("config5", CONFIG5).plan
    blocks("fresh", 0.45, folded=plan)
    assert plan["quiet_dropped"] == 395
    cool = 8192
    for step, v in enumerate((0.45, 0.9, 1.0, 0.0, 0.45)):
        twin = with_control(CONFIG5, "decay", v)
        want = model("config5 decay %r" % v, twin).plan
        assert want["in_force"] and want["quiet_dropped"] == {0.45: 395, 0.9: 379, 1.0: 379, 0.0: 403}[v]
        b.set_register("decay", v)
        for o in w.o.values():
            o.set_register("decay", v)
        blocks("decay %r" % v, v)
        hits, builds, background = counters()
        rest(cool + 1024)      # (the cooling is looked at every 1024 sample periods)
        b.prepare(40)
        w.plan_for(twin)
        blocks("decay %r folded in" % v, v, folded=want)
        after = counters()
        assert after[0] > hits and after[1] == builds, (v, (hits, builds, background), after)
        if v == 0.45:
            # the code of the loaded text: in the cache since the first block
            assert step == 0 or after[2] == background, (v, (hits, builds, background), after)
        else:
            assert after[2] > background, "a newly built loop was swapped in on the running handle"
        cool *= 2
    w.state(b, "decay back at 0.45")
    # a per-instance write: decay has a row again, whatever its values
    b.set_register_i("decay", 70, 0.9)
    w.set(70, "decay", 0.9)
    blocks("decay of instance 70", 0.45)
    # an armed track: no loop
    track = np.array([0.3, 0.5, 0.2, 0.3], dtype=np.float32)
    assert b.set_register_track("damp", track, 8) == 0
    x = quiet5(32, seed=3, watched=lanes, level=0.2)
    ref = {i: np.empty((32, 1), dtype=np.float32) for i in w.o}
    for k, v in enumerate(track):
        for i, o in w.o.items():
            o.set_register("damp", float(v))
            ref[i][8 * k:8 * k + 8, 0] = o.process_block(x[8 * k:8 * k + 8, 0, i].copy())
    w.outputs(b.process_block(x), ref, "track")
    assert b.info("xlate_quiet") == 0 and b.info("xlate_quiet_left") == 0 and "quiet loop" not in b.tier_note()
    fe = gpu.FrontEnd(1)
    assert fe.load_text(CONFIG5) and fe.track_register("damp") == 0
    assert "track" in fe.quiet_plan(128)["why"]
    # the track has ended.  damp stays a register that can have a track - arming one again never translates (DESIGN.md section
    # 4.5; include/fx8010_amd.h fxp_track_register) - so the code in force stays the code without a loop
    for S in (8, 40):
        w.run(b, quiet5(S, seed=S % 7, watched=lanes, level=0.2), "after the track", predict=False)
        assert b.info("xlate_quiet") == 0 and b.info("xlate_quiet_left") == 0 and "quiet loop" not in b.tier_note()
    w.state(b, "the end")
    b.close()


# ------------------------------------------------------------------------------------------------ every launch path
PATHS = ["pitched", "in_place", "imajor", "bus", "bus_feed", "meters", "two_shards"]


@pytest.mark.parametrize("path", PATHS)
def test_every_launch_path_with_a_wavefront_leaving(gpu, translated, path):
    """config5, N = 192, 40 samples, one loud input sample (1.5 at sample 5) in lane 70: the path's result against a plain handle
    given the equivalent input, bit for bit; the oracle on the watched lanes; the loop in force; the count as predicted (a handle
    of two shards - 128 and 64 lanes - has a second loud sample, in lane 150, and reports the sum over its shards)."""
    import torch

    N, S, K = 192, 40, 4
    rng = np.random.default_rng(17)
    devices = [0, 0] if path == "two_shards" else None
    lanes = sorted(set(WATCH5) | {68, 69, 71, 150})
    b, w = config5_pair(gpu, N, lanes, devices=devices)
    plain, wp = config5_pair(gpu, N, lanes)
    x = quiet5(S, watched=lanes, level=0.2)
    if path == "bus":
        G = b.bus_groups(K)
        xg = np.ascontiguousarray(x[:, :, ::K])
        xg[5, 0, 70 // K] = 1.5
        x = expand(xg, K, N)
    elif path == "bus_feed":
        # source columns 0 .. 3 carry the wavefronts' streams and column 4 the loud sample: instance n hears column n // 64,
        # instance 70 the sum of columns 1 and 4, instance 3 nothing
        src = np.zeros((S, 1, 5), dtype=np.float32)
        src[:, :, :3] = x[:, :, ::64]
        src[5, 0, 4] = 1.5
        count = np.ones(N, dtype=np.int64)
        count[70], count[3] = 2, 0
        off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        sources = np.concatenate([([i // 64, 4] if i == 70 else ([] if i == 3 else [i // 64])) for i in range(N)]).astype(np.int64)
        assert b.bus_set_feeds(5, off, sources) == 0
        x = feed_model(src, off, sources, None, None, False, S)
        assert x[5, 0, 70] > 1.0 and not x[:, 0, 3].any()
    else:
        x[5, 0, 70] = 1.5
        if path == "two_shards":   # (one in either shard)
            x[7, 0, 150] = -1.5
    loud = 2 if path == "two_shards" else 1
    ref, left = wp.block(x)
    yp = plain.process_block(x)
    wp.outputs(yp, ref, "plain")
    assert plain.info("xlate_quiet_left") == left == loud
    _, want = w.block(x)   # (the same oracles' twins, in this handle's wavefronts)
    if path in ("pitched", "in_place"):
        P = N + 59
        d_in = torch.zeros((S, 1, P), dtype=torch.float32, device="cuda")
        d_in[:, :, :N] = torch.from_numpy(x).to("cuda")
        d_out = d_in if path == "in_place" else torch.full((S, 1, P), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert b.process_block_dev_pitched(d_in[:, :, :N], d_out[:, :, :N], S) == 0
        assert b.sync() == 0
        got = d_out.cpu().numpy()
        y = np.ascontiguousarray(got[:, :, :N])
        assert (got[:, :, N:] == (0.0 if path == "in_place" else -7.0)).all()
    elif path == "imajor":
        y = np.ascontiguousarray(b.process_block_imajor(np.ascontiguousarray(x.transpose(2, 0, 1))).transpose(1, 2, 0))
        assert b.info("imajor_blocks") == 1
    elif path == "bus":
        g = gains_for(rng, 1, N)
        taps = tap_list(rng, N, 9)
        off, members = structure(rng, N, (0, 1, 5, 70))
        sg = gains_for(rng, 1, int(off[-1]))
        assert b.bus_set_gains(g) == 0 and b.bus_set_taps(taps) == 0 and b.bus_set_sends(off, members, sg) == 0
        mix, tapped, aux = b.process_block_bus(xg, K, True, True, taps=True, aux=True)
        assert same_words(mix, gain_mix_model(yp, g, g, False, S, K)), "the mix"
        assert np.array_equal(bits(tapped), bits(yp[:, :, taps])), "the taps"
        assert same_words(aux, send_model(yp, off, members, sg, sg, False, S)), "the sends"
        assert b.info("bus_blocks") == 1 and mix.shape == (S, 1, G)
        y = None
    elif path == "bus_feed":
        y = b.process_block_bus_feed(src)
        assert b.info("bus_feed_blocks") == 1
    elif path == "meters":
        assert b.meter_enable() == 0
        y = b.process_block(x)
        assert same_meters(b.meter_read(), meter_model(yp)) and b.meter_samples() == S
    else:
        assert [s[2] for s in b.shards()] == [128, 64]
        y = b.process_block(x)
    if y is not None:
        assert np.array_equal(bits(y), bits(yp)), path
        w.outputs(y, ref, path)
    assert b.info("xlate_quiet") == 1 and b.info("kernel") >= 9
    assert b.info("xlate_quiet_left") == want == loud, (path, b.info("xlate_quiet_left"), want)
    for r in STATE5 + ["out"]:
        assert np.array_equal(bits(b.get_register_array(r)), bits(plain.get_register_array(r))), r
    w.state(b, path)
    for h in (b, plain):
        h.close()


# ------------------------------------------------------------------------------------------------ instance operations between launches
def test_instance_operations_between_launches(gpu, translated):
    """lane 70 starts with lp1 = 1.0, which falls by 0.7 a sample: after a block of two it is still above the bound.  copy_instances
    of that lane into wavefront 2 and its record - saved while its wavefront was outside the loop - loaded into wavefront 0 make
    all three leave in the next launch; reset_instances of two of them, and the third's decay, bring everybody back"""
    lanes = sorted(set(WATCH5) | {10, 150})
    b, w = config5_pair(gpu, 192, lanes)
    b.set_register_i("lp1", 70, 1.0)
    w.set(70, "lp1", 1.0)
    x = quiet5(2, watched=lanes, level=0.05)
    _, left = w.run(b, x, "a loud lane")
    assert left == 1 and b.info("xlate_quiet_left") == 1
    assert max(abs(w.o[70].get_register(r)) for r in ROWS5) > 0.25, "lane 70's state is still outside the loop's bounds"
    image = b.save_instances([70])                 # taken while wavefront 1 is outside the loop
    assert image.size == 64 + 4 * b.info("instance_words")
    b.copy_instances([70], [150])                  # into wavefront 2
    assert b.load_instances([10], image) == 0      # and, as a record, into wavefront 0
    for i in (10, 150):                            # their oracles become twins of lane 70's: replay
        twin = Oracle(1)
        assert twin.load_text(CONFIG5)
        twin.set_register("lp1", 1.0)
        twin.process_block(x[:, 0, 70].copy())
        w.o[i] = twin
    _, left = w.run(b, quiet5(2, seed=1, watched=lanes, level=0.05), "after the copy and the load")
    assert left == 3 and b.info("xlate_quiet_left") == 3, (left, b.info("xlate_quiet_left"))
    w.state(b, "after the copy and the load")
    b.reset_instances([70, 150])
    w.reset(70)
    w.reset(150)
    _, left = w.run(b, quiet5(24, seed=2, watched=lanes, level=0.05), "after the reset")
    assert left == 0 and b.info("xlate_quiet_left") == 0
    w.state(b, "the end")
    assert b.info("xlate_quiet") == 1
    b.close()
