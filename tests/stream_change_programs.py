"""Programs and stimulus of the stream-change sweep: a base program with ONE trigger record spliced in
front of a chosen instruction, so that a wavefront leaves the translated tier's fast stream (or its quiet loop) for the exact
stream at that record, in a chosen sample.  Shared by test_stream_change.py (translation, firing against the oracle and the live-in
walk of the exact streams, without a GPU) and test_gpu_stream_change.py (the sweep on the device).  The corpus is fixed by names
and seeds: counts asserted elsewhere depend on it.

The triggers read `tin`, the input of channel 1 (added unless the base has one), which is quiet but for the trigger words:
  wrap     macw trg, tin, tin, big      big = 1.2e38: +Inf exactly when tin = 3.0, finite for |tin| <= 1.  The input is the A
                                         operand: X and Y inputs are read through A's channel.
  wrapint  macintw trg, tin, tin, big   the same overflow through the other inline shape and the handler's other operand order
  delay    xdelay read, trd, at, 0 in front of instruction j, macs tuse, 0, trd, 0.5 `gap` instructions later, xdelay write, tin,
           at, 0 in front of `end`, xtramsize 3 (idelay / itramsize where the xTRAM is taken): tin = 2.0 comes back three samples
           later - a value outside the class of its row - and the wavefront leaves at the wait in front of the first use
  lut      log trg, tin, 3, 0           tin = 2.5: no leave - the wavefront takes the guarded LOG behind the loop and comes back
                                         into the fast stream in the middle of the sample; out-of-domain flag 16 on that instance
  loud     interp trg, tin, 0.5, tin    tin = 1.5, for the two bases that have a quiet loop (gen2, wide1) only: the one trigger the
                                         quiet plan admits.  The plan refuses every other kind (MACW / MACINTW: "a handler call", LOG,
                                         a delay-line read in the middle of the program): of their 480 spliced programs 2 keep a
                                         quiet loop (wide1, the delay read at position 0), so those kinds sweep the fast stream of
                                         gen2 and wide1, not their quiet loop.  A wavefront can leave the quiet loop at the head of
                                         a sample only: the word above the input's bound of 1 sends it to the steady fast loop there,
                                         wherever the record that reads it stands; trg saturates at 1.0 in that sample.
"""
import os
import re
import sys

import numpy as np

import fx8010_programs as progs
import quiet_programs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stress_fuzz  # noqa: E402

OPS = ("macs", "macsn", "macints", "macintw", "acc3", "macmv", "macw", "macwn", "skip", "andxor", "tstneg", "limit", "limitn", "log",
       "exp", "interp", "idelay", "xdelay", "end")
KINDS = ("wrap", "wrapint", "delay", "lut", "loud")
TRIGGER_WORD = {"wrap": 3.0, "wrapint": 3.0, "delay": 2.0, "lut": 2.5, "loud": 1.5}
QUIET_BASES = ("gen2", "wide1")
BIG = "120000000000000000000000000000000000000.0"    # 1.2e38 as a decimal literal
DELAY = 3                                            # slots of the trigger's delay line: samples until the hand-back


def _op(line):
    return line.split(";")[0].strip().split(" ")[0].lower()


def _instruction_lines(lines):
    return [k for k, l in enumerate(lines) if _op(l) in OPS]


def positions(text):
    """the instruction lines of a program, `end` included: position j is `in front of instruction j`"""
    lines = text.split("\n")
    return [lines[k] for k in _instruction_lines(lines)]


def free_line(text):
    """'x' / 'i': the delay line a program leaves free for the delay trigger (the xTRAM first), None: both are taken"""
    if not re.search(r"^xtramsize ", text, re.M) and not re.search(r"^xdelay ", text, re.M):
        return "x"
    if not re.search(r"^itramsize ", text, re.M) and not re.search(r"^idelay ", text, re.M):
        return "i"
    return None


def trigger_input(text):
    """(name of the input of channel 1, whether the base declares it already)"""
    m = re.search(r"^input (\S+) 1\s*$", text, re.M)
    return (m.group(1), True) if m else ("tin", False)


def with_trigger(text, j, kind, gap=1):
    """`text` with a trigger of `kind` spliced in front of instruction j (see the module's first lines); two channels"""
    assert kind in KINDS
    lines = text.split("\n")
    at = _instruction_lines(lines)
    assert 0 <= j < len(at) and _op(lines[at[-1]]) == "end"
    names = set(re.findall(r"^(?:static|control|input|output|const)\s+(\S+)", text, re.M))
    tin, declared = trigger_input(text)
    head, body = [] if declared else ["input tin 1"], {}
    if kind in ("wrap", "wrapint"):
        new = ["trg", "big"]
        head += ["static big = " + BIG, "static trg"]
        body[j] = ["%s trg, %s, %s, big" % ("macw" if kind == "wrap" else "macintw", tin, tin)]
    elif kind == "lut":
        new = ["trg"]
        head += ["static trg"]
        body[j] = ["log trg, %s, 3, 0" % tin]
    elif kind == "loud":
        new = ["trg"]
        head += ["static trg"]
        body[j] = ["interp trg, %s, 0.5, %s" % (tin, tin)]
    else:
        t = free_line(text)
        assert t is not None, "the delay trigger needs a free delay line"
        new = ["trd", "tuse"]
        head += ["%stramsize %d " % (t, DELAY), "static trd", "static tuse"]
        body[j] = ["%sdelay read, trd, at, 0" % t]
        use = min(j + gap - 1, len(at) - 1)
        body.setdefault(use, []).append("macs tuse, 0, trd, 0.5")
        body.setdefault(len(at) - 1, []).append("%sdelay write, %s, at, 0" % (t, tin))
    assert not (set(new) | (set() if declared else {"tin"})) & names, "the trigger's names are taken"
    out = lines[:at[0]] + head
    for k in range(at[0], len(lines)):
        if k in at:
            out += body.get(at.index(k), [])
        out.append(lines[k])
    return "\n".join(out)


# ---------------------------------------------------------------------------------------------------- the corpus
RECORD_WORDS = ("itramsize 3 \ninput in 0\noutput out 0\ncontrol k = 0.125\nstatic a\nstatic b\nstatic c\nstatic t\nstatic rd\n"
                "interp a, in, k, a\nmacs a, in, 0, 0\nidelay read, rd, at, 0\ninterp b, rd, k, b\nandxor t, 2, 2, 0\nidelay write, t, at, 0\n"
                "interp c, a, 0.5, c\nmacs out, b, c, 0.25\nend")     # test_gpu_parity.py: ..._finds_the_record_words_set
HEAD_OF_SAMPLE = ("input in 0\noutput out 0\ncontrol c = 0.3\nstatic rd\nstatic xd\nitramsize 7 \nxtramsize 30 \nstatic r4\nstatic r5\nstatic r7\n"
                  "static r8\nstatic r9\nstatic r10\nstatic r13\n"
                  "xdelay read, xd, at, 0\nxdelay read, xd, at, 0\nxdelay write, in, at, 0\nskip ccr, ccr, 3, 4\nlimit r9, xd, 0, r8\n"
                  "macs r5, r13, r7, c\nmacints r9, ccr, 0.125, r5\nandxor r10, in, r4, c\nmacs out, xd, r9, 0.5\nidelay read, rd, at, 0\nend")
                                                                       # test_gpu_parity.py: ..._at_the_head_of_a_sample
# RECORD_WORDS without the delay line: the second INTERP blends the input, which is not zero in the first sample of a launch as
# the delay line's word is.  The fast stream drops the first INTERP (dead: `a` is written again), so a wavefront that a trigger
# sends away in front of the second one has never loaded the fp64 (1 - X) into s[22:23] - in the first sample of a launch.
RECORD_WORDS_INPUT = ("input in 0\noutput out 0\ncontrol k = 0.125\nstatic a\nstatic b\nstatic c\nstatic t\n"
                      "interp a, in, k, a\nmacs a, in, 0, 0\nmacs t, in, 0.5, 0.25\ninterp b, in, k, b\ninterp c, a, k, t\nmacs out, b, c, 0.25\nend")
PRODUCT_CACHE_SEEDS = (1, 2, 3)
# seeds of _random() whose programs load, are single-pass and translate; short and long ones, with one to eighteen SKIPs.  random2
# seed 5 is not among them: five of its positions lie behind `skip ccr, ccr, 8, n`, which every lane takes in every sample (16
# candidate lanes per wavefront fire no more often than 4) - records that never run tell nothing about a leave.
RANDOM_SEEDS = (4, 5, 0, 6, 28, 13)
RANDOM2_SEEDS = (4, 12, 0, 6, 28, 29)


def _product_cache(seed):
    return stress_fuzz.product_cache_program(np.random.default_rng(880000 + seed), 40)


def _random(gen, seed):
    rng = np.random.default_rng(770000 + seed)
    return gen(rng, int(rng.integers(8, 100)), int(rng.integers(3, 40)))


def corpus():
    """[(name, text, staged)]: staged says whether the default tier may cut the program into stages (config4 and config5 are
    swept on the unstaged variant only)"""
    out = [(n, progs.CONFIGS[n](), n not in ("config4", "config5")) for n in ("config1_logtube", "config2", "config3", "config4", "config5")]
    out.append(("mixed_stages", progs.PROBE_PROGRAMS["mixed_stages"](), True))
    out.append(("record_words", RECORD_WORDS, True))
    out.append(("record_words_input", RECORD_WORDS_INPUT, True))
    out.append(("head_of_sample", HEAD_OF_SAMPLE, True))
    out += [("product_cache%d" % s, _product_cache(s), True) for s in PRODUCT_CACHE_SEEDS]
    out += [("random%d" % s, _random(stress_fuzz.random_program, s), True) for s in RANDOM_SEEDS]
    out += [("random2_%d" % s, _random(stress_fuzz.random_program2, s), True) for s in RANDOM2_SEEDS]
    quiet = dict(quiet_programs.GENERATED + quiet_programs.GENERATED_WIDE)
    out += [(n, quiet[n], True) for n in ("gen2", "wide1")]
    return out


# ---------------------------------------------------------------------------------------------------- positions
def shadows(text):
    """positions j at which a spliced record lies inside the shadow of a SKIP with a literal count n > 0 at instruction i: i < j <= i + n"""
    inside = set()
    for i, l in enumerate(positions(text)):
        if _op(l) == "skip":
            m = re.match(r"^-?\d+$", l.split(",")[-1].strip())
            if m and int(m.group(0)) > 0:
                inside.update(range(i + 1, i + int(m.group(0)) + 1))
    return inside


def _thin(values, cap):
    values = sorted(set(values))
    if len(values) <= cap:
        return values
    return sorted({values[int(round(k * (len(values) - 1) / (cap - 1)))] for k in range(cap)})


def swept_positions(text):
    """every position of a program of at most 64 instructions; of a longer one 24 evenly spread positions and the position
    directly behind every SKIP, delay-line record, LOG / EXP and INTERP with a constant X, thinned evenly to at most 48"""
    instr = positions(text)
    n = len(instr)
    if n <= 64:
        return list(range(n))
    uniform = set(re.findall(r"^control\s+(\S+)", text, re.M))
    picks = set(_thin(range(n), 24))
    for i, l in enumerate(instr[:-1]):
        op = _op(l)
        x = l.split(",")[2].strip() if op == "interp" else ""
        if op in ("skip", "idelay", "xdelay", "log", "exp") or (op == "interp" and (x in uniform or re.match(r"^-?[\d.]+$", x))):
            picks.add(i + 1)
    return _thin(picks, 48)


# kinds of the sweep: (name, trigger kind, gap); `delay_shadow` puts the delay-line read inside SKIP shadows on purpose
SWEEP_KINDS = (("wrap", "wrap", 1), ("wrapint", "wrapint", 1), ("lut", "lut", 1), ("delay1", "delay", 1), ("delay3", "delay", 3),
               ("delay_shadow", "delay", 1), ("loud", "loud", 1))
DELAY_SHADOW_PROGRAMS = ("mixed_stages", "product_cache1")


def sweep_cases():
    """[(program name, sweep kind, text of the base, trigger kind, gap, positions, staged)]"""
    out = []
    for name, text, staged in corpus():
        swept, inside = swept_positions(text), shadows(text)
        for sweep, kind, gap in SWEEP_KINDS:
            if kind == "loud":
                if name not in QUIET_BASES:
                    continue
                instr = positions(text)     # (a record in front of a leading delay-line read would move that read into the program)
                at = [j for j in swept if not all(_op(l) in ("idelay", "xdelay") and " read" in l for l in instr[:j + 1])]
            elif kind != "delay":
                at = swept
            elif free_line(text) is None:
                continue
            elif sweep == "delay_shadow":
                if name not in DELAY_SHADOW_PROGRAMS:
                    continue
                at = sorted(inside)          # a delay-line record inside a shadow: the whole lowering goes to per-lane handlers
            else:
                at = [j for j in swept if j not in inside]
            out.append((name, sweep, text, kind, gap, at, staged))
    return out


# ---------------------------------------------------------------------------------------------------- stimulus and reference
WAVES, N = 6, 5 * 64 + 27          # the last wavefront is ragged
CONTROL_WAVE = 4                   # never triggered: stays in the fast stream
BLOCKS = {"delay": (6, 5)}         # every other kind: (5, 4)
# the sample in which each wavefront meets its trigger (blocks of 5 and 4): wavefront 0 in the first sample of a launch (delay lines
# are read in place), 1 in a steady sample, 2 in the last sample of block 1 (the last-sample streams), 3 in the first sample of the
# next launch, the ragged wavefront 5 in a steady sample of block 2.  The delay trigger (blocks of 6 and 5) hands its word back
# three samples after it went in: it cannot come back in the first sample of the first launch, so wavefront 0 meets it in the
# earliest sample there is (3), 1 in the next, 2 in the last sample of block 1, 3 in the first of block 2, 5 in a steady one.
TRIGGER_SAMPLE = {0: 0, 1: 2, 2: 4, 3: 5, 5: 7}
HAND_BACK_SAMPLE = {0: 3, 1: 4, 2: 5, 3: 6, 5: 8}


def blocks_of(kind):
    return BLOCKS.get(kind, (5, 4))


def trigger_sample(kind, wave):
    return (HAND_BACK_SAMPLE if kind == "delay" else TRIGGER_SAMPLE).get(wave)


def lanes_of(wave):
    first, last = 64 * wave, min(N, 64 * wave + 64) - 1
    return first, last


def trigger_lanes(wave):
    """lanes 3, 31, 32 and 60 of the wavefront; of the ragged one, which ends at lane 26: 3, 10, 17 and its last valid lane"""
    first, last = lanes_of(wave)
    return [first + l for l in ((3, 31, 32, 60) if last - first == 63 else (3, 10, 17, last - first))]


def compared_lanes(wave):
    """lane 0, the last valid lane, the trigger lanes and four fixed others"""
    first, last = lanes_of(wave)
    others = [first + l for l in (7, 21, 40, 55, 12, 17) if first + l <= last][:4]
    return sorted({first, last} | set(trigger_lanes(wave)) | set(others))


def stimulus(kind):
    """[S, 2, N]: channel 0 is the programs' stimulus, channel 1 half of it but for the trigger words"""
    S = sum(blocks_of(kind))
    x = np.empty((S, 2, N), dtype=np.float32)
    x[:, 0, :] = progs.stimulus(N, S)
    x[:, 1, :] = progs.stimulus(N, S) * np.float32(0.5)
    for w in range(WAVES):
        s = trigger_sample(kind, w)
        if s is not None:
            x[s - (DELAY if kind == "delay" else 0), 1, trigger_lanes(w)] = TRIGGER_WORD[kind]
    return x


def _written(text):
    return {l.split(None, 1)[1].split(",")[0].strip() for l in positions(text) if _op(l) not in ("end", "skip", "idelay", "xdelay")}


def watched_registers(text, kind):
    """the trigger's registers, ccr and up to four of the base program's own: statics that its instructions write (the first three
    and the last one), then others"""
    own = [r for r in re.findall(r"^static\s+(\S+)", text, re.M) if r not in ("noise", "big")]
    first = [r for r in own if r in _written(text)]
    first = first[:3] + first[-1:] if len(first) > 4 else first
    return (["trd", "tuse"] if kind == "delay" else ["trg"]) + ["ccr"] + (first + [r for r in own if r not in first])[:4]


def preset_registers(text, kind):
    """the watched registers of the base program that some instruction writes: they start every batch at small non-zero values
    (preset_value), so that the first sample of the first launch does not run on an all-zero state - a stale (1 - X) of an
    INTERP would not show on b = 0.  (A register that nothing writes is a uniform of the translated code: left alone.)"""
    return [r for r in watched_registers(text, kind) if r in _written(text) and r not in ("trg", "trd", "tuse", "ccr")]


def preset_value(k, lane, kind=None):
    """register k of preset_registers() in `lane`: one of 30 values of magnitude 1/64 .. 29/64, never zero; a quarter of that for
    the loud trigger, so that no wavefront starts above the quiet loop's bound of 0.25 on a checked row"""
    return float(np.float32((((lane * 7 + k * 13) % 30) - 15 + 0.5) / (128.0 if kind == "loud" else 32.0)))


class LaneRun:
    """one oracle over the blocks of one lane, stepped a sample at a time: per sample the trigger register's bits and the
    out-of-domain flags, per block the output words, the watched registers and the instruction counter"""

    def __init__(self, oracle_class, text, kind, x_lane, registers, lane, presets):
        o = oracle_class(2)
        assert o.load_text(text), o.errors()
        for k, r in enumerate(presets):
            o.set_register(r, preset_value(k, lane, kind))
        reg = "trd" if kind == "delay" else "trg"
        self.trigger, self.ood, self.out, self.regs, self.count, self.ood_block = [], [], [], [], [], []
        s = 0
        for length in blocks_of(kind):
            ys = []
            for _ in range(length):
                ys.append(o.process_block(np.ascontiguousarray(x_lane[s:s + 1]).reshape(1, 2)))
                self.trigger.append(o.get_register_bits(reg))
                self.ood.append(o.ood_flags())
                s += 1
            self.out.append(np.concatenate(ys, axis=0))
            self.regs.append({r: o.get_register_bits(r) for r in registers})
            self.count.append(o.instruction_counter())
            self.ood_block.append(o.ood_flags())

    def fired(self, kind, s):
        """the trigger did what it is there for in sample s, and not before"""
        finite = lambda w: (w & 0x7f800000) != 0x7f800000   # noqa: E731
        if kind == "delay":
            return self.trigger[s] == 0x40000000 and all(w != 0x40000000 for w in self.trigger[:s]) and self.ood[s] == 0
        if kind == "lut":
            return self.ood[s] & 16 == 16 and (s == 0 or self.ood[s - 1] & 16 == 0)
        if kind == "loud":
            return self.trigger[s] == 0x3f800000 and all(w != 0x3f800000 for w in self.trigger[:s])
        return not finite(self.trigger[s]) and all(finite(w) for w in self.trigger[:s])


def fired_waves(oracle_class, text, kind, x, presets):
    """{wavefront: the first trigger lane of it in which the trigger fires in the wavefront's sample, or None}"""
    out = {}
    for w in range(WAVES):
        s = trigger_sample(kind, w)
        if s is None:
            continue
        out[w] = None
        for lane in trigger_lanes(w):
            if LaneRun(oracle_class, text, kind, x[:, :, lane], (), lane, presets).fired(kind, s):
                out[w] = lane
                break
    return out
