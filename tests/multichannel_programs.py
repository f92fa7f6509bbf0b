"""Programs of two to four channels for the multichannel parity tests: program texts and generators only (neither the library
nor the reference is imported here).  Shared by test_oracle_vs_ref.py (the restatement against the compiled reference),
tests/golden/make_golden.py (multichannel.json) and test_gpu_multichannel.py (every tier on the device).

The rule all of them turn on (source/FX8010.cpp:1053-1061, 1229-1233): in an instruction with an INPUT operand, A, X and Y - as
far as they are inputs - are refreshed from inputBuffer[A.IOIndex], and the refreshed value stays in the register.  IOIndex is 0
for a register that is neither input nor output and the channel of an output register.  csrc/fx_decode.cpp (sections 3 and 7)
lowers that into an input aliased onto its channel's PCM row (one consistent channel, read outside every SKIP shadow, no delay
target), an input with a row of its own and prefix refreshes (everything else), channels without an input row, and one output
latch row per channel.  The texts are fixed by their names and seeds: counts asserted elsewhere depend on them."""
import numpy as np


def _program(decls, body):
    return "\n".join(list(decls) + list(body) + ["end"])


def _io(channels, ins=None, outs=None):
    ins = range(channels) if ins is None else ins
    outs = range(channels) if outs is None else outs
    return ["input i%d %d" % (c, c) for c in ins] + ["output o%d %d" % (c, c) for c in outs]


def _late_reads_staged():
    """the filter chain of fx8010_programs.config2() over four channels: 31 x (INTERP ; MACS), channel 0 feeds the chain from its
    first record on, channels 1 and 2 come in through an A of their own in the last quarter only (records 48 ..), channel 3 is
    never read; the four outputs are written in the four quarters of the 67 records"""
    L = _io(4, ins=(0, 1, 2)) + ["control cutoff = 0.1", "static t"] + ["static s%d" % i for i in range(31)]
    body, prev = [], "i0"
    for i in range(31):
        body.append("interp s%d, s%d, cutoff, %s" % (i, i, prev))
        if i < 24:
            body.append("macs t, s%d, i0, 0.05" % i)
        else:
            body.append("macs t, %s, s%d, 0.05" % ("i1" if i < 28 else "i2", i))
        prev = "t"
        if i in (4, 12, 20):
            body.append("macs o%d, 0, t, 1.0" % (i // 8))
    body.append("macs o3, 0, t, 1.0")
    return _program(L, body)


# name -> (channels, text, registers to compare)
DIRECTED = {
    # l as A on its own channel, then as X under an A of channel 1, then under a static A (channel 0) again; r as A (channel 1)
    # and as Y under a static A: neither can be an alias, both get rows of their own and a prefix refresh per reading record
    "conflict": (2, _program(["input l 0", "input r 1", "output ol 0", "output or 1", "static t", "static u", "static v"],
                             ["macs t, l, 0.5, 0.5", "macs u, r, l, 0.5", "macs v, t, l, 0.25", "macs ol, t, u, 0.5",
                              "macs or, v, -0.5, r"]), ("l", "r", "t", "u", "v", "ol", "or", "ccr")),
    # A is the output register of channel 1: X / Y inputs under it are read through channel 1 (l, the input of channel 0, too);
    # under the output of channel 0 and under a literal they are read through channel 0
    "a_is_output": (2, _program(["input l 0", "input r 1", "output ol 0", "output or 1", "static t"],
                                ["macs or, 0, r, 0.5", "macs t, or, l, 0.5", "macs ol, or, 0.25, r", "macs or, ol, l, r"]),
                    ("l", "r", "t", "ol", "or", "ccr")),
    # the inputs of channels 1 .. 3 only ever under a literal, a static or channel 0's input as A: all of them hear channel 0,
    # channels 1 .. 3 have no input row at all
    "a_is_literal": (4, _program(_io(4) + ["static k = 0.25", "static t"],
                                 ["macs o0, 0, i1, 0.5", "macs o1, 0.125, i2, i3", "macs o2, k, 0.5, i3", "macs t, i0, i1, 0.5",
                                  "macs o3, t, i2, 0.75"]), ("i0", "i1", "i2", "i3", "t", "o0", "o1", "o2", "o3", "ccr")),
    # m (channel 2) is read inside a SKIP shadow only: in the samples whose SKIP fires (l negative) its register keeps the last
    # refreshed value; r is read inside the shadow through channel 1 and outside it through channel 0
    "shadow_only": (3, _program(["input l 0", "input r 1", "input m 2", "output ol 0", "output or 1", "output om 2",
                                 "static s", "static t", "static u"],
                                ["macs s, l, 0, 0", "skip ccr, ccr, 6, 2", "macs t, r, 0.5, 0.5", "macs om, m, t, 0.5",
                                 "macs u, l, r, 0.5", "macs ol, u, t, 0.5", "macs or, t, u, -0.5"]),
                    ("l", "r", "m", "s", "t", "u", "ol", "or", "om", "ccr")),
    # leading delay-line reads into input registers: r (iTRAM) is read again inside a shadow only - where the SKIP fires its
    # register still holds the delayed word -, l2 (xTRAM, a second input register of channel 0) outside every shadow
    "delay_into_input": (2, _program(["itramsize 7 ", "xtramsize 5 ", "input l 0", "input r 1", "input l2 0", "output ol 0",
                                      "output or 1", "static t"],
                                     ["idelay read, r, at, 0", "xdelay read, l2, at, 0", "macs t, l, 0, 0", "skip ccr, ccr, 6, 1",
                                      "macs ol, 0, r, 0.5", "macs or, t, l2, 0.5", "idelay write, l, at, 0", "xdelay write, t, at, 0"]),
                         ("l", "r", "l2", "t", "ol", "or", "ccr")),
    # what the input registers hold after a block: r is shadow-only (the value of the last sample whose SKIP did not fire, or a
    # written one), l ends on channel 2's word (read through m's channel last), m is an alias of channel 2's row
    "stale_register": (3, _program(["input l 0", "input r 1", "input m 2", "output ol 0", "output or 1", "output om 2",
                                    "static s", "static t", "static u"],
                                   ["macs s, l, 0, 0", "skip ccr, ccr, 6, 1", "macs t, r, 0.5, 0.5", "macs u, m, l, 0.5",
                                    "macs ol, t, s, 0.5", "macs or, s, u, 0.25", "macs om, u, t, 0.5"]),
                       ("l", "r", "m", "s", "t", "u", "ol", "or", "om", "ccr")),
    # four channels, only input 2 is read (always as A: through its own channel), only outputs 1 and 3 are written
    "sparse4": (4, _program(["input x 2", "output a 1", "output b 3", "static t"],
                            ["macs t, x, 0.5, 0.5", "macs a, x, t, 0.25", "macs b, x, t, -0.5"]), ("x", "t", "a", "b", "ccr")),
    # two output registers on channel 1: ob, oa, then ob again inside a shadow - the last executed writer's word goes out
    "two_outputs_one_channel": (2, _program(["input l 0", "input r 1", "output oa 1", "output ob 1", "output ol 0", "static s"],
                                            ["macs ob, l, 0.125, 0.5", "macs oa, r, 0.5, 0.5", "macs s, l, 0, 0", "skip ccr, ccr, 6, 1",
                                             "macs ob, r, l, 0.25", "macs ol, l, oa, 0.5"]), ("l", "r", "s", "oa", "ob", "ol", "ccr")),
    # three channels (an odd count for the PCM address arithmetic), every input as A, X and Y
    "three_all": (3, _program(_io(3) + ["static t0", "static t1", "static t2"],
                              ["macs t0, i0, i1, i2", "macs t1, i1, i2, i0", "macs t2, i2, i0, i1", "macs o0, t0, t1, 0.5",
                               "macs o1, i1, t2, 0.25", "macs o2, i2, t0, -0.5"]),
                  ("i0", "i1", "i2", "t0", "t1", "t2", "o0", "o1", "o2", "ccr")),
    "late_reads_staged": (4, _late_reads_staged(), ("i0", "i1", "i2", "t", "s0", "s15", "s30", "o0", "o1", "o2", "o3", "ccr")),
}

OPS3 = ["macs", "macsn", "macints", "acc3", "macw", "macwn", "macintw", "macmv", "tstneg", "limit", "limitn", "interp", "andxor"]


def generated(seed):
    """(channels, text, registers): the random_program of test_oracle_vs_ref.py over 2 .. 4 channels - one to channels + 1 input
    registers and as many output registers on random channels, so that channels repeat and others stay unused; inputs and outputs
    among the sources, outputs among the destinations; the leading iTRAM read goes into r5 or into an input register.  The
    literals 3, 7 and 15 among the sources drive many bodies into saturation, so every output is closed with a blend of an input
    under the output as A - read through the OUTPUT's channel -: which channel's word went where shows in the output words of
    every seed, not only in the registers."""
    rng = np.random.default_rng(606000 + seed)
    channels = int(rng.integers(2, 5))
    ins = ["in%d" % k for k in range(int(rng.integers(1, channels + 2)))]
    outs = ["out%d" % k for k in range(len(ins))]
    n_instr = int(rng.integers(5, 60))
    regs = ["r%d" % i for i in range(6)]
    lits = ["0", "0.5", "-0.25", "1.0", "0.125", "2", "-1", "0.999", "3", "7", "15"]
    pick = lambda v: str(v[int(rng.integers(0, len(v)))])   # noqa: E731
    L = ["input %s %d" % (n, rng.integers(0, channels)) for n in ins] + ["output %s %d" % (n, rng.integers(0, channels)) for n in outs]
    L += ["control c = 0.3", "static noise", "itramsize 11 ", "xtramsize 23 "] + ["static %s" % r for r in regs]
    L.append("idelay read, %s, at, 0" % (pick(ins) if rng.integers(0, 2) else "r5"))
    L.append("xdelay read, r4, at, 0")
    src = lambda: pick(regs + lits + ins + ["c"] + outs + ["ccr", "noise"])   # noqa: E731
    body = []
    for i in range(n_instr):
        kind = rng.integers(0, 100)
        dst = pick(regs + outs)
        if kind < 70:
            body.append("%s %s, %s, %s, %s" % (pick(OPS3), dst, src(), src(), src()))
        elif kind < 80:
            body.append("%s %s, %s, %d, 0" % (pick(["log", "exp"]), dst, pick(ins + ["c", "0.5", "-0.25"]), rng.integers(0, 32)))
        elif kind < 90 and i + 4 < n_instr:
            body.append("skip ccr, ccr, %s, %d" % (pick(["0", "2", "6", "8", "16", "20"]), rng.integers(0, 3)))
        else:
            body.append("macs %s, %s, %s, %s" % (dst, src(), src(), src()))
    body += ["idelay write, r0, at, 0", "xdelay write, r1, at, 0"]
    body += ["macs %s, %s, r2, 0.5" % (o, o) for k, o in enumerate(outs) if k == 0 or rng.integers(0, 2)]
    body += ["interp %s, %s, 0.5, %s" % (o, o, pick(ins)) for o in outs]
    return channels, _program(L, body), tuple(regs + ["ccr"] + ins + outs)


def generated_chain(seed):
    """(channels, text, registers): a chain the stage planner cuts (the shape of late_reads_staged, 40 .. 56 INTERP / MACS pairs)
    over 3 or 4 channels, with the channel each MACS hears, the position of the input in it (A: its own channel, X: channel 0 under
    the static A) and the records that write the outputs drawn at random"""
    rng = np.random.default_rng(707000 + seed)
    channels = int(rng.integers(3, 5))
    pairs = int(rng.integers(40, 57))
    L = _io(channels) + ["control cutoff = 0.1", "static t"] + ["static s%d" % i for i in range(pairs)]
    writes = {int(p): int(c) for c, p in enumerate(sorted(rng.choice(np.arange(2, pairs - 1), size=channels - 1, replace=False)))}
    body, prev = [], "i%d" % rng.integers(0, channels)
    for i in range(pairs):
        body.append("interp s%d, s%d, cutoff, %s" % (i, i, prev))
        inp = "i%d" % rng.integers(0, channels)
        body.append("macs t, %s, s%d, 0.05" % (inp, i) if rng.integers(0, 2) else "macs t, s%d, %s, 0.05" % (i, inp))
        prev = "t"
        if i in writes:
            body.append("macs o%d, 0, t, 1.0" % writes[i])
    body.append("macs o%d, o%d, t, 0.5" % (channels - 1, int(rng.integers(0, channels))))
    regs = ["i%d" % c for c in range(channels)] + ["o%d" % c for c in range(channels)] + ["t", "s0", "s%d" % (pairs - 1), "ccr"]
    return channels, _program(L, body), tuple(regs)


def stimulus(progs, n, samples, channels, seed=0):
    """[S, channels, N]: fx8010_programs.stimulus with one stream per instance AND channel (channel c of instance n is instance
    c * N + n of the generator, `seed` moves the whole block)"""
    return np.ascontiguousarray(progs.stimulus(n * channels, samples, first_instance=seed * 65536).reshape(samples, channels, n))
