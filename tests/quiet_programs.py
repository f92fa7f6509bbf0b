"""Generated programs for the quiet-loop tests (fx_xlate.hpp QuietPlan): SKIP-free, with delay lines whose reads open the program,
so that every one of them is eligible for a quiet loop.  Shared by test_xlate_quiet.py (the plan's soundness, without a GPU) and
test_gpu_quiet_states.py (the loop on the device).  The texts are fixed by their seeds: counts asserted elsewhere depend on them."""
import re

import numpy as np


def generated(seed):
    """a SKIP-free program of MACS / MACSN / ACC3 / INTERP over a few state registers, with delay lines whose reads open the
    program (such reads are issued a sample ahead, and their values are in their rows at the head of the sample)"""
    rng = np.random.default_rng(424200 + seed)
    n_regs, n_instr = int(rng.integers(4, 24)), int(rng.integers(150, 400))
    regs = ["r%d" % i for i in range(n_regs)]
    coef = ["0.3", "0.5", "-0.25", "0.125", "0.7", "-0.6", "0.05", "k", "0.999", "1.0", "0"]
    lines = ["input in 0", "output out 0", "control k = 0.4"] + ["static %s" % r for r in regs]
    delays = int(rng.integers(0, 3))   # 0: none, 1: xTRAM, 2: both
    if delays >= 1:
        lines += ["xtramsize 37 ", "static xd"]
    if delays == 2:
        lines += ["itramsize 11 ", "static rd"]
    body = []
    if delays >= 1:
        body.append("xdelay read, xd, at, 0")
    if delays == 2:
        body.append("idelay read, rd, at, 0")
    pool = regs + (["xd"] if delays >= 1 else []) + (["rd"] if delays == 2 else [])
    for _ in range(n_instr):
        op = str(rng.choice(["macs", "macs", "macs", "macsn", "macsn", "acc3", "interp"]))
        dst = str(rng.choice(regs))
        row = lambda: str(rng.choice(pool + ["in"]))   # noqa: E731
        c = lambda: str(rng.choice(coef))              # noqa: E731
        if op == "acc3":
            body.append("acc3 %s, %s, %s, %s" % (dst, row(), row(), rng.choice([row(), c()])))
        elif op == "interp":
            body.append("interp %s, %s, %s, %s" % (dst, row(), rng.choice(["0.3", "0.5", "k", "0.125"]), row()))
        else:
            a = rng.choice([row(), "0"])
            x, y = (row(), c()) if rng.integers(0, 4) else (row(), row())
            body.append("%s %s, %s, %s, %s" % (op, dst, a, x, y))
    if delays >= 1:
        body.append("xdelay write, %s, at, 0" % rng.choice(regs))
    if delays == 2:
        body.append("idelay write, %s, at, 0" % rng.choice(regs))
    body += ["macs out, %s, %s, 0.5" % (regs[0], regs[1]), "end"]
    return "\n".join(lines + body)


GENERATED = [("gen%d" % s, generated(s)) for s in range(12)]


def generated_wide(seed, channels=None):
    """generated() and what else a quiet plan admits: LIMIT / LIMITN with rows and constants in every operand position (the PCM
    input as X or Y among them), folded moves (macs r, x, 0, 0), fully constant records, both delay lines with leading reads whose
    rows nothing writes again - and, for every third seed, two channels (two input and two output rows).  `channels` asks for
    that many (in0 .. / out0 ..: every input in every operand position, so under the A of any channel) instead."""
    rng = np.random.default_rng(515100 + seed)
    stereo = seed % 3 == 1
    n_regs, n_instr = int(rng.integers(4, 20)), int(rng.integers(120, 320))
    regs = ["r%d" % i for i in range(n_regs)]
    ins = ["inl", "inr"] if stereo else ["in"]
    outs = ["outl", "outr"] if stereo else ["out"]
    if channels is not None:
        ins, outs = ["in%d" % c for c in range(channels)], ["out%d" % c for c in range(channels)]
    coef = ["0.3", "0.5", "-0.25", "0.125", "0.7", "-0.6", "0.05", "k", "0.999", "1.0", "0"]
    lines = ["input %s %d" % (n, i) for i, n in enumerate(ins)] + ["output %s %d" % (n, i) for i, n in enumerate(outs)]
    lines += ["control k = 0.4"] + ["static %s" % r for r in regs]
    delays = int(rng.integers(0, 3))   # 0: none, 1: xTRAM, 2: both
    if delays >= 1:
        lines += ["xtramsize 37 ", "static xd"]
    if delays == 2:
        lines += ["itramsize 11 ", "static rd"]
    body = []
    if delays >= 1:
        body.append("xdelay read, xd, at, 0")
    if delays == 2:
        body.append("idelay read, rd, at, 0")
    pool = regs + (["xd"] if delays >= 1 else []) + (["rd"] if delays == 2 else [])
    pick = lambda v: str(v[int(rng.integers(0, len(v)))])   # noqa: E731
    row = lambda: pick(pool + ins)                          # noqa: E731
    c = lambda: pick(coef)                                  # noqa: E731
    any_ = lambda: row() if rng.integers(0, 3) else c()     # noqa: E731
    for _ in range(n_instr):
        op = pick(["macs", "macs", "macs", "macsn", "macsn", "acc3", "interp", "limit", "limitn", "mov", "const"])
        dst = pick(regs)
        if op == "acc3":
            body.append("acc3 %s, %s, %s, %s" % (dst, row(), row(), any_()))
        elif op == "interp":
            body.append("interp %s, %s, %s, %s" % (dst, row(), pick(["0.3", "0.5", "k", "0.125"]), row()))
        elif op in ("limit", "limitn"):
            body.append("%s %s, %s, %s, %s" % (op, dst, any_(), any_(), any_()))
        elif op == "mov":
            body.append("macs %s, %s, 0, 0" % (dst, row()))
        elif op == "const":
            body.append("%s %s, %s, %s, %s" % (pick(["macs", "macsn", "acc3"]), dst, c(), c(), c()))
        else:
            a = row() if rng.integers(0, 2) else "0"
            x, y = (row(), c()) if rng.integers(0, 4) else (row(), row())
            body.append("%s %s, %s, %s, %s" % (op, dst, a, x, y))
    if delays >= 1:
        body.append("xdelay write, %s, at, 0" % pick(regs))
    if delays == 2:
        body.append("idelay write, %s, at, 0" % pick(regs))
    for k, o in enumerate(outs):
        body.append("macs %s, %s, %s, 0.5" % (o, regs[k % n_regs], regs[(k + 1) % n_regs]))
    body.append("end")
    return "\n".join(lines + body)


WIDE_SEEDS = tuple(range(12))
GENERATED_WIDE = [("wide%d" % s, generated_wide(s)) for s in WIDE_SEEDS]

# the probe the LIMIT rule was first seen with: gen0 with four records in front of `end`
LIMIT_EDIT = ("gen0_limit", GENERATED[0][1][:-3] + "limit r0, r1, r2, r3\nlimitn r1, r0, r2, 0.5\nmacs r2, r3, 0, 0\nlimit r3, in, r0, r1\nend")


def delay_edit(text):
    """both delay lines carry the input times +-0.5, exactly: in = 0.5 comes back as +0.25 in the xTRAM's read row 37 samples
    later and as -0.25 in the iTRAM's 11 samples later, the next float above 0.5 as the next floats beyond +-0.25"""
    text = text.replace("static xd", "static xd\nstatic q").replace("static rd", "static rd\nstatic p")
    text = re.sub(r"xdelay write, \w+, at, 0", "macs q, 0, in, 0.5\nxdelay write, q, at, 0", text)
    return re.sub(r"idelay write, \w+, at, 0", "macsn p, 0, in, 0.5\nidelay write, p, at, 0", text)


DELAY_EDIT = ("gen3_delay", delay_edit(GENERATED[3][1]))


# ---- directed programs for the signs of zero (ZERO_PROGRAMS): bodies above that get a loop, with records spliced in whose results
# differ from the reference's in the sign of a zero - or in a smallest denormal against a zero - if one of the translator's IEEE
# shortcuts (fx_xlate.cpp: zeroAddsOf, zeroPlusScaled, unit multipliers, the product cache, INTERP's one fma, host-folded records)
# is wrong.  Every directed record writes a register of its own, so that the state after a block shows each of them.
#
# The literal -0: the reference's parser does yield a negative zero for the text "-0" (pyoracle.Oracle: `macmv c, -0, 0, 0`
# leaves 0x80000000 in c), and so does this project's front end - the records carry the uniform 0x80000000.
ZERO_C = ["1.0", "-1.0", "0.5", "0.50000006", "0.75", "-0.6", "0.999", "1.5", "4.0", "0.25", "0.001"]


def splice(text, statics, records):
    """`records` in front of the delay-line writes (or of the output record), their registers behind the last `static`"""
    lines = text.split("\n")
    k = max(i for i, l in enumerate(lines) if l.startswith("static "))
    lines[k + 1:k + 1] = ["static %s" % s for s in statics]
    e = min(i for i, l in enumerate(lines) if re.match(r"[xi]delay write|macsn? [qp], |macs out", l))
    lines[e:e] = records
    return "\n".join(lines)


def scaled(x, tag, swapped=()):
    """(registers, records): macs r, 0, x, c and macsn r, 0, x, c for every c of ZERO_C; for the c at the indices `swapped` also
    with the multiplier in the X position"""
    regs, recs = [], []
    for k, c in enumerate(ZERO_C):
        for op in ("macs", "macsn"):
            r = "%s%s%d" % (tag, op[3:] or "p", k)
            regs.append(r)
            recs.append("%s %s, 0, %s, %s" % (op, r, x, c))
            if k in swapped:
                regs.append(r + "x")
                recs.append("%s %sx, 0, %s, %s" % (op, r, c, x))
    return regs, recs


def zero_family(base, parts, statics=(), records=()):
    regs, recs = list(statics), list(records)
    for x, tag, swapped in parts:
        a, b = scaled(x, tag, swapped)
        regs += a
        recs += b
    return splice(base, regs, recs + ([ZU_TAIL] if "zu" in regs else []))


# rows of every kind an X can come from: written this sample by a sum (zs: clean), a product on top of a row that may be -0 (zp),
# an INTERP (zi), LIMIT / LIMITN (zl, zln), a folded move (zm), a fully constant record (zc); zu is a state row that only the LAST
# directed record writes (ZU_TAIL: a blend that hands a -0 and a denormal of the input on) - every record in front of that one
# reads what the sample before left there
ZU_TAIL = "interp zu, in, 0.5, in"
PRODUCERS = (["zu", "zs", "zp", "zi", "zl", "zln", "zm", "zc"],
             ["macs zs, 0, in, 0.25", "macs zp, zu, in, 0.25", "interp zi, in, 0.5, zu", "limit zl, in, zu, in", "limitn zln, zu, in, 0.001",
              "macs zm, in, 0, 0", "macs zc, 0.3, 0.5, 0.25"])

# acc3 r, A, X, 0 over the kinds of (A, X): (in, in) - the add must stay -, a sum and its mirror image, a non-zero uniform and
# its mirror image, a product, an INTERP result, a LIMIT pick, and the leading delay-line read rows beside a sum, the input
# and each other
ZERO_ACC3 = ["acc3 a0, in, in, 0", "acc3 a1, zs, in, 0", "acc3 a2, in, zs, 0", "acc3 a3, 0.3, in, 0", "acc3 a4, in, 0.3, 0",
             "acc3 a5, zp, in, 0", "acc3 a6, zi, in, 0", "acc3 a7, zl, in, 0", "acc3 a8, xd, zs, 0", "acc3 a9, xd, in, 0",
             "acc3 a10, rd, xd, 0", "acc3 a11, zm, zu, 0", "acc3 a12, zc, in, 0", "acc3 a13, zln, zs, 0"]

# the literal -0 as a uniform operand in every position
ZERO_MINUS = ["macmv n0, -0, 0, 0", "macs n1, -0, in, 0.75", "macsn n2, -0, in, 0.75", "acc3 n3, -0, in, 0", "acc3 n4, in, -0, 0",
              "acc3 n5, -0, -0, 0", "acc3 n6, in, zu, -0", "macs n7, 0, in, -0", "macsn n8, 0, in, -0", "macs n9, 0, -0, in",
              "interp n10, -0, 0.5, in", "interp n11, in, 0.5, -0", "limit n12, in, -0, 0", "limitn n13, -0, in, zu",
              "macs n14, n0, 0, 0", "acc3 n15, n0, n0, 0", "macs n16, 0, n0, 1.0", "macs n17, -0, -0, 0.5", "macsn n18, -0, 0.5, 0"]

# 0 + X * 1.0 whose saturation stays and whose X cannot be -0: the copy of a uniform above 1 (the one way to a clean row outside
# [-1, 1]) - with the unit multiplier in Y and in X, a negative X, -1.0, and the same shapes over rows that are not clean
ZERO_UNIT = ["macmv w0, 4.0, 0, 0", "macs u0, 0, w0, 1.0", "macmv w1, -1.5, 0, 0", "macs u1, 0, 1.0, w1", "macs u2, 0, w0, -1.0",
             "macsn u3, 0, w1, 1.0", "macs w2, w0, 0, 0", "macs u4, 0, w2, 1.0", "macs u5, 0, in, 1.0", "macs u6, 0, 1.0, zu",
             "macsn u7, 0, in, -1.0", "acc3 u8, w0, in, 0", "acc3 u9, w1, w0, 0"]


def minus_zero_delays(text):
    """delay_edit() with the literal -0 as the A of both records: the lines carry the input times +-0.5 exactly AND a -0 where
    the reference has one ((-0) + (-0) * 0.5 = -0, (-0) - (+0) * 0.5 = -0; with A = +0 neither line could ever hold a -0)"""
    return delay_edit(text).replace("macs q, 0, in, 0.5", "macs q, -0, in, 0.5").replace("macsn p, 0, in, 0.5", "macsn p, -0, in, 0.5")


ZERO_DELAY = ["acc3 d0, xd, rd, 0", "acc3 d1, rd, zs, 0", "macs d2, 0, xd, 1.0", "macsn d3, 0, rd, 1.0", "macs d4, xd, rd, -1.0",
              "interp d5, xd, 0.5, rd", "limit d6, xd, rd, 0", "macs d7, xd, 0, 0", "acc3 d8, q, p, 0"]

_G, _W = dict(GENERATED), dict(GENERATED_WIDE)
ZERO_PROGRAMS = [
    # X = the PCM input, every c, the multiplier also in X: with 0.7 of the body more than six constants above 0.5 in magnitude,
    # so that the six most frequent are fused into one v_fma_f32 and the others stay v_mul_f32 + v_add_f32 in the same stream
    ("zero_pool", zero_family(_G["gen10"], [("in", "i", (0, 3, 4, 5, 8))], ["e0", "e1"], ["macs e0, 0, in, 0.7", "macs e1, 0, e0, 0.7"])),
    ("zero_state_read", zero_family(_W["wide9"], [("zu", "s", (1,)), ("xd", "x", (3,)), ("rd", "y", ())], ["zu"])),
    ("zero_sum_product", zero_family(_G["gen2"], [("zs", "s", (4,)), ("zp", "p", (5,))], *PRODUCERS)),
    ("zero_interp_limit", zero_family(_W["wide5"], [("zi", "i", ()), ("zl", "l", (7,)), ("zln", "m", ())], *PRODUCERS)),
    ("zero_move_const", zero_family(_W["wide6"], [("zm", "m", (6,)), ("zc", "c", (9,))], *PRODUCERS)),
    ("zero_acc3", splice(DELAY_EDIT[1], PRODUCERS[0] + ["a%d" % k for k in range(len(ZERO_ACC3))], PRODUCERS[1] + ZERO_ACC3 + [ZU_TAIL])),
    ("zero_minus", splice(_G["gen7"], ["zu"] + ["n%d" % k for k in range(len(ZERO_MINUS))], ZERO_MINUS + [ZU_TAIL])),
    ("zero_unit", splice(_W["wide11"], ["zu", "w0", "w1", "w2"] + ["u%d" % k for k in range(10)], ZERO_UNIT + [ZU_TAIL])),
    ("zero_delay", splice(minus_zero_delays(_G["gen3"]), ["zs"] + ["d%d" % k for k in range(len(ZERO_DELAY))], ["macs zs, 0, in, 0.25"] + ZERO_DELAY)),
]


def sweep_program(c):
    """out = 0 + in * c with the multiplier also in X and 0 - in * c beside it, padded with a state row: the program of the
    denormal sweep (test_gpu_zero_signs.py) - it translates, and needs no quiet loop"""
    return ("input in 0\noutput out 0\nstatic a\nstatic b\nstatic pad\nmacs a, 0, %s, in\nmacsn b, 0, in, %s\nmacs pad, pad, in, 0.25\n"
            "macs out, 0, in, %s\nend" % (c, c, c))
