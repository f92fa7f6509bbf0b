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


def generated_wide(seed):
    """generated() and what else a quiet plan admits: LIMIT / LIMITN with rows and constants in every operand position (the PCM
    input as X or Y among them), folded moves (macs r, x, 0, 0), fully constant records, both delay lines with leading reads whose
    rows nothing writes again - and, for every third seed, two channels (two input and two output rows)."""
    rng = np.random.default_rng(515100 + seed)
    stereo = seed % 3 == 1
    n_regs, n_instr = int(rng.integers(4, 20)), int(rng.integers(120, 320))
    regs = ["r%d" % i for i in range(n_regs)]
    ins = ["inl", "inr"] if stereo else ["in"]
    outs = ["outl", "outr"] if stereo else ["out"]
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
