"""Directed programs for the sum groups of the quiet loop (fx_xlate.hpp SumGroup; fxp_translate stream 6), shared by
test_xlate_sum_groups.py (plan and emitted code, without a GPU) and test_gpu_sum_groups.py (the loop on the device).

Every program opens with the same bank - 12 one-pole states s_i and 40 taps `macs t_i, s_j, in, 0.5` whose saturations are idle only
under the quiet plan's head bounds (0.25 for s_i, 1 for the PCM input), which is what puts a quiet loop in force - and then runs one or
more accumulator chains over the t_i (running bound 0.75 each).  A chain starts at `macs a, 0, t0, 1.0`; its first few links are
idle by the plan's running bound, the rest are kept saturations: the links the groups are made of."""

BANK, STATES = 40, 12


def _program(chain, statics=("a",), out="a"):
    lines = ["input in 0", "output out 0", "control k = 0.3"]
    lines += ["static s%d" % i for i in range(STATES)] + ["static t%d" % i for i in range(BANK)] + ["static %s" % s for s in statics]
    body = ["interp s%d, s%d, k, in" % (i, i) for i in range(STATES)]
    body += ["macs t%d, s%d, in, 0.5" % (i, i % STATES) for i in range(BANK)]
    body += chain
    body += ["macs out, 0, %s, 0.5" % out, "end"]
    return "\n".join(lines + body)


def _links(acc, n, op=lambda k: "macs", y=lambda k: "0.05", first=0):
    return ["%s %s, %s, t%d, %s" % (op(k), acc, acc, (first + k) % BANK, y(k)) for k in range(n)]


def macsn_links():
    """every other link subtracts"""
    return _program(["macs a, 0, t0, 1.0"] + _links("a", 30, op=lambda k: "macsn" if k % 2 else "macs"))


def rewritten_addend():
    """acc3 a, a, u, 0 with u written again before the group's test: the addend is copied"""
    chain = ["macs a, 0, t0, 1.0"]
    for k in range(24):
        chain.append("macs u, 0, t%d, 0.5" % (k % BANK))
        chain.append("acc3 a, a, u, 0" if k % 4 == 3 else "macs a, a, u, 0.05")
    return _program(chain, statics=("a", "u"))


def two_chains():
    """links of a and of b by turns: one set of group registers, so only the chain that starts first is grouped"""
    chain = ["macs a, 0, t0, 1.0", "macs b, 0, t1, 1.0"]
    for k in range(24):
        chain.append("macs a, a, t%d, 0.05" % (k % BANK))
        chain.append("macs b, b, t%d, 0.05" % ((k + 7) % BANK))
    chain.append("macs a, a, b, 0.5")
    return _program(chain, statics=("a", "b"))


def reader_in_mid_chain():
    """q reads a between two links: the group closes in front of it and q sees saturated bits"""
    chain = ["macs a, 0, t0, 1.0"] + _links("a", 18) + ["macs q, 0, a, 0.5"] + _links("a", 12, first=18) + ["macs a, a, q, 0.125"]
    return _program(chain, statics=("a", "q"))


def one_link():
    """a chain of one kept link: no group"""
    return _program(["macs a, 0, t0, 1.0", "macs a, a, t1, 1.0"])


def long_chain():
    """more links than one group holds: several groups, the value carried from one to the next in spare registers"""
    return _program(["macs a, 0, t0, 1.0"] + _links("a", 70))


def row_by_row():
    """addends that are products of two rows (bound 0.5625: every such sum is watched) among small ones"""
    return _program(["macs a, 0, t0, 1.0"] + _links("a", 28, y=lambda k: "t%d" % ((k + 3) % BANK) if k % 5 == 4 else "0.05"))


def ccr_addend():
    """`macs a, a, ccr, 0.05` in mid-chain: the running bound of the CCR (row 0) is +inf whatever the plan checks, so the record is
    no link - it keeps its own saturation and, reading and writing a, cuts the chain in two.  (As an operand the CCR is the float
    0, 2, 6, 8, 16 or 20 that the instruction in front of it left: 0.05 times it is up to 1.0.)"""
    chain = ["macs a, 0, t0, 1.0"] + _links("a", 14) + ["macs a, a, ccr, 0.05"] + _links("a", 12, first=14)
    return _program(chain)


def config5_controls_as_rows():
    """config5 with damp, decay and diff as register-file rows - what a control that moves per instance is: statics with the
    controls' values that copy themselves every sample.  Every product with one of them is row x row (bound 1 x 1 where the plan
    does not check the row); the m chain's own multipliers stay the literals 0.05 and 0.01"""
    import fx8010_programs as P
    text = P.CONFIGS["config5"]()
    for name, value in (("damp", "0.3"), ("decay", "0.45"), ("diff", "0.6")):
        assert "control %s = %s" % (name, value) in text
        text = text.replace("control %s = %s" % (name, value), "static %s = %s" % (name, value))
    # (three instructions more than config5: the copies that make them rows)
    return text.replace("\nend", "\nmacs damp, damp, 0, 0\nmacs decay, decay, 0, 0\nmacs diff, diff, 0, 0\nend")


EDGE_REGS = 25


def edge_values():
    """a chain whose every value a register write sets exactly: a = e0, a += e_k / 4 for k = 1 .. 12, a += e_k / 32 for k = 13 .. 24.
    The e_k only copy themselves.  The plan checks e0 .. e12 at 0.25, so the first twelve links are idle (0.25 + 12 / 16 = 1);
    checking the others would idle nothing, so they stay unchecked (bound 1) and their links are kept: a chain whose start (bound
    1) is watched and whose addends (bound 2^-5) are small - covered sums between the watched ones, as many as a group holds, and
    T = 1 - that many / 32, rounded as the bound pass rounds.  All powers of two: a test can put the start at T, one float beside it, at +-1.0, carry -0 (a = e0 - 0 keeps the sign of a
    zero) or denormals through the chain, with every checked e_k inside its bound"""
    chain = ["macsn a, e0, 0, 0"] + ["macs a, a, e%d, %s" % (k, "0.25" if k <= 12 else "0.03125") for k in range(1, EDGE_REGS)]
    chain += ["macs e%d, e%d, 0, 0" % (k, k) for k in range(EDGE_REGS)]    # (written, so that they are rows and not constants)
    return _program(chain, statics=["a"] + ["e%d" % k for k in range(EDGE_REGS)])


EDGE = ("edge_values", edge_values())
DIRECTED = [("macsn_links", macsn_links()), ("rewritten_addend", rewritten_addend()), ("two_chains", two_chains()),
            ("reader_in_mid_chain", reader_in_mid_chain()), ("one_link", one_link()), ("long_chain", long_chain()),
            ("row_by_row", row_by_row()), ("ccr_addend", ccr_addend()), ("config5_rows", config5_controls_as_rows())]
