"""The quiet loop of the translator (fx_xlate.hpp QuietPlan; fxp_translate stream 5), without a GPU.

A quiet loop is the steady fast stream without the saturations that cannot fire while the rows its head checks stay inside their
bounds.  Checked here: the encoder against llvm-mc, that the five other streams are what they were before the loop existed,
which programs get a loop, the hazard lint - and the plan's soundness against an independent restatement: a float32 numpy model
of the steady records is fed head states at and inside the plan's bounds, and at every record whose saturation the plan drops
the unsaturated value must lie in [-1, 1]."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import fx8010_amd as A
import fx8010_programs as P

from test_xlate import assemble, needs_llvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BENCH = ("config1_shipped", "config2", "config3", "config4", "config5")
# handler slots of the records (fx_asm.hpp AsmSlot)
ENDSAMPLE, NOP, MOV, LIMIT, LIMITN, TRAM_IR, TRAM_IW, TRAM_XR, TRAM_XW, MACS, SLOTS = 0, 1, 4, 10, 11, 14, 15, 16, 17, 20, 84


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


def front_end(text):
    fe = A.FrontEnd(1)
    assert fe.load_text(text), fe.errors()
    return fe


# ------------------------------------------------------------------------------------------------ encoder, layout
@needs_llvm
def test_quiet_stream_reassembles_to_the_same_bytes():
    loops = 0
    for name, text in [("config5", P.CONFIGS["config5"]())] + GENERATED:
        fe = front_end(text)
        for vgprs in ((0, 128) if name == "config5" else (0,)):
            code, listing = fe.translate(vgprs, 5)
            plan = fe.quiet_plan(vgprs)
            assert bool(code) == plan["in_force"], name
            if not code:
                continue
            loops += 1
            assert assemble(listing) == code, "%s: encoder and assembler disagree" % name
            ops = [l.split()[0] for l in listing.split("\n") if l and not l.startswith(";")]
            assert ops.count("v_med3_f32") == plan["sites"] - plan["quiet_dropped"], name
            assert ops.count("v_max3_f32") + 2 >= plan["check_instructions"] >= ops.count("v_max3_f32") + 1, name
            assert listing.count("; quiet check") == 1
    assert loops >= 6, loops   # config5 twice and a good part of the generated programs


def test_streams_0_to_4_are_what_they_were():
    """sha256 of the five streams of the benchmark programs, recorded from the build before the quiet loop existed"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "xlate_stream_hashes.json")))["streams"]
    assert sorted({k.split("/")[0] for k in gold}) == sorted(BENCH)
    for key, want in sorted(gold.items()):
        name, vgprs = key.split("/v")
        fe = front_end(P.CONFIGS[name]())
        assert [hashlib.sha256(fe.translate(int(vgprs), s)[0]).hexdigest() for s in range(5)] == want, key
    listing = front_end(P.CONFIGS["config5"]()).translate(128, 0)[1]
    assert sum(l.startswith("v_med3_f32") for l in listing.split("\n")) == 301


def test_config5_plan():
    fe = front_end(P.CONFIGS["config5"]())
    plan = fe.quiet_plan(128)
    assert plan["in_force"] and plan["eligible"]
    assert (plan["sites"], plan["fast_dropped"], plan["quiet_dropped"]) == (503, 202, 395)
    assert len(plan["dropped"]) == 395 and plan["dropped"] == sorted(set(plan["dropped"]))
    names = {n: b for _, n, b in plan["checked"]}
    assert names["in"] == 1.0 and all(b == 0.25 for n, b in names.items() if n != "in")
    assert {"d0", "d1", "d2", "d3", "lp0", "lp3", "y0", "y39"} <= set(names) and not {"m", "u", "v"} & set(names)
    assert plan["check_instructions"] <= 31
    assert plan["quiet_dropped"] - plan["fast_dropped"] >= 4 * plan["check_instructions"]
    # the same plan whatever the VGPR build
    small = fe.quiet_plan(0)
    assert small["dropped"] == plan["dropped"] and small["checked"] == plan["checked"]


def test_eligibility():
    """config2 (the gain does not pay for the check), config3 (its plan gains nothing from a bound on the input: the program
    saturates where the input enters), config4 (LOG / EXP) get no quiet loop - and a program with a control track, with a SKIP, or under the DANE delay-line model neither"""
    for name in ("config2", "config3", "config4"):
        fe = front_end(P.CONFIGS[name]())
        plan = fe.quiet_plan(0)
        assert not plan["in_force"] and plan["why"], name
        assert fe.translate(0, 5)[0] == b"", name
    fe = front_end(P.CONFIGS["config5"]())
    assert fe.track_register("damp") == 0
    assert not fe.quiet_plan(128)["eligible"] and fe.translate(128, 5)[0] == b""
    skip = P.CONFIGS["config5"]().replace("end", "macs u, u, 0, 0\nskip ccr, ccr, 8, 1\nmacs v, v, 0, 0\nmacs u, u, 0, 0\nend")
    assert "SKIP" in front_end(skip).quiet_plan(0)["why"]
    fe = A.FrontEnd(1)
    fe.set_option(A.OPT_TRAM_DANE)
    assert fe.load_text(P.CONFIGS["config5_dane"]())
    assert not fe.quiet_plan(0)["eligible"]
    with pytest.raises(RuntimeError):
        front_end(P.CONFIGS["config2"]()).translate_staged(8, 0, 5)


def test_hazard_lint_passes_over_the_quiet_stream():
    import gfx950_lint as L
    if not os.path.exists(os.path.join(L.LLVM, "llvm-objdump")):
        pytest.skip("llvm tools not available")
    linted = 0
    for name, text in [("config5", P.CONFIGS["config5"]())] + GENERATED:
        fe = front_end(text)
        if not fe.translate(0, 5)[0]:
            continue
        listing, size = L.image_listing(fe, 128 if name == "config5" else 0)
        assert "; quiet check" in listing
        ins = L.disassemble_listing(listing)
        assert ins[-1].addr + ins[-1].size == size
        findings = L.lint_hazards(ins, assume_entry_defs={"vcc", "s62", "s63", "s64", "s65", "s66", "s67"})
        problems = L.lint_index_mode(ins, entries=L.stream_entries(ins))
        assert not findings and not problems, (name, findings[:5], problems[:5])
        linted += 1
    assert linted >= 6


# ------------------------------------------------------------------------------------------------ soundness of the plan
def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def run_records(records, rows, lead, dropped):
    """One sample of the steady records on `rows` (float32 [row, case]), as the reference computes it: fp32 multiply, fp32 add,
    saturation; INTERP in fp64 with the record's (1 - X).  Returns, per dropped record, the largest |unsaturated value|."""
    worst = {}
    dropped = set(dropped)
    one = np.float32(1.0)

    def val(word, uniform):
        return np.full(rows.shape[1], f32(word), dtype=np.float32) if uniform else rows[word]

    for i, w in enumerate(records):
        slot = int(w[0])
        if slot == ENDSAMPLE:
            break
        if i < lead or slot in (NOP, TRAM_IW, TRAM_XW):
            continue
        dst = int(w[5])
        if slot in (TRAM_IR, TRAM_XR):
            raise AssertionError("a delay-line read behind the leading ones in an eligible program")
        if slot == MOV:
            rows[dst] = val(w[2], w[6] & 1)
            continue
        assert MACS <= slot < SLOTS, slot
        rel = slot - MACS
        family, kind = rel // 16, (rel % 16) // 2
        uA, uX, uY = bool(kind & 1), bool(kind & 2), bool(kind & 4)
        if kind == 7:
            rows[dst] = val(w[2], True)
            continue
        if family <= 1:
            p = val(w[3], True) if (uX and uY) else val(w[3], uX) * val(w[4], uY)
            u = val(w[2], uA) + p if family == 0 else val(w[2], uA) - p
        elif family == 2:
            s = val(w[2], True) if (uA and uX) else val(w[2], uA) + val(w[3], uX)
            u = s + val(w[4], uY)
        else:
            a = val(w[2], uA).astype(np.float64)
            if uX:
                omx = np.array([int(w[6]) | (int(w[7]) << 32)], dtype=np.uint64).view(np.float64)[0]
                p = val(w[3], True) if uY else val(w[3], True) * val(w[4], False)
            else:
                x = val(w[3], False)
                omx = 1.0 - x.astype(np.float64)
                p = x * val(w[4], uY)
            u = (omx * a + p.astype(np.float64)).astype(np.float32)
        assert u.dtype == np.float32
        if i in dropped:
            worst[i] = float(np.max(np.abs(u)))
        rows[dst] = np.minimum(np.maximum(u, -one), one)
        if rel & 1:
            rows[0] = 0   # (the CCR row: wild, never read by an eligible program's arithmetic)
    return worst


def head_states(plan, n_rows, wild, cases, kind, rng):
    """[row, case]: the checked rows at +-bound (kind 0), at the bound exactly (1), at random values inside it (2); every other
    row of the bounded class at +-1, wild rows at finite values well outside"""
    sign = lambda shape: rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=shape)   # noqa: E731
    rows = sign((n_rows, cases))
    for r in range(n_rows):
        if wild[r]:
            rows[r] *= np.float32(8.0)
    for r, _, b in plan["checked"]:
        b = np.float32(b)
        if kind == 0:
            rows[r] = sign(cases) * b
        elif kind == 1:
            rows[r] = b
        else:
            rows[r] = rng.uniform(-1.0, 1.0, size=cases).astype(np.float32) * b
    return rows


def soundness(name, text, cases):
    fe = front_end(text)
    plan = fe.quiet_plan(0)
    if not plan["eligible"]:
        return None
    records = plan["records"]
    fe.lower()
    n_rows = int(max(int(w[5]) for w in records) + 1)
    n_rows = max(n_rows, 1 + max(r for r, _, _ in plan["checked"])) if plan["checked"] else n_rows
    # wild rows: the CCR, and whatever the plan checks at 1 (the PCM input)
    wild = np.zeros(n_rows, dtype=bool)
    wild[0] = True
    for r, _, b in plan["checked"]:
        wild[r] = b == 1.0
    lead = 0
    while int(records[lead][0]) in (TRAM_IR, TRAM_XR):
        lead += 1
    rng = np.random.default_rng(99)
    seen = set()
    for kind in (0, 1, 2):
        worst = run_records(records, head_states(plan, n_rows, wild, cases, kind, rng), lead, plan["dropped"])
        assert set(worst) == set(plan["dropped"]), (name, "every dropped record is reached")
        over = {i: v for i, v in worst.items() if not v <= 1.0}
        assert not over, (name, kind, sorted(over.items())[:5])
        seen |= set(worst)
    return len(seen)


def test_plan_is_sound_for_config5():
    assert soundness("config5", P.CONFIGS["config5"](), 2000) == 395


def test_plan_is_sound_for_generated_programs():
    checked = dropped = 0
    for name, text in GENERATED:
        n = soundness(name, text, 200)
        assert n is not None, (name, "generated programs are eligible")
        checked += 1
        dropped += n
    assert checked == 12 and dropped > 200, (checked, dropped)


def test_the_model_would_catch_an_unsound_plan():
    """the restatement is no rubber stamp: with a checked row ABOVE its bound a dropped saturation does fire in it"""
    fe = front_end(P.CONFIGS["config5"]())
    plan = fe.quiet_plan(0)
    records = plan["records"]
    n_rows = int(max(int(w[5]) for w in records) + 1)
    rows = np.full((n_rows, 4), np.float32(1.0))
    worst = run_records(records, rows, 4, plan["dropped"])
    assert max(worst.values()) > 1.0
