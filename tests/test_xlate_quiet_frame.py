"""The frame of the quiet loop (fxp_translate stream 5), without a GPU: the adds of a uniform +0 that the loop
does not emit because their other side cannot be -0 (fx_xlate.cpp zeroAddsOf, `zero_adds_dropped` of the quiet plan).

Checked here: the encoder against llvm-mc and the hazard lint; config5's counts - 24 adds fewer than the pinned fast stream, the
rest of the loop as it was; each rule of the "cannot be -0" pass in float32 numpy; and the pass itself against the float32 model of
test_xlate_quiet.py, stepped one record at a time so that the value in front of every such add can be looked at: over head states
full of +0, -0 and denormals it never has the bit pattern 0x80000000 where the add is dropped - and does where an add is kept."""
import os
import re
import sys

import numpy as np

import fx8010_programs as P

from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT
from test_xlate import assemble, needs_llvm
from test_xlate_quiet import ENDSAMPLE, MACS, SLOTS, TRAM_IR, TRAM_XR, f32, front_end, head_states, run_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ALL_PROGRAMS = [("config5", P.CONFIGS["config5"]())] + GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]
MINUS_ZERO = 0x80000000
# a program whose ACC3 adds +0 to a sum that CAN be -0: both addends are the PCM input, straight from memory
KEPT_ADD = ("kept_add", "input in 0\noutput out 0\nstatic c\nacc3 c, in, in, 0\nmacs out, 0, c, 0.5\nend")


def ops_of(listing):
    return [l for l in listing.split("\n") if l and not l.startswith(";")]


def loop_body(listing):
    """the instructions of the loop body: up to and including the branch back to its head (the first backward branch)"""
    lines = ops_of(listing)
    for k, l in enumerate(lines):
        m = re.match(r"s_cbranch_scc[01] (\d+)$", l)
        if m and int(m.group(1)) >= 0x8000:
            return lines[:k + 1]
    raise AssertionError("no backward branch")


def zero_adds(lines):
    """v_add_f32 with a literal 0 as a source"""
    return sum(bool(re.match(r"v_add_f32_e32 v\d+, 0, v\d+$", l)) for l in lines)


def plan_drops(fe):
    return len(fe.quiet_plan(0)["zero_adds_dropped"]) > 0


# ------------------------------------------------------------------------------------------------ encoder, lint
@needs_llvm
def test_quiet_streams_reassemble_and_lint_clean():
    import gfx950_lint as L
    have_objdump = os.path.exists(os.path.join(L.LLVM, "llvm-objdump"))
    loops = linted = 0
    for name, text in ALL_PROGRAMS:
        fe = front_end(text)
        for vgprs in ((0, 128) if name == "config5" else (0,)):
            code, listing = fe.translate(vgprs, 5)
            if not code:
                continue
            loops += 1
            assert assemble(listing) == code, "%s: encoder and assembler disagree" % name
            if name != "config5" and not plan_drops(fe):
                continue
            linted += 1
            if have_objdump:
                text_all, size = L.image_listing(fe, vgprs)
                ins = L.disassemble_listing(text_all)
                assert ins[-1].addr + ins[-1].size == size
                findings = L.lint_hazards(ins, assume_entry_defs={"vcc", "s62", "s63", "s64", "s65", "s66", "s67"})
                problems = L.lint_index_mode(ins, entries=L.stream_entries(ins))
                assert not findings and not problems, (name, findings[:5], problems[:5])
    assert loops == 22 and linted >= 10, (loops, linted)


# ------------------------------------------------------------------------------------------------ config5
def config5_streams(vgprs=128):
    fe = front_end(P.CONFIGS["config5"]())
    return fe, fe.translate(vgprs, 5)[1], fe.translate(vgprs, 0)[1]


def test_config5_drops_24_adds_of_zero_all_on_the_m_chain():
    fe, quiet, fast = config5_streams()
    assert zero_adds(ops_of(fast)) - zero_adds(ops_of(quiet)) == 24
    plan = fe.quiet_plan(128)
    z = plan["zero_adds_dropped"]
    assert len(z) == 24 and z == sorted(set(z))
    records = plan["records"]
    acc3 = [i for i, w in enumerate(records) if MACS + 32 <= int(w[0]) < MACS + 48]
    m_row = int(records[acc3[0]][5])            # acc3 m, lp0, lp1, lp2
    last = [w for w in records if MACS <= int(w[0]) < SLOTS][-1]
    assert int(last[3]) == m_row                # macs out, 0, m, 0.5
    for i in z:
        assert i in acc3 and int(records[i][5]) == m_row and int(records[i][2]) == m_row, i
    # the plan proper is what it was
    assert (plan["sites"], plan["fast_dropped"], plan["quiet_dropped"]) == (503, 202, 395) and plan["check_instructions"] <= 31
    assert sum(l.startswith("v_med3_f32") for l in ops_of(quiet)) == 108
    assert fe.quiet_plan(0)["zero_adds_dropped"] == z


def test_config5_differs_from_the_fast_stream_in_nothing_else():
    """the loop body of stream 5 against stream 0's: the same scalar and memory instructions, line for line (the delay-line
    taps, the loop control), once the vector instructions and what the quiet loop adds at its head are set aside"""
    _, quiet, fast = config5_streams()
    frame = lambda lines: [l for l in lines if l.startswith(("global_", "s_add", "s_lshl", "s_cselect", "s_min", "s_cmp_lt_i32", "s_cmp_ge_i32"))]   # noqa: E731
    assert frame(loop_body(quiet)) == frame(loop_body(fast))


# ------------------------------------------------------------------------------------------------ the rules
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rule_values():
    rng = np.random.default_rng(7)
    tiny = f32(1)
    special = np.array([0.0, -0.0, tiny, -tiny, 1.0, -1.0, f32(0x00800000), -f32(0x00800000)], dtype=np.float32)
    rnd = np.concatenate([rng.uniform(-1.0, 1.0, 200), rng.uniform(-1.0, 1.0, 100) * 1e-38, rng.uniform(-1.0, 1.0, 100) * 1e-44]).astype(np.float32)
    return np.concatenate([special, rnd, -rnd])


def test_rule_a_sum_with_one_clean_addend_is_clean():
    v = rule_values()
    clean = v[bits(v) != MINUS_ZERO]
    a, b = np.meshgrid(clean, v, indexing="ij")
    assert not np.any(bits(a + b) == MINUS_ZERO) and not np.any(bits(b + a) == MINUS_ZERO)
    assert not np.any(bits(a - b) == MINUS_ZERO)      # MACSN: A - p with a clean A
    mz = np.float32(-0.0)
    assert bits(mz + mz)[()] == MINUS_ZERO and bits(mz - np.float32(0.0))[()] == MINUS_ZERO   # ... and only then
    assert bits(np.float32(0.0) + mz)[()] == 0                                               # the uniform +0 is clean


def test_rule_the_saturation_keeps_clean_clean():
    v = rule_values() * np.float32(3.0)
    clean = v[bits(v) != MINUS_ZERO]
    sat = np.minimum(np.maximum(clean, np.float32(-1.0)), np.float32(1.0))
    assert not np.any(bits(sat) == MINUS_ZERO)
    assert bits(np.minimum(np.maximum(np.float32(-0.0), np.float32(-1.0)), np.float32(1.0)))[()] == MINUS_ZERO   # an unclean value stays unclean


def test_rule_products_interp_results_and_picks_are_not_clean():
    tiny = f32(1)
    assert bits(np.float32(0.0) * np.float32(-1.0))[()] == MINUS_ZERO
    assert bits(tiny * np.float32(-0.25))[()] == MINUS_ZERO                       # an underflow keeps the sign
    blend = (np.float64(0.7) * np.float64(np.float32(-0.0)) + np.float64(np.float32(-0.0))).astype(np.float32)
    assert bits(blend)[()] == MINUS_ZERO
    a, x, y = np.float32(0.5), np.float32(-0.0), np.float32(0.25)
    assert bits(np.where(a >= y, x, y).astype(np.float32))[()] == MINUS_ZERO      # LIMIT hands X on


def test_rule_zero_plus_scaled_as_one_fma_is_the_sum_it_replaces():
    """fma(X, c, +0) for |c| > 0.5: the bits of (X * c) + (+0), never -0 (the double product of two floats is exact: one rounding)"""
    v = rule_values()
    for c in (0.7, -0.7, 0.999, -0.6, 0.50000006, 4.0):
        c32 = np.float32(c)
        fma = (v.astype(np.float64) * np.float64(c32) + 0.0).astype(np.float32)
        two = v * c32 + np.float32(0.0)
        assert np.array_equal(bits(fma), bits(two)), c
        assert not np.any(bits(fma) == MINUS_ZERO), c


# ------------------------------------------------------------------------------------------------ the pass against the model
def candidates(records):
    """records with an add of the uniform +0 the pass may drop: {index: callable(rows) -> the value in front of that add}"""
    out = {}
    for i, w in enumerate(records):
        slot = int(w[0])
        if slot == ENDSAMPLE:
            break
        if not MACS <= slot < SLOTS:
            continue
        rel = slot - MACS
        family, kind = rel // 16, (rel % 16) // 2
        uA, uX, uY = bool(kind & 1), bool(kind & 2), bool(kind & 4)
        val = lambda word, uniform, rows: np.full(rows.shape[1], f32(word), dtype=np.float32) if uniform else rows[word]   # noqa: E731
        if family == 2 and kind != 7 and uY and int(w[4]) == 0 and not (uA and uX):
            out[i] = lambda rows, w=w, uA=uA, uX=uX: val(int(w[2]), uA, rows) + val(int(w[3]), uX, rows)
        elif family == 0 and uA and int(w[2]) == 0 and uX != uY and int(w[3] if uX else w[4]) == 0x3f800000:
            out[i] = lambda rows, w=w, uX=uX: rows[int(w[4] if uX else w[3])].copy()
    return out


def zero_states(plan, n_rows, wild, cases, rng):
    """head states [row, case]: every row (the PCM input and the delay-line reads' rows among them) draws from +0, -0, +- the
    smallest denormal and a random value inside the plan's bounds"""
    rows = head_states(plan, n_rows, wild, cases, 2, rng)
    inside = rng.uniform(-1.0, 1.0, size=rows.shape).astype(np.float32)
    for r in range(n_rows):
        if not wild[r] and r not in [c for c, _, _ in plan["checked"]]:
            rows[r] = inside[r]                                   # (bounded class, unchecked: inside [-1, 1])
    tiny = f32(1)
    pick = rng.integers(0, 8, size=rows.shape)
    for k, v in enumerate((np.float32(0.0), np.float32(-0.0), tiny, -tiny)):
        rows[pick == k] = v
    return rows


def stepped(records, rows, lead, probes):
    """one sample of the model of test_xlate_quiet.py (run_records), one record at a time; in front of every record of `probes`
    its callable looks at the rows.  Returns {record: value in front of its +0 add}; rows end as run_records leaves them."""
    seen = {}
    for i, w in enumerate(records):
        if int(w[0]) == ENDSAMPLE:
            break
        if i < lead:
            continue
        if i in probes:
            seen[i] = probes[i](rows)
        run_records(records[i:i + 1], rows, 0, ())
    return seen


def frame_soundness(name, text, cases=400):
    fe = front_end(text)
    plan = fe.quiet_plan(0)
    assert plan["eligible"], name
    records = plan["records"]
    n_rows = 1 + max(int(w[5]) for w in records)
    n_rows = max([n_rows] + [r + 1 for r, _, _ in plan["checked"]])
    wild = np.zeros(n_rows, dtype=bool)
    wild[0] = True
    for r, _, b in plan["checked"]:
        wild[r] = b == 1.0
    lead = 0
    while int(records[lead][0]) in (TRAM_IR, TRAM_XR):
        lead += 1
    cand = candidates(records)
    dropped = plan["zero_adds_dropped"]
    assert set(dropped) <= set(cand), (name, "only adds of a uniform +0 are dropped")
    rng = np.random.default_rng(31)
    rows = zero_states(plan, n_rows, wild, cases, rng)
    whole = rows.copy()
    seen = stepped(records, rows, lead, cand)
    run_records(records, whole, lead, ())
    assert np.array_equal(bits(rows), bits(whole)), (name, "stepping the model changes nothing")
    hit = {i: bool(np.any(bits(v) == MINUS_ZERO)) for i, v in seen.items()}
    for i in dropped:
        assert i in hit and not hit[i], (name, i, "the value in front of a dropped add is -0")
    kept = [i for i in hit if i not in dropped]
    return len(dropped), [i for i in kept if hit[i]], kept


def test_dropped_adds_never_see_minus_zero_config5():
    dropped, kept_hit, kept = frame_soundness("config5", P.CONFIGS["config5"](), 1000)
    assert dropped == 24 and not kept


def test_dropped_adds_never_see_minus_zero_generated_programs():
    total = with_kept = 0
    for name, text in GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT, KEPT_ADD]:
        dropped, kept_hit, kept = frame_soundness(name, text)
        print(name, "adds of +0 dropped %d, kept %d (of which -0 seen in front: %d)" % (dropped, len(kept), len(kept_hit)))
        total += dropped
        with_kept += bool(kept_hit)
    assert total >= 10, total
    assert with_kept >= 1


def test_an_add_whose_sum_can_be_minus_zero_is_kept():
    """acc3 c, in, in, 0: (-0) + (-0) is -0 and the add of +0 makes it +0 - not in the list, and the model does see -0 in front of it"""
    name, text = KEPT_ADD
    fe = front_end(text)
    plan = fe.quiet_plan(0)
    assert plan["eligible"] and plan["zero_adds_dropped"] == []
    dropped, kept_hit, kept = frame_soundness(name, text)
    assert dropped == 0 and len(kept) == 1 and kept_hit == kept
    # ... and once one addend is clean - c = 0 + in * 0.5 in front - the same add goes
    clean = text.replace("acc3 c, in, in, 0", "macs c, 0, in, 0.5\nacc3 c, c, in, 0")
    assert len(front_end(clean).quiet_plan(0)["zero_adds_dropped"]) == 1
    assert frame_soundness("kept_add_clean", clean)[0] == 1
