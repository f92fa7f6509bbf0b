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

from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT, ZERO_ACC3, ZERO_C, ZERO_PROGRAMS, sweep_program
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


def frame_setup(name, text):
    """(front end, plan, records, rows of the register file, wild rows, leading delay-line reads) of an eligible program"""
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
    return fe, plan, records, n_rows, wild, lead


def frame_soundness(name, text, cases=400):
    fe, plan, records, n_rows, wild, lead = frame_setup(name, text)
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


# ------------------------------------------------------------------------------------------------ the directed family
# adds of +0 the plan drops, per program: (ACC3 form (A + X) + 0, MACS form 0 + X * 1.0 under a kept saturation)
ZERO_DROPS = {"zero_pool": (1, 0), "zero_state_read": (0, 0), "zero_sum_product": (2, 0), "zero_interp_limit": (0, 0), "zero_move_const": (0, 0),
              "zero_acc3": (9, 0), "zero_minus": (0, 0), "zero_unit": (2, 2), "zero_delay": (2, 0)}
# ... and of the corpus (the programs whose loop drops one run on the device at zero-rich states: test_gpu_zero_signs.py)
CORPUS_DROPS = {"config5": 24, "gen0": 1, "gen3": 1, "gen5": 1, "gen6": 1, "gen10": 1, "wide3": 1, "gen0_limit": 1, "gen3_delay": 1, "gen2": 2, "gen4": 2,
                "gen8": 1, "gen9": 1}


def reg_file_base():
    """the VGPR of register-file row 0, from the code's own constant"""
    header = open(os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc", "fx_xlate_emit.hpp")).read()
    return int(re.search(r"constexpr int kRegFileBase = (\d+);", header).group(1))


def forms(plan):
    family = [(int(plan["records"][i][0]) - MACS) // 16 for i in plan["zero_adds_dropped"]]
    assert set(family) <= {0, 2}
    return family.count(2), family.count(0)


def acc3_of_rows(records, a, x):
    """indices of the records acc3 r, row a, row x, +0"""
    return [i for i, w in enumerate(records) if MACS + 32 <= int(w[0]) < MACS + 48 and (int(w[0]) - MACS) % 16 // 2 == 4 and
            (int(w[2]), int(w[3]), int(w[4])) == (a, x, 0)]


def test_corpus_counts_of_dropped_adds_are_all_of_the_acc3_form():
    for name, text in ALL_PROGRAMS:
        plan = front_end(text).quiet_plan(0)
        assert forms(plan) == (CORPUS_DROPS.get(name, 0), 0), name
        assert plan["in_force"] or name in ("gen8", "gen9", "wide0", "wide2", "wide7", "wide8"), name


def test_zero_programs_are_in_force_and_drop_what_is_pinned():
    assert 8 <= len(ZERO_PROGRAMS) <= 12 and sorted(ZERO_DROPS) == sorted(n for n, _ in ZERO_PROGRAMS)
    minus = 0
    for name, text in ZERO_PROGRAMS:
        fe = front_end(text)
        plan = fe.quiet_plan(0)
        assert plan["eligible"] and plan["in_force"], (name, plan["why"])
        assert forms(plan) == ZERO_DROPS[name], (name, forms(plan))
        assert fe.translate(0, 5)[0]
        # what the fast loop has and the quiet loop has not is one add of a literal 0 per dropped record, nothing else of that kind
        quiet, fast = loop_body(fe.translate(0, 5)[1]), loop_body(fe.translate(0, 0)[1])
        assert zero_adds(fast) - zero_adds(quiet) == sum(ZERO_DROPS[name]), name
        minus += any(MINUS_ZERO in (int(w[2]), int(w[3]), int(w[4])) for w in plan["records"] if MACS <= int(w[0]) < SLOTS or int(w[0]) in (4, 10, 11))
    assert minus >= 2, "the literal -0 reaches the records as the uniform 0x80000000"


def test_dropped_adds_never_see_minus_zero_zero_programs():
    with_kept = 0
    for name, text in ZERO_PROGRAMS:
        dropped, kept_hit, kept = frame_soundness(name, text)
        print(name, "adds of +0 dropped %d (ACC3 form %d, MACS form %d), kept %d (of which -0 seen in front: %d)" % ((dropped,) + ZERO_DROPS[name] + (len(kept), len(kept_hit))))
        assert dropped == sum(ZERO_DROPS[name]), name
        with_kept += bool(kept_hit)
    assert with_kept >= 6, "most programs of the family have an add that must stay, and the model sees why"


def test_zero_acc3_drops_exactly_the_adds_with_a_clean_side():
    """the directed ACC3 records of zero_acc3, a0 .. a13 in program order: dropped where A or X is a sum, a non-zero uniform, a
    folded move (in + the folded product +0: a sum) or a constant record; kept - with -0 seen in front - for (in, in), a product
    over a row that may be -0, an INTERP result, a LIMIT pick and the leading delay-line read rows beside the input or each other"""
    name, text = "zero_acc3", dict(ZERO_PROGRAMS)["zero_acc3"]
    _, plan, records, _, _, _ = frame_setup(name, text)
    cand = sorted(i for i in candidates(records) if (int(records[i][0]) - MACS) // 16 == 2)
    directed = cand[-len(ZERO_ACC3):]
    assert len(directed) == 14 and directed == list(range(directed[0], directed[0] + 14)), "a0 .. a13 are consecutive records"
    dropped, kept_hit, kept = frame_soundness(name, text, 2000)
    got = [k for k, i in enumerate(directed) if i in plan["zero_adds_dropped"]]
    assert got == [1, 2, 3, 4, 8, 11, 12, 13], got
    assert [k for k, i in enumerate(directed) if i in kept_hit] == [0, 5, 6, 7, 9, 10]
    # (in, in): both addends the input row
    in_row = [r for r, n, b in plan["checked"] if n == "in"][0]
    assert acc3_of_rows(records, in_row, in_row) == [directed[0]] and directed[0] in kept_hit


def pool_of(records):
    """the multipliers of "R = 0 + X * c", |c| > 0.5 finite and not +-1, of the MACS family: the six most frequent, first seen first"""
    count = {}
    for w in records:
        slot = int(w[0])
        if slot == ENDSAMPLE:
            break
        if not MACS <= slot < MACS + 16:
            continue
        kind = (slot - MACS) // 2
        if not kind & 1 or int(w[2]) != 0 or kind & 6 not in (2, 4):
            continue
        c = int(w[3] if kind & 6 == 2 else w[4])
        if 0x3f000000 < c & 0x7fffffff < 0x7f800000 and c & 0x7fffffff != 0x3f800000:
            count[c] = count.get(c, 0) + 1
    order = sorted(count, key=lambda c: -count[c])    # (stable: ties stay in the order of first appearance)
    return order[:6], order[6:]


LITERAL = {0x3f000000: "0.5", 0x3f800000: "1.0", 0xbf800000: "-1.0", 0x40800000: "4.0", 0x40000000: "2.0", 0xbf000000: "-0.5", 0xc0000000: "-2.0", 0xc0800000: "-4.0"}


def literal(c):
    return LITERAL.get(c, "0x%08x" % c)


def test_pooled_constants_are_fused_and_the_others_multiplied_and_added():
    """zero_pool has more than six multipliers above 0.5 in magnitude: in streams 0 and 5 alike v_fma_f32 appears for exactly the
    six that sit in s88 .. s93, the others are v_mul_f32 then v_add_f32 with a literal 0, and 0.5 and +-1.0 are never fused"""
    text = dict(ZERO_PROGRAMS)["zero_pool"]
    fe = front_end(text)
    records = fe.quiet_plan(0)["records"]
    pooled, others = pool_of(records)
    f = lambda v: int(np.float32(v).view(np.uint32))   # noqa: E731
    assert len(pooled) == 6 and others and set(pooled) | set(others) >= {f(v) for v in (0.50000006, 0.75, -0.6, 0.999, 1.5, 4.0, 0.7)}
    base = reg_file_base()
    in_reg = "v%d" % (base + 1)
    for stream in (0, 5):
        listing = fe.translate(0, stream)[1]
        sgpr = {int(m.group(1)): int(m.group(2), 16) for m in re.finditer(r"^s_mov_b32 s(8[89]|9[0-3]), (0x[0-9a-f]+)$", listing, re.M)}
        inline = {int(m.group(1)): int(np.float32(float(m.group(2))).view(np.uint32)) for m in re.finditer(r"^s_mov_b32 s(8[89]|9[0-3]), (-?\d\.\d)$", listing, re.M)}
        sgpr.update(inline)
        assert sorted(sgpr.values()) == sorted(pooled), (stream, sgpr, pooled)
        body = loop_body(listing)
        fused = set()
        for l in body:
            if l.startswith("v_fma_f32"):
                m = re.match(r"v_fma_f32 v\d+, v\d+, s(\d+), 0$", l)
                assert m, (stream, l)
                fused.add(sgpr[int(m.group(1))])
        assert fused == set(pooled), (stream, fused)
        assert not fused & {f(0.5), f(1.0), f(-1.0)}
        for c in others + [f(0.5), f(0.25), f(0.001)]:
            at = [k for k, l in enumerate(body) if re.match(r"v_mul_f32_e32 v\d+, %s, %s$" % (re.escape(literal(c)), in_reg), l)]
            assert at, (stream, literal(c), "the multiplication of the input by an unpooled constant")
            product = lambda k: re.match(r"v_mul_f32_e32 (v\d+),", body[k]).group(1)   # noqa: E731
            assert any(re.match(r"v_add_f32_e32 v\d+, 0, %s$" % product(k), body[k + 1]) for k in at), (stream, literal(c), [body[k:k + 2] for k in at])
        # +-1.0 is never multiplied: 0 + in and 0 - in on the input's own row
        assert any(re.match(r"v_add_f32_e32 v\d+, 0, %s$" % in_reg, l) for l in body) and any(re.match(r"v_sub_f32_e32 v\d+, 0, %s$" % in_reg, l) for l in body)
        assert not any(re.match(r"v_mul_f32_e32 v\d+, -?1\.0, ", l) for l in body), stream


def test_the_macs_form_is_emitted_and_its_median_reads_row_x():
    """zero_unit: `macmv w0, 4.0` makes w0 a clean row OUTSIDE [-1, 1] - the copy of a uniform above 1 is the one way to such a row,
    every sum, constant record and copy of those carries a running bound <= 1 and its 0 + X * 1.0 loses the saturation instead -
    so `macs u0, 0, w0, 1.0` keeps its saturation and the plan drops its add: family 0 in zero_adds_dropped, the quiet loop's
    v_med3_f32 reads row X itself where the fast loop adds the literal 0 into v2 first.  The same with the multiplier in X."""
    text = dict(ZERO_PROGRAMS)["zero_unit"]
    fe = front_end(text)
    plan = fe.quiet_plan(0)
    records = plan["records"]
    marked = [i for i in plan["zero_adds_dropped"] if (int(records[i][0]) - MACS) // 16 == 0]
    assert len(marked) == 2
    base = reg_file_base()
    quiet, fast = loop_body(fe.translate(0, 5)[1]), loop_body(fe.translate(0, 0)[1])
    for i in marked:
        w = records[i]
        kind = (int(w[0]) - MACS) % 16 // 2
        assert kind in (3, 5) and int(w[2]) == 0 and int(w[3] if kind == 3 else w[4]) == 0x3f800000 and i not in plan["dropped"]
        x, r = base + int(w[4] if kind == 3 else w[3]), base + int(w[5])
        assert "v_med3_f32 v%d, v%d, -1.0, 1.0" % (r, x) in quiet
        assert "v_med3_f32 v%d, v%d, -1.0, 1.0" % (r, x) not in fast
        k = fast.index("v_med3_f32 v%d, v2, -1.0, 1.0" % r)
        assert fast[k - 1] == "v_add_f32_e32 v2, 0, v%d" % x
    dropped, kept_hit, kept = frame_soundness("zero_unit", text, 2000)
    assert dropped == 4


def test_the_sweep_program_fuses_exactly_where_the_rule_says():
    """macs r, 0, in, c of the denormal sweep: one v_fma_f32 each (c in either position) in the fast stream for |c| > 0.5 but +-1.0,
    none otherwise - and never one in the exact stream"""
    for c in ZERO_C:
        fe = front_end(sweep_program(c))
        fast, exact = ops_of(fe.translate(0, 0)[1]), ops_of(fe.translate(0, 1)[1])
        fused = sum(l.startswith("v_fma_f32") for l in fast)
        assert fused == (2 if abs(float(c)) > 0.5 and abs(float(c)) != 1.0 else 0), (c, fused)
        assert not any(l.startswith("v_fma_f32") for l in exact), c
