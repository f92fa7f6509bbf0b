"""The emitted vector body of the steady fast stream (0) and of the quiet stream (5), executed on the CPU (valu_model.py) and compared
word for word with the float32 model of the records (test_xlate_quiet.run_records) - from head states full of +0, -0, the
smallest denormals and random values inside the plan's bounds (test_xlate_quiet_frame.zero_states).  test_xlate_quiet*.py model
the records, not the code: a wrong operand row in an emission path, an add dropped where the plan did not say so or a fused
multiply-add where the rule does not hold shows here without a GPU.

One sample is evaluated: from just behind the last branch of the head check to the branch back to the loop's head.  The rows a
load of that stretch overwrites (the leading delay-line reads' rows: the next sample's values arrive in the middle of this one)
are left out of the comparison - named from the plan, and the test fails when the listing loads over any other row."""
import re

import numpy as np
import pytest

import fx8010_programs as P

from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT, ZERO_PROGRAMS
from test_xlate_quiet import run_records
from test_xlate_quiet_frame import KEPT_ADD, bits, frame_setup, reg_file_base, zero_states
from valu_model import UnknownMnemonic, Valu

CORPUS = [("config5", P.CONFIGS["config5"]())] + GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]
CASES = 192
KNOWN = {"v_mul_f32_e32", "v_add_f32_e32", "v_sub_f32_e32", "v_subrev_f32_e32", "v_med3_f32", "v_fma_f32", "v_mov_b32_e32", "v_cvt_f64_f32_e32",
         "v_fma_f64", "v_mul_f64", "v_add_f64", "v_cvt_f32_f64_e32", "v_cndmask_b32_e32", "v_cmp_lt_f32_e32", "v_cmp_ge_f32_e32", "v_max3_f32"}


def sample_body(listing):
    """the lines of one sample: behind the last branch of the head check (in a quiet stream the one of the quiet check), up to the
    first backward branch"""
    lines = [l for l in listing.split("\n") if l]
    start = next((k for k, l in enumerate(lines) if l.startswith("; quiet check")), 0)
    k = next(k for k in range(start, len(lines)) if lines[k].startswith("s_cmp_lg_u64"))
    assert lines[k + 1].startswith("s_cbranch_scc1"), lines[k:k + 2]
    for e in range(k + 2, len(lines)):
        m = re.match(r"s_cbranch_scc[01] (\d+)$", lines[e])
        if m and int(m.group(1)) >= 0x8000:
            return lines[k + 2:e + 1]
    raise AssertionError("no backward branch")


def pool_words(listing):
    """SGPRs that hold a constant for the whole loop: set once, behind the loop's code"""
    return [l for l in listing.split("\n") if re.match(r"s_mov_b32 s(8[89]|9[0-3]), ", l)]


def emitted_against_model(name, text, vgprs, stream, body=None, seed=31):
    """-> (differing (row, case, emitted word, model word), rows left out, mnemonics executed)"""
    fe, plan, records, n_rows, wild, lead = frame_setup(name, text)
    listing = fe.translate(vgprs, stream)[1]
    assert listing, (name, stream)
    rows = zero_states(plan, n_rows, wild, CASES, np.random.default_rng(seed))
    base = reg_file_base()
    m = Valu(CASES)
    for r in range(n_rows):
        m.v[base + r] = bits(rows[r]).copy()
    m.run(pool_words(listing))
    m.executed.clear()
    m.run(sample_body(listing) if body is None else body)
    want = rows.copy()
    run_records(records, want, lead, ())
    # rows a load of this stretch writes: exactly the leading delay-line reads' rows (the PCM input is loaded into a staging
    # register below the register file; its rows would be the only others allowed)
    input_rows = {r for r, _, b in plan["checked"] if b == 1.0}
    read_rows = {int(w[5]) for w in records[:lead]}
    left_out = {v - base for v in m.loaded if v >= base}
    assert read_rows <= left_out <= read_rows | input_rows and len(left_out) <= 4, (name, stream, sorted(left_out), sorted(read_rows), sorted(input_rows))
    diff = []
    for r in range(1, n_rows):        # (row 0 is the CCR: no eligible program reads it, the model writes a placeholder)
        if r in left_out:
            continue
        got, ref = m.v[base + r], bits(want[r])
        for c in np.nonzero(got != ref)[0]:
            diff.append((r, int(c), int(got[c]), int(ref[c])))
    return diff, left_out, m.executed


def in_force(programs):
    out = []
    for name, text in programs:
        if frame_setup(name, text)[1]["in_force"]:
            out.append(name)
    return out


CORPUS_IN_FORCE = in_force(CORPUS)
ZERO_NAMES = [n for n, _ in ZERO_PROGRAMS]
TEXTS = dict(CORPUS + ZERO_PROGRAMS)
SEEN = {}


@pytest.mark.parametrize("stream", [0, 5], ids=["fast", "quiet"])
@pytest.mark.parametrize("name", CORPUS_IN_FORCE + ZERO_NAMES)
def test_emitted_body_computes_the_records(name, stream):
    for vgprs in ((0, 128) if name == "config5" else (0,)):
        diff, left_out, executed = emitted_against_model(name, TEXTS[name], vgprs, stream)
        assert not diff, (name, vgprs, stream, ["row %d case %d: emitted %08x model %08x" % d for d in diff[:8]])
        assert set(executed) <= KNOWN
        for op, n in executed.items():
            SEEN[op] = SEEN.get(op, 0) + n


def test_every_in_force_program_is_covered_and_the_mnemonics_are_the_listed_ones():
    assert len(CORPUS_IN_FORCE) == 21 and len(ZERO_NAMES) >= 8
    if len(SEEN):   # (filled by the cases above when the module runs as a whole)
        assert {"v_mul_f32_e32", "v_add_f32_e32", "v_sub_f32_e32", "v_med3_f32", "v_fma_f32", "v_mov_b32_e32", "v_cvt_f64_f32_e32", "v_fma_f64",
                "v_cvt_f32_f64_e32", "v_cndmask_b32_e32"} <= set(SEEN), sorted(SEEN)


def test_an_unknown_vector_mnemonic_is_refused_by_name():
    m = Valu(4)
    m.v[33] = np.zeros(4, dtype=np.uint32)
    with pytest.raises(UnknownMnemonic, match="v_rcp_f32_e32"):
        m.step("v_rcp_f32_e32 v2, v33")
    with pytest.raises(UnknownMnemonic, match="image_load"):
        m.step("image_load v2, v33")
    with pytest.raises(KeyError):
        m.step("v_add_f32_e32 v2, 0, v40")      # a register nothing has written
    m.step("s_waitcnt vmcnt(0)")
    m.step("global_load_dword v44, v1, s[86:87]")
    assert m.loaded == [44] and not m.executed


def test_the_evaluator_rounds_once():
    """fma(x, c, 0) against mul-then-add where they differ (a product that underflows to half a denormal), fp64 fma against two
    roundings, signs of an exact zero"""
    from valu_model import F32, F64, fma_exact
    tiny = float(np.float32(1e-45))
    assert fma_exact(tiny, 0.5, 0.0, *F32) == 0.0 and fma_exact(tiny, 0.50000006, 0.0, *F32) == tiny
    assert fma_exact(3 * tiny, 0.5, 0.0, *F32) == 2 * tiny        # 1.5 ulp: to even
    assert np.copysign(1.0, fma_exact(-0.0, 0.75, 0.0, *F32)) == 1.0 and np.copysign(1.0, fma_exact(-0.0, 0.75, -0.0, *F32)) == -1.0
    assert np.copysign(1.0, fma_exact(1.0, 1.0, -1.0, *F64)) == 1.0
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -(1.0 + 2.0 ** -29)
    assert fma_exact(a, b, c, *F64) == 2.0 ** -60 and a * b + c == 0.0
    m = Valu(2)
    m.v[33] = np.array([1, 0x80000001], dtype=np.uint32)
    m.s[88] = int(np.float32(0.75).view(np.uint32))
    m.step("v_fma_f32 v2, v33, s88, 0")
    assert m.v[2].tolist() == [1, 0x80000001]
    m.step("v_mul_f32_e32 v3, 0.5, v33")
    m.step("v_add_f32_e32 v2, 0, v3")
    assert m.v[3].tolist() == [0, 0x80000000] and m.v[2].tolist() == [0, 0]
    m.step("v_med3_f32 v4, -|v33|, -1.0, 1.0")
    assert m.v[4].tolist() == [0x80000001, 0x80000001]


def test_the_evaluator_fails_on_a_listing_without_a_kept_add():
    """kept_add (acc3 c, in, in, 0): its add of +0 must stay.  With the listing as emitted every word agrees; with that one
    v_add_f32 ..., 0, ... deleted by this test the evaluator reports words that differ, all of them 0x80000000 against 0x00000000"""
    name, text = KEPT_ADD
    diff, _, _ = emitted_against_model(name, text, 0, 0)
    assert not diff
    fe = frame_setup(name, text)[0]
    body = sample_body(fe.translate(0, 0)[1])
    adds = [k for k, l in enumerate(body) if re.match(r"v_add_f32_e32 (v\d+), 0, \1$", l)]
    assert len(adds) == 1, [body[k] for k in adds]
    assert re.match(r"v_add_f32_e32 v2, v(\d+), v\1$", body[adds[0] - 1]), "in + in in front of it"
    diff, _, _ = emitted_against_model(name, text, 0, 0, body=body[:adds[0]] + body[adds[0] + 1:])
    assert diff and all((got, ref) == (0x80000000, 0) for _, _, got, ref in diff), diff[:4]
    assert len({r for r, _, _, _ in diff}) == 1
