"""Sum groups of the quiet loop (fx_xlate.hpp SumGroup; fxp_translate stream 6), without a GPU.

Stream 6 is the quiet loop (stream 5) with the saturations of an accumulator chain tested once per group of links and re-done, in
a stub behind the loop, only where a lane's watched partial sum is above the chain's threshold T.  Checked here: stream 5 is byte
for byte what it was before groups existed; the encoder against llvm-mc and the hazard lint over the image laid out with stream 6;
config5's plan and counts; the emitted body of stream 6, stubs included, executed on the CPU (valu_model_sums.py) against the
float32 model of the records from calm states, from the bound-tight states of test_xlate_quiet.py's search and from states that
drive a chain above T and above 1 - and that the execution does catch a test with one watched register deleted; the coverage rule
restated in float32 numpy, with its tightness; the directed programs of sum_group_programs.py."""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import fx8010_programs as P

from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT
from sum_group_programs import DIRECTED
from test_xlate import assemble, needs_llvm
from test_xlate_emitted import pool_words, sample_body
from test_xlate_quiet import MACS, front_end, model, run_records, searched
from test_xlate_quiet_frame import bits, frame_setup, reg_file_base, zero_states
from valu_model_sums import REPAIR, TEST, ValuSums, stubs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CONFIG5 = P.CONFIGS["config5"]()
QUIET_CORPUS = [("config5", CONFIG5)] + GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]
GROUPED = [("config5", CONFIG5)] + DIRECTED    # programs whose plan is looked at in the 128-register build (spare VGPRs for groups)
TEXTS = dict(QUIET_CORPUS + DIRECTED)
ONE = np.float32(1.0)


def ops_of(listing):
    return [l.split()[0] for l in listing.split("\n") if l and not l.startswith(";")]


def body_and_stubs(listing):
    """(mnemonics of the loop body - up to the first backward branch -, mnemonics of the repair stubs)"""
    lines = [l for l in listing.split("\n") if l]
    end = next(k for k, l in enumerate(lines) if re.match(r"s_cbranch_scc[01] (\d+)$", l) and int(l.split()[1]) >= 0x8000)
    return [l.split()[0] for l in lines[:end + 1] if not l.startswith(";")], [l.split()[0] for s in stubs_of(listing) for l in s]


# ------------------------------------------------------------------------------------------------ stream 5 is what it was
def test_stream_5_reproduces_its_pinned_hashes():
    """sha256 of stream 5 of config5 (both builds) and of every corpus program with a loop, recorded from the build before sum groups"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "xlate_quiet_stream_hashes.json")))["streams"]
    seen = 0
    for name, text in QUIET_CORPUS:
        fe = front_end(text)
        for vgprs in ((0, 128) if name == "config5" else (0,)):
            code = fe.translate(vgprs, 5)[0]
            key = "%s/v%d" % (name, vgprs)
            assert bool(code) == (key in gold), key
            if code:
                assert hashlib.sha256(code).hexdigest() == gold[key], key
                seen += 1
    assert seen == len(gold) == 22
    # ... and in the 128-register build, where config5's image carries stream 6, stream 5 still reads the same
    assert front_end(CONFIG5).translate(128, 6)[0]


# ------------------------------------------------------------------------------------------------ encoder, lint
@needs_llvm
def test_stream_6_reassembles_and_the_image_lints_clean():
    import gfx950_lint as L
    have_objdump = os.path.exists(os.path.join(L.LLVM, "llvm-objdump"))
    loops = 0
    for name, text in GROUPED + GENERATED[:4]:
        fe = front_end(text)
        code, listing = fe.translate(128, 6)
        plan = fe.quiet_plan(128)
        assert bool(code) == bool(plan["sum_groups"]), name
        if not code:
            continue
        loops += 1
        assert assemble(listing) == code, "%s: encoder and assembler disagree" % name
        assert listing.count(TEST) == listing.count(REPAIR) == len(plan["sum_groups"]), name
        if have_objdump:
            text_all, size = L.image_listing(fe, 128, quiet_stream=6)
            ins = L.disassemble_listing(text_all)
            assert ins[-1].addr + ins[-1].size == size
            findings = L.lint_hazards(ins, assume_entry_defs={"vcc", "s62", "s63", "s64", "s65", "s66", "s67"})
            problems = L.lint_index_mode(ins, entries=L.stream_entries(ins))
            assert not findings and not problems, (name, findings[:5], problems[:5])
    assert loops >= 7, loops


# ------------------------------------------------------------------------------------------------ config5's plan
def test_config5_plan_groups_the_whole_m_chain():
    fe = front_end(CONFIG5)
    plan = fe.quiet_plan(128)
    records = plan["records"]
    assert (plan["sites"], plan["fast_dropped"], plan["quiet_dropped"], len(plan["zero_adds_dropped"])) == (503, 202, 395, 24)
    groups = plan["sum_groups"]
    last = [w for w in records if MACS <= int(w[0]) < MACS + 64][-1]
    m_row = int(last[3])                                    # macs out, 0, m, 0.5
    assert groups and all(g["row"] == m_row for g in groups)
    links = [i for g in groups for i in g["links"]]
    assert links == sorted(set(links)) and len(links) == plan["sum_links"]
    # every kept saturation on m whose A operand is m is a link of a group
    kept = [i for i, w in enumerate(records) if MACS <= int(w[0]) < MACS + 48 and int(w[5]) == m_row and int(w[2]) == m_row and
            ((int(w[0]) - MACS) % 16) // 2 in (0, 2, 4, 6) and i not in plan["dropped"]]
    kept = [i for i in kept if not ((int(records[i][0]) - MACS) % 16 // 2) & 1]      # (A is a row)
    assert set(kept) == set(links) and len(links) >= 90, (len(kept), len(links))
    assert groups[0]["first"] and groups[-1]["last"] and sum(g["first"] for g in groups) == sum(g["last"] for g in groups) == 1
    assert all(2 <= len(g["links"]) <= 12 and g["watched"][-1] for g in groups)
    assert all(0.5 < g["threshold"] <= 1.0 and g["threshold"] == groups[0]["threshold"] for g in groups)
    # counts of the listing: the loop body keeps every other v_med3_f32, the stubs hold the links'; one compare per group
    listing5, listing6 = fe.translate(128, 5)[1], fe.translate(128, 6)[1]
    assert ops_of(listing5).count("v_med3_f32") == 108
    body, stubs = body_and_stubs(listing6)
    assert body.count("v_med3_f32") == 108 - len(links) and stubs.count("v_med3_f32") == len(links)
    head_compares = body_and_stubs(listing5)[0].count("v_cmp_lt_f32_e32")
    assert body.count("v_cmp_lt_f32_e32") - head_compares == len(groups)
    # the smallest build has no spare registers: no groups, an empty stream 6, the same plan otherwise
    small = fe.quiet_plan(0)
    assert not small["sum_groups"] and fe.translate(0, 6)[0] == b"" and small["dropped"] == plan["dropped"]


# ------------------------------------------------------------------------------------------------ executing the emitted code
def run_stream_6(name, rows, wave=None, valid=None, mutate=None):
    """one sample of stream 6's body (stubs included) from head state `rows` -> (differing (row, case), evaluator)"""
    fe, plan, records, n_rows, wild, lead = frame_setup(name, TEXTS[name])
    listing = fe.translate(128, 6)[1]
    assert listing, name
    body = sample_body(listing)
    if mutate:
        body = mutate(body)
    base = reg_file_base()
    m = ValuSums(rows.shape[1], stubs_of(listing), wave=wave, valid=valid)
    for r in range(n_rows):
        m.v[base + r] = bits(rows[r]).copy()
    m.run(pool_words(listing))
    m.executed.clear()
    m.run(body)
    want = rows.copy()
    run_records(records, want, lead, ())
    left_out = {v - base for v in m.loaded if v >= base}
    diff = [(r, int(c)) for r in range(1, n_rows) if r not in left_out for c in np.nonzero(m.v[base + r] != bits(want[r]))[0]]
    return diff, m


# (one_link has no stream 6; ccr_addend computes a CCR - compares and selects the evaluator and the record model do not have - and
# runs on the device against the oracle instead: tests/test_gpu_sum_groups.py)
EXECUTED = [n for n, _ in GROUPED if n not in ("one_link", "ccr_addend")]


def calm_rows(name, cases, seed=3):
    fe, plan, records, n_rows, wild, lead = frame_setup(name, TEXTS[name])
    rows = zero_states(plan, n_rows, wild, cases, np.random.default_rng(seed))
    return (rows * np.float32(0.125)).astype(np.float32)


def tight_rows(name):
    """the end states of the search of test_xlate_quiet.py (they reach 1.0 at kept saturations) and their negations"""
    m = model(name, TEXTS[name])
    _, state, _ = searched(name, TEXTS[name])
    flat = state.reshape(m.n_rows, -1)
    return np.concatenate([flat, -flat], axis=1).astype(np.float32)


def link_values(name, rows):
    """|unsaturated value| at every link of every group, [link, case], from the record model"""
    fe, plan, records, n_rows, wild, lead = frame_setup(name, TEXTS[name])
    groups = fe.quiet_plan(128)["sum_groups"]
    values = {}
    run_records(records, rows.copy(), lead, (), values)
    return groups, {i: np.abs(values[i]) for g in groups for i in g["links"]}


@pytest.mark.parametrize("name", EXECUTED)
def test_calm_states_take_no_branch_and_equal_the_model(name):
    rows = calm_rows(name, 96)
    groups, values = link_values(name, rows)
    T = groups[0]["threshold"]
    assert max(float(v.max()) for v in values.values()) < T, "calm states stay below T"
    diff, m = run_stream_6(name, rows)
    assert not diff, (name, diff[:6])
    assert m.tests == len(groups) and not any(f.any() for f in m.fired) and m.repairs.sum() == 0
    assert not any(op.startswith("stub:") for op in m.executed)


@pytest.mark.parametrize("name", EXECUTED)
def test_states_above_the_threshold_run_the_stub_and_equal_the_model(name):
    """tight states, all lanes one wavefront and one lane per wavefront: some lane is above T but not above 1 at a watched sum, some
    lane above 1; every row equals the record model word for word either way"""
    rows = tight_rows(name)
    groups, values = link_values(name, rows)
    T = groups[0]["threshold"]
    top = np.max(np.stack(list(values.values())), axis=0)
    assert (top > 1.0).any(), "the search reaches above 1 at a link"
    for wave in (None, 1):
        diff, m = run_stream_6(name, rows, wave=wave)
        assert not diff, (name, wave, diff[:6])
        assert m.repairs.sum() > 0 and m.executed.get("stub:v_med3_f32", 0) > 0
    # one lane per wavefront: a wavefront repairs a group exactly when its lane is above T at a watched sum - or the group's
    # start is (the previous group's end after ITS repair; the chain's start where the plan watches it)
    fired = np.array(m.fired)                                            # [group, lane]
    between = [k for k, g in enumerate(groups) if any(T < values[i][c] <= 1.0 for c in range(rows.shape[1]) for i, w in zip(g["links"], g["watched"]) if w)]
    assert between or name != "config5", "config5: a watched sum between T and 1"
    for k, g in enumerate(groups):
        watched = np.max(np.stack([values[i] for i, w in zip(g["links"], g["watched"]) if w]), axis=0) > T
        assert (fired[k] | ~watched).all(), (name, k, "a lane above T at a watched sum fires")


def test_a_deleted_watched_register_is_caught():
    """config5: in the test of one group, one watched register is replaced by another operand of the same v_max3_f32.  Among the
    states of the climb - its end states and the sign vertices it starts from, scaled down by a factor per lane - there is a lane in which ONLY that register
    sends the wavefront to the stub (the group's start and the sums watched before it are inside T, the group's end is above 1 -
    and nothing watches it again: it is the next group's start): with one lane per wavefront the execution reports a mismatch there, and none
    with the listing as emitted.  (A lane between T and 1 needs no repair: deleting its watch changes no word.)"""
    m = model("config5", CONFIG5)
    rng = np.random.default_rng(21)
    quieter = m.vertices(2048, rng) * rng.uniform(0.2, 1.0, size=2048).astype(np.float32)    # (so that a chain passes 1 once, late)
    rows = np.concatenate([tight_rows("config5"), quieter], axis=1).astype(np.float32)
    groups, values = link_values("config5", rows)
    T = groups[0]["threshold"]
    pick = None
    for k, g in enumerate(groups):
        w = [i for i, on in zip(g["links"], g["watched"]) if on]
        if len(w) != 3 or k == 0 or k + 1 == len(groups):
            continue
        start_ok = values[groups[k - 1]["links"][-1]] <= T
        # (... and no later link of the chain saturates: a later saturation would heal the one that was skipped, and only the
        # chain's end is observable)
        later = np.max(np.stack([values[i] for h in groups[k + 1:] for i in h["links"]]), axis=0)
        lanes = np.nonzero(start_ok & (values[w[0]] <= T) & (values[w[1]] <= T) & (values[w[2]] > 1.0) & (later < 1.0))[0]
        if len(lanes):
            pick = (k, g, lanes)
            break
    assert pick, "no state of the climb isolates a watched sum"
    k, g, lanes = pick
    body = sample_body(front_end(CONFIG5).translate(128, 6)[1])
    at = [j + 1 for j, l in enumerate(body) if l == TEST][k]
    regs = [r for r, on in zip(g["dst_reg"], g["watched"]) if on]
    assert body[at] == "v_max3_f32 v2, |v%d|, |v%d|, |v%d|" % tuple(regs), body[at]
    mutated = "v_max3_f32 v2, |v%d|, |v%d|, |v%d|" % (regs[0], regs[1], regs[1])
    diff, _ = run_stream_6("config5", rows, wave=1)
    assert not diff
    diff, _ = run_stream_6("config5", rows, wave=1, mutate=lambda b: b[:at] + [mutated] + b[at + 1:])
    assert diff and {c for _, c in diff} & set(int(c) for c in lanes), (diff[:4], lanes[:4])


def test_lanes_without_an_instance_never_fire():
    rows = tight_rows("config5")
    valid = np.zeros(rows.shape[1], dtype=bool)
    diff, m = run_stream_6("config5", rows, valid=valid)
    assert m.repairs.sum() == 0 and not any(f.any() for f in m.fired)
    assert diff, "(and then the loud lanes are not repaired: the mask is what keeps garbage lanes from firing, not the values)"


# ------------------------------------------------------------------------------------------------ the coverage rule, restated
def restated_pass(T, groups, addends=None):
    """the coverage pass in float32 numpy: from T at the start of every group and at every watched sum, add each covered link's
    addend (default: its running bound from the plan) as the instruction adds -> the largest |covered sum| (0 without one)"""
    top = np.float32(0)
    for g in groups:
        s = np.float32(T)
        for k, w in enumerate(g["watched"]):
            if w:
                s = np.float32(T)
                continue
            b = np.float32(g["addend_bound"][k] if addends is None else addends[g["links"][k]])
            s = np.float32(s + b)
            top = max(top, np.float32(abs(s)))
    return top


def reached_addends(name, groups):
    """the largest |addend| of every link that the record model reaches from the sign vertices of the plan's head bounds"""
    from test_xlate_quiet_frame import stepped
    fe, plan, records, n_rows, wild, lead = frame_setup(name, TEXTS[name])
    rows = model(name, TEXTS[name]).vertices(512, np.random.default_rng(12))

    def probe(w):
        family, kind = (int(w[0]) - MACS) // 16, ((int(w[0]) - MACS) % 16) // 2
        val = lambda rows, word, uniform: np.full(rows.shape[1], np.array([word], dtype=np.uint32).view(np.float32)[0]) if uniform else rows[int(word)]   # noqa: E731
        if family == 2:
            return lambda rows: float(np.abs(val(rows, w[3], False)).max())
        return lambda rows: float(np.abs(val(rows, w[3], kind & 2) * val(rows, w[4], kind & 4)).max())

    return stepped(records, rows, lead, {i: probe(records[i]) for g in groups for i in g["links"]})


COVERAGE = [n for n, _ in GROUPED if n != "one_link"]


@pytest.mark.parametrize("name", COVERAGE)
def test_no_covered_sum_exceeds_one_and_the_threshold_is_tight(name):
    """per chain, with the plan's own running bounds of the addends (exported by fxp_quiet_plan; each at least what the record model
    reaches at the sign vertices of the head bounds): started at T, at the float below T and at 0, with every covered addend AT
    its bound, no covered |sum| is above 1 - nor with random and adversarial (all +bound, all -bound, alternating) addends inside
    the bounds; started at the next float above T a covered sum IS above 1, unless the chain has no covered sum at all (T = 1)"""
    fe = front_end(TEXTS[name])
    groups = fe.quiet_plan(128)["sum_groups"]
    assert groups, name
    reached = reached_addends(name, groups)
    chains, chain = [], []
    for g in groups:
        chain.append(g)
        if g["last"]:
            chains.append(chain)
            chain = []
    assert not chain
    rng = np.random.default_rng(8)
    for chain in chains:
        T = np.float32(chain[0]["threshold"])
        assert all(np.float32(g["threshold"]) == T for g in chain) and 0 <= T <= ONE
        for g in chain:
            assert all(np.isfinite(b) and reached[i] <= np.float32(b) for i, b in zip(g["links"], g["addend_bound"])), (name, g["links"][0])
        assert chain[0]["watch_start"] == (not np.float32(chain[0]["start_bound"]) <= T)
        for start in (T, np.nextafter(T, np.float32(0)), np.float32(0)):
            assert restated_pass(start, chain) <= ONE, (name, float(start))
        for trial in range(24):
            sign = {0: lambda k: 1.0, 1: lambda k: -1.0, 2: lambda k: (-1.0) ** k}.get(trial, lambda k: rng.uniform(-1, 1))
            addends = {i: np.float32(b * sign(k)) for g in chain for k, (i, b) in enumerate(zip(g["links"], g["addend_bound"]))}
            for start in (T, -T):
                assert restated_pass(start, chain, addends) <= ONE, (name, trial)
        covered = any(not w for g in chain for w in g["watched"])
        if covered:
            assert T < ONE and restated_pass(np.nextafter(T, np.float32(2)), chain) > ONE, (name, "T is not the largest float that passes")
        else:
            assert T == ONE, (name, "no covered sum: every sum is watched at T = 1")


def test_degenerate_chain_and_config5_threshold():
    """config5: three times 0.05 * 1 (u is a saturated row: bound 1) between two watched sums; a chain without a small addend
    watches every sum at T = 1"""
    plan = front_end(CONFIG5).quiet_plan(128)
    T = np.float32(plan["sum_groups"][0]["threshold"])
    b = np.float32(np.float32(0.05) * ONE)
    chain = lambda t: np.float32(np.float32(np.float32(t + b) + b) + b)   # noqa: E731
    assert chain(T) <= ONE < chain(np.nextafter(T, np.float32(2)))
    text = TEXTS["long_chain"].replace(", 0.05", ", 0.5")
    groups = front_end(text).quiet_plan(128)["sum_groups"]
    assert groups and all(all(g["watched"]) and g["threshold"] == 1.0 for g in groups)


# ------------------------------------------------------------------------------------------------ directed programs
def plan_of(name):
    fe = front_end(TEXTS[name])
    return fe, fe.quiet_plan(128)


def test_directed_plans():
    # MACSN links subtract
    _, p = plan_of("macsn_links")
    assert p["sum_groups"] and any(any(g["negate"]) and not all(g["negate"]) for g in p["sum_groups"])
    # a row addend written again before the test is copied into a spare register; one that is not is read in place
    fe, p = plan_of("rewritten_addend")
    rowlinks = [(g, k) for g in p["sum_groups"] for k in range(len(g["links"])) if g["addend_row"][k] >= 0]
    assert rowlinks and any(g["addend_reg"][k] >= 0 for g, k in rowlinks)
    assert any(g["addend_reg"][k] < 0 for g, k in rowlinks), "the last link of a group is read in place: the test follows it"
    # two chains by turns: one is grouped, the other keeps its saturations
    fe, p = plan_of("two_chains")
    assert len({g["row"] for g in p["sum_groups"]}) == 1
    body, stubs = body_and_stubs(fe.translate(128, 6)[1])
    assert body.count("v_med3_f32") == ops_of(fe.translate(128, 5)[1]).count("v_med3_f32") - p["sum_links"] > 0
    # a reader in mid-chain closes the group in front of it: two chains, each with a first and a last group, row canonical at the reader
    _, p = plan_of("reader_in_mid_chain")
    assert sum(g["first"] for g in p["sum_groups"]) == 2 == sum(g["last"] for g in p["sum_groups"])
    reader = next(i for i, w in enumerate(p["records"]) if MACS <= int(w[0]) < MACS + 16 and int(w[3]) == p["sum_groups"][0]["row"] and int(w[5]) != int(w[3]) and int(w[2]) == 0 and i > p["sum_groups"][0]["links"][0])
    assert all(not (g["links"][0] < reader < g["links"][-1]) for g in p["sum_groups"])
    # a chain of one link: no group, no stream 6
    fe, p = plan_of("one_link")
    assert p["in_force"] and not p["sum_groups"] and fe.translate(128, 6)[0] == b""
    # more links than a group holds: several groups, the value carried in two registers by turns, row R at the end
    _, p = plan_of("long_chain")
    g = p["sum_groups"]
    base = reg_file_base()
    assert len(g) >= 5 and g[0]["start_reg"] == base + g[0]["row"] and g[-1]["dst_reg"][-1] == base + g[0]["row"]
    assert all(g[k + 1]["start_reg"] == g[k]["dst_reg"][-1] for k in range(len(g) - 1))
    assert all(g[k]["dst_reg"][-1] != g[k]["start_reg"] for k in range(len(g)))
    # products of two rows are addends like any other (large: watched)
    _, p = plan_of("row_by_row")
    recs = p["records"]
    rr = [(g, k) for g in p["sum_groups"] for k, i in enumerate(g["links"]) if ((int(recs[i][0]) - MACS) % 16) // 2 == 0]
    assert rr and all(g["watched"][k] and g["addend_reg"][k] >= 0 and g["addend_row"][k] < 0 for g, k in rr)


def test_a_ccr_addend_is_no_link_and_cuts_the_chain():
    """the running bound of row 0 (the CCR) is +inf: `macs a, a, ccr, 0.05` keeps its own saturation in stream 6 and stands between
    two chains, each with a first and a last group"""
    fe, p = plan_of("ccr_addend")
    recs = p["records"]
    a_row = p["sum_groups"][0]["row"]
    ccr = [i for i, w in enumerate(recs) if MACS <= int(w[0]) < MACS + 16 and int(w[5]) == a_row and int(w[2]) == a_row and 0 in (int(w[3]), int(w[4]))
           and ((int(w[0]) - MACS) % 16) // 2 in (2, 4)]
    assert len(ccr) == 1, ccr
    i = ccr[0]
    links = [j for g in p["sum_groups"] for j in g["links"]]
    assert i not in links and i not in p["dropped"]
    assert sum(g["first"] for g in p["sum_groups"]) == 2 == sum(g["last"] for g in p["sum_groups"])
    assert max(j for j in p["sum_groups"][0]["links"]) < i < min(j for j in p["sum_groups"][-1]["links"])
    body, stubs = body_and_stubs(fe.translate(128, 6)[1])
    assert body.count("v_med3_f32") == ops_of(fe.translate(128, 5)[1]).count("v_med3_f32") - p["sum_links"] >= 1


def test_config5_with_controls_as_rows_keeps_the_m_chain():
    """damp / decay / diff as rows: far fewer saturations are idle (products of two rows), the m chain's addends are still
    literal multiples of u, so its links are grouped with the same watch pattern and T as config5's"""
    fe, p = plan_of("config5_rows")
    ref = front_end(CONFIG5).quiet_plan(128)
    assert p["in_force"] and p["quiet_dropped"] < ref["quiet_dropped"]
    assert p["sum_groups"] and len({g["row"] for g in p["sum_groups"]}) == 1
    assert p["sum_groups"][0]["threshold"] == ref["sum_groups"][0]["threshold"]
    assert p["sum_links"] >= 90      # (three rows more: a few spare registers fewer, the chain's last links may stay ungrouped)


def test_an_image_fingerprint_tells_the_two_loops_apart():
    fe = front_end(CONFIG5)
    assert fe.translate(128, 5)[0] != fe.translate(128, 6)[0]
    assert len(fe.translate(128, 6)[0]) > len(fe.translate(128, 5)[0])
