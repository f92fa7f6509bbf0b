"""The quiet loop of the translator (fx_xlate.hpp QuietPlan; fxp_translate stream 5), without a GPU.

A quiet loop is the steady fast stream without the saturations that cannot fire while the rows its head checks stay inside their
bounds.  Checked here: the encoder against llvm-mc, that the five other streams are what they were before the loop existed,
which programs get a loop, the hazard lint - and the plan's soundness against an independent restatement: a float32 numpy model
of the steady records is fed head states at and inside the plan's bounds, and at every record whose saturation the plan drops
the unsaturated value must lie in [-1, 1]."""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import fx8010_amd as A
import fx8010_programs as P

from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT
from test_xlate import assemble, needs_llvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BENCH = ("config1_shipped", "config2", "config3", "config4", "config5")
# handler slots of the records (fx_asm.hpp AsmSlot)
ENDSAMPLE, NOP, MOV, LIMIT, LIMITN, TRAM_IR, TRAM_IW, TRAM_XR, TRAM_XW, MACS, SLOTS = 0, 1, 4, 10, 11, 14, 15, 16, 17, 20, 84


def front_end(text):
    fe = A.FrontEnd(max(1, len(re.findall(r"^input ", text, re.M))))
    assert fe.load_text(text), fe.errors()
    return fe


# ------------------------------------------------------------------------------------------------ encoder, layout
@needs_llvm
def test_quiet_stream_reassembles_to_the_same_bytes():
    loops = 0
    for name, text in [("config5", P.CONFIGS["config5"]())] + GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]:
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
    assert loops == 22, loops   # config5 twice, 10 of the 12 generated programs, 8 of the 12 wide ones, the two edits


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
    for name, text in [("config5", P.CONFIGS["config5"]())] + GENERATED + GENERATED_WIDE[:4]:
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
    assert linted == 13, linted   # config5, 10 generated programs, wide1 and wide3


# ------------------------------------------------------------------------------------------------ soundness of the plan
def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def run_records(records, rows, lead, dropped, values=None, limits=True):
    """One sample of the steady records on `rows` (float32 [row, case]), as the reference computes it: fp32 multiply, fp32 add,
    saturation; INTERP in fp64 with the record's (1 - X); LIMIT / LIMITN pick X or Y and do not saturate.  Returns, per dropped
    record, the largest |unsaturated value|; `values` (a dict), when given, receives the unsaturated values of EVERY saturating
    record, per case.  limits=False writes 0 where a LIMIT / LIMITN writes its pick (to see what depends on those records)."""
    worst = {}
    dropped = set(dropped)
    one = np.float32(1.0)

    def val(word, uniform):
        if uniform:
            return np.full(rows.shape[1], f32(word), dtype=np.float32)
        assert word < rows.shape[0], "a row operand outside the register file: the record's uniform flags are not the encoder's"
        return rows[word]

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
        if slot in (LIMIT, LIMITN):
            # uniform flags as fx_asm.cpp encodeAsmStream writes them into every generic record: w6 = UA | UX << 1 | UY << 2 | ccr << 3
            a, x, y = val(w[2], w[6] & 1), val(w[3], w[6] & 2), val(w[4], w[6] & 4)
            rows[dst] = (np.where(a >= y, x, y) if slot == LIMIT else np.where(a < y, x, y)) if limits else 0
            rows[0] = 0   # (the CCR row)
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
        if values is not None:
            values[i] = u
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


# ------------------------------------------------------------------------------------------------ a search for the worst state
class Model:
    """the steady records of a program with its quiet plan, ready for run_records"""

    def __init__(self, name, text):
        self.name, self.text = name, text
        fe = front_end(text)
        self.plan = plan = fe.quiet_plan(0)
        self.records = records = plan["records"]
        self.lead = 0
        while int(records[self.lead][0]) in (TRAM_IR, TRAM_XR):
            self.lead += 1
        n = 1 + max(int(w[5]) for w in records)
        self.n_rows = max([n] + [r + 1 for r, _, _ in plan["checked"]])
        self.dropped = set(plan["dropped"])
        # rows the PCM input arrives in (checked at 1: row 1 + channel), rows a leading delay-line read fills, and the checked rows
        # a register write before the launch reaches (everything else the device holds at 0 when a fresh handle starts)
        self.input_rows = [r for r, _, b in plan["checked"] if b == 1.0]
        self.read_rows = [int(w[5]) for w in records[:self.lead]]
        self.settable = [(r, n) for r, n, b in plan["checked"] if b < 1.0 and n is not None and r not in self.read_rows]
        self.wild = np.zeros(self.n_rows, dtype=bool)
        self.wild[0] = True
        self.wild[self.input_rows] = True

    def vertices(self, cases, rng, loud=1.0, reachable=False):
        rows = head_states(self.plan, self.n_rows, self.wild, cases, 0, rng)
        rows[self.input_rows] *= np.float32(loud)
        if reachable:
            keep = np.zeros(self.n_rows, dtype=bool)
            keep[self.input_rows + [r for r, _ in self.settable]] = True
            rows[~keep] = 0
        return rows

    def climb(self, targets, starts, rng, loud=1.0, reachable=False):
        """Coordinate ascent on |unsaturated value| of every target record, from `starts` random vertices each: flip the sign of one
        head row at a time - all flips are columns of one run_records call - keep the best flip, stop when none improves.
        Returns (value [target, start], head state [row, target, start], largest |value| seen per saturating record)."""
        free = (self.input_rows + [r for r, _ in self.settable]) if reachable else list(range(1, self.n_rows))
        T, F = len(targets), len(free)
        state = self.vertices(T * starts, rng, loud, reachable)
        value = np.zeros(T * starts, dtype=np.float32)
        seen = {}
        active = np.ones(T * starts, dtype=bool)
        while active.any():
            cols = np.nonzero(active)[0]
            big = np.repeat(state[:, cols], 1 + F, axis=1)
            for f, r in enumerate(free):
                big[r, 1 + f::1 + F] *= np.float32(-1.0)
            values = {}
            run_records(self.records, big, self.lead, (), values)
            for i, u in values.items():
                seen[i] = max(seen.get(i, 0.0), float(np.max(np.abs(u))))
            for k, j in enumerate(cols):
                u = np.abs(values[targets[j // starts]][k * (1 + F):(k + 1) * (1 + F)])
                best = int(np.argmax(u))
                value[j] = u[best]
                if best == 0 or not u[best] > u[0]:
                    active[j] = False
                else:
                    state[free[best - 1], j] *= np.float32(-1.0)
        return value.reshape(T, starts), state.reshape(self.n_rows, T, starts), seen


def search_targets(m):
    """every eighth dropped record, the eight that come closest to 1 over 256 random vertices, and config5's record 9 (where the
    search over all of its 395 records, 25 s long, finds 1.0)"""
    dropped = sorted(m.dropped)
    values = {}
    run_records(m.records, m.vertices(256, np.random.default_rng(5)), m.lead, (), values)
    near = sorted(dropped, key=lambda i: -float(np.max(np.abs(values[i]))))[:8]
    return sorted(set(dropped[::8]) | set(near) | ({9} & m.dropped))


_MODELS = {}


def model(name, text):
    if name not in _MODELS:
        _MODELS[name] = Model(name, text)
    return _MODELS[name]


_SEARCHES = {}


def searched(name, text, loud=1.0, reachable=False):
    """the search over one program, run once: (value, state, seen) of Model.climb over search_targets"""
    key = (name, loud, reachable)
    if key not in _SEARCHES:
        m = model(name, text)
        _SEARCHES[key] = m.climb(search_targets(m), 3, np.random.default_rng(4242), loud, reachable)
    return _SEARCHES[key]


def tight_states(name, text, count):
    """For the device tests: `count` head states of a fresh handle - ({register: value} to write, [first input sample per
    channel]) - the best of the search first, each followed by its negation, then random vertices.  Only rows a register write
    reaches before the first launch vary; every other row holds what a fresh handle holds, 0."""
    m = model(name, text)
    value, state, _ = searched(name, text, reachable=True)
    flat = state.reshape(m.n_rows, -1)
    order = np.argsort(-value.reshape(-1), kind="stable")
    heads, have = [], set()
    for j in order:
        for sign in (1.0, -1.0):
            h = flat[:, j] * np.float32(sign)
            if h.tobytes() not in have:
                have.add(h.tobytes())
                heads.append(h)
    extra = m.vertices(max(count, 1), np.random.default_rng(77), reachable=True)
    heads += [extra[:, k] for k in range(extra.shape[1])]
    out = []
    channels = max(1, len(re.findall(r"^input ", text, re.M)))
    assert all(1 <= r <= channels for r in m.input_rows), "the PCM input of channel c arrives in row 1 + c"
    for h in heads[:count]:
        out.append(({n: float(h[r]) for r, n in m.settable}, {r - 1: float(h[r]) for r in m.input_rows}))
    return out


ALL_PROGRAMS = [("config5", P.CONFIGS["config5"]())] + GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]


def kept_sites(m, seen):
    return {i: v for i, v in seen.items() if i not in m.dropped}


def test_wide_programs_cover_what_the_plan_admits():
    eligible = in_force = with_limit = stereo = 0
    for name, text in GENERATED_WIDE:
        m = model(name, text)
        eligible += m.plan["eligible"]
        in_force += m.plan["in_force"]
        slots = {int(w[0]) for w in m.records}
        kinds = {(int(w[0]) - MACS) % 16 // 2 for w in m.records if MACS <= int(w[0]) < SLOTS}
        with_limit += m.plan["in_force"] and bool(slots & {LIMIT, LIMITN})
        stereo += len(re.findall(r"^input ", text, re.M)) == 2
        assert 7 in kinds and MOV in slots, name
    assert eligible == len(GENERATED_WIDE) >= 12
    assert 3 * in_force >= 2 * len(GENERATED_WIDE) and with_limit >= 3 and stereo >= 2, (in_force, with_limit, stereo)
    m = model(*LIMIT_EDIT)
    assert m.plan["in_force"] and (m.plan["sites"], m.plan["quiet_dropped"]) == (224, 155)
    assert {LIMIT, LIMITN} <= {int(w[0]) for w in m.records}


def test_plan_is_sound_for_wide_programs():
    dropped = 0
    for name, text in GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]:
        n = soundness(name, text, 200)
        assert n is not None, name
        dropped += n
    assert dropped > 400, dropped


@pytest.mark.parametrize("name", [n for n, _ in ALL_PROGRAMS])
def test_the_search_finds_tight_states_and_nothing_above_one(name):
    """at the end of a climb no dropped record is above 1 - and for a program with a loop the climb does reach 1 (0.999 at the
    least: the plan's bounds are tight, and such states are what the device tests start from) while a saturation that the loop
    KEEPS does fire"""
    text = dict(ALL_PROGRAMS)[name]
    m = model(name, text)
    assert m.plan["eligible"], name
    for reachable in (False, True):
        value, _, seen = searched(name, text, reachable=reachable)
        over = {i: v for i, v in seen.items() if i in m.dropped and not v <= 1.0}
        assert not over, (name, sorted(over.items())[:5])
        assert set(seen) >= m.dropped
        # (what the device tests start from is as tight: config5 alone needs its delay lines' read rows for that)
        assert not m.plan["in_force"] or name == "config5" or value.max() >= 0.999, (name, reachable, float(value.max()))
    value, _, seen = searched(name, text)
    print(name, "in force" if m.plan["in_force"] else "no loop", "targets", value.shape[0], "largest dropped %.9g" % value.max(),
          "kept sites above 1: %d of %d" % (sum(v > 1.0 for v in kept_sites(m, seen).values()), len(kept_sites(m, seen))))
    if m.plan["in_force"]:
        assert value.max() >= 0.999, (name, float(value.max()))
        assert any(v > 1.0 for v in kept_sites(m, seen).values()), name


def test_a_loud_input_fires_dropped_saturations_in_the_model():
    """teeth: with the PCM input's head magnitude at 1.5 instead of 1, at least half of the generated programs with a loop show a
    dropped record above 1 (config5 takes its input through x 0.25: for it the rows-at-1.0 check above stays)"""
    fired = loops = 0
    for name, text in GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT]:
        m = model(name, text)
        if not m.plan["in_force"]:
            continue
        loops += 1
        _, _, seen = searched(name, text, loud=1.5)
        over = sum(v > 1.0 for i, v in seen.items() if i in m.dropped)
        print(name, "dropped records above 1 with the input at 1.5:", over)
        fired += over > 0
    assert loops >= 10 and 2 * fired >= loops, (fired, loops)


def test_the_bound_rule_of_limit_carries_dropped_saturations():
    """teeth of the LIMIT / LIMITN part of the model: in every program with a loop and such records, what they write reaches
    records whose saturation the plan drops - with 0 in its place the states found above give other values there - so those
    saturations are dropped on the strength of the bound rule for LIMIT / LIMITN, and the model above is what checks it"""
    programs = [(n, t) for n, t in GENERATED_WIDE if model(n, t).plan["in_force"]]   # (gen0_limit has them at its end: heads)
    assert len(programs) == 8
    for name, text in programs:
        m = model(name, text)
        assert {LIMIT, LIMITN} & {int(w[0]) for w in m.records}, name
        _, state, _ = searched(name, text)
        heads = state.reshape(m.n_rows, -1)
        with_, without = {}, {}
        run_records(m.records, heads.copy(), m.lead, (), with_)
        run_records(m.records, heads.copy(), m.lead, (), without, limits=False)
        changed = [i for i in sorted(m.dropped) if not np.array_equal(with_[i], without[i])]
        top = lambda v: max(float(np.max(np.abs(v[i]))) for i in m.dropped)   # noqa: E731
        print(name, "dropped records that depend on a LIMIT / LIMITN: %d of %d, largest value %.6g, without them %.6g" % (
            len(changed), len(m.dropped), top(with_), top(without)))
        assert changed, name
