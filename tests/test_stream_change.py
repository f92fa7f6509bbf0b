"""Leaving the fast stream at every record, without a GPU: the sweep's spliced programs
(stream_change_programs.py) translate in every stream - a silent fall-back to the interpreter would hollow out
test_gpu_stream_change.py -, their triggers fire in the oracle at the chosen samples, and no exact stream reads, behind a sync
point, a scratch register that it has not written since."""
import functools
import re

import numpy as np
import pytest

import fx8010_amd as A
import stream_change_programs as SC
from pyoracle import Oracle

STAGED_VGPRS = 128       # the build whose spare registers hold a stage's packets (test_stages.py translates the same one)
STAGE_COUNTS = (2, 3, 4)


# ---------------------------------------------------------------------------------------------------- the live-in walk
# Volatile: scratch that the two streams of a class do not set alike - the temporaries v2..v13, vcc, the record words and the
# return address s16..s25, the handlers' scratch s[62:67] and the inline delay-line scratch s84 / s[86:87].
VOLATILE = ({"v%d" % k for k in range(2, 14)} | {"vcc"} | {"s%d" % k for k in range(16, 26)} | {"s%d" % k for k in range(62, 68)} |
            {"s84", "s86", "s87"})
# Carried (not data of the test: the walk allows every register outside VOLATILE; this says why, by the line of fx_xlate_emit.hpp
# that names each group): the register-file rows v32 and up, kRegFileBase (:438); v14, v15 kVNumSkip / kVShadowCount (:439); v1
# kVLane4 (:446), v16..v19 kVCursor (:449), v22 kVOod (:448), v23..v26 kVInput (:475), v27 kVInstance4 (:476), v29 kVClassMask
# (:447), v30 kVRing (:485); the frame the prologue sets - s2 kSWave (:482), s3 / s9 kSSample / kSNumSamples (:471), s5 / s8
# kSLoaded / kSGroupSamples (:492), s6 kSSteadyLeft (:491), s7 kSGroupLeft (:490), s[12:15] kSPcmIn / kSPcmOut (:472), s[26:27]
# kSEventPtr (:479), s28 kSEventNext (:478), s[32:33] kSEntry (:442), s[34:35] kSEndSample (:443), s[36:39] / s56, s57 / s46, s47
# kSTramBase / kSTramSize / kSTramSlots (:469), s[40:41] kSLut (:467), s45 / s68 kSSampleBytes / kSChannelBytes (:473), s[58:59]
# kSValidLanes (:474), s[88:93] kSLutXthr / kSLutX1 / kSLutSeg (:468); the taint mask s[78:79] kSTaint (:445); the uniform cursors
# s80..s83 kSCursor (:450); s85 kSOod (:451), a launch-long accumulator; s94 kSPrefetched (:477), s95 kSHoistOk (:484); and
# s[22:23] of kSRecord (:440) in a staged program whose cold entry loads the one (1 - X) of its INTERPs (omxHoisted_: hoisted_pair).

_NO_DST = ("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_setpc", "s_waitcnt", "s_nop", "s_endpgm", "s_barrier", "s_sleep", "s_set_gpr_idx",
           "s_setprio", "s_sethalt", "s_setreg", "s_icache", "s_dcache", "s_trap", "s_sendmsg", "global_store", "ds_write", "buffer_store",
           "v_nop", "s_code_end")
# a handler call (fx_xlate.cpp call): the generic handlers read the record words w2..w6 and return through s[24:25]
CALL_READS = frozenset({"s18", "s19", "s20", "s21", "s22", "s24", "s25"})
_ENDS = ("s_branch", "s_setpc_b64", "s_endpgm", "s_swappc_b64")


def _operands(rest):
    out, depth, cur = [], 0, ""
    for ch in rest:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _registers(operand):
    regs = set()
    for kind, a, b in re.findall(r"\b([vs])\[(\d+):(\d+)\]", operand):
        regs.update("%s%d" % (kind, r) for r in range(int(a), int(b) + 1))
    regs.update("%s%s" % (k, n) for k, n in re.findall(r"\b([vs])(\d+)\b", operand))
    if re.search(r"\bvcc\b", operand):
        regs.add("vcc")
    return regs


@functools.lru_cache(maxsize=None)
def reads_and_writes(line):
    """(registers read, registers written) of one line of a listing.  Destinations: VOPC e32 writes the vcc it names first, a
    VOP3 compare its SGPR pair, a carry-out pair is a destination (v_subbrev_co_u32_e64 v6, s[64:65], ...); v_cndmask_b32_e32 names
    the vcc it reads; s_cbranch_vcc* reads vcc; a multiply-accumulate reads its destination."""
    parts = line.split(None, 1)
    mnem, ops = parts[0], _operands(parts[1]) if len(parts) > 1 else []
    n_dst = 0 if mnem.startswith(_NO_DST) else (2 if ("_co_" in mnem or mnem.startswith(("v_div_scale", "v_mad_u64", "v_mad_i64"))) else 1)
    n_dst = min(n_dst, len(ops))
    writes, reads = set(), set()
    for o in ops[:n_dst]:
        writes |= _registers(o)
    for o in ops[n_dst:]:
        reads |= _registers(o)
    if "mac_" in mnem or mnem.startswith(("v_writelane", "v_swap")):
        reads |= writes
    if mnem.startswith("s_cbranch_vcc"):
        reads.add("vcc")
    return reads, writes


@functools.lru_cache(maxsize=None)
def _size(line):
    """bytes of one instruction of a listing (the model of test_xlate.branch_targets, checked there against the assembler and
    here against the length of the code)"""
    if line.startswith(";") or not line:
        return 0
    op = line.split()[0]
    eight = (op.endswith("_e64") or op in ("v_med3_f32", "v_med3_i32", "v_fma_f32", "v_fma_f64", "v_add_f64", "v_mul_f64")
             or op.startswith(("global_", "ds_", "s_memrealtime")) or re.search(r"0x[0-9a-f]+", line) is not None)
    return 8 if eight else 4


def live_in_faults(listing, code_bytes=None, carried=()):
    """Behind every `; sync point` of an exact stream's listing - where a wavefront of the fast stream may arrive, with whatever THAT
    stream left in the scratch registers - and up to the next one or an unconditional s_branch / s_setpc_b64 / s_endpgm, no instruction
    may read a VOLATILE register that has not been written since the sync point.  A forward dataflow over the listing: conditional
    branches are followed on both sides (into the deferred code behind the loop and back: targets resolved through the instruction
    sizes), a register counts as written at a join only when it is on every path.  Returns (sync points, [(line, text, register)]).
    A handler call counts as a read of the record words w2..w6 and of the return address (CALL_READS: no handler reads more).
    Not seen: what happens inside a handler (the walk ends at the call), and exec - a write under a partial exec is taken as a
    write.  Those are the device sweep's job (test_gpu_stream_change.py)."""
    lines = listing.rstrip("\n").split("\n")
    sizes = [_size(l) for l in lines]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    if code_bytes is not None:
        assert int(offs[-1]) == code_bytes, "instruction size model"
    by_offset = {}
    for k in range(len(lines) - 1, -1, -1):
        by_offset[int(offs[k])] = k         # (a comment shares its offset with the instruction behind it: the comment wins)
    volatile = VOLATILE - set(carried)
    rw = [(set(), set()) if l.startswith(";") or not l else reads_and_writes(l) for l in lines]
    marks = [k for k, l in enumerate(lines) if l.startswith("; sync point")]
    faults = set()
    for start in marks:
        state = {start + 1: frozenset()}
        work = [start + 1]
        while work:
            k = work.pop()
            if k >= len(lines) or lines[k].startswith("; sync point"):
                continue
            have = state[k]
            reads, writes = rw[k]
            if lines[k] == "s_setpc_b64 s[62:63]":
                reads = reads | CALL_READS
            for r in reads & volatile:
                if r not in have:
                    faults.add((k, lines[k], r))
            after = have | (writes & volatile)
            mnem = lines[k].split()[0] if lines[k] else ""
            nxt = []
            if not mnem.startswith(_ENDS):
                nxt.append(k + 1)
            m = re.match(r"^(s_branch|s_cbranch_\w+) (\d+)$", lines[k])
            if m:
                simm = int(m.group(2))
                target = int(offs[k + 1]) + 4 * (simm - 65536 if simm >= 32768 else simm)
                if target in by_offset:
                    nxt.append(by_offset[target])       # (a target outside the listing is another stream: nothing to follow)
            for t in nxt:
                if t not in state:
                    state[t] = after
                    work.append(t)
                elif not state[t] <= after:
                    state[t] = state[t] & after
                    work.append(t)
    return len(marks), sorted(faults)


def hoisted_pair(listing):
    """s22, s23 where the cold entry of a staged stream loads them once (fx_xlate.cpp omxHoisted_) and the loop never writes them"""
    lines = listing.rstrip("\n").split("\n")
    stub = len(lines) - 1
    while stub > 0 and not lines[stub - 1].startswith(("s_branch", "s_setpc")):
        stub -= 1
    in_stub = {m.group(1) for l in lines[stub:] for m in [re.match(r"^s_mov_b32 (s2[23]),", l)] if m}
    in_loop = {m.group(1) for l in lines[:stub] for m in [re.match(r"^s_mov_b32 (s2[23]),", l)] if m}
    return ("s22", "s23") if in_stub == {"s22", "s23"} and not in_loop else ()


def test_the_walk_parses_destinations():
    assert reads_and_writes("v_cmp_u_f32_e32 vcc, v2, v2") == ({"v2"}, {"vcc"})
    assert reads_and_writes("v_cmp_lt_f32_e64 s[62:63], v3, v4") == ({"v3", "v4"}, {"s62", "s63"})
    assert reads_and_writes("v_subbrev_co_u32_e64 v6, s[64:65], 0, v6, s[62:63]") == ({"v6", "s62", "s63"}, {"v6", "s64", "s65"})
    assert reads_and_writes("v_addc_co_u32_e32 v6, vcc, 0, v6, vcc") == ({"v6", "vcc"}, {"v6", "vcc"})
    assert reads_and_writes("v_cndmask_b32_e32 v38, v5, v2, vcc") == ({"v5", "v2", "vcc"}, {"v38"})
    assert reads_and_writes("global_store_dword v27, v35, s[86:87]") == ({"v27", "v35", "s86", "s87"}, set())
    assert reads_and_writes("global_load_dword v42, v1, s[86:87] offset:16 nt") == ({"v1", "s86", "s87"}, {"v42"})
    assert reads_and_writes("s_cbranch_vccnz 18") == ({"vcc"}, set())
    assert reads_and_writes("s_setpc_b64 s[62:63]") == ({"s62", "s63"}, set())
    assert reads_and_writes("v_fma_f64 v[6:7], s[22:23], v[8:9], v[10:11]") == ({"s22", "s23", "v8", "v9", "v10", "v11"}, {"v6", "v7"})
    # a made-up stream: s22 written in front of the sync point only; v3 written on one side of a branch only
    listing = ("s_mov_b32 s22, 0\n; sync point\nv_mov_b32_e32 v2, v40\ns_cbranch_scc0 2\nv_mov_b32_e32 v3, v2\ns_nop 0\nv_add_f32_e32 v40, v3, v2\n"
               "v_fma_f64 v[6:7], s[22:23], v[8:9], v[10:11]\ns_branch 65527")
    n, faults = live_in_faults(listing)
    assert n == 1 and {(k, r) for k, _, r in faults} == {(6, "v3"), (7, "s22"), (7, "s23"), (7, "v8"), (7, "v9"), (7, "v10"), (7, "v11")}


# ---------------------------------------------------------------------------------------------------- the spliced corpus
def translated(text, streams=(0, 1, 2, 3, 4)):
    """(front end, {stream: (code, listing)}) of a two-channel program"""
    fe = A.FrontEnd(2)
    assert fe.load_text(text), fe.errors()
    return fe, {s: fe.translate(0, s) for s in streams}


LEAVE = re.compile(r"^s_cmp_lg_u64 s\[78:79\], 0\ns_cbranch_scc1 \d+$", re.M)     # leaveIfTainted


def two_channels(text):
    """a base program as the sweep runs it: with the input of channel 1 declared (and read by nothing)"""
    if SC.trigger_input(text)[1]:
        return text
    lines = text.split("\n")
    k = next(i for i, l in enumerate(lines) if SC._op(l) in SC.OPS)
    return "\n".join(lines[:k] + ["input tin 1"] + lines[k:])


CASES = SC.sweep_cases()


@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_spliced_programs_translate_with_a_leave_behind_the_trigger(case):
    """streams 0-4 of every spliced program (5 where the quiet plan admits it, every stage of every cut the planner accepts for
    the staged bases); against the base program, the fast stream has gained a taint check with its s_cbranch_scc1 and the exact
    stream of the same class a sync point; for the wrap triggers both are found at the trigger's own record (anchored); the numbers
    of quiet loops and of stage cuts translated are asserted"""
    name, sweep, base, kind, gap, at, staged = case
    _, plain = translated(two_channels(base), (0, 1))
    leaves, syncs, checks = len(LEAVE.findall(plain[0][1])), plain[1][1].count("; sync point"), plain[0][1].count("s_or_b64 s[78:79], s[78:79], ")
    instr = SC.positions(base)
    quiet = marks = cuts = 0
    for j in at:
        text = SC.with_trigger(base, j, kind, gap)
        fe, have = translated(text)
        for s in range(4):          # (stream 4, the run-once code, is empty where there is no LOG / EXP table to stage)
            assert have[s][0], (name, sweep, j, s)
        # The trigger's row is checked (one more s_or_b64 into the taint mask than the base has; inside a SKIP shadow a delay-line
        # read is a call of the per-lane handler, which taints the wavefront itself) and every check is followed by a leave.  The
        # leaves and sync points themselves are not one more than the base's: the trigger waits for the delay-line reads pending
        # beside it, so a wait of the base - its leave and sync point - may merge with the trigger's.
        fast = have[0][1].split("\n")
        taints = [k for k, l in enumerate(fast) if l.startswith("s_or_b64 s[78:79], s[78:79], ")]
        assert sweep in ("delay_shadow", "loud") or len(taints) > checks, (name, sweep, j, "no taint check of the trigger's row")
        for k in taints:
            after = "\n".join(fast[k + 1:k + 60])
            assert LEAVE.search(after), (name, sweep, j, k, "a taint check without a leave behind it")
        assert len(LEAVE.findall(have[0][1])) >= min(leaves, 1) + (1 if sweep == "delay_shadow" else 0), (name, sweep, j)
        for s in (1, 3):
            assert have[s][1].count("; sync point") >= len(LEAVE.findall(have[s - 1][1])), (name, sweep, j, s, "a leave without a sync point")
            n, faults = live_in_faults(have[s][1], len(have[s][0]))      # the live-in walk of this spliced program's exact streams
            assert n > 0 and not faults, (name, sweep, j, s, faults[:4])
            marks += n
        if kind in ("wrap", "wrapint"):
            anchored(have, (name, sweep, j))
        if name in SC.QUIET_BASES and fe.quiet_plan(0)["in_force"]:
            code, listing = fe.translate(0, 5)
            assert code and LEAVE.search(listing) and "; quiet check" in listing, (name, sweep, j)
            quiet += 1
        if staged:
            for stages in STAGE_COUNTS:
                k = fe.translate_staged(stages, 0, 0, STAGED_VGPRS)[2]
                cuts += k > 1
                for st in range(k if k > 1 else 0):
                    for s in range(5):
                        fe.translate_staged(stages, st, s, STAGED_VGPRS)     # (raises when the translation fails)
    print(name, sweep, "spliced programs", len(at), "sync points walked", marks, "quiet loops", quiet, "stage cuts", cuts)
    # the quiet plan admits the loud trigger at every position, and of the others only a delay-line read that leads wide1 (the plan
    # refuses a handler call, LOG / EXP and a delay-line read in the middle of a program): what those kinds sweep on gen2 and wide1
    # is the fast stream
    assert quiet == QUIET_LOOPS.get((name, sweep), 0), (name, sweep, quiet)
    # the planner cuts these at every position, for 2, 3 and 4 stages
    if name in CUT_EVERYWHERE and kind != "delay":
        assert cuts == len(STAGE_COUNTS) * len(at), (name, sweep, cuts)


QUIET_LOOPS = {("gen2", "loud"): 47, ("wide1", "loud"): 48, ("wide1", "delay1"): 1, ("wide1", "delay3"): 1}
CUT_EVERYWHERE = ("config1_logtube", "config2", "record_words_input")
BIG_WORD = "0x7eb48e52"       # 1.2e38, the Y of the wrap triggers: the one record of a spliced program that names it


def anchored(have, where):
    """the wrap trigger's own record, found by its literal: in the fast streams the class check of its result, the OR into the
    taint mask and the leave follow it within the record; in the exact streams its handler call and, behind it, a sync point"""
    for s in (0, 2):
        fast = have[s][1].split("\n")
        k = next(i for i, l in enumerate(fast) if BIG_WORD in l)
        tail = "\n".join(fast[k:k + 40])
        assert re.search(r"^v_cmp_class_f32_e32 vcc, v\d+, v29\ns_or_b64 s\[78:79\], s\[78:79\], vcc\ns_cmp_lg_u64 s\[78:79\], 0\ns_cbranch_scc1 \d+$",
                         tail, re.M), (where, s, "no taint check and leave behind the trigger record")
    for s in (1, 3):
        exact = have[s][1].split("\n")
        k = next(i for i, l in enumerate(exact) if BIG_WORD in l)
        tail = "\n".join(exact[k:k + 12])
        assert re.search(r"^s_setpc_b64 s\[62:63\]\n; sync point$", tail, re.M), (where, s, "no sync point behind the trigger's call")


# ---------------------------------------------------------------------------------------------------- firing, against the oracle alone
# wavefront cases left out per program (every other program: none): SKIP shadows that all four trigger lanes skip in that sample
LEFT_OUT = {"config4": 87, "mixed_stages": 18, "product_cache2": 30, "random6": 12, "random28": 18, "random2_12": 3, "random2_0": 24,
            "random2_28": 75, "random2_29": 15}


def test_the_triggers_fire_in_the_oracle_at_the_chosen_samples(capsys):
    """With the device test's stimulus and preset registers the trigger register of a spliced program is finite before the
    wavefront's sample and not finite in it (delay: trd == 2.0 with the out-of-domain flags 0; lut: flag 16 from that sample on), in at least one of the
    wavefront's four trigger lanes.  A case is one wavefront - one sample phase - of one spliced program; one without such a lane
    (the record lies in a SKIP shadow that every candidate lane skips in that sample) is left out of what the device sweep counts
    as a leave: at most 10 % of the cases of any program, at most 5 % over all, and every program with a SKIP keeps a fired case
    inside a shadow.  (The device sweep runs and compares the left-out wavefronts all the same.)
  The loud trigger fires when trg is 1.0 in the wavefront's
    sample and not before.  LEFT_OUT holds the count per program and is asserted, so that it cannot go stale."""
    tried = fired = 0
    table = []
    for name, text, _ in SC.corpus():
        n = ok = shadow_ok = spots = 0
        for cname, sweep, base, kind, gap, at, _ in CASES:
            if cname != name:
                continue
            x = SC.stimulus(kind)
            inside = SC.shadows(base)
            presets = SC.preset_registers(base, kind)
            spots += len(at)
            for j in at:
                hit = SC.fired_waves(Oracle, SC.with_trigger(base, j, kind, gap), kind, x, presets)
                n += len(hit)
                ok += sum(lane is not None for lane in hit.values())
                shadow_ok += j in inside and any(lane is not None for lane in hit.values())
        table.append((name, spots, n, ok, n - ok))
        assert n - ok <= 0.10 * n, (name, n, ok)
        assert n - ok == LEFT_OUT.get(name, 0), (name, n, ok)
        assert shadow_ok > 0 or not SC.shadows(text), (name, "no fired case inside a SKIP shadow")
        tried += n
        fired += ok
    with capsys.disabled():
        for row in table:
            print("%-16s spliced programs %4d: cases tried %4d fired %4d left out %3d" % row)
        print("all: tried %d fired %d left out %d" % (tried, fired, tried - fired))
    assert tried - fired <= 0.05 * tried, (tried, fired)


# ---------------------------------------------------------------------------------------------------- the walk over the corpus
def test_no_exact_stream_reads_scratch_it_has_not_written_since_a_sync_point(capsys):
    """live_in_faults() over the exact streams 1 and 3 of the unspliced corpus, of one spliced program of every case (the middle
    position; test_spliced_programs_translate... walks every position) and over the exact streams of every stage of the cuts the
    planner accepts (there with s[22:23] carried where the cold entry loads the pair: hoisted_pair).  Generalises test_xlate.py's
    _record_word_faults from s16..s23 under v_* reads to every scratch register under every read, on every path between two sync
    points."""
    walked = marks = 0
    texts = [(name, "base", two_channels(text), staged) for name, text, staged in SC.corpus()]
    for name, sweep, base, kind, gap, at, staged in CASES:
        j = at[len(at) // 2]
        texts.append((name, "%s@%d" % (sweep, j), SC.with_trigger(base, j, kind, gap), staged))
    for name, what, text, staged in texts:
        fe, have = translated(text, (1, 3))
        for s in (1, 3):
            code, listing = have[s]
            n, faults = live_in_faults(listing, len(code))
            assert not faults, (name, what, s, faults[:4])
            walked += 1
            marks += n
        for stages in STAGE_COUNTS if staged else ():
            k = fe.translate_staged(stages, 0, 0, STAGED_VGPRS)[2]
            for st in range(k if k > 1 else 0):
                for s in (1, 3):
                    code, listing = fe.translate_staged(stages, st, s, STAGED_VGPRS)[:2]
                    n, faults = live_in_faults(listing, len(code), carried=hoisted_pair(listing))
                    assert not faults, (name, what, stages, st, s, faults[:4])
                    walked += 1
                    marks += n
    with capsys.disabled():
        print("live-in walk: %d exact streams, %d sync points" % (walked, marks))
    assert marks > 1000
