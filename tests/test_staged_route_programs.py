"""The premise of tests/test_gpu_staged_routes.py, checked where there is no GPU: the planner cuts the three programs of
staged_route_programs.py as those tests expect, and the registers they compare by name are stored at the end of a block by
DIFFERENT stages (FrontEnd.stage_store) - so a by-list write between two blocks lands in rows that several wavefronts of a
workgroup load separately, and a stage that stored stale rows would show in a named register.  CPU only."""
import numpy as np
import pytest

import fx8010_amd as A
import staged_route_programs as SP

SKIP, IDELAY, XDELAY, END = 0xF, 0x10, 0x11, 0x12      # fx_model.hpp Opcode
R_INPUT, R_OUTPUT, R_READ = 3, 4, 8                     # fx_model.hpp RegType


def front_end(name):
    channels, text, named, control = SP.PROGRAMS[name]
    fe = A.FrontEnd(channels)
    assert fe.load_text(text), fe.errors()
    return fe


def rows_of(fe, channels):
    """register name -> register-file row: the allocation of fx_decode.cpp (sections 1, 3 and 4) for a program without forced
    rows, restated - row 0 is the CCR, then one input row per channel an instruction hears, one output latch per channel, then
    every register that lives per instance in register order; an input register read outside every SKIP shadow through one
    channel only is that channel's input row.  (test_the_row_table_agrees_with_the_quiet_plan checks it against the rows the
    library itself reports.)"""
    regs, ins = fe.registers(), fe.instructions()
    P = len(ins)
    lane = [False] * len(regs)
    lane[0] = True
    for r, (name, kind, io, bits) in enumerate(regs):
        lane[r] = lane[r] or kind == R_OUTPUT
    shadow = [False] * P
    for k, (op, r, a, x, y, has_in, has_out, has_noise) in enumerate(ins):
        if op not in (SKIP, IDELAY, XDELAY, END):
            lane[r] = True
        if op in (IDELAY, XDELAY) and regs[r][1] == R_READ:
            lane[a] = True
        if has_noise:
            lane[[q for q in (a, x, y) if regs[q][0] == "noise"][0]] = True
        if op == SKIP:
            assert not lane[y], "a SKIP count that lives per instance shadows everything: not one of these programs"
            count = int(np.array([regs[y][3]], dtype=np.uint32).view(np.float32)[0])
            for j in range(1, (1 if count < 0 else count) + 1):
                shadow[(k + j) % P] = True
    seen, uncond, target = {}, set(), set()
    for k, (op, r, a, x, y, has_in, has_out, has_noise) in enumerate(ins):
        if op in (IDELAY, XDELAY) and regs[r][1] == R_READ:
            target.add(a)
        if not has_in:
            continue
        for q in (a, x, y):
            if regs[q][1] == R_INPUT:
                seen[q] = regs[a][2] if seen.get(q, regs[a][2]) == regs[a][2] else -1
                if not shadow[k]:
                    uncond.add(q)
    alias = {q: c for q, c in seen.items() if c >= 0 and q in uncond and q not in target}
    for q in seen:
        lane[q] = True
    row, nxt, in_row = {regs[0][0]: 0}, 1, {}
    for c in range(channels):
        if any(i[5] and regs[i[2]][2] == c for i in ins):
            in_row[c] = nxt
            nxt += 1
    nxt += channels      # the output latches
    for r in range(1, len(regs)):
        if lane[r]:
            if r in alias:
                row[regs[r][0]] = in_row[alias[r]]
            else:
                row[regs[r][0]] = nxt
                nxt += 1
    return row, nxt


@pytest.mark.parametrize("name", sorted(SP.PROGRAMS))
def test_the_planner_cuts_the_three_programs(name):
    fe = front_end(name)
    got = []
    for asked in (2, 4, 8):
        try:
            got.append(fe.translate_staged(asked)[2])
        except RuntimeError:
            got.append(1)
    assert tuple(got) == SP.CUTS[name], got
    assert SP.CUTS[name][1] >= 2      # FX_STAGES=4, what the S handles of the GPU tests ask for, gives staged code


@pytest.mark.parametrize("name", ["config2", "chain3"])
def test_the_row_table_agrees_with_the_quiet_plan(name):
    """the library reports (row, register) for the rows its quiet plan checks: every such pair is in the restated table"""
    fe = front_end(name)
    row, used = rows_of(fe, SP.PROGRAMS[name][0])
    pairs = [(r, n) for r, n, bound in fe.quiet_plan()["checked"] if n is not None]
    assert len(pairs) >= 8, pairs
    assert all(row[n] == r for r, n in pairs), [(r, n, row[n]) for r, n in pairs if row[n] != r]
    fe.translate_staged(4)
    assert used <= len(fe.stage_store)      # (bookkeeping rows follow the registers')


@pytest.mark.parametrize("name, asked, least", [("config2", 4, 3), ("config2", 8, 3), ("chain3", 4, 3), ("chain3", 8, 3), ("mixed", 4, 2), ("mixed", 8, 3), ("mixed_e", 4, 2), ("mixed_e", 8, 3)])
def test_the_named_registers_are_stored_by_different_stages(name, asked, least):
    """the registers test_gpu_staged_routes.py writes by list and compares by name belong to at least three stages (two where
    the planner makes two: mixed_stages under FX_STAGES=4); the delay-line registers and the first filter state belong to
    stage 0, the output to the last stage, and the control every stage reads has no row while it is folded into the code"""
    channels, text, named, control = SP.PROGRAMS[name]
    fe = front_end(name)
    k = fe.translate_staged(asked)[2]
    row, used = rows_of(fe, channels)
    store = fe.stage_store
    assert k >= 2 and len(store) >= used and all(0 <= s < k for s in store)
    stage = {n: store[row[n]] for n in named}
    assert len(set(stage.values())) >= least, stage
    assert stage["s0"] == 0 and stage["out" if channels == 1 else "o%d" % (channels - 1)] == k - 1, stage
    if name.startswith("mixed"):
        assert stage["rd"] == stage["a"] == 0, stage
    assert control not in row
