"""valu_model.Valu extended by what the quiet loop with sum groups (fxp_translate stream 6; fx_xlate.hpp SumGroup) adds to a sample's
body: the scalar half of a group's test - `s_and_b64 s[62:63], vcc, s[58:59]`, `s_or_b64 s[62:63], s[62:63], s[4:5]`,
`s_cmp_lg_u64 s[62:63], 0`, `s_cbranch_scc1` into the group's repair stub behind the loop - and the stub's own scalar lines
(`s_and_b64 s[4:5], vcc, s[58:59]` / `s_mov_b64 s[4:5], 0`, `s_add_u32 s6, s6, 1`, the `s_branch` back).

A wavefront is `wave` consecutive cases (default: all of them); lane masks are boolean columns.  A branch is taken by every case of a
wavefront in which a valid case fires, as on the device: the stub then runs on ALL cases of that wavefront.  The k-th `; sum group
test` of the body belongs to the k-th `; sum group repair` behind the loop (the translator defers the stubs in the order of the
tests)."""
import re

import numpy as np

from valu_model import Valu

TEST, REPAIR = "; sum group test", "; sum group repair"


def stubs_of(listing):
    """the repair stubs of a listing, in order: the lines between each `; sum group repair` and the s_branch that ends it"""
    lines = [l for l in listing.split("\n") if l]
    out = []
    for k, l in enumerate(lines):
        if l == REPAIR:
            e = next(e for e in range(k + 1, len(lines)) if lines[e].startswith("s_branch "))
            out.append(lines[k + 1:e])
    return out


class ValuSums(Valu):
    def __init__(self, cases, stubs, wave=None, valid=None):
        Valu.__init__(self, cases)
        self.stubs = stubs
        self.wave = wave or cases
        self.valid = np.ones(cases, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        self.mask = {62: np.zeros(cases, dtype=bool), 4: np.zeros(cases, dtype=bool)}   # s[62:63], s[4:5] as lane columns
        self.repairs = np.zeros((cases + self.wave - 1) // self.wave, dtype=np.int64)    # s6, per wavefront
        self.fired = []          # per test of the body, in order: boolean per wavefront
        self.tests = 0
        self.scc = None          # per wavefront
        self.pending = False     # the next s_cbranch_scc1 is a group's

    def _per_wave(self, lanes):
        pad = (-len(lanes)) % self.wave
        return np.concatenate([lanes, np.zeros(pad, dtype=bool)]).reshape(-1, self.wave).any(axis=1)

    def step(self, line):
        line = line.strip()
        if line == TEST:
            self.pending = True
            return
        if self.pending:
            if line.startswith("v_"):
                return Valu.step(self, line)
            if line == "s_and_b64 s[62:63], vcc, s[58:59]":
                self.mask[62] = self.vcc & self.valid
            elif line == "s_or_b64 s[62:63], s[62:63], s[4:5]":
                self.mask[62] = self.mask[62] | self.mask[4]
            elif line == "s_cmp_lg_u64 s[62:63], 0":
                self.scc = self._per_wave(self.mask[62])
            elif re.match(r"s_cbranch_scc1 \d+$", line):
                self.pending = False
                self.fired.append(self.scc.copy())
                stub = self.stubs[self.tests]
                self.tests += 1
                lanes = np.repeat(self.scc, self.wave)[:self.cases]
                if lanes.any():
                    self._repair(stub, lanes)
            else:
                raise AssertionError("a line the group's test does not have: " + line)
            return
        return Valu.step(self, line)

    def _repair(self, stub, lanes):
        sub = Valu(int(lanes.sum()))
        sub.v = {n: col[lanes].copy() for n, col in self.v.items()}
        sub.s = dict(self.s)
        for l in stub:
            if l == "s_and_b64 s[4:5], vcc, s[58:59]":
                self.mask[4][lanes] = sub.vcc & self.valid[lanes]
            elif l == "s_mov_b64 s[4:5], 0":
                self.mask[4][lanes] = False
            elif l == "s_add_u32 s6, s6, 1":
                self.repairs += self._per_wave(lanes)
            else:
                assert l.startswith("v_"), l
                sub.step(l)
        for n, col in sub.v.items():
            if n not in self.v:
                self.v[n] = np.zeros(self.cases, dtype=np.uint32)
            self.v[n][lanes] = col
        for op, n in sub.executed.items():
            self.executed["stub:" + op] = self.executed.get("stub:" + op, 0) + n
