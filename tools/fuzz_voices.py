"""Random programs x random sequences of the BY-LIST STATE CALLS against a voice model made of oracle objects.

    python tools/fuzz_voices.py [first_seed] [count]
    python tools/fuzz_voices.py <seed> 1 verbose     one sequence, every step printed, the whole state of the tracked instances
                                                     compared in front of each step

The calls: fxb_set_registers_list / fxb_get_registers_list, fxb_copy_instances, fxb_reset_instances, fxb_save_instances,
fxb_load_instances, fxb_load_instances_rotated, fxb_set_tram_list / fxb_get_tram_list - in any order, between blocks of 1-40
samples, broadcast / per-instance / array register writes, dense control tracks, list schedules and fxb_prepare, as
tools/fuzz_api.py draws them.  Programs come from four generators by seed (seed % 4): stress_fuzz.random_program (ring lines that
move uniformly), stress_fuzz.random_program2 (write offsets, delay instructions in SKIP shadows: lines that are no rings, positions
that differ per lane), fuzz_tram.random_tram_program in the reference model and in the DANE model.  A fifth generator is reached
through FX_FUZZ_GEN=4 only: fuzz_stages.random_program, the feed-forward programs the stage planner CUTS (delay lines, noise, SKIP,
LOG / EXP) - the first of at most 8 draws that the front end cuts into two or more stages when four are asked.

The seed ranges of the test suite (SLICES): main (seeds 0.., the four generators by seed), wild (FX_FUZZ_WILD=1), dane (generator 3)
and staged (generator 4 under FX_STAGES=4, schedules from step 12 on: the by-list calls between blocks of staged code;
cover["staged_blocks"] counts, per device block, whether it ran as a pipeline of stages).

The MODEL is written from the contract in include/fx8010_amd.h: one oracle object per TRACKED instance (0, N-1, N//2 and the
instances the list operations of the sequence mostly name, at most 12), the last broadcast value per register (a reset needs it),
and a table of saved records as cloned oracles.  Whether a call is ACCEPTED is decided by the model's reading of the header, never
by what the device answers; a call the model refuses must fail on the device, name its reason where the header says so, and
change nothing.  After every block the outputs of the tracked instances are compared bit for bit, NaN words included; a sequence
whose oracle leaves the parity domain ends there (counted).  run(seed, device=False) runs the model alone (no GPU): that is how
tests/test_voice_sequences_model.py counts what the sequences of a seed range cover.  Every random draw of a step is made with
or without a device, so both runs walk the same sequence; cover["stream"] is a digest of the random stream in front of every
step, which tests/test_gpu_voice_sequences.py compares between the two.

Environment: FX_KERNEL / FX_INST_PER_LANE select the tier as everywhere; FX_FUZZ_SHARDS=n a multi-shard handle; FX_FUZZ_WILD=1
list sets and windows carry values beyond +-1, denormals, +-0, NaN payloads and Inf; FX_FUZZ_GEN=<0..4> pins the generator
(3: the DANE model, 4: programs the stage planner cuts); FX_FUZZ_BREAK=<name> makes the MODEL wrong in one respect (BREAKS below) - the detection tests show that
the sequences notice each; it never touches the library.  FX_FUZZ_TRACKS_FROM=<step>: the steps in front of it run a plain block
where they would arm schedules (the staged range: a handle that has armed one runs no staged code any more).
"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fx8010-emulator-core_amd/python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import fuzz_api  # noqa: E402
import fuzz_tram  # noqa: E402
import fx8010_amd as A  # noqa: E402
import fx8010_programs as P  # noqa: E402
import stress_fuzz  # noqa: E402
from fuzz_api import same, value  # noqa: E402
from pyoracle import Oracle  # noqa: E402

BREAKS = ("copy_drops_lfsr", "reset_zeroes_positions", "reset_uses_initial_not_last_broadcast", "logical_window_off_by_one",
          "rotated_load_unrotated", "list_set_skips_last_entry")
# the operation kinds whose acceptance the header rules on; COVER[kind] = [accepted, refused]
KINDS = ("tracks_list", "set_registers_list", "get_registers_list", "copy", "reset", "save", "load", "load_rotated", "set_tram_list", "get_tram_list")
STEPS = 36
MAX_TRACKED = 12
LINE = ("iTRAM", "xTRAM")

# patterns for FX_FUZZ_WILD: beyond +-1, denormals, +-0, quiet NaNs with payloads, Inf (registers travel through C floats on the
# oracle's side, which quiets a signalling NaN: those go into delay memory only)
WILD_WORDS = np.array([0x40200000, 0xC0400000, 0x3F800001, 0x42C80000, 0x7149F2CA, 0x800116C2, 0x00000001, 0x807FFFFF, 0x00000000, 0x80000000,
                       0x7FC00000, 0xFFC12345, 0x7FC00001, 0x7F800000, 0xFF800000], dtype=np.uint32)
WILD_TRAM_ONLY = np.array([0x7F812345, 0xFFA00000], dtype=np.uint32)


def new_cover(stages=False):
    """stages: also count, per device block, whether it ran as a pipeline of stages (cover["staged_blocks"]: only a run with a
    device fills it, so a caller that compares a device run with the model alone asks for it and leaves it out of the comparison)"""
    c = {k: [0, 0] for k in KINDS}
    c.update(sequences=0, loaded=0, left_domain=0, rotated_nonzero=0, logical_wrap=0, blocks=0, state_reads=0, second_handles=0, kernels={}, sharded_handles=0, stream=0)
    # device blocks by FXB_INFO_WAVES_PER_WG behind them: plain / scheduled = [one wavefront per workgroup, a pipeline of stages] of the
    # blocks that armed no schedule / a track or a list schedule; kernels: FXB_INFO_KERNEL of the staged ones; sequences: those
    # in which at least one block was staged
    if stages:
        c["staged_blocks"] = {"plain": [0, 0], "scheduled": [0, 0], "kernels": {}, "sequences": 0}
    # the model's side of it (no device needed): blocks that armed no schedule, on a handle that [never armed one so far, has armed one]
    c["plain_blocks"] = [0, 0]
    return c


COVER = new_cover()

# the seed ranges of the test suite: tests/test_gpu_voice_sequences.py runs them on the device, tier by tier, and
# tests/test_voice_sequences_model.py counts what the same sequences cover with the model alone.  name: (first, count, environment)
SLICES = {"main": (0, 20, {}), "wild": (300, 20, {"FX_FUZZ_WILD": "1"}), "dane": (200, 20, {"FX_FUZZ_GEN": "3"}),
          "staged": (463, 20, {"FX_FUZZ_GEN": "4", "FX_STAGES": "4", "FX_FUZZ_TRACKS_FROM": "12"})}
STAGED_DRAWS, STAGED_ASKED = 8, 4


class Mismatch(Exception):
    pass


class LeftDomain(Exception):
    pass


def generate(seed, rng, gen):
    """-> text, options"""
    if gen == 0:
        return stress_fuzz.random_program(rng, int(rng.integers(6, 70)), int(rng.integers(3, 30))), 0
    if gen == 1:
        return stress_fuzz.random_program2(rng, int(rng.integers(6, 70)), int(rng.integers(3, 30))), 0
    if gen == 4:
        import fuzz_stages      # (here: it brings torch along where there is one, which the other generators need not wait for)
        for _ in range(STAGED_DRAWS):
            text = fuzz_stages.random_program(rng, int(rng.integers(3, 9)), int(rng.integers(3, 9)))
            if stages_cut(text, STAGED_ASKED) >= 2:
                break
        return text, 0
    return fuzz_tram.random_tram_program(rng, gen == 3), (A.OPT_TRAM_DANE if gen == 3 else 0)


def stages_cut(text, asked):
    """how many stages the front end cuts a program into when `asked` are asked for (no GPU); 1 where it refuses"""
    fe = A.FrontEnd(1)
    if not fe.load_text(text):
        return 1
    try:
        return fe.translate_staged(asked)[2]
    except RuntimeError:
        return 1


class Program:
    """what the model has to know about a program text: names, which registers the program itself can change, the delay lines"""

    def __init__(self, text, options):
        self.text, self.options, self.dane = text, options, bool(options & A.OPT_TRAM_DANE)
        decl = [l.split() for l in text.split("\n") if l.startswith(("static ", "control "))]
        self.declared = [d[1] for d in decl if d[1] != "noise"]
        self.names = list(dict.fromkeys(self.declared + ["out", "ccr"]))
        self.controls = [d[1] for d in decl if d[0] == "control"]
        self.changed = {"out", "ccr", "in"}      # the result of an instruction, the CCR, an input or an output register
        self.writes, self.reads = [False, False], [False, False]
        self.lut_inputs = set()
        for l in text.split("\n"):
            parts = l.split(None, 1)
            if len(parts) != 2 or parts[0] in ("static", "control", "input", "output", "itramsize", "xtramsize", "name", "engine", "comment"):
                continue
            ops = [o.strip() for o in parts[1].split(",")]
            if parts[0] in ("idelay", "xdelay"):
                which = 0 if parts[0] == "idelay" else 1
                if ops[0] == "read":
                    self.reads[which] = True
                    self.changed.add(ops[1])
                else:
                    self.writes[which] = True
            elif parts[0] != "skip":
                self.changed.add(ops[0])
                if parts[0] in ("log", "exp"):
                    self.lut_inputs.add(ops[1])      # (LOG / EXP of a value outside [-1, 1] is outside the parity domain)
        fe = A.FrontEnd(1)
        if options:
            fe.set_option(options)
        self.loads = bool(fe.load_text(text)) and fe.lower() == 0
        if self.loads:
            self.Z = list(fe.tram_sizes())
            self.A = [fe.lower_info("itram_slots"), fe.lower_info("xtram_slots")]       # FXB_INFO_ITRAM_SLOTS / _XTRAM_SLOTS
            self.tram_ops = fe.lower_info("tram_ops")
            self.ring = [self.A[w] > 0 and self.A[w] == self.Z[w] for w in (0, 1)]       # "L is a RING when A == Z"

    def fresh(self):
        o = Oracle(1)
        if self.options:
            o.set_option(self.options)
        if not o.load_text(self.text):
            raise RuntimeError("the oracle refuses a program the front-end loads")
        return o

    def slot(self, which, p, a):
        """the header's slot of logical word a: (p - 1 - a) mod Z, under FX_OPT_TRAM_DANE (p + 1 + a) mod Z"""
        if BREAK() == "logical_window_off_by_one":
            a = a + 1
        Z = self.Z[which]
        return (p + 1 + a) % Z if self.dane else (p - 1 - a) % Z


def BREAK():
    return os.environ.get("FX_FUZZ_BREAK", "")


class Handle:
    """a batch on the device (None: the model alone) and the voice model of its tracked instances"""

    def __init__(self, prog, N, tracked, device, shards, first_sample=0):
        self.prog, self.N, self.tracked = prog, N, list(tracked)
        self.b = None
        self.sharded = bool(device) and shards > 1 and (N + 63) // 64 >= shards      # (a shard holds whole wavefronts: fewer of them than shards is one batch)
        if device:
            self.b = A.Batch(N, 1, devices=[0] * shards) if self.sharded else A.Batch(N, 1, 0)
            if prog.options:
                self.b.set_option(prog.options)
            if not self.b.load_text(prog.text):
                raise Mismatch("the batch refuses a program the front-end loads: %s" % (self.b.errors(),))
        self.o = {n: prog.fresh() for n in self.tracked}
        self.broadcast = {}
        self.x = P.stimulus(N, 1700, first_sample=first_sample)
        self.pos = 0
        self.trackable = False      # a schedule has been armed: a register of this handle is trackable from then on

    def take(self, S):
        xs = self.x[self.pos:self.pos + S]
        self.pos += S
        return xs

    def untracked(self):
        return [n for n in range(self.N) if n not in self.o]

    # ---- the voice model: what each by-list call does to the tracked oracles, by include/fx8010_amd.h.  No random draws and no
    # device in here: the runner below draws the arguments, decides acceptance with these, and makes the device's call beside them

    def line_of(self, o, w):
        """the A allocated slots of line w of an oracle"""
        return o.tram(w, self.prog.A[w]).copy()

    def model_set_registers(self, keys, L, vals):
        """fxb_set_registers_list: set_register_i of vals[k, i] on register keys[k] of instance L[i]"""
        for k, key in enumerate(keys):
            for i, n in enumerate(L):
                if n in self.o and not (BREAK() == "list_set_skips_last_entry" and i == len(L) - 1):
                    self.o[n].set_register(key, float(vals[k, i]))

    def model_copy(self, src, dst):
        """fxb_copy_instances: dst[k] becomes a bit-for-bit copy of src[k] - every state row and all delay memory, so the position
        rows travel too; a destination is never a source, so the order of the pairs does not matter"""
        new = {}
        for s, d in zip(src, dst):
            if d in self.o:
                new[d] = self.o[s].clone()
                if BREAK() == "copy_drops_lfsr":
                    new[d].seed_noise(*self.o[d].lfsr())
        self.o.update(new)

    def model_reset(self, L):
        """fxb_reset_instances: a fresh object, registers at the last broadcast value (else the program's initial one), the four
        positions kept"""
        for n in L:
            if n in self.o:
                o = self.prog.fresh()
                if BREAK() != "reset_uses_initial_not_last_broadcast":
                    for name, v in self.broadcast.items():
                        o.set_register(name, v)
                o.set_cursors([0, 0, 0, 0] if BREAK() == "reset_zeroes_positions" else self.o[n].cursors())
                self.o[n] = o

    def rotation(self, rec_o, dst_o):
        """fxb_load_instances_rotated: -> (d per line, the lines on which the header refuses the record)"""
        prog = self.prog
        d, bad = [0, 0], []
        cs, cd = rec_o.cursors(), dst_o.cursors()
        for w in (0, 1):
            Z = prog.Z[w]
            if prog.A[w] == 0 or Z < 1:
                continue
            if not all(0 <= v < Z for v in cs[2 * w:2 * w + (1 if prog.dane else 2)]):
                bad.append(w)
                continue
            dw, dr = (cd[2 * w] - cs[2 * w]) % Z, (cd[2 * w + 1] - cs[2 * w + 1]) % Z
            if prog.dane:
                d[w] = dw
            elif prog.writes[w] and prog.reads[w]:
                if dw != dr:
                    bad.append(w)
                    continue
                d[w] = dw
            elif prog.writes[w]:
                d[w] = dw
            elif prog.reads[w]:
                d[w] = dr
            if d[w] != 0 and not prog.ring[w]:
                bad.append(w)
        return d, bad

    def model_load(self, entries, dst, rotated):
        """fxb_load_instances / _rotated of saved records (cloned oracles; None: an untracked instance's) into dst.
        -> (new, why, where): new[d] = (the oracle d becomes, whether a line was rotated by d != 0), nothing applied yet; why: the
        reason the header refuses the call (then `where` lists the (line, entry) pairs a rotated load may name), else None"""
        prog = self.prog
        new, why, where = {}, None, []
        for k, (e, d) in enumerate(zip(entries, dst)):
            if e is None or d not in self.o:
                continue       # (only where no delay-line instruction runs: nothing to decide, nothing to model)
            if prog.tram_ops == 0:
                new[d] = (e.clone(), False)
            elif not rotated:
                if e.cursors() != self.o[d].cursors():
                    return {}, "the position words of a record differ from its destination's", []
                new[d] = (e.clone(), False)
            else:
                rot, bad = self.rotation(e, self.o[d])
                if bad:
                    why = "a record cannot be rotated"
                    where += [(LINE[w], k) for w in bad]
                    continue
                c = e.clone()
                c.set_cursors(self.o[d].cursors())    # the four position rows keep the destination's values
                for w in (0, 1):
                    if prog.ring[w] and rot[w] and BREAK() != "rotated_load_unrotated":
                        c.set_tram(w, 0, np.roll(self.line_of(e, w), rot[w]))      # slot (j + d) mod Z takes the record's slot j
                new[d] = (c, any(rot))
        return ({}, why, where) if why else (new, None, [])

    def window_slots(self, o, w, first, n_words, logical):
        """the slots of words first .. first + n_words - 1 of line w in one oracle: slot k, or with FXB_TRAM_LOGICAL the header's
        formula from the oracle's own write position"""
        if not logical:
            return np.arange(first, first + n_words, dtype=np.int64)
        p = o.cursors()[2 * w]
        return np.array([self.prog.slot(w, p, first + j) for j in range(n_words)], dtype=np.int64)

    def model_set_window(self, o, w, slots, words):
        if slots.size:
            line = self.line_of(o, w)
            line[slots] = words
            o.set_tram(w, 0, line)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def run(seed, verbose=False, edit=None, device=True, cover=None, probe=None):
    """one sequence; True when everything compared was equal (or the sequence left the parity domain), False on a mismatch.
    probe(kind, handle, ...) is called with what the model did for a copy and for a record loaded back at once (the model's own
    consistency is checked through it, tests/test_voice_sequences_model.py); edit: a function text -> text applied to the generated
    program, as in tools/fuzz_api.py"""
    cover = COVER if cover is None else cover
    wild = os.environ.get("FX_FUZZ_WILD") == "1"
    shards = int(os.environ.get("FX_FUZZ_SHARDS", "1"))
    was = fuzz_api.WILD
    fuzz_api.WILD = False      # (value() below draws the same numbers whatever the environment was when fuzz_api was imported)
    try:
        return _run(seed, verbose, device, cover, wild, shards, probe, edit)
    except LeftDomain:
        cover["left_domain"] += 1
        return True
    except Mismatch as e:
        print("MISMATCH seed %d: %s" % (seed, e))
        return False
    finally:
        fuzz_api.WILD = was


def _run(seed, verbose, device, cover, wild, shards, probe, edit):
    rng = np.random.default_rng(990000 + seed)
    gen = int(os.environ.get("FX_FUZZ_GEN", seed % 4))
    text, options = generate(seed, rng, gen)
    if edit:
        text = edit(text)      # (tools/fuzz_api_reduce.py <seed> voices deletes instructions with it)
    prog = Program(text, options)
    cover["sequences"] += 1
    if not prog.loads:
        return True
    cover["loaded"] += 1
    N = int(rng.choice([1, 63, 64, 65, 130, 200]))
    extra = [int(v) for v in rng.permutation(N)[:int(rng.integers(2, 10))]]
    tracked = list(dict.fromkeys([0, N - 1, N // 2] + extra))[:MAX_TRACKED]
    H = Handle(prog, N, sorted(tracked), device, shards)
    cover["sharded_handles"] += int(H.sharded)
    handles = [H]
    records = []      # (entries: [oracle clone or None], image or None)
    pool = prog.names if len(prog.names) <= 8 else list(dict.fromkeys(prog.controls + [str(v) for v in rng.choice(prog.names, size=6, replace=False)] + ["out", "ccr"]))
    step = -1
    ran_staged = []      # (not empty: a block of this sequence ran as a pipeline of stages)
    tracks_from = int(os.environ.get("FX_FUZZ_TRACKS_FROM", "0"))
    if verbose:
        print(text)
        print("N", N, "tracked", H.tracked, "names", pool, "A", prog.A, "Z", prog.Z, "ring", prog.ring, "tram_ops", prog.tram_ops, "dane", prog.dane)

    def say(*a):
        if verbose:
            print("  ", *a)

    def word(key):
        """a register value of a list set (wild: not for the operand of a LOG / EXP, which would leave the parity domain at once)"""
        if wild and rng.uniform() < 0.25 and key not in prog.lut_inputs:
            return float(WILD_WORDS.view(np.float32)[int(rng.integers(0, WILD_WORDS.size))])
        return value(rng)

    def window(shape):
        v = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
        if wild:
            every = np.concatenate([WILD_WORDS, WILD_TRAM_ONLY])
            hit = rng.uniform(size=shape) < 0.25
            v.view(np.uint32)[hit] = every[rng.integers(0, every.size, size=int(hit.sum()))]
        elif v.size and rng.integers(0, 3) == 0:
            v.reshape(-1)[int(rng.integers(0, v.size))] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]   # a payload in every mode
        return v

    def draw_list(h, kmax=6, distinct=True, only_tracked=False):
        """global instance numbers: mostly tracked ones, any order; now and then long (more than one wavefront of entries)"""
        if not only_tracked and distinct and rng.uniform() < 0.12:
            L = rng.permutation(h.N)[:int(rng.integers(1, h.N + 1))]
        else:
            count = int(rng.integers(1, kmax + 1))
            L = []
            for _ in range(count):
                n = int(rng.choice(h.tracked)) if only_tracked or rng.uniform() < 0.75 else int(rng.integers(0, h.N))
                if not distinct or n not in L:
                    L.append(n)
            L = np.array(L)
        if rng.integers(0, 2):
            L = np.sort(L)
        return [int(v) for v in L]

    def outside(h):
        return int(rng.choice([h.N, -1, h.N + 64, 2 ** 40]))

    def refused(h, kind, call, *reasons):
        """a call the model refuses: the device must return the error and (checked by the state read that follows) change nothing"""
        cover[kind][1] += 1
        say(kind, "REFUSED by the model:", *reasons)
        if h.b is None:
            return
        try:
            call()
        except (RuntimeError, KeyError) as e:
            say("  device:", str(e)[:160])
            return str(e)
        raise Mismatch("step %d %s: the device accepted a call the header refuses (%s)" % (step, kind, reasons))

    def accepted(h, kind, call):
        cover[kind][0] += 1
        if h.b is None:
            return None
        try:
            return call()
        except (RuntimeError, KeyError) as e:
            raise Mismatch("step %d %s: the device refused a call the header accepts: %s" % (step, kind, e))

    def state_read(h, why):
        """every named register and ccr, positions, the first min(A, 64) slots of both lines, LFSR words, counter of every tracked instance"""
        if h.b is None:
            return
        b, T = h.b, h.tracked
        names = prog.names
        got = b.get_registers_list(names, T)
        img = b.save_state()
        hdr = np.frombuffer(img[:64].tobytes(), dtype=np.int32)
        rows = img[64:64 + int(hdr[6]) * h.N * 4].view(np.uint32).reshape(int(hdr[6]), h.N)
        nregs = int(hdr[5])
        trams = [b.get_tram_list(w, T, 0, min(prog.A[w], 64)) if prog.A[w] > 0 else None for w in (0, 1)]
        for i, n in enumerate(T):
            o = h.o[n]
            for k, r in enumerate(names):
                gb, rb = int(got[k, i:i + 1].view(np.uint32)[0]), o.get_register_word(r)
                if gb != rb:
                    raise Mismatch("step %d (%s) REGISTER %s[%d] device %08x oracle %08x kernel %d" % (step, why, r, n, gb, rb, b.info("kernel")))
            if b.get_cursors_i(n) != o.cursors():
                raise Mismatch("step %d (%s) POSITIONS [%d] device %s oracle %s" % (step, why, n, b.get_cursors_i(n), o.cursors()))
            for w in (0, 1):
                if trams[w] is not None and not np.array_equal(bits(trams[w][i]), bits(o.tram(w, trams[w].shape[1]))):
                    raise Mismatch("step %d (%s) %s [%d] device %s oracle %s" % (step, why, LINE[w], n, ["%08x" % v for v in bits(trams[w][i])[:12]],
                                                                                 ["%08x" % v for v in bits(o.tram(w, trams[w].shape[1]))[:12]]))
            lfsr = [int(v) for v in rows[nregs + 1 + 4: nregs + 1 + 6, n].view(np.int32)]
            if lfsr != o.lfsr():
                raise Mismatch("step %d (%s) LFSR [%d] device %s oracle %s" % (step, why, n, lfsr, o.lfsr()))
            if b.instruction_counter_i(n) != o.instruction_counter():
                raise Mismatch("step %d (%s) COUNTER [%d] device %d oracle %d" % (step, why, n, b.instruction_counter_i(n), o.instruction_counter()))

    def block(h, S, plans=(), lists=()):
        xs = h.take(S)
        cover["blocks"] += 1
        if plans or lists:
            h.trackable = True
        else:
            cover["plain_blocks"][int(h.trackable)] += 1
        y = h.b.process_block(xs) if h.b is not None else None
        if h.b is not None:
            cover["kernels"][h.b.info("kernel")] = cover["kernels"].get(h.b.info("kernel"), 0) + 1      # (FXB_INFO_KERNEL: the tier the block ran on)
        if h.b is not None and "staged_blocks" in cover:
            staged, sb = h.b.info("waves_per_wg") >= 2, cover["staged_blocks"]
            sb["scheduled" if plans or lists else "plain"][int(staged)] += 1
            if staged:
                sb["kernels"][h.b.info("kernel")] = sb["kernels"].get(h.b.info("kernel"), 0) + 1
                sb["sequences"] += int(not ran_staged)
                ran_staged.append(seed)
        for n in h.tracked:
            o = h.o[n]
            if not plans and not lists:
                ref = o.process_block(xs[:, n].copy())
            else:
                ref = np.empty(S, dtype=np.float32)
                for t in range(S):
                    for name, period, vals in plans:
                        if t % period == 0 and t // period < vals.shape[0]:
                            v = vals[t // period]
                            o.set_register(name, float(v if vals.ndim == 1 else v[n]))
                    for name, first, period, vals, where in lists:
                        if n in where and t >= first and (t - first) % period == 0 and (t - first) // period < vals.shape[0]:
                            o.set_register(name, float(vals[(t - first) // period, where[n]]))
                    ref[t] = o.process_block(xs[t:t + 1, n].copy())[0]
            if o.ood_flags():
                raise LeftDomain()
            if y is not None and not same(ref, y[:, n]):
                rb, yb = bits(ref), bits(y[:, n])
                at = int(np.nonzero(rb != yb)[0][0])
                raise Mismatch("step %d block of %d samples, instance %d, sample %d: oracle %08x device %08x; kernel %d" % (step, S, n, at, rb[at], yb[at], h.b.info("kernel")))
        for name, period, vals in plans:      # a broadcast schedule is a row of broadcast writes: its last applied step is the register's broadcast value
            if vals.ndim == 1:
                h.broadcast[name] = float(vals[min(vals.shape[0] - 1, (S - 1) // period)])

    def save(h, L):
        say("save_instances", L, "-> record", len(records))
        image = accepted(h, "save", lambda: h.b.save_instances(L))
        records.append(([h.o[n].clone() if n in h.o else None for n in L], image, list(L), handles.index(h), h.pos))
        records[:] = records[-5:]

    def mark():
        # where the random stream stands: a run with the device and a run of the model alone must draw the same numbers, step by
        # step (the GPU tests compare this digest and every count with the model-only run of the same range)
        cover["stream"] = zlib.crc32(repr((seed, step, rng.bit_generator.state["state"])).encode(), cover["stream"])

    for step in range(STEPS):
        mark()
        if verbose:
            for k, h in enumerate(handles):
                try:
                    state_read(h, "BEFORE the step, handle %d" % k)
                except Mismatch as e:
                    print("  ", e)
            print("step", step, "kernel", H.b.info("kernel") if H.b is not None else "-")
        h = handles[int(rng.integers(0, len(handles)))] if rng.uniform() < 0.3 else H
        b = h.b
        op = int(rng.integers(0, 100))
        refuse = rng.uniform() < 0.22
        if op < 20:
            S = int(rng.choice([1, 3, 8, 16, 33, 40]))
            say("block", S, "handle", handles.index(h))
            block(h, S)
        elif op < 24:
            # register writes as tools/fuzz_api.py draws them, and the noise seeds of one instance
            how = int(rng.integers(0, 4))
            name = str(rng.choice(pool))
            if how == 0:
                v = value(rng)
                say("set_register", name, v)
                if b is not None:
                    b.set_register(name, v)
                for o in h.o.values():
                    o.set_register(name, v)
                h.broadcast[name] = v
            elif how == 1:
                n, v = int(rng.choice(h.tracked)), value(rng)
                say("set_register_i", name, n, v)
                if b is not None:
                    b.set_register_i(name, n, v)
                h.o[n].set_register(name, v)
            elif how == 2:
                vals = np.array([value(rng) for _ in range(h.N)], dtype=np.float32)
                say("set_register_array", name)
                if b is not None:
                    b.set_register_array(name, vals)
                for n in h.tracked:
                    h.o[n].set_register(name, float(vals[n]))
            else:
                n = int(rng.choice(h.tracked))
                s1, s2 = int(rng.integers(-2 ** 31, 2 ** 31)), int(rng.integers(-2 ** 31, 2 ** 31))
                say("seed_noise_i", n)
                if b is not None:
                    b.seed_noise_i(n, s1, s2)
                h.o[n].seed_noise(s1, s2)
        elif op < 26:
            # (every draw of a step is made whether or not there is a device: the model alone must walk the same sequence)
            n_samples, wait = int(rng.choice([1, 8, 40])), bool(rng.integers(0, 2))
            say("prepare", n_samples, wait)
            if b is not None:
                b.prepare(n_samples, wait)
        elif op < 32 and step < tracks_from:
            # (FX_FUZZ_TRACKS_FROM: a register that has had a schedule stays trackable for the life of the handle, and code with a
            # trackable register is not cut into stages - the staged range keeps its schedules for the later steps)
            S = int(rng.choice([1, 5, 16, 33]))
            say("block", S, "in place of a scheduled one, handle", handles.index(h))
            block(h, S)
        elif op < 32:
            # dense tracks and list schedules of one block (fuzz_api op 12); a list schedule on a register the program itself can
            # change is refused and arms nothing
            S = int(rng.choice([1, 5, 16, 33]))
            plans, lists = [], []
            names = [r for r in pool if r != "ccr"]
            for name in rng.choice(names, size=int(rng.integers(0, min(len(names), 3) + 1)), replace=False):
                period = int(rng.choice([1, 2, 3, 8]))
                steps = int(rng.integers(1, S // period + 3))
                shape = (steps,) if rng.integers(0, 2) else (steps, h.N)
                vals = np.array([value(rng) for _ in range(int(np.prod(shape)))], dtype=np.float32).reshape(shape)
                if b is not None:
                    b.set_register_track(str(name), vals, period)
                plans.append((str(name), period, vals))
                say("track", name, "period", period, "steps", steps, "per-instance" if vals.ndim == 2 else "broadcast")
            free = [r for r in dict.fromkeys(prog.controls + names) if r not in [p[0] for p in plans]]
            for name in free[:int(rng.integers(1, 3))]:
                L = draw_list(h)
                first, period = int(rng.integers(0, S + 2)), int(rng.choice([1, 2, 3, 8]))
                steps = int(rng.integers(1, S // period + 3))
                vals = np.array([[word(name) for _ in L] for _ in range(steps)], dtype=np.float32)
                call = lambda: b.set_register_tracks_list(name, L, vals, first=first, period=period)
                if name in prog.changed:
                    refused(h, "tracks_list", call, "a register the program itself can change", name)
                else:
                    say("list schedule", name, "first", first, "period", period, "steps", steps, "voices", L)
                    accepted(h, "tracks_list", call)
                    lists.append((name, first, period, vals, {n: k for k, n in enumerate(L) if n in h.o}))
            say("block with schedules", S)
            block(h, S, plans, lists)
        elif op < 40:
            keys = [str(v) for v in rng.choice(pool, size=int(rng.integers(1, min(4, len(pool)) + 1)), replace=False)]
            L = draw_list(h)
            if refuse:
                if len(L) >= 2 and rng.integers(0, 3) == 0:
                    L[-1], why = L[0], "an instance listed twice"
                elif rng.integers(0, 2):
                    keys, why = keys + [keys[0]], "two keys that name one register"
                else:
                    L[int(rng.integers(0, len(L)))], why = outside(h), "an instance outside 0..N-1"
            vals = np.array([[word(key) for _ in L] for key in keys], dtype=np.float32)
            call = lambda: b.set_registers_list(keys, L, vals)
            if refuse:
                refused(h, "set_registers_list", call, why)
                state_read(h, "after a refused set_registers_list")
            else:
                say("set_registers_list", keys, L)
                accepted(h, "set_registers_list", call)
                h.model_set_registers(keys, L, vals)
        elif op < 44:
            keys = [str(v) for v in rng.choice(pool, size=int(rng.integers(1, 5)))]
            L = draw_list(h, distinct=False)
            if refuse:
                L[int(rng.integers(0, len(L)))] = outside(h)
                refused(h, "get_registers_list", lambda: b.get_registers_list(keys, L), "an instance outside 0..N-1")
            else:
                say("get_registers_list", keys, L)
                got = accepted(h, "get_registers_list", lambda: b.get_registers_list(keys, L))
                for k, key in enumerate(keys):
                    for i, n in enumerate(L):
                        if got is not None and n in h.o and int(got[k, i:i + 1].view(np.uint32)[0]) != h.o[n].get_register_word(key):
                            raise Mismatch("step %d get_registers_list %s[%d] device %08x oracle %08x" % (step, key, n, int(got[k, i:i + 1].view(np.uint32)[0]), h.o[n].get_register_word(key)))
        elif op < 52:
            # copy: a destination that is tracked takes a tracked source (the model has to know what arrives)
            dst = draw_list(h, kmax=5)
            src = []
            for d in dst:
                cands = [n for n in (h.tracked if d in h.o or rng.uniform() < 0.7 else range(h.N)) if n not in dst]
                src.append(int(rng.choice(cands)) if cands else None)
            if None in src:
                refuse = True      # (N == 1, or every tracked instance is a destination: only a refusal can be drawn)
                src = [s if s is not None else dst[0] for s in src]
                why = "a destination among the sources"
            elif refuse:
                if len(dst) >= 2 and rng.integers(0, 2):
                    dst[-1], why = dst[0], "a repeated destination"
                else:
                    src[int(rng.integers(0, len(src)))], why = dst[0], "a destination among the sources"
            call = lambda: b.copy_instances(src, dst)
            if refuse:
                refused(h, "copy", call, why, src, dst)
                state_read(h, "after a refused copy")
            else:
                say("copy_instances", src, "->", dst)
                accepted(h, "copy", call)
                h.model_copy(src, dst)
                if probe:
                    probe("copy", h, [(s, d) for s, d in zip(src, dst) if d in h.o])
        elif op < 58:
            L = draw_list(h)
            if refuse:
                L[int(rng.integers(0, len(L)))] = outside(h)
                refused(h, "reset", lambda: b.reset_instances(L), "an instance outside 0..N-1")
                state_read(h, "after a refused reset")
            else:
                say("reset_instances", L)
                accepted(h, "reset", lambda: b.reset_instances(L))
                h.model_reset(L)
        elif op < 64:
            L = draw_list(h, distinct=bool(rng.integers(0, 4)), only_tracked=bool(rng.integers(0, 5)))
            if refuse:
                L[int(rng.integers(0, len(L)))] = outside(h)
                refused(h, "save", lambda: b.save_instances(L), "an instance outside 0..N-1")
            else:
                save(h, L)
        elif op < 80:
            rotated = op >= 72
            at_once = False
            kind = "load_rotated" if rotated else "load"
            if op % 4 == 0 and len(handles) == 1:
                # a second handle of the same program that has run another number of samples (another instance count, other inputs)
                N2 = int(rng.choice([1, 63, 64, 65, 130, 200]))
                h2 = Handle(prog, N2, sorted(set([0, N2 - 1, N2 // 2])), device, shards, first_sample=5000)
                handles.append(h2)
                cover["sharded_handles"] += int(h2.sharded)
                cover["second_handles"] += 1
                say("second handle, N", N2)
                block(h2, int(rng.integers(1, 41)))
            if len(handles) > 1 and rng.uniform() < 0.4:
                h = handles[1]
                b = h.b
            usable = [r for r in records if prog.tram_ops == 0 or None not in r[0]]
            if not rotated and rng.uniform() < 0.6:
                # a plain load wants the positions the destination holds now: a record of this handle that no block has aged, taken
                # here if there is none (undo before further processing; in a program whose lines move uniformly, also a move to
                # other instances)
                fresh = [r for r in usable if handles[r[3]] is h and r[4] == h.pos]
                if not fresh:
                    save(h, draw_list(h, only_tracked=True))
                    fresh = records[-1:]
                    at_once = True
                usable = fresh
            if not usable:
                continue
            entries, image, saved_from, saved_on, _ = usable[int(rng.integers(0, len(usable)))]
            if rng.integers(0, 2) and handles[saved_on] is h and len(set(saved_from)) == len(saved_from):
                dst = list(saved_from)                   # back where they came from: undo
            else:
                free_t, free_u = [int(v) for v in rng.permutation(h.tracked)], [int(v) for v in rng.permutation(h.untracked())]
                dst = []
                for e in entries:
                    # (where delay-line instructions run the header decides by the destination's positions: a tracked one)
                    into = free_u if e is None else (free_t if prog.tram_ops > 0 or not free_u or rng.uniform() < 0.8 else free_u)
                    dst.append(into.pop() if into else None)
                if None in dst:
                    continue
            if refuse and (rng.integers(0, 2) or prog.dane):      # (the DANE model has no phases that disagree: its refusals are these)
                dst[int(rng.integers(0, len(dst)))] = outside(h)
                call = (lambda: b.load_instances_rotated(dst, image)) if rotated else (lambda: b.load_instances(dst, image))
                refused(h, kind, call, "an instance outside 0..N-1")
                state_read(h, "after a refused " + kind)
                continue
            call = (lambda: b.load_instances_rotated(dst, image)) if rotated else (lambda: b.load_instances(dst, image))
            new, why, where = h.model_load(entries, dst, rotated)
            if why:
                msg = refused(h, kind, call, why, where)
                if rotated and msg is not None and not any(line in msg and "entry %d" % k in msg for line, k in where):
                    raise Mismatch("step %d load_instances_rotated: the error does not name a line and list entry the header refuses (%s): %s" % (step, where, msg))
                state_read(h, "after a refused " + kind)
            else:
                say(kind, "record of", saved_from, "->", dst, "handle", handles.index(h))
                accepted(h, kind, call)
                if probe and at_once and dst == saved_from:
                    probe("loaded_back_at_once", h, [(h.o[d], c) for d, (c, _) in new.items()])
                for d, (c, moved) in new.items():
                    cover["rotated_nonzero"] += int(moved)
                    h.o[d] = c
        elif op < 95:
            get = op >= 89
            kind = "get_tram_list" if get else "set_tram_list"
            w = int(rng.integers(0, 2))
            logical = bool(rng.integers(0, 2))
            Aw, Z = prog.A[w], prog.Z[w]
            L = draw_list(h, distinct=not get)
            why = None
            if logical and not prog.ring[w]:
                why = "FXB_TRAM_LOGICAL on a line that is no ring or that the program does not have"
                first, n_words = 0, 1
            elif logical:
                first = int(rng.choice([0, Z - 1, int(rng.integers(0, Z))]))
                n_words = int(rng.choice([1, Z, Z, int(rng.integers(1, Z + 1))]))
            else:
                first = int(rng.choice([0, Aw, int(rng.integers(0, Aw + 1))]))
                n_words = int(rng.choice([0, Aw - first, int(rng.integers(0, Aw - first + 1))]))
            if refuse and why is None:
                how = int(rng.integers(0, 3))
                if how == 0 and logical:
                    first, n_words, why = [(Z, 1), (0, Z + 1), (0, 0), (-1, 1)][int(rng.integers(0, 4))] + ("a logical window outside 0 <= first < Z, 1 <= n_words <= Z",)
                elif how == 0:
                    first, n_words, why = [(Aw, 1), (0, Aw + 1), (-1, 1), (Aw + 1, 0)][int(rng.integers(0, 4))] + ("a window outside 0 <= first, first + n_words <= A",)
                elif how == 1 and not get and len(L) >= 2:
                    L[-1], why = L[0], "an instance listed twice in a set"
                else:
                    L[int(rng.integers(0, len(L)))], why = outside(h), "an instance outside 0..N-1"
            broadcast = (not get) and bool(rng.integers(0, 3) == 0)
            vals = None if get else window((n_words,) if broadcast else (len(L), n_words))
            call = (lambda: b.get_tram_list(w, L, first, n_words, logical=logical)) if get else (lambda: b.set_tram_list(w, L, first, vals, logical=logical))
            if why is not None:
                refused(h, kind, call, why, LINE[w], "first", first, "n_words", n_words, "logical" if logical else "physical")
                state_read(h, "after a refused " + kind)
                continue
            say(kind, LINE[w], L, "first", first, "n_words", n_words, "logical" if logical else "physical", "broadcast" if broadcast else "")
            got = accepted(h, kind, call)
            wraps = False
            for i, n in enumerate(L):
                if n not in h.o:
                    continue
                o = h.o[n]
                slots = h.window_slots(o, w, first, n_words, logical)
                wraps = wraps or (logical and n_words > 1 and bool(np.any(np.abs(np.diff(slots)) != 1)))
                if get:
                    ref = h.line_of(o, w)[slots] if n_words else np.zeros(0, np.float32)
                    if got is not None and not np.array_equal(bits(got[i]), bits(ref)):
                        raise Mismatch("step %d get_tram_list %s instance %d first %d n_words %d %s: device %s oracle %s" % (
                            step, LINE[w], n, first, n_words, "logical" if logical else "physical", ["%08x" % v for v in bits(got[i])[:12]], ["%08x" % v for v in bits(ref)[:12]]))
                else:
                    h.model_set_window(o, w, slots, vals if broadcast else vals[i])
            if wraps:
                cover["logical_wrap"] += 1
        else:
            say("state read")
            cover["state_reads"] += 1
            state_read(h, "state read")
    step = STEPS
    mark()
    for h in handles:
        state_read(h, "the end of the sequence")
    return True


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    if len(sys.argv) > 3 and sys.argv[3] == "verbose":
        return 0 if run(first, True) else 1
    cover = new_cover(stages=True)
    bad = [s for s in range(first, first + count) if not run(s, cover=cover)]
    print("voice fuzz:", count, "sequences (%d programs loaded, %d left the parity domain), failures" % (cover["loaded"], cover["left_domain"]), bad)
    print("  accepted / refused:", {k: tuple(cover[k]) for k in KINDS}, "rotated loads with d != 0:", cover["rotated_nonzero"], "logical windows that wrap:", cover["logical_wrap"], "blocks by kernel:", cover["kernels"],
          "blocks by stages [one wavefront, a pipeline]:", cover["staged_blocks"])
    return 1 if bad or cover["loaded"] < count // 2 else 0


if __name__ == "__main__":
    sys.exit(main())
