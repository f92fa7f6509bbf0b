"""Two to four channels on the device, every tier against the oracle: the programs of tests/multichannel_programs.py (the
input-refresh rule through A's channel as csrc/fx_decode.cpp lowers it: aliased inputs, inputs with prefix refreshes, channels
without an input row, output latches nothing writes), the reference's own words for them (tests/golden/multichannel.json), random
multichannel programs, the stage planner's handling of input and output channels, the quiet loop's per-channel input checks and
the launch paths around the kernel.

Inputs differ per instance AND per channel (multichannel_programs.stimulus), so that a word taken from the wrong channel or the
wrong lane shows; every instance is compared with an oracle run of its own: output words, instruction counter, registers, flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fx8010_programs as progs
import multichannel_programs as mc
import quiet_programs
from pyoracle import Oracle
from test_gpu_golden import load as load_golden, run_case, tier  # noqa: F401  (tier: the six tiers of the golden tests)
from test_gpu_parity import bits, k, same_with_nan  # noqa: F401  (k: the nine tiers of the parity tests)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Pair:
    """a handle and one oracle per compared instance, driven side by side"""

    def __init__(self, gpu, channels, text, n, instances=None, devices=None):
        self.n, self.ch, self.text = n, channels, text
        self.b = gpu.Batch(n, channels, 0) if devices is None else gpu.Batch(n, channels, devices=devices)
        assert self.b.load_text(text), self.b.errors()
        self.picks = list(range(n)) if instances is None else list(instances)
        self.o = {}
        for i in self.picks:
            self.o[i] = Oracle(channels)
            assert self.o[i].load_text(text), self.o[i].errors()

    def set_register(self, reg, value, instance=None):
        if instance is None:
            assert self.b.set_register(reg, value) == 0
        else:
            assert self.b.set_register_i(reg, instance, value) == 0
        for i, o in self.o.items():
            if instance in (None, i):
                o.set_register(reg, value)

    def reference(self, x):
        """x: [S, channels, N] -> {instance: [S, channels]}"""
        return {i: o.process_block(np.ascontiguousarray(x[:, :, i])) for i, o in self.o.items()}

    def outputs(self, y, ref, what=""):
        for i, r in ref.items():
            got = np.ascontiguousarray(y[:, :, i])
            bad = np.nonzero(bits(r).reshape(-1) != bits(got).reshape(-1))[0]
            assert bad.size == 0, "%s instance %d: first mismatch at sample %d channel %d: ref %08x got %08x" % (
                what, i, bad[0] // self.ch, bad[0] % self.ch, bits(r).reshape(-1)[bad[0]], bits(got).reshape(-1)[bad[0]])

    def block(self, x, what=""):
        ref = self.reference(x)
        y = self.b.process_block(x)
        self.outputs(y, ref, what)
        return y

    def read_back(self, regs, instances, what=""):
        """the per-instance getter (fxb_get_register_i)"""
        for r in regs:
            for i in instances:
                assert self.b.get_register_bits_i(r, i) == self.o[i].get_register_bits(r), "%s instance %d register %s read on its own" % (what, i, r)

    def state(self, regs, what="", counters=None, in_domain=None):
        """registers (one read per register for all instances), per-instance counters, flags; in_domain: compare only these"""
        picks = [i for i in self.picks if in_domain is None or i in in_domain]
        for r in regs:
            got = bits(self.b.get_register_array(r))
            for i in picks:
                assert int(got[i]) == self.o[i].get_register_bits(r), "%s instance %d register %s: ref %08x got %08x" % (
                    what, i, r, self.o[i].get_register_bits(r), int(got[i]))
        for i in (picks if counters is None else [i for i in counters if i in picks]):
            assert self.b.instruction_counter_i(i) == self.o[i].instruction_counter(), "%s instance %d instruction counter" % (what, i)
        flags = 0
        for o in self.o.values():
            flags |= o.ood_flags()
        if len(self.picks) == self.n:   # the handle's flags are those of all its instances, inside the domain or not
            assert self.b.ood_flags() == flags, "%s flags: ref %x got %x" % (what, flags, self.b.ood_flags())
        if in_domain is None:
            assert flags == 0 and self.b.ood_flags() == 0, what
            if len(self.picks) == self.n:
                assert self.b.instruction_counter() == sum(o.instruction_counter() for o in self.o.values()), what


# ------------------------------------------------------------------------------------------------ the directed programs, every tier
@pytest.mark.parametrize("name", sorted(mc.DIRECTED))
def test_directed_programs(gpu, k, name):
    """130 instances (a ragged last wavefront), 33 samples as blocks of 17 and 16: stale input registers and output latches cross
    a launch.  stale_register: between the blocks the input registers are written - r (read inside a SKIP shadow only) in every
    instance, l (an input with prefix refreshes) and m (an alias of channel 2's row) in single ones - and read back at once;
    every fourth instance then hears a negative channel 0 throughout the second block, so that its SKIP fires in every sample
    and the written r is what the register still holds afterwards."""
    channels, text, regs = mc.DIRECTED[name]
    N, S = 130, 33
    x = mc.stimulus(progs, N, S, channels)
    if name == "stale_register":
        x[17:, 0, ::4] = -np.abs(x[17:, 0, ::4]) - np.float32(0.001)
    p = Pair(gpu, channels, text, N)
    p.block(x[:17], name)
    p.state(regs, name + " after block 1")
    if name == "stale_register":
        p.set_register("r", 0.625)
        p.set_register("l", -0.375, instance=4)
        p.set_register("l", 0.875, instance=65)
        p.set_register("m", 0.3125, instance=129)
        p.set_register("m", -0.75, instance=8)
        p.state(("l", "r", "m"), name + " after the writes", counters=[])
        p.read_back(("l", "r", "m"), (4, 8, 65, 129), name + " after the writes")
    p.block(x[17:], name)
    p.state(regs, name + " after block 2")
    if name == "stale_register":   # the case is what it claims to be: the written word survives exactly where the SKIP always fired
        p.read_back(("l", "r", "m"), (4, 8, 65, 129), name + " after block 2")
        held = [i for i in range(N) if p.o[i].get_register_bits("r") == 0x3F200000]
        assert set(range(0, N, 4)) <= set(held) and len(held) < N // 2, held
    if isinstance(k, str) and k in ("default", "unstaged", "xlate_v256"):
        assert p.b.info("kernel") >= 9, p.b.tier_note()


def test_more_than_four_channels_are_refused(gpu):
    with pytest.raises(RuntimeError):
        gpu.Batch(64, 5, 0)


# ------------------------------------------------------------------------------------------------ the reference's own words
def test_reference_vectors(gpu, tier):
    """tests/golden/multichannel.json through the golden tests' own run_case: the words, registers, counters and loader diagnostics
    of the unmodified reference, without the oracle in between"""
    cases = load_golden("multichannel.json")
    assert len(cases) == 29
    for case in cases:
        run_case(gpu, case)


# ------------------------------------------------------------------------------------------------ random programs
@pytest.mark.parametrize("chunk", range(3))
@pytest.mark.parametrize("kernel", ["default", "asm", "hip"])
def test_generated_programs(gpu, monkeypatch, kernel, chunk):
    """48 programs of multichannel_programs.generated in chunks of 16, 70 instances x 64 samples in two launches; an instance the
    oracle reports outside the parity domain is not compared - and at least 90 % of the runs of a chunk must be compared"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    if kernel != "default":
        monkeypatch.setenv("FX_KERNEL", kernel)
    N, S = 70, 64
    runs = inside = 0
    for seed in range(chunk * 16, chunk * 16 + 16):
        channels, text, regs = mc.generated(seed)
        x = mc.stimulus(progs, N, S, channels, seed=seed)
        p = Pair(gpu, channels, text, N)
        refs = [p.reference(x[:40]), p.reference(x[40:])]
        ok = {i for i, o in p.o.items() if o.ood_flags() == 0}
        runs, inside = runs + N, inside + len(ok)
        what = "seed %d (kernel %d)\n%s\n" % (seed, p.b.info("kernel"), text)
        for ref, y in zip(refs, [p.b.process_block(x[:40]), p.b.process_block(x[40:])]):
            p.outputs(y, {i: r for i, r in ref.items() if i in ok}, what)
        p.state(regs, what, in_domain=ok)
    print("generated multichannel programs, chunk %d on %s: %d of %d runs inside the parity domain" % (chunk, kernel, inside, runs))
    assert 10 * inside >= 9 * runs, (inside, runs)


# ------------------------------------------------------------------------------------------------ stages
STAGED = [("late_reads_staged", mc.DIRECTED["late_reads_staged"]), ("chain0", mc.generated_chain(0)), ("chain1", mc.generated_chain(1))]


def staged_run(gpu, name, asked, N):
    """40 samples - five barrier periods of eight - as blocks of 13 and 27; returns the handle.  With 4 101 instances every output
    word of every instance is compared, registers and counters on a sample of them."""
    channels, text, regs = dict(STAGED)[name]
    x = mc.stimulus(progs, N, 40, channels, seed=3)
    p = Pair(gpu, channels, text, N)
    for lo, hi in ((0, 13), (13, 40)):
        p.block(x[lo:hi], "%s in %d stages, block %d:%d" % (name, asked, lo, hi))
    p.state(regs, name, counters=sorted(set(range(0, N, max(1, N // 40))) | {63, 64, N - 1}))
    f = gpu.FrontEnd(channels)
    assert f.load_text(text)
    try:
        planned = f.translate_staged(asked)[2]
    except RuntimeError as e:
        planned = "refused (%s)" % e
    got = p.b.info("waves_per_wg")
    print("%s, %d instances: %d stage(s) asked, the planner's answer: %s, the handle runs %d (%s)" % (name, N, asked, planned, got, p.b.tier_note()))
    assert p.b.info("kernel") >= 9
    if planned == asked:
        assert got == asked, (name, asked, got, p.b.tier_note())
    return p.b


@pytest.mark.parametrize("N", [67, 4096 + 5])
@pytest.mark.parametrize("asked", [1, 2, 4, 8])
@pytest.mark.parametrize("name", [n for n, _ in STAGED])
def test_programs_in_stages(gpu, monkeypatch, name, asked, N):
    """stage 0 loads every input channel (through the LDS input ring), later stages see an input as a row handed over at a cut,
    every output channel is stored by the stage of its last write"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES_TUNE", "FX_STAGES_GROUP"):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setenv("FX_STAGES", str(asked))
    staged_run(gpu, name, asked, N)


NO_RING_SIZES = {name: (67, 4096 + 5) for name, _ in STAGED}


def no_ring_child():
    """(in a child process that has loaded the diagnostics build) the sweep of test_programs_in_stages without the input ring:
    stage 0 fetches its PCM input in the sample loop itself"""
    import fx8010_amd
    assert os.environ.get("FX_STAGES_NO_RING") == "1" and fx8010_amd.load().fxb_diag_build() == 1
    hashes = []
    for name, _ in STAGED:
        for asked in (1, 2, 4, 8):
            os.environ["FX_STAGES"] = str(asked)
            for N in NO_RING_SIZES[name]:
                hashes.append(staged_run(fx8010_amd, name, asked, N).info("xlate_code_hash"))
    print("HASHES " + " ".join(str(h) for h in hashes))


def test_programs_in_stages_without_the_input_ring(gpu, monkeypatch):
    """FX_STAGES_NO_RING=1 exists in the diagnostics build only (fx_knobs.hpp): one child process with that library runs the whole
    sweep; a second one without the knob shows that the knob changed the staged code"""
    from test_gpu_quiet_frame import diagnostics_library
    lib = diagnostics_library()
    code = "import sys; sys.path[:0] = %r; import test_gpu_multichannel as T; T.no_ring_child()" % (
        [os.path.join(ROOT, "tests"), os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")],)
    env = {key: v for key, v in os.environ.items() if not key.startswith("FX_")}
    env.update(FX8010_AMD_LIB=lib, FX_STAGES_NO_RING="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    print(r.stdout)
    without = [int(h) for h in r.stdout.split("HASHES ")[1].split()]
    with_ring = []
    for name, _ in STAGED:
        for asked in (1, 2, 4, 8):
            monkeypatch.setenv("FX_STAGES", str(asked))
            for N in NO_RING_SIZES[name]:
                channels, text, _ = dict(STAGED)[name]
                b = gpu.Batch(N, channels, 0)
                assert b.load_text(text)
                for S in (13, 27):   # (the child's blocks: the code depends on their lengths)
                    b.process_block(np.zeros((S, channels, N), dtype=np.float32))
                with_ring.append((asked, b.info("waves_per_wg"), b.info("xlate_code_hash")))
    assert len(without) == len(with_ring)
    changed = [h != w[2] for h, w in zip(without, with_ring) if w[1] > 1]
    assert changed and any(changed), "the knob changed no staged code"


# ------------------------------------------------------------------------------------------------ per-channel taint in the quiet loop
TAINT_PROGRAMS = {"stereo": (2, quiet_programs.generated_wide(5, channels=2)), "four_channels": (4, quiet_programs.generated_wide(7, channels=4))}
TAINT_WORDS = {"beyond_one": np.float32(1.5), "nan": np.float32(np.nan), "inf": np.float32(np.inf)}
TAINT_BLOCKS = ((0, 23), (23, 40))
_TAINT = {}


def taint_case(gpu, program, case):
    """(x, per block {instance: reference}, per block the set of wavefronts that leave the quiet loop, registers, final register
    words, counters) - from the oracles alone (test_gpu_quiet_states.Watch and the rule of that module's first lines), computed
    once per program and case and shared by the tiers.

    2 C + 1 full wavefronts and a tail of 8 lanes, all at +-0.1, where every one of them stays in the loop.  Wavefront c < C hears
    ONE bad word, on channel c alone, in the first block (lane 3 + 7 c of it, sample 5 + 3 c); wavefront C + c one on channel c
    alone in the second block (lane 40 + c, sample 30 + c).  So in every tainted wavefront the first and only offending word
    comes in on its own channel while all other channels are clean, and wavefront 2 C and the tail never see one."""
    if (program, case) not in _TAINT:
        from test_gpu_quiet_states import Watch
        channels, text = TAINT_PROGRAMS[program]
        N = 64 * (2 * channels + 1) + 8
        x = (mc.stimulus(progs, N, 40, channels, seed=11) * np.float32(0.1 / 0.9)).astype(np.float32)
        for c in range(channels):
            x[5 + 3 * c, c, 64 * c + 3 + 7 * c] = TAINT_WORDS[case]
            x[30 + c, c, 64 * (channels + c) + 40 + c] = -TAINT_WORDS[case]
        w = Watch(gpu, text, range(N), N)
        assert w.plan["in_force"] and sorted(w.in_channels) == list(range(channels)), w.plan["why"]
        refs, left = [], []
        for lo, hi in TAINT_BLOCKS:
            S, never, leaves = hi - lo, set(), set()
            for i, o in w.o.items():
                if any(not abs(o.get_register(r)) <= 1.0 for r in w.bounded):
                    never.add(i // 64)
            ref = {i: np.empty((S, channels), dtype=np.float32) for i in w.o}
            for s in range(S):
                for i, o in w.o.items():
                    head = s <= S - 2 and i // 64 not in leaves and i // 64 not in never
                    out = head and (any(not abs(float(x[lo + s, c, i])) <= 1.0 for c in w.in_channels) or
                                    any(abs(o.get_register(r)) > bound for r, bound in w.checked))
                    ref[i][s] = o.process_block(np.ascontiguousarray(x[lo + s:lo + s + 1, :, i]))
                    if head and not out:
                        out = any(not abs(o.get_register(r)) <= bound for r, bound in w.reads)
                    if out:
                        leaves.add(i // 64)
            refs.append(ref)
            left.append(leaves)
        regs = [r for r in w.registers if r != "noise"]
        words = {r: np.array([w.o[i].get_register_bits(r) for i in range(N)], dtype=np.uint32) for r in regs}
        counters = [w.o[i].instruction_counter() for i in range(N)]
        assert all(o.ood_flags() == 0 for o in w.o.values())
        _TAINT[(program, case)] = (x, refs, left, regs, words, counters)
    return _TAINT[(program, case)]


@pytest.mark.parametrize("case", sorted(TAINT_WORDS))
@pytest.mark.parametrize("program", sorted(TAINT_PROGRAMS))
def test_one_tainted_channel_per_wavefront(gpu, k, program, case):
    """SKIP-free programs with a quiet loop (quiet_programs.generated_wide with two and with four channels); the input of
    taint_case: one wavefront per channel and block whose only word beyond +-1 / NaN / Inf comes in on that channel.  Every word
    of every lane is the oracle's, NaN words included (same_with_nan, as test_non_finite_values_follow_the_reference applies it on
    every tier), and so are all registers and counters.  On the translated tiers the quiet loop is what ran, and exactly the
    wavefronts the oracles predict left it in either launch: the tainted ones - a channel whose check was missing would keep its
    wavefront in - and never the clean full wavefront or the tail."""
    channels, text = TAINT_PROGRAMS[program]
    x, refs, left, regs, words, counters = taint_case(gpu, program, case)
    N = x.shape[2]
    # the case is what it claims to be
    assert left[0] == set(range(channels)), left
    assert set(range(channels, 2 * channels)) <= left[1] <= set(range(2 * channels)), left
    translated = isinstance(k, str) and k in ("default", "unstaged", "xlate_v256")
    b = gpu.Batch(N, channels, 0)
    assert b.load_text(text), b.errors()
    for (lo, hi), ref, leaves in zip(TAINT_BLOCKS, refs, left):
        y = b.process_block(x[lo:hi])
        for i, r in ref.items():
            assert same_with_nan(r, y[:, :, i], k), "%s %s: instance %d (wavefront %d), block %d:%d" % (program, case, i, i // 64, lo, hi)
        if translated:
            assert b.info("kernel") >= 9 and b.info("xlate_quiet") == 1, b.tier_note()
            assert b.info("xlate_quiet_left") == len(leaves), (program, case, lo, b.info("xlate_quiet_left"), sorted(leaves))
    for r in regs:
        got = bits(b.get_register_array(r))
        bad = np.nonzero(got != words[r])[0]
        assert bad.size == 0, "%s %s register %s instance %d: ref %08x got %08x" % (program, case, r, bad[0], words[r][bad[0]], got[bad[0]])
    for i in sorted(set(range(0, N, 9)) | {64 * w + 3 + 7 * w for w in range(channels)} | {N - 1}):
        assert b.instruction_counter_i(i) == counters[i], i
    assert b.instruction_counter() == sum(counters) and b.ood_flags() == 0
    if case == "nan":   # the bad word does reach an output
        assert any(np.isnan(r).any() for ref in refs for r in ref.values())


# ------------------------------------------------------------------------------------------------ launch paths
@pytest.mark.parametrize("path", ["pitched", "imajor", "two_shards"])
@pytest.mark.parametrize("kernel", ["default", "asm", "hip"])
def test_launch_paths_with_four_channels(gpu, monkeypatch, kernel, path):
    """a_is_literal (four channels, three of them without an input row) through a pitched device block, an instance-major block
    and a handle of two shards on one device: against the plain host path of a handle of the same kind, and against the oracle on
    three instances; state carried over two blocks"""
    import torch
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    if kernel != "default":
        monkeypatch.setenv("FX_KERNEL", kernel)
    channels, text, regs = mc.DIRECTED["a_is_literal"]
    N, S = 130, 33
    x = mc.stimulus(progs, N, S, channels, seed=5)
    devices = [0, 0] if path == "two_shards" else None
    p = Pair(gpu, channels, text, N, instances=(0, 64, N - 1), devices=devices)
    plain = Pair(gpu, channels, text, N, instances=())   # (one device, the host path)
    if path == "two_shards":
        assert len(p.b.shards()) == 2 and sum(s[2] for s in p.b.shards()) == N
    for lo, hi in ((0, 17), (17, S)):
        xb = np.ascontiguousarray(x[lo:hi])
        want = plain.b.process_block(xb)
        ref = p.reference(xb)
        if path == "pitched":
            P = N + 37
            d_in = torch.zeros((hi - lo, channels, P), dtype=torch.float32, device="cuda")
            d_in[:, :, :N] = torch.from_numpy(xb).to("cuda")
            d_out = torch.full((hi - lo, channels, P), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert p.b.process_block_dev_pitched(d_in[:, :, :N], d_out[:, :, :N], hi - lo) == 0
            assert p.b.sync() == 0
            got = d_out.cpu().numpy()
            assert (got[:, :, N:] == -7.0).all(), "words beyond the instances' columns were written"
            y = np.ascontiguousarray(got[:, :, :N])
        elif path == "imajor":
            y = np.ascontiguousarray(p.b.process_block_imajor(np.ascontiguousarray(xb.transpose(2, 0, 1))).transpose(1, 2, 0))
        else:
            y = p.b.process_block(xb)
        assert np.array_equal(bits(y), bits(want)), (path, lo)
        p.outputs(y, ref, path)
    if path == "imajor":
        assert p.b.info("imajor_blocks") == 2
    for r in regs:
        assert np.array_equal(bits(p.b.get_register_array(r)), bits(plain.b.get_register_array(r))), r
    p.state(regs, path)
