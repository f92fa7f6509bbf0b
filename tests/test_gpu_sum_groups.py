"""Sum groups of the quiet loop on the device (fx_xlate.hpp SumGroup): N = 130 - two wavefronts and a tail of
two lanes - blocks of 2, 3 and 40 samples, one oracle per instance; outputs, registers, delay memory, cursors and instruction
counters bit for bit (test_gpu_quiet_states.Watch), FXB_INFO_XLATE_QUIET_LEFT as Watch predicts it, and
FXB_INFO_XLATE_QUIET_REPAIRS as a float32 numpy model of the PROGRAM TEXT predicts it - never from the code under test.

The prediction: at the head of every sample the model takes each lane's registers from its oracle, runs the program's instructions
in float32 (fp32 multiply, fp32 add, saturation; INTERP in fp64) and looks at the unsaturated value of every link.  A wavefront
that runs the sample in the quiet loop repairs a group when a lane WITH an instance holds a watched sum above the chain's T, a
start above T where the plan watches the start, or - the value a repair of the group in front left - an end of that group above T.
Only the plan's groups, watch marks and T come from the library (the plan is checked on its own in test_xlate_sum_groups.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fx8010_programs as progs
from sum_group_programs import DIRECTED, EDGE, EDGE_REGS
from test_gpu_quiet_states import Watch, bits, channels_of, handle, noise
from test_xlate_quiet import MACS, SLOTS, front_end, tight_states

pytestmark = pytest.mark.gpu

CONFIG5 = progs.CONFIGS["config5"]()
PROGRAMS = dict([("config5", CONFIG5)] + DIRECTED + [EDGE])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
ONE = np.float32(1.0)


@pytest.fixture
def translated(monkeypatch):
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(k, raising=False)
    # (the directed programs have no delay line: a batch this small would cut them into stages, which have no quiet loop)
    monkeypatch.setenv("FX_STAGES", "1")


# ------------------------------------------------------------------------------------------------ the model of the program text
class TextModel:
    """the arithmetic instructions of a program text, in order, for whole columns of lanes"""

    def __init__(self, text):
        self.controls, self.instr, self.reads, self.inputs = {}, [], [], []
        for line in text.split("\n"):
            t = line.split()
            if not t:
                continue
            if t[0] == "control":
                self.controls[t[1]] = np.float32(float(t[3]))
            elif t[0] == "input":
                self.inputs.append(t[1])
            elif t[0] in ("macs", "macsn", "acc3", "interp"):
                self.instr.append((t[0],) + tuple(x.strip() for x in line.split(None, 1)[1].split(",")))
            elif t[0] in ("xdelay", "idelay") and t[1].startswith("read"):
                self.reads.append(line.split(",")[1].strip())

    def sample(self, regs):
        """regs {name: float32 column} at the head of a sample (delay-line reads' registers included) -> per arithmetic
        instruction (|A operand|, |unsaturated result|); regs end as the sample leaves them"""
        lanes = len(next(iter(regs.values())))

        def val(name):
            if name in regs:
                return regs[name]
            if name in self.controls:
                return np.full(lanes, self.controls[name], dtype=np.float32)
            return np.full(lanes, np.float32(float(name)), dtype=np.float32)

        out = []
        for op, r, a, x, y in self.instr:
            A, X, Y = val(a), val(x), val(y)
            if op == "macs":
                u = A + X * Y
            elif op == "macsn":
                u = A - X * Y
            elif op == "acc3":
                u = (A + X) + Y
            else:
                u = ((1.0 - X.astype(np.float64)) * A.astype(np.float64) + (X * Y).astype(np.float64)).astype(np.float32)
            assert u.dtype == np.float32
            out.append((np.abs(A), np.abs(u)))
            res = np.minimum(np.maximum(u, -ONE), ONE)
            regs[r] = res
            # setCCR of the result: 8 zero, 6 / 2 inside (-1, 0) / (0, 1), 16 / 20 exactly +1 / -1 - as a float
            regs["ccr"] = np.select([res == 0, (res < 0) & (res > -1), (res > 0) & (res < 1), res == 1, res == -1], [8.0, 6.0, 2.0, 16.0, 20.0], 0.0).astype(np.float32)
        return out


class SumWatch(Watch):
    """Watch, and the repairs of every launch as TextModel predicts them"""

    def __init__(self, gpu, text, n):
        Watch.__init__(self, gpu, text, range(n), n)
        self.model = TextModel(text)
        fe = front_end(text)
        plan = fe.quiet_plan(128)
        self.groups = plan["sum_groups"]
        arithmetic = [i for i, w in enumerate(plan["records"]) if MACS <= int(w[0]) < SLOTS]
        assert len(arithmetic) == len(self.model.instr), "one record per arithmetic instruction, in order"
        self.instr_of = {rec: k for k, rec in enumerate(arithmetic)}
        self.names = [r for r in self.registers]
        self.fired = []     # (launch, sample, wavefront, group, block length) of every predicted repair
        self.left = []      # (launch, sample, wavefront) of every predicted leave

    def block(self, x, predict=True):
        S = x.shape[0]
        never, leaves = set(), set()
        lanes = sorted(self.o)
        for i in lanes:
            if any(not abs(self.o[i].get_register(r)) <= 1.0 for r in self.bounded):
                never.add(self.wave[i])
        ref = {i: np.empty((S, self.ch), dtype=np.float32) for i in lanes}
        repairs = 0
        self.launch = getattr(self, "launch", -1) + 1
        for s in range(S):
            head = {i: s <= S - 2 and self.wave[i] not in leaves and self.wave[i] not in never for i in lanes}
            regs = {r: np.array([self.o[i].get_register(r) for i in lanes], dtype=np.float32) for r in self.names}
            for c, name in enumerate(self.model.inputs):
                regs[name] = x[s, c, lanes].astype(np.float32)
            out = {i: head[i] and (any(not abs(float(x[s, c, i])) <= 1.0 for c in self.in_channels) or
                                   any(abs(self.o[i].get_register(r)) > b for r, b in self.checked)) for i in lanes}
            for i in lanes:
                ref[i][s] = self.o[i].process_block(np.ascontiguousarray(x[s:s + 1, :, i]).reshape(1, self.ch) if self.ch > 1 else x[s:s + 1, 0, i].copy())
                if head[i] and not out[i]:
                    out[i] = any(not abs(self.o[i].get_register(r)) <= b for r, b in self.reads)
            for i in lanes:
                if out[i] and self.wave[i] not in leaves:
                    leaves.add(self.wave[i])
                    self.left.append((self.launch, s, self.wave[i]))
            # the sample's chain values: the delay-line reads' registers hold what the oracle shows AFTER the sample
            for r in self.model.reads:
                regs[r] = np.array([self.o[i].get_register(r) for i in lanes], dtype=np.float32)
            values = self.model.sample(regs)
            # (the model is no rubber stamp of itself: what it leaves in every register is what the oracle holds behind the sample)
            for r in self.names:
                have = np.array([self.o[i].get_register(r) for i in lanes], dtype=np.float32)
                assert np.array_equal(bits(have), bits(regs[r])), ("the model of the program text and the oracle differ", r, s)
            for wave in sorted({self.wave[i] for i in lanes}):
                cols = [k for k, i in enumerate(lanes) if self.wave[i] == wave]
                if not head[lanes[cols[0]]] or wave in leaves:
                    continue
                for g, group in enumerate(self.groups):
                    T = np.float32(group["threshold"])
                    over = np.zeros(len(cols), dtype=bool)
                    for rec, w in zip(group["links"], group["watched"]):
                        if w:
                            over |= values[self.instr_of[rec]][1][cols] > T
                    if group["watch_start"]:
                        over |= values[self.instr_of[group["links"][0]]][0][cols] > T
                    if not group["first"]:
                        over |= values[self.instr_of[self.groups[g - 1]["links"][-1]]][1][cols] > T
                    if over.any():
                        repairs += 1
                        self.fired.append((self.launch, s, wave, g, S))
        self.repairs = repairs
        return ref, len(leaves)


def drive(gpu, name, states_per_block=65, calm_scale=0.125, level=0.9, blocks=(2, 3, 40)):
    """the blocks of test_gpu_quiet_states.test_tight_states on `name`: wavefront 0 (and lane 128 of the tail) from the search's
    tight states, wavefront 1 (and lane 129) calm; everything compared, both counters as predicted"""
    text = PROGRAMS[name]
    N, ch = 130, channels_of(text)
    b = handle(gpu, text, N)
    w = SumWatch(gpu, text, N)
    states = tight_states(name, text, len(blocks) * states_per_block)
    rng = np.random.default_rng(11)
    tight = list(range(64)) + [128]
    calm = list(range(64, 128)) + [129]
    total = 0
    for k, S in enumerate(blocks):
        x = noise(N, S, ch, level, seed=k)
        x[:, :, calm] *= np.float32(calm_scale)
        for j, i in enumerate(tight):
            regs, inputs = states[k * states_per_block + j]
            for r, v in regs.items():
                b.set_register_i(r, i, v)
                w.set(i, r, v)
            for c, v in inputs.items():
                x[0, c, i] = v
        if k == 0:
            for i in calm:
                for r, bound in w.checked:
                    v = float(np.float32(rng.uniform(-1.0, 1.0) * bound / 8))
                    b.set_register_i(r, i, v)
                    w.set(i, r, v)
        _, left = w.run(b, x, "%s block %d" % (name, k))
        got_left, got_repairs = b.info("xlate_quiet_left"), b.info("xlate_quiet_repairs")
        print(name, "block of", S, "left", got_left, "predicted", left, "repairs", got_repairs, "predicted", w.repairs)
        assert got_left == left, (name, k, S)
        assert got_repairs == w.repairs, (name, k, S)
        total += w.repairs
    w.state(b, name)
    assert b.info("xlate_quiet") == 1 and b.info("xlate_sum_groups") == len(w.groups), b.tier_note()
    assert b.info("xlate_sum_links") == sum(len(g["links"]) for g in w.groups)
    b.close()
    return w, total


@pytest.mark.parametrize("name", ["config5"] + [n for n, _ in DIRECTED])
def test_tight_states_repair_as_predicted(gpu, translated, name):
    w, total = drive(gpu, name)
    calm_fired = [f for f in w.fired if f[2] == (0, 1)]
    assert not calm_fired, "the calm wavefront never repairs"
    if not w.groups:
        assert total == 0
        return
    assert total > 0, "the tight states drive a chain above T"
    if name == "config5":
        last = len(w.groups) - 1
        mine = [f for f in w.fired if f[2] == (0, 0)]
        assert any(f[3] == 0 for f in mine), "the first group of a sample"
        assert any(f[3] == last for f in mine), "the last group of a sample"
        per_sample = {}
        for f in mine:
            per_sample[f[:2]] = per_sample.get(f[:2], 0) + 1
        assert max(per_sample.values()) >= 2, "two groups of one sample"
        assert any(f[1] == 0 for f in mine), "the first sample of a launch"
        assert any(f[1] == f[4] - 2 for f in mine), "the last sample of a block that the loop runs"


def test_a_run_at_benchmark_like_levels_never_repairs(gpu, translated):
    """config5 from a fresh handle at the benchmark's stimulus: no repair, nobody leaves"""
    N = 130
    b = handle(gpu, CONFIG5, N)
    w = SumWatch(gpu, CONFIG5, N)
    for k, S in enumerate((3, 40)):
        x = np.ascontiguousarray(progs.stimulus(N, S).reshape(S, 1, N))
        _, left = w.run(b, x, "benchmark stimulus, block %d" % k)
        assert w.repairs == 0 and left == 0
        assert b.info("xlate_quiet_repairs") == 0 and b.info("xlate_quiet_left") == 0
    w.state(b)
    b.close()


# ------------------------------------------------------------------------------------------------ edge values
def test_edge_values_in_lanes_of_their_own(gpu, translated):
    """edge_values: a = e0, a += e_k / 4 (k = 1 .. 12, idle), a += e_k / 32 (k = 13 .. 24, the kept chain); its start is watched and
    every value is a sum of a few powers of two.  In the 128-register build a group holds four covered sums, so T is the largest
    float with fl(T + 4 / 32) <= 1: the float above 0.875 (the sum rounds to even, down to 1.0).  One case per launch, in a
    lane of its own: the start exactly T (no repair), the next float above (repair) and below (none), exactly +-1.0 (repair; the
    bits stay), -0.0 carried through the whole chain, denormal addends, covered sums that climb from T to exactly 1.0."""
    name, text = EDGE
    fe = front_end(text)
    groups = fe.quiet_plan(128)["sum_groups"]
    assert groups and groups[0]["watch_start"]
    T = np.float32(groups[0]["threshold"])
    assert T == np.nextafter(np.float32(0.875), np.float32(2)), T
    tiny = float(np.array([1], dtype=np.uint32).view(np.float32)[0])
    quarter = {"e%d" % k: 0.25 for k in range(0, 11)}             # a = 0.875 behind the idle links
    at_t = dict(quarter, e11=2.0 ** -22)                           # + 2^-24: exactly T
    cases = {
        0: at_t,
        1: dict(quarter, e11=2.0 ** -21),                          # one float above T: repairs
        2: dict(quarter),                                          # 0.875: one float below
        3: {"e%d" % k: 0.25 for k in range(0, 13)},                # exactly 1.0 at the start of the kept chain
        4: {"e%d" % k: -0.25 for k in range(0, 13)},
        5: {"e%d" % k: -0.0 for k in range(EDGE_REGS)},            # -0 all the way
        6: dict(at_t, e13=1.0, e14=1.0, e15=1.0, e16=1.0),         # covered sums climb to exactly 1.0; the watched one behind them fires
        7: dict({"e0": tiny}, **{"e%d" % k: 4 * tiny * (-1) ** k for k in range(1, EDGE_REGS)}),
        8: dict({k: -v for k, v in at_t.items()}, e13=-1.0, e14=-1.0, e15=-1.0, e16=-1.0),
        9: dict({"e%d" % k: 0.25 for k in range(0, 13)}, **{"e%d" % k: 1.0 for k in range(13, EDGE_REGS)}),
    }
    # one case per launch, in a lane of its own, on a fresh pair of handle and oracles each: the repair count is that lane's
    for lane, regs in cases.items():
        N = 130
        b = handle(gpu, text, N)
        w = SumWatch(gpu, text, N)
        for r, v in regs.items():
            b.set_register_i(r, lane, v)
            w.set(lane, r, v)
        x = np.zeros((3, 1, N), dtype=np.float32)
        _, left = w.run(b, x, "edge case %d" % lane)
        got = b.info("xlate_quiet_repairs")
        assert b.info("xlate_quiet") == 1 and b.info("xlate_sum_groups") == len(groups), b.tier_note()
        print("edge case", lane, "repairs", got, "predicted", w.repairs, "left", left)
        assert got == w.repairs and b.info("xlate_quiet_left") == left == 0, (lane, got, w.repairs)
        if lane in (0, 2, 5, 7):
            assert got == 0, lane
        if lane in (1, 3, 4):
            assert got >= 1, lane
        w.state(b, "edge case %d" % lane)
        b.close()


# ------------------------------------------------------------------------------------------------ repair, then leave
def test_repair_then_leave(gpu, translated):
    """config5, one block of 40: wavefront 0 starts from the search's tight states and repairs in the first samples; at sample 6 one
    of its lanes hears 1.5, above the head check's bound of the input, and the wavefront leaves for the fast loop - through the
    exit path that stores the pair {sample, repairs so far}.  Wavefront 1 stays calm.  Predicted and asserted: a repair of
    wavefront 0 at a sample before its leave in the same launch, QUIET_LEFT = 1, and QUIET_REPAIRS = the model's count, which is
    all wavefront 0's"""
    N, S, AT = 130, 40, 6
    b = handle(gpu, CONFIG5, N)
    w = SumWatch(gpu, CONFIG5, N)
    states = tight_states("config5", CONFIG5, 65)
    x = noise(N, S, 1, 0.9, seed=0)
    calm = list(range(64, 128)) + [129]
    x[:, :, calm] *= np.float32(0.125)
    for j, i in enumerate(list(range(64)) + [128]):
        regs, inputs = states[j]
        for r, v in regs.items():
            b.set_register_i(r, i, v)
            w.set(i, r, v)
        for c, v in inputs.items():
            x[0, c, i] = v
    x[AT, 0, 5] = 1.5
    _, left = w.run(b, x, "repair, then leave")
    wave0 = (0, 0)
    assert (0, AT, wave0) in w.left and left >= 1
    before = [f for f in w.fired if f[0] == 0 and f[2] == wave0 and f[1] < AT]
    assert before, "wavefront 0 repairs before it leaves"
    assert not [f for f in w.fired if f[2] == wave0 and f[1] >= AT], "no repair is counted once the wavefront runs the fast loop"
    assert [f for f in w.fired if f[2] == (0, 1)] == [], "the calm wavefront never repairs"
    assert b.info("xlate_quiet_left") == left
    assert b.info("xlate_quiet_repairs") == w.repairs >= len(before)
    print("repair then leave: repairs", w.repairs, "of wavefront 0 before sample", AT, ":", len(before), "left", left)
    w.state(b, "repair, then leave")
    # the launch after it enters the loop afresh: both counters start from nothing
    _, left = w.run(b, noise(N, 3, 1, 0.05, seed=2), "the launch after")
    assert b.info("xlate_quiet_left") == left and b.info("xlate_quiet_repairs") == w.repairs
    b.close()


# ------------------------------------------------------------------------------------------------ two shards on one GPU
def test_two_shards_sum_their_repairs(gpu, translated):
    N = 130
    b = handle(gpu, CONFIG5, N, devices=[0, 0])
    w = SumWatch(gpu, CONFIG5, N)
    shards = b.shards()
    w.wave = {}
    for k, (_, first, count) in enumerate(shards):
        for i in range(first, first + count):
            w.wave[i] = (k, (i - first) // 64)
    states = tight_states("config5", CONFIG5, N)
    x = noise(N, 3, 1, 0.9, seed=0)
    for i in range(N):                            # every lane of both shards from a tight state
        regs, inputs = states[i % 60]              # (the best of the search in both shards)
        for r, v in regs.items():
            b.set_register_i(r, i, v)
            w.set(i, r, v)
        for c, v in inputs.items():
            x[0, c, i] = v
    _, left = w.run(b, x, "two shards")
    assert b.info("xlate_quiet_left") == left
    assert b.info("xlate_quiet_repairs") == w.repairs
    assert w.repairs > 0
    print("two shards: repairs", w.repairs, "by shard", sorted({f[2][0] for f in w.fired}))
    assert {f[2][0] for f in w.fired} == {0, 1}, "both shards repair"
    w.state(b)
    b.close()


# ------------------------------------------------------------------------------------------------ switch on and off
def diagnostics_library():
    lib = os.path.join(CSRC, "build", "diag", "libfx8010_amd.so")
    sources = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".cpp", ".hpp", ".hip", ".h", ".S", ".inc"))]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in sources):
        subprocess.check_call(["make", "-s", "-j16", "-C", CSRC, "diag"])
    return lib


CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%(py)r, %(oracle)r]
import fx8010_amd, fx8010_programs as progs
x = np.load(%(x)r)
b = fx8010_amd.Batch(x.shape[2], 1, 0)
assert b.load_text(progs.CONFIGS["config5"]())
for i, v in enumerate(np.load(%(lp)r)):
    b.set_register_i("lp0", int(i), float(v))
y = b.process_block(x)
regs = np.array([[b.get_register_bits_i(r, i) for r in ("m", "u", "v", "out", "lp0", "y7")] for i in range(x.shape[2])], dtype=np.uint32)
np.savez(%(out)r, y=y, regs=regs, hash=np.array([b.info("xlate_code_hash")], dtype=np.int64), groups=np.array([b.info("xlate_sum_groups")]),
         repairs=np.array([b.info("xlate_quiet_repairs")]), left=np.array([b.info("xlate_quiet_left")]))
b.close()
"""


def test_the_switch_off_against_on(gpu, translated, tmp_path):
    """config5, 40 samples, lp0 of wavefront 0 at +-0.25 (the chain repairs): the diagnostics build with FX_XLATE_SUMGROUPS=0 - the
    loop without groups, stream 5 - gives the words of the release library (a fresh process each: a process keeps one library)"""
    N = 130
    x = noise(N, 40, 1, 0.9, seed=5)
    x[:, :, 64:] *= np.float32(0.125)
    lp = np.where(np.arange(N) < 64, 0.25 * (-1.0) ** np.arange(N), 0.0).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "lp.npy", lp)

    def child(out, lib, **env):
        e = dict(os.environ)
        e.pop("FX8010_AMD_LIB", None)
        if lib:
            e["FX8010_AMD_LIB"] = lib
        e.update(env)
        code = CHILD % {"py": os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), "oracle": os.path.join(ROOT, "oracle"),
                        "x": str(tmp_path / "x.npy"), "lp": str(tmp_path / "lp.npy"), "out": str(tmp_path / out)}
        subprocess.run([sys.executable, "-c", code], env=e, check=True, timeout=120)
        return np.load(tmp_path / out)

    on = child("on.npz", None)
    off = child("off.npz", diagnostics_library(), FX_XLATE_SUMGROUPS="0")
    assert int(on["groups"][0]) > 0 and int(off["groups"][0]) == 0
    assert int(on["hash"][0]) != int(off["hash"][0]), "the switch changes the generated code"
    assert int(off["repairs"][0]) == 0 and int(on["left"][0]) == int(off["left"][0])
    for k in ("y", "regs"):
        assert np.array_equal(np.ascontiguousarray(on[k]).view(np.uint8), np.ascontiguousarray(off[k]).view(np.uint8)), k
    print("repairs with groups:", int(on["repairs"][0]), "left:", int(on["left"][0]))
