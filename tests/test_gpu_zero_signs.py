"""Signed zeros and denormals on the device across the translator's IEEE shortcuts (fx_xlate.cpp zeroAddsOf,
zeroPlusScaled, unit multipliers, the product cache, INTERP's one fma, host-folded records): a wrong one leaves 0x80000000 where
the reference has 0x00000000, or the other way round, or a smallest denormal where the reference has a zero - values ordinary
signals do not produce.  So the states and inputs here are made of them: +0, -0, the three smallest denormals, the largest
denormal and the smallest normal number of either sign, and random values at an eighth of a row's bound.

N = 130 - two wavefronts and a tail of two lanes - one pyoracle.Oracle per instance, blocks of 2, 3 and 40 samples on one handle
(40 exceeds the 37 slots of the programs' xTRAM and the 11 of their iTRAM: what was written to the lines comes back), compared
bit for bit on outputs, every register that is not a control, cursors, both delay memories and instruction counters.  The
programs: the ten of the corpus whose quiet loop drops an add of +0, and the directed family quiet_programs.ZERO_PROGRAMS.
FXB_INFO_XLATE_QUIET_LEFT is predicted by test_gpu_quiet_states.Watch from the oracles."""
import re
import zlib

import numpy as np
import pytest

from quiet_programs import DELAY_EDIT, GENERATED, GENERATED_WIDE, LIMIT_EDIT, ZERO_C, ZERO_PROGRAMS, sweep_program
from test_gpu_quiet_states import Watch, bits, handle, noise

pytestmark = pytest.mark.gpu

N = 130
CORPUS = dict(GENERATED + GENERATED_WIDE + [LIMIT_EDIT, DELAY_EDIT])
DROPPING = ["gen0", "gen3", "gen5", "gen6", "gen10", "wide3", "gen0_limit", "gen3_delay", "gen2", "gen4"]   # (test_xlate_quiet_frame.CORPUS_DROPS)
LEAVING = ["gen0", "gen3", "gen5", "gen6", "wide3", "gen0_limit", "gen4"]   # constants of their own end the quiet loop: see the first test
ZERO = [n for n, _ in ZERO_PROGRAMS]
TEXTS = dict([(n, CORPUS[n]) for n in DROPPING] + ZERO_PROGRAMS)
EDGE = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00000002, 0x80000002, 0x00000003, 0x80000003,
                 0x007fffff, 0x807fffff, 0x00800000, 0x80800000], dtype=np.uint32).view(np.float32)


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def rng_of(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


def settable(text):
    """state rows a register write reaches and the program keeps as rows: statics that an instruction writes, but for the rows the
    leading delay-line reads fill"""
    statics = re.findall(r"^static (\w+)", text, re.M)
    written = set(re.findall(r"^(?:macs|macsn|acc3|interp|limit|limitn|macmv) (\w+),", text, re.M))
    reads = set(re.findall(r"^[xi]delay read, (\w+),", text, re.M))
    return [r for r in statics if r in written and r not in reads]


def bounded_rows(text):
    """the state rows of the bounded class (fx_xlate.cpp: every value in [-1, 1] - their writers saturate or pass a bounded value
    on), by name: a wavefront that holds a NaN in one of them at launch never enters the quiet loop, whether the loop checks the
    row or not (test_gpu_quiet_states.py, first lines).  Wild: what a LIMIT / LIMITN may pick from the PCM input, a uniform above
    1 or a wild row, and a MACMV of one of those - to a fixed point, as the translator does it."""
    wild = set(re.findall(r"^input (\w+)", text, re.M))
    is_wild = lambda t: t in wild or (re.match(r"-?[\d.]+$", t) is not None and abs(float(t)) > 1.0)   # noqa: E731
    picks = [(m.group(1), m.group(2).split(", ")) for m in re.finditer(r"^(?:limitn?|macmv) (\w+), (.*)$", text, re.M)]
    ops = [(m.group(1), m.group(2)) for m in re.finditer(r"^(limitn?|macmv) (\w+),", text, re.M)]
    changed = True
    while changed:
        changed = False
        for (op, dst), (_, operands) in zip(ops, picks):
            sources = operands[:1] if op == "macmv" else operands[1:3]
            if dst not in wild and any(is_wild(t) for t in sources):
                wild.add(dst)
                changed = True
    return [r for r in re.findall(r"^static (\w+)", text, re.M) if r not in wild]


def watch(gpu, text, n=N):
    return Watch(gpu, text, range(n), n, bounded=bounded_rows(text))


def set_states(b, w, text, rng):
    """every settable row of every instance: one of EDGE, or - one time in 13 - a random value at an eighth of the row's bound
    (a state row's bound is the 0.25 the plan has for every row of the bounded class, whether its loop ends up checking it or not)"""
    assert all(bound == 0.25 for _, bound in w.checked + w.reads)
    for r in settable(text):
        pick = rng.integers(0, len(EDGE) + 1, size=N)
        inside = (rng.uniform(-1.0, 1.0, size=N) * 0.25 / 8).astype(np.float32)
        for i in range(N):
            v = float(EDGE[pick[i]] if pick[i] < len(EDGE) else inside[i])
            b.set_register_i(r, i, v)
            w.set(i, r, v)


def drawn(rng, S, seed):
    """[S, 1, N]: per instance and sample one of EDGE, or - one time in four - quiet noise scaled by 1e-36"""
    x = noise(N, S, 1, 0.9, seed=seed) * np.float32(1e-36)
    pick = rng.integers(0, len(EDGE) + 4, size=x.shape)
    for k, v in enumerate(EDGE):
        x[pick == k] = v
    return np.ascontiguousarray(x, dtype=np.float32)


def blocks_of(rng):
    """2 samples of -0 everywhere, 3 samples of zeros whose sign alternates with sample + instance, 40 drawn ones"""
    s, i = np.meshgrid(np.arange(3), np.arange(N), indexing="ij")
    alternating = np.where((s + i) & 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32).reshape(3, 1, N)
    out = [np.full((2, 1, N), np.float32(-0.0)), alternating, drawn(rng, 40, 2)]
    assert (bits(out[0]) == 0x80000000).all() and {0, 0x80000000} == set(bits(out[1]).reshape(-1).tolist())
    assert set(bits(EDGE).tolist()) <= set(bits(out[2]).reshape(-1).tolist())
    return out


# ------------------------------------------------------------------------------------------------ the quiet loop
@pytest.mark.parametrize("name", DROPPING + ZERO)
def test_quiet_loop_at_zero_rich_states(gpu, clean_env, name):
    """every value set here is far inside the bounds, and in the first block every wavefront runs the quiet loop to the end;
    whether one leaves later is Watch's word, from the oracles, and the handle must say the same: the directed family and gen2,
    gen10 and gen3_delay stay to the end of every launch, while the other seven programs of the corpus add constants of their
    own (acc3 r, a, x, 0.7 ...) that carry a checked row past 0.25 within a few samples whatever the input - their wavefronts
    leave in the block of 3 or of 40 samples, and what they compute from there on is compared all the same"""
    text = TEXTS[name]
    rng = rng_of(name)
    b = handle(gpu, text, N)
    w = watch(gpu, text)
    set_states(b, w, text, rng)
    for k, x in enumerate(blocks_of(rng)):
        _, left = w.run(b, x, "%s block %d" % (name, k))
        assert b.info("xlate_quiet_left") == left, (name, k, left, b.info("xlate_quiet_left"))
        assert left == 0 or (k > 0 and name in LEAVING), (name, k, left)
        assert b.info("xlate_quiet") == 1, b.tier_note()
    w.state(b, name)
    assert b.info("kernel") >= 9
    b.close()


# ------------------------------------------------------------------------------------------------ the fast and the exact stream beside it
@pytest.mark.parametrize("name", DROPPING + ZERO)
def test_fast_and_exact_streams_of_the_same_code(gpu, clean_env, name):
    """lane 70 hears 1.5 at sample 0 of the first block - wavefront 1 runs the steady fast loop (the fused multiply-adds of stream 0)
    - and lane 129 a NaN - the tail runs the exact stream (mul + add at the same states); wavefront 0 stays in the quiet loop"""
    text = TEXTS[name]
    rng = rng_of(name, 1)
    b = handle(gpu, text, N)
    w = watch(gpu, text)
    set_states(b, w, text, rng)
    for k, x in enumerate(blocks_of(rng)):
        if k == 0:
            x[0, 0, 70], x[0, 0, 129] = 1.5, np.nan
        _, left = w.run(b, x, "%s block %d" % (name, k))
        assert b.info("xlate_quiet_left") == left, (name, k, left, b.info("xlate_quiet_left"))
        assert k > 0 or left == 2, "wavefront 1 and the tail leave at sample 0, wavefront 0 stays"
        assert b.info("xlate_quiet") == 1, b.tier_note()
    w.state(b, name)
    assert b.info("kernel") >= 9
    b.close()


# ------------------------------------------------------------------------------------------------ the other tiers
TIERS = {"asm": ("FX_KERNEL", "asm", lambda k: 1 <= k <= 8), "hip": ("FX_KERNEL", "hip", lambda k: k == 0),
         "unstaged": ("FX_STAGES", "1", lambda k: k >= 9), "xlate_v256": ("FX_KERNEL", "xlate_v256", lambda k: k == 15)}


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("name", ZERO)
def test_other_tiers(gpu, clean_env, name, tier):
    """the directed family on the interpreter, the HIP C++ kernel, the translation in one stage and in the 256-VGPR build: one
    block of 45 samples - 2 of -0, 3 of alternating zeros, 40 drawn - from the same states"""
    var, value, kernel_ok = TIERS[tier]
    clean_env.setenv(var, value)
    text = TEXTS[name]
    rng = rng_of(name, 2)
    b = handle(gpu, text, N)
    w = watch(gpu, text)
    set_states(b, w, text, rng)
    w.run(b, np.concatenate(blocks_of(rng), axis=0), "%s on %s" % (name, tier), predict=False)
    w.state(b, name)
    assert kernel_ok(b.info("kernel")), (tier, b.info("kernel"), b.tier_note())
    b.close()


# ------------------------------------------------------------------------------------------------ the fused multiply, denormal by denormal
def sweep_values():
    """+-k * 2**-149 for k = 0 .. 8, the largest denormal, the smallest normal number and 1.0, of either sign"""
    words = list(range(9)) + [0x007fffff, 0x00800000, 0x3f800000]
    return np.array(words + [v | 0x80000000 for v in words], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("tier", ["default", "asm", "hip"])
@pytest.mark.parametrize("c", ZERO_C)
def test_denormal_sweep_of_zero_plus_scaled(gpu, clean_env, c, tier):
    """out = 0 + in * c - one v_fma_f32 in the translated fast stream for |c| > 0.5 (zeroPlusScaled: "a non-zero X never underflows
    to zero"), mul + add everywhere else - with the multiplier also in X, and 0 - in * c beside it: 24 values of X, one per
    instance and sample, N = 70 (a wavefront and a tail of 6).  (Which c the translated code fuses: test_xlate_quiet_frame.py.)"""
    if tier != "default":
        clean_env.setenv("FX_KERNEL", tier)
    text = sweep_program(c)
    values = sweep_values()
    n, S = 70, len(values)
    x = np.stack([np.roll(values, i) for i in range(n)], axis=1).reshape(S, 1, n)
    assert S == 24 and all(set(bits(x[:, 0, i]).tolist()) == set(bits(values).tolist()) for i in (0, n - 1))
    b = handle(gpu, text, n)
    w = watch(gpu, text, n)
    w.run(b, np.ascontiguousarray(x), "c = %s on %s" % (c, tier), predict=False)
    w.state(b, c)
    kernel = b.info("kernel")
    assert {"default": kernel >= 9, "asm": 1 <= kernel <= 8, "hip": kernel == 0}[tier], (tier, kernel, b.tier_note())
    b.close()
