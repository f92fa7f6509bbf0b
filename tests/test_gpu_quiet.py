"""The quiet loop on the device (fx_xlate.hpp QuietPlan): config5 on 192 instances - three wavefronts - against the oracle, bit for
bit on outputs, registers, instruction counters, delay memory and cursors, with FXB_INFO_XLATE_QUIET / _QUIET_LEFT telling
which wavefronts stayed in the loop.  Every wavefront starts every launch in the quiet loop; one leaves it - for the steady
fast loop, at the same point of the same sample - when a lane holds a checked row above its bound at the head of a sample, or
for the exact stream when a value is not finite."""
import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

N = 192
TEXT = progs.CONFIGS["config5"]()
WATCH = (0, 1, 63, 64, 70, 100, 127, 128, 150, 191)   # first / last lanes of each wavefront, the instance the cases disturb
REGS = (["u", "v", "m"] + ["d%d" % k for k in range(4)] + ["w%d" % k for k in range(4)] + ["lp%d" % k for k in range(4)] +
        ["y%d" % k for k in range(40)] + ["out"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def quiet_input(samples, level=0.9, seed=0):
    """uniform noise at +-level * 0.9 / 0.9 (the benchmark's distribution at level 0.9), one stream per instance"""
    return (progs.stimulus(N, samples, first_instance=1000 * seed) * np.float32(level / 0.9)).astype(np.float32)


@pytest.fixture
def translated(monkeypatch):
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(k, raising=False)


def run(gpu, blocks, sets=(), watch=WATCH):
    """blocks: inputs [S, N] launched one after the other; sets: (register, instance, value) written before the first.
    Returns the batch and FXB_INFO_XLATE_QUIET_LEFT after every launch; everything is compared with the oracle."""
    b = gpu.Batch(N, 1, 0)
    assert b.load_text(TEXT), b.errors()
    oracles = {}
    for i in watch:
        oracles[i] = Oracle(1)
        assert oracles[i].load_text(TEXT)
    for reg, inst, value in sets:
        b.set_register_i(reg, inst, value)
        if inst in oracles:
            oracles[inst].set_register(reg, value)
    left = []
    for x in blocks:
        y = b.process_block(x)
        left.append(b.info("xlate_quiet_left"))
        for i, o in oracles.items():
            ref = o.process_block(x[:, i].copy())
            bad = np.nonzero(bits(ref) != bits(y[:, i]))[0]
            assert bad.size == 0, "instance %d: first mismatch at sample %d of a block of %d: ref %08x got %08x" % (
                i, bad[0], x.shape[0], bits(ref)[bad[0]], bits(y[:, i])[bad[0]])
    for i, o in oracles.items():
        assert b.instruction_counter_i(i) == o.instruction_counter(), i
        for r in REGS:
            assert b.get_register_bits_i(r, i) == o.get_register_bits(r), (i, r)
        assert b.get_cursors_i(i) == o.cursors(), i
        assert np.array_equal(bits(b.get_tram_i(1, i, 8192)), bits(o.tram(1, 8192))), i
    assert b.ood_flags() == 0
    return b, left


def test_a_quiet_input_stays_in_the_quiet_loop(gpu, translated):
    """input +-0.9 over 2304 samples (past the delay line's read-back at 2048): nobody leaves"""
    b, left = run(gpu, [quiet_input(2304)])
    assert b.info("xlate_quiet") == 1 and "quiet loop" in b.tier_note()
    assert left == [0]
    assert b.info("xlate_unsaturated") == 395


def test_b_one_loud_state_row_sends_its_wavefront_away(gpu, translated):
    b, left = run(gpu, [quiet_input(96)], sets=[("y3", 70, 0.5)])
    assert b.info("xlate_quiet") == 1 and left == [1]


def test_c_loud_input_where_saturations_fire(gpu, translated):
    x = quiet_input(160, level=4.0)
    assert np.abs(x).max() > 3.0
    b, left = run(gpu, [x])
    assert left == [3]
    assert max(abs(np.float32(np.array([b.get_register_bits_i("w0", i)], dtype=np.uint32).view(np.float32)[0])) for i in WATCH) <= 1.0


def test_d_a_checked_row_at_the_bound_stays(gpu, translated):
    b, left = run(gpu, [quiet_input(96)], sets=[("y3", 70, 0.25)])
    assert left == [0]


def test_e_the_next_float_above_the_bound_leaves(gpu, translated):
    above = float(np.nextafter(np.float32(0.25), np.float32(1.0)))
    b, left = run(gpu, [quiet_input(96)], sets=[("y3", 70, above)])
    assert left == [1]


def test_f_an_infinity_goes_to_the_exact_stream(gpu, translated):
    x = quiet_input(64)
    x[5, 70] = np.inf
    b = gpu.Batch(N, 1, 0)
    assert b.load_text(TEXT)
    y = b.process_block(x)
    assert b.info("xlate_quiet_left") == 1
    for i in WATCH:
        o = Oracle(1)
        assert o.load_text(TEXT)
        ref = o.process_block(x[:, i].copy())
        assert np.array_equal(bits(ref), bits(y[:, i])), i
        assert b.instruction_counter_i(i) == o.instruction_counter()
        for r in REGS:
            assert b.get_register_bits_i(r, i) == o.get_register_bits(r), (i, r)
        assert np.array_equal(bits(b.get_tram_i(1, i, 8192)), bits(o.tram(1, 8192))), i
        assert b.get_cursors_i(i) == o.cursors()


def test_g_a_loud_sample_in_the_last_steady_sample(gpu, translated):
    for samples in (40, 41):
        x = quiet_input(samples)
        x[samples - 2, 70] = 4.0    # the last sample the steady loop runs; the block's last one runs the last-sample stream
        b, left = run(gpu, [x])
        assert left == [1]
        x = quiet_input(samples)
        x[samples - 1, 70] = 4.0    # ... and in that one nothing is left to leave
        b, left = run(gpu, [x])
        assert left == [0]


def test_h_short_blocks(gpu, translated):
    x = quiet_input(1 + 2 + 33 + 1)
    b, left = run(gpu, [x[0:1], x[1:3], x[3:36], x[36:37]])
    assert left == [0, 0, 0, 0]


def test_i_the_next_launch_starts_quiet_again(gpu, translated):
    first, second = quiet_input(48), quiet_input(48, seed=1)
    first[3, 70] = 1.5          # above the input's bound: its wavefront leaves at sample 3 and stays away for the launch
    b, left = run(gpu, [first, second])
    assert left == [1, 0]


@pytest.mark.parametrize("kernel", ["asm", "hip"])
def test_j_other_tiers_have_no_quiet_loop(gpu, monkeypatch, kernel):
    monkeypatch.setenv("FX_KERNEL", kernel)
    b = gpu.Batch(N, 1, 0)
    assert b.load_text(TEXT)
    b.process_block(quiet_input(8))
    assert b.info("xlate_quiet") == 0 and b.info("xlate_quiet_left") == 0
