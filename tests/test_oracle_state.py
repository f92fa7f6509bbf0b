"""The oracle's state accessors (oracle/fx8010_oracle.h: fxo_clone, fxo_set_tram, fxo_set_cursors): what lets a test model the
product's per-instance state operations - copy, reset, save / load, windows of delay memory - with oracle objects instead of a
twin handle.  A clone must carry on exactly like its original; the writers must be the inverse of the readers, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle
from test_dane_tram import CHORUS, TWO_TAPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAMS = [("config2", progs.config2, 0), ("config3", progs.config3, 0), ("config4", progs.config4, 0), ("config5", progs.config5, 0),
            ("chorus_dane", lambda: CHORUS, 1), ("two_taps_dane", lambda: TWO_TAPS, 1), ("two_taps", lambda: TWO_TAPS, 0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def whole_state(o):
    sizes = o.tram_sizes()
    return {"registers": o.registers(), "cursors": o.cursors(), "lfsr": o.lfsr(), "counter": o.instruction_counter(), "flags": o.ood_flags(),
            "itram": bits(o.tram(0, 8192)).tobytes(), "xtram": bits(o.tram(1, max(2 * sizes[1], 64))).tobytes()}


@pytest.mark.parametrize("name, text, options", PROGRAMS, ids=[p[0] for p in PROGRAMS])
@pytest.mark.parametrize("k, m", [(0, 40), (37, 61), (200, 3)])
def test_a_clone_carries_on_like_its_original(name, text, options, k, m):
    o = Oracle(1)
    if options:
        o.set_option(options)
    assert o.load_text(text())
    o.seed_noise(0x1234567, -0x7654321)
    x = progs.stimulus(1, k + m)[:, 0].copy()
    o.process_block(x[:k])
    if k:
        o.set_register(o.registers()[-1][0], 0.375)     # (a value the program text does not hold)
    c = o.clone()
    assert whole_state(c) == whole_state(o)
    assert c.controls() == o.controls() and c.instructions() == o.instructions() and c.ready()
    ya, yb = o.process_block(x[k:]), c.process_block(x[k:])
    assert np.array_equal(bits(ya), bits(yb))
    assert whole_state(c) == whole_state(o)
    # two objects, not two names of one: the original moves on alone
    before = whole_state(c)
    o.process_block(x[:5])
    o.close()
    assert whole_state(c) == before
    assert np.array_equal(bits(c.clone().process_block(x[:9])), bits(c.process_block(x[:9])))


PATTERNS = np.array([0x3F800000, 0x7FC00000, 0xFFC12345, 0x7F812345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0xBF000000],
                    dtype=np.uint32)


@pytest.mark.parametrize("which, have", [(0, 8192), (1, 1048576)])
def test_set_tram_is_the_inverse_of_tram(which, have):
    o = Oracle(1)
    assert o.load_text(TWO_TAPS)
    words = PATTERNS.view(np.float32)
    for first in (0, 7, have - words.size):
        assert o.set_tram(which, first, words) == words.size
        assert np.array_equal(bits(o.tram(which, first + words.size))[first:], PATTERNS)
    assert np.array_equal(bits(o.tram(1 - which, 64)), np.zeros(64, np.uint32))      # the other line is untouched
    # refused: nothing written
    image = bits(o.tram(which, have)).copy()
    for first in (have - words.size + 1, have, -1, 2 ** 31 - 4):
        assert o.set_tram(which, first, words) == 0
    assert o.set_tram(2, 0, words) == 0 and o.set_tram(-1, 0, words) == 0
    assert o.set_tram(which, 5, words[:0]) == 0
    assert np.array_equal(bits(o.tram(which, have)), image)


def test_a_written_window_is_what_the_program_reads():
    """a word put where the next read of a one-tap line looks comes out of the program"""
    o = Oracle(1)
    assert o.load_text("input in 0\noutput out 0\nitramsize 8 \nstatic r\nidelay read, r, at, 0\nidelay write, in, at, 0\nmacs out, r, 0, 0\nend")
    o.process_block(np.zeros(3, np.float32))
    o.set_tram(0, o.cursors()[1], np.array([0.625], np.float32))
    assert o.process_block(np.zeros(1, np.float32))[0] == np.float32(0.625)


def test_set_cursors_is_the_inverse_of_cursors():
    o = Oracle(1)
    assert o.load_text(TWO_TAPS)
    o.process_block(progs.stimulus(1, 11)[:, 0].copy())
    assert o.cursors() != [5, 63, 499, 0]
    o.set_cursors([5, 63, 499, 0])
    assert o.cursors() == [5, 63, 499, 0]
    c = o.clone()
    c.set_cursors([1, 2, 3, 4])
    assert o.cursors() == [5, 63, 499, 0] and c.cursors() == [1, 2, 3, 4]


def test_stand_alone_program_under_the_sanitizers():
    """oracle/state_check.c - clone, window writes, carry on, free - built with -fsanitize=address,undefined and run as a program
    of its own (nothing is loaded into python under a sanitizer); the leak check is on"""
    out = subprocess.run(["gcc", "-print-file-name=libasan.so"], stdout=subprocess.PIPE, text=True).stdout.strip()
    if not (os.path.isabs(out) and os.path.exists(out)):
        pytest.skip("gcc has no libasan runtime here")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "state_check"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "oracle", "_variants", "state_check")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "state_check ok" in r.stdout, r.stdout[-4000:]
