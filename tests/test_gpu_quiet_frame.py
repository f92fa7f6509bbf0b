"""The frame of the quiet loop on the device: the adds of +0 that are not emitted, on 130 instances - two
wavefronts and a tail of two lanes - against one oracle per instance, bit for bit on outputs, every register, delay memory,
cursors and instruction counters; FXB_INFO_XLATE_QUIET_LEFT == 0 says that every wavefront ran the quiet loop to the end of every
launch.  Signs of zero (a dropped add whose other side could be -0 after all would leave a -0 where the reference has +0) - and
the diagnostics build with the part switched off against the release library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
N = 130


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def registers_of(text):
    return re.findall(r"^static (\w+)", text, re.M) + ["out"]


def xtram_size(text):
    return int(re.search(r"^xtramsize (\d+)", text, re.M).group(1))


def quiet_input(samples, seed=0):
    """the benchmark's distribution (uniform in +-0.9), one stream per instance"""
    return progs.stimulus(N, samples, first_instance=1000 * seed).astype(np.float32)


@pytest.fixture
def translated(monkeypatch):
    for k in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(k, raising=False)


def run(gpu, text, blocks, sets=()):
    """blocks: inputs [S, N] launched one after the other; sets: (register, value) written to EVERY instance before the first.
    Everything is compared with one oracle per instance; returns the batch."""
    b = gpu.Batch(N, 1, 0)
    assert b.load_text(text), b.errors()
    oracles = []
    for i in range(N):
        o = Oracle(1)
        assert o.load_text(text)
        oracles.append(o)
    for reg, value in sets:
        for i, o in enumerate(oracles):
            b.set_register_i(reg, i, value)
            o.set_register(reg, value)
    at = 0
    for x in blocks:
        y = b.process_block(x)
        assert b.info("xlate_quiet") == 1 and b.info("xlate_quiet_left") == 0, (at, b.info("xlate_quiet"), b.info("xlate_quiet_left"))
        for i, o in enumerate(oracles):
            ref = o.process_block(x[:, i].copy())
            bad = np.nonzero(bits(ref) != bits(y[:, i]))[0]
            assert bad.size == 0, "instance %d: first mismatch at sample %d (block from %d, %d long): ref %08x got %08x" % (
                i, at + bad[0], at, x.shape[0], bits(ref)[bad[0]], bits(y[:, i])[bad[0]])
        at += x.shape[0]
    size = xtram_size(text)
    for i, o in enumerate(oracles):
        assert b.instruction_counter_i(i) == o.instruction_counter(), i
        for r in registers_of(text):
            assert b.get_register_bits_i(r, i) == o.get_register_bits(r), (i, r)
        assert b.get_cursors_i(i) == o.cursors(), i
        assert np.array_equal(bits(b.get_tram_i(1, i, size)), bits(o.tram(1, size))), i
    assert b.ood_flags() == oracles[0].ood_flags() == 0
    return b


def cut(x, lengths):
    assert sum(lengths) == x.shape[0]
    out, at = [], 0
    for n in lengths:
        out.append(x[at:at + n])
        at += n
    return out


CONFIG5 = progs.CONFIGS["config5"]()
MINUS_ZERO_ROWS = ["m", "u", "v"] + ["lp%d" % k for k in range(4)] + ["y0", "y7", "y20", "y39"]


@pytest.mark.parametrize("pattern", ["minus", "alternating"])
def test_signs_of_zero(gpu, translated, pattern):
    """-0.0 in the input and in m, u, v, lp*, some y* before the first block: every zero keeps the reference's sign"""
    x = np.full((45, N), np.float32(-0.0))
    if pattern == "alternating":
        s, i = np.meshgrid(np.arange(45), np.arange(N), indexing="ij")
        x = np.where((s + i) & 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    assert (bits(x) == 0x80000000).any()
    b = run(gpu, CONFIG5, cut(x, [2, 3, 40]), sets=[(r, -0.0) for r in MINUS_ZERO_ROWS])
    assert b.info("xlate_unsaturated") == 395


def test_zero_signs_under_a_signal(gpu, translated):
    """... and with a signal that decays into denormals and zeros of both signs (the input stops after 8 samples)"""
    x = quiet_input(40) * np.float32(1e-36)
    x[8:] = np.float32(-0.0)
    run(gpu, CONFIG5, cut(x, [2, 3, 35]), sets=[(r, -0.0) for r in MINUS_ZERO_ROWS])


def diagnostics_library():
    """csrc/build/diag/libfx8010_amd.so (fx_knobs.hpp: the translate-time switches exist only there), built when it is missing or
    older than a source"""
    lib = os.path.join(CSRC, "build", "diag", "libfx8010_amd.so")
    sources = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".cpp", ".hpp", ".hip", ".h", ".S", ".inc"))]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in sources):
        subprocess.check_call(["make", "-s", "-j16", "-C", CSRC, "diag"])
    return lib


def test_the_part_off_against_on(gpu, translated, tmp_path):
    """config5, 40 samples: the diagnostics build with FX_XLATE_ZEROADD=0 - a quiet loop with every add - gives the words and the
    state of the release library (a fresh process each: a process keeps one library)"""
    x = quiet_input(40, seed=3)
    np.save(tmp_path / "x.npy", x)
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r]\n"
            "import fx8010_amd as A, fx8010_programs as P\n"
            "x = np.load(sys.argv[1]); b = A.Batch(x.shape[1], 1, 0); assert b.load_text(P.CONFIGS['config5']())\n"
            "y = b.process_block(x)\n"
            "assert b.info('xlate_quiet') == 1 and b.info('xlate_quiet_left') == 0\n"
            "regs = np.array([[b.get_register_bits_i(r, i) for r in sys.argv[3].split(',')] for i in range(x.shape[1])], dtype=np.uint32)\n"
            "tram = np.stack([b.get_tram_i(1, i, 8192) for i in range(x.shape[1])])\n"
            "np.savez(sys.argv[2], y=y, regs=regs, tram=tram, cursors=np.array([b.get_cursors_i(i) for i in range(x.shape[1])]), hash=np.uint64(b.info('xlate_code_hash')))\n"
            ) % (os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle"))

    def child(out, lib, **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
        env.update(knobs)
        if lib:
            env["FX8010_AMD_LIB"] = lib
        else:
            env.pop("FX8010_AMD_LIB", None)
        subprocess.run([sys.executable, "-c", code, str(tmp_path / "x.npy"), str(tmp_path / out), ",".join(registers_of(CONFIG5))], env=env, check=True, timeout=120)
        return np.load(tmp_path / out)

    on = child("on.npz", None)
    off = child("off.npz", diagnostics_library(), FX_XLATE_ZEROADD="0")
    assert int(on["hash"]) != int(off["hash"]), "the switch changes the generated code"
    for k in ("y", "regs", "tram", "cursors"):
        assert np.array_equal(np.ascontiguousarray(on[k]).view(np.uint8), np.ascontiguousarray(off[k]).view(np.uint8)), k
