"""Per-instance state calls without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process (the binding reads FX8010_AMD_LIB once, at
import; this file is also that child).  The stand-ins of the two kernels (tests/hipstub/fx_instances_stub.cpp) do the real moves
in stream order, with an addressing written out independently of the kernels'.  Every check is equality of 32-bit patterns: a
whole-batch image with distinct words in every state row and delay-memory slot goes in through fxb_load_state, copy / reset /
save + load are applied, the image comes back through fxb_save_state and must equal the same operation done in numpy on the
records of the image.  Launches are counted; refusals launch nothing and change nothing.  Parity with the emulation itself is
tests/test_gpu_instances.py."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_NOTREADY, FX_E_ARG = -2, -3
PLAIN = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
TRAMS = ("itramsize 64 \nxtramsize 500 \ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 7\n"
         "xdelay write, in, at, 3\nxdelay read, xr, at, 403\nmacs out, r1, xr, vol\nend")
LONG = ("itramsize 8192 \nxtramsize 8192 \ninput in 0\noutput out 0\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 8000\n"
        "xdelay write, in, at, 0\nxdelay read, xr, at, 8100\nmacs out, r1, xr, 0.5\nend")
EDGES = [0, 63, 64, 127, 128, 199]   # both sides of every wavefront boundary of N = 200, and its last instance
SCRATCH = 64 << 20


def run_child(which, marker, devices=1, asan=False):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    if asan:
        found = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
        if not found:
            pytest.skip("no ASan runtime on this machine")
        subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasanlib"])
        env.update(FX8010_AMD_LIB=os.path.join(CSRC, "build", "stubasan", "libfx8010_amd.so"), LD_PRELOAD=found[-1],
                   ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    else:
        subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
        env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


def test_instance_indexing_on_the_hip_stand_in():
    run_child("indexing", "instances indexing ok")


def test_instance_records_hold_the_words_of_the_whole_batch_image():
    run_child("consistency", "instances consistency ok")


def test_instance_refusals_launch_nothing_and_change_nothing():
    run_child("refusals", "instances refusals ok")


def test_instance_calls_above_the_scratch_limit_run_in_pieces():
    run_child("pieces", "instances pieces ok")


def test_instance_reset_keeps_the_delay_line_positions():
    run_child("reset", "instances reset ok")


def test_instance_load_checks_the_positions_and_promotes_registers():
    run_child("load", "instances load ok")


def test_instance_calls_between_blocks_on_other_streams():
    run_child("streams", "instances streams ok")


def test_instances_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "instances shards ok", devices=3)


def test_instance_indexing_and_refusals_under_asan():
    run_child("indexing", "instances indexing ok", asan=True)
    run_child("refusals", "instances refusals ok", asan=True)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")]
    import fx8010_amd as A
    assert "stub" in os.path.abspath(A.LIB_PATH), "run with FX8010_AMD_LIB = the stand-in build (csrc/build/stub or build/stubasan)"
    lib = A.load()
    for f in ("fxstub_kernels_run", "fxstub_cross_device_errors", "fxstub_inst_gathers", "fxstub_inst_scatters"):
        getattr(lib, f).restype = C.c_long
    return A, lib


class Image:
    """a whole-batch image (fxb_save_state) taken apart: the header fields and the records [n, W] it holds"""

    def __init__(self, raw):
        self.raw = np.array(raw, dtype=np.uint8)
        self.n = int(self.raw[8:16].view(np.int64)[0])
        self.channels, self.regs, self.rows, self.islots, self.xslots = (int(v) for v in self.raw[16:36].view(np.int32))
        self.words = self.rows + self.islots + self.xslots
        self.cursors = self.regs + self.channels   # the first of the four position rows

    def records(self):
        body = self.raw[64:].view(np.uint32)
        a, b = self.rows * self.n, self.rows * self.n + self.n * self.islots
        return np.concatenate([body[:a].reshape(self.rows, self.n).T, body[a:b].reshape(self.n, self.islots), body[b:].reshape(self.n, self.xslots)], axis=1).copy()

    def with_records(self, rec):
        assert rec.shape == (self.n, self.words) and rec.dtype == np.uint32
        out = self.raw.copy()
        r, i = self.rows, self.rows + self.islots
        out[64:] = np.concatenate([rec[:, :r].T.ravel(), rec[:, r:i].ravel(), rec[:, i:].ravel()]).view(np.uint8)
        return out


def distinct(b, seed, same_cursors=True):
    """an image of b's shape with distinct words in every state row and delay-memory slot (NaN patterns among them), loaded into b;
    same_cursors: the four position rows hold one value per row, as on a handle that has run.  Distinct words in the rows of the
    literals that are delay-line offsets make those per-instance, and the delay memory grows to what any offset can reach: the
    image is built again for the shape the handle has after the first load."""
    for _ in range(3):
        img = Image(b.save_state())
        rec = (np.arange(img.n * img.words, dtype=np.uint64) * 2654435761 + seed).astype(np.uint32).reshape(img.n, img.words)
        rec[::7, ::5] |= 0x7FC00000   # quiet NaNs with payloads
        rec[3::11, 1::3] = (rec[3::11, 1::3] & 0x003FFFFF) | 0x7F800001   # signalling NaNs
        if same_cursors:
            rec[:, img.cursors:img.cursors + 4] = np.array([5, 9, 77, 401], dtype=np.uint32) + seed % 3
        b.load_state(img.with_records(rec))
        if Image(b.save_state()).words == img.words:
            break
    assert np.array_equal(state_of(b), rec)
    return img, rec


def state_of(b):
    return Image(b.save_state()).records()


def instance_records(image, words):
    """the records of an instance image: [count, W]"""
    raw = np.asarray(image, dtype=np.uint8)
    assert raw[:4].tobytes() == b"FXSI" and int(raw[8:16].view(np.int64)[0]) * words * 4 + 64 == raw.size
    return raw[64:].view(np.uint32).reshape(-1, words)


class Counts:
    """(gathers, scatters) since the last look: the stand-in's own counters and the handle's selectors must agree"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        self.b.sync()
        return (self.lib.fxstub_inst_gathers(), self.lib.fxstub_inst_scatters(), self.b.info("instance_gathers"), self.b.info("instance_scatters"), self.lib.fxstub_kernels_run())

    def expect(self, what, gathers, scatters):
        now = self.now()
        got = tuple(a - b for a, b in zip(now, self.seen))
        assert got == (gathers, scatters, gathers, scatters, 0), (what, got, (gathers, scatters))
        self.seen = now


def i64(v):
    return np.ascontiguousarray(np.atleast_1d(v), dtype=np.int64)


def fresh_record(A, text, N, img, writes=()):
    """the record of an instance of a handle that has processed nothing, after the broadcast `writes`: its state rows, and zeroes
    for as much delay memory as `img` has"""
    f = A.Batch(N, 1, 0)
    assert f.load_text(text), f.errors()
    for key, v in writes:
        assert f.set_register(key, v) == 0
    rec = state_of(f)
    assert (rec == rec[0]).all() and not rec[0, img.rows:].any()
    return np.concatenate([rec[0, :img.rows], np.zeros(img.words - img.rows, dtype=np.uint32)])


def child_indexing():
    A, lib = stub_library()
    N = 200
    for text in (TRAMS, PLAIN):
        b = A.Batch(N, 1, 0)
        assert b.load_text(text), b.errors()
        img, rec = distinct(b, 17)
        assert b.instance_words == img.words and b.instance_image_size(3) == 64 + 3 * img.words * 4
        assert (img.islots > 0 and img.xslots > 0) == (text is TRAMS)
        count = Counts(lib, b)
        # copy: scattered over every wavefront boundary, consecutive, one source fanned out to 70 destinations
        for src, dst in (([0, 63, 128, 199], [64, 127, 1, 130]), (list(range(10, 40)), list(range(100, 130))), ([64] * 70, list(range(65, 128)) + list(range(192, 199)))):
            b.copy_instances(src, dst)
            rec[dst] = rec[src]
            count.expect("copy", 1, 1)
            assert np.array_equal(state_of(b), rec), ("copy", src[:4], dst[:4])
        # save: records in list order, repeats allowed; load: into other instances of the same handle
        for src, dst in ((EDGES, [5, 70, 6, 129, 190, 62]), (list(range(120, 140)), list(range(20, 40)))):
            image = b.save_instances(src)
            count.expect("save", 1, 0)
            assert np.array_equal(instance_records(image, img.words), rec[src])
            b.load_instances(dst, image)
            rec[dst] = rec[src]
            count.expect("load", 0, 1)
            assert np.array_equal(state_of(b), rec), ("load", src[:4], dst[:4])
        assert np.array_equal(instance_records(b.save_instances([7, 7, 199]), img.words), rec[[7, 7, 199]])
        count.expect("save with a repeat", 1, 0)
        # reset: a fresh record everywhere but in the four position rows
        fresh = fresh_record(A, text, 64, img)
        keep = slice(img.cursors, img.cursors + 4)
        for group in (EDGES, list(range(60, 70))):
            b.reset_instances(group)
            held = rec[group, keep].copy()
            rec[group] = fresh
            rec[group, keep] = held
            count.expect("reset", 0, 1)
            assert np.array_equal(state_of(b), rec), ("reset", group[:4])
        # empty lists: nothing happens
        assert b.copy_instances([], []) == 0 and b.reset_instances([]) == 0 and b.load_instances([], b.save_instances([])) == 0
        count.expect("empty", 0, 0)
        assert np.array_equal(state_of(b), rec)
    # without a program
    e = A.Batch(8, 1, 0)
    one = i64([0])
    assert lib.fxb_reset_instances(e._h, C.c_void_p(one.ctypes.data), 1) == FX_E_NOTREADY
    assert lib.fxb_copy_instances(e._h, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), 0) == FX_E_NOTREADY
    assert lib.fxstub_cross_device_errors() == 0
    print("instances indexing ok")


def child_consistency():
    A, lib = stub_library()
    for text, N in ((TRAMS, 200), (PLAIN, 130)):
        b = A.Batch(N, 1, 0)
        assert b.load_text(text), b.errors()
        img, rec = distinct(b, 5, same_cursors=False)
        image = b.save_instances(np.arange(N))
        assert np.array_equal(instance_records(image, img.words), Image(b.save_state()).records())
        assert np.array_equal(instance_records(image, img.words), rec)
        # the header is the whole-batch header with its own magic and n = count
        assert np.array_equal(image[16:64], img.raw[16:64]) and image[4:8].view(np.uint32)[0] == img.raw[4:8].view(np.uint32)[0]
    print("instances consistency ok")


def child_refusals():
    A, lib = stub_library()
    N = 200
    b = A.Batch(N, 1, 0)
    assert b.load_text(TRAMS), b.errors()
    img, rec = distinct(b, 29)
    before = b.save_state()
    o = A.Batch(16, 1, 0)   # an image of the program without delay lines
    assert o.load_text(PLAIN), o.errors()
    alien = o.save_instances([1, 2, 3])
    count = Counts(lib, b)
    p = lambda a: C.c_void_p(a.ctypes.data if a is not None else 0)
    good = b.save_instances([1, 2, 3])
    count.expect("the image the refusals are tried with", 1, 0)

    def refused(what, rc):
        assert rc == FX_E_ARG, (what, rc, b.last_error())
        assert b.last_error(), what
        count.expect(what, 0, 0)
        assert np.array_equal(b.save_state(), before), what

    a3, b3 = i64([1, 2, 3]), i64([4, 5, 6])
    refused("copy: negative count", lib.fxb_copy_instances(b._h, p(a3), p(b3), -1))
    refused("copy: null source list", lib.fxb_copy_instances(b._h, p(None), p(b3), 3))
    refused("copy: null destination list", lib.fxb_copy_instances(b._h, p(a3), p(None), 3))
    refused("copy: source beyond the batch", lib.fxb_copy_instances(b._h, p(i64([1, N, 3])), p(b3), 3))
    refused("copy: negative source", lib.fxb_copy_instances(b._h, p(i64([1, -1, 3])), p(b3), 3))
    refused("copy: destination beyond the batch", lib.fxb_copy_instances(b._h, p(a3), p(i64([4, 5, N])), 3))
    refused("copy: repeated destination", lib.fxb_copy_instances(b._h, p(a3), p(i64([4, 5, 4])), 3))
    refused("copy: destination among the sources", lib.fxb_copy_instances(b._h, p(a3), p(i64([4, 3, 6])), 3))
    refused("copy: onto itself", lib.fxb_copy_instances(b._h, p(a3), p(a3), 3))
    refused("reset: negative count", lib.fxb_reset_instances(b._h, p(a3), -2))
    refused("reset: null list", lib.fxb_reset_instances(b._h, p(None), 2))
    refused("reset: beyond the batch", lib.fxb_reset_instances(b._h, p(i64([0, N])), 2))
    refused("reset: repeated", lib.fxb_reset_instances(b._h, p(i64([9, 9])), 2))
    buf = np.zeros(good.size, dtype=np.uint8)
    refused("save: short buffer", lib.fxb_save_instances(b._h, p(a3), 3, p(buf), buf.size - 1))
    refused("save: null buffer", lib.fxb_save_instances(b._h, p(a3), 3, p(None), buf.size))
    refused("save: null list", lib.fxb_save_instances(b._h, p(None), 3, p(buf), buf.size))
    refused("save: beyond the batch", lib.fxb_save_instances(b._h, p(i64([0, 1, N])), 3, p(buf), buf.size))
    refused("save: negative count", lib.fxb_save_instances(b._h, p(a3), -1, p(buf), buf.size))
    assert not buf.any(), "a refused save wrote to the buffer"
    refused("load: truncated", lib.fxb_load_instances(b._h, p(b3), 3, p(good), good.size - 4))
    refused("load: no header", lib.fxb_load_instances(b._h, p(b3), 3, p(good), 63))
    refused("load: null image", lib.fxb_load_instances(b._h, p(b3), 3, p(None), good.size))
    refused("load: another count than the image's", lib.fxb_load_instances(b._h, p(b3), 2, p(good), good.size))
    refused("load: repeated destination", lib.fxb_load_instances(b._h, p(i64([4, 4, 6])), 3, p(good), good.size))
    refused("load: beyond the batch", lib.fxb_load_instances(b._h, p(i64([4, 5, N])), 3, p(good), good.size))
    refused("load: null list", lib.fxb_load_instances(b._h, p(None), 3, p(good), good.size))
    whole = good.copy()
    whole[:4] = before[:4]
    refused("load: a whole-batch image's kind", lib.fxb_load_instances(b._h, p(b3), 3, p(whole), whole.size))
    for at, what in ((4, "version"), (16, "channels"), (20, "registers"), (24, "state rows"), (28, "iTRAM slots"), (32, "xTRAM slots")):
        other = good.copy()
        other[at:at + 4].view(np.int32)[0] += 1
        refused("load: another " + what, lib.fxb_load_instances(b._h, p(b3), 3, p(other), other.size))
    for value in (-1, 1 << 40):
        other = good.copy()
        other[8:16].view(np.int64)[0] = value
        refused("load: a damaged count", lib.fxb_load_instances(b._h, p(b3), 3, p(other), other.size))
    refused("load: another program", lib.fxb_load_instances(b._h, p(b3), 3, p(alien), alien.size))
    assert lib.fxb_instance_image_size(b._h, -1) == FX_E_ARG
    # ... and the good image still loads
    assert b.load_instances([4, 5, 6], good) == 0
    count.expect("the good image", 0, 1)
    rec[[4, 5, 6]] = rec[[1, 2, 3]]
    assert np.array_equal(state_of(b), rec)
    print("instances refusals ok")


def child_pieces():
    A, lib = stub_library()
    N = 2200
    b = A.Batch(N, 1, 0)
    assert b.load_text(LONG), b.errors()
    W = b.instance_words
    per = SCRATCH // (W * 4)
    assert W > 16384 and 1000 < per < 1100, (W, per)
    rng = np.random.default_rng(3)
    rec = rng.integers(0, 1 << 32, (N, W), dtype=np.uint64).astype(np.uint32)
    cursors = b.info("num_registers") + 1
    # (the registers and the positions of a handle that has processed nothing: other words in the rows of the literals that are
    # delay-line offsets would make those per-instance and the delay memory grow)
    rec[:, :cursors + 4] = instance_records(b.save_instances([0]), W)[0, :cursors + 4]
    image = np.empty(64 + N * W * 4, dtype=np.uint8)
    image[:64] = b.save_instances([])[:64]
    image[8:16].view(np.int64)[0] = N
    image[64:] = rec.view(np.uint8).ravel()
    count = Counts(lib, b)
    b.load_instances(np.arange(N), image)
    count.expect("load of 2200 records: three pieces", 0, 3)
    src, dst = np.arange(per + 1), np.arange(1100, 1100 + per + 1)
    b.copy_instances(src, dst)
    rec[dst] = rec[src]
    count.expect("copy of one record more than a piece holds: two pieces", 2, 2)
    b.copy_instances(src[:per], dst[:per])
    count.expect("exactly a piece", 1, 1)
    back = b.save_instances(np.arange(N)[::-1])
    count.expect("save of 2200 records: three pieces", 3, 0)
    assert np.array_equal(instance_records(back, W), rec[::-1])
    b.reset_instances(np.arange(N))
    count.expect("reset: one record, one launch whatever the list", 0, 1)
    print("instances pieces ok")


def child_reset():
    A, lib = stub_library()
    N = 200
    b = A.Batch(N, 1, 0)
    assert b.load_text(TRAMS), b.errors()
    assert b.set_register("vol", 0.75) == 0
    x = np.zeros((8, N), dtype=np.float32)
    b.process_block(x)
    assert b.set_register_i("vol", 64, 0.125) == 0
    img, rec = distinct(b, 41, same_cursors=False)   # every instance with positions of its own: each keeps ITS four words
    assert b.set_register("vol", 0.3) == 0           # the last broadcast write is what a reset instance gets
    rec = state_of(b)
    fresh = fresh_record(A, TRAMS, 64, img, [("vol", 0.3)])
    keep = slice(img.cursors, img.cursors + 4)
    b.reset_instances(EDGES)
    want = rec.copy()
    want[EDGES] = fresh
    want[EDGES, keep] = rec[EDGES, keep]
    got = state_of(b)
    assert np.array_equal(got, want)
    assert np.array_equal(got[EDGES, keep], rec[EDGES, keep]) and not np.array_equal(got[0, keep], got[63, keep])
    # latches, LFSR seeds, flags, counter, delay memory as ensureState makes them
    tail = got[0, img.cursors + 4:img.rows]
    assert list(tail) == [0x70F4F854, 0xE1E9F0A7, 0, 0, 0] and not got[0, img.rows:].any() and got[0, img.regs] == 0
    assert b.get_register_i("vol", 0) == np.float32(0.3) and b.instruction_counter_i(199) == 0
    print("instances reset ok")


def child_load():
    A, lib = stub_library()
    N = 200
    a, b = A.Batch(N, 1, 0), A.Batch(64, 1, 0)
    for h in (a, b):
        assert h.load_text(TRAMS), h.errors()
    distinct(a, 7)    # positions 5 + 1, ...
    img_b, rec_b = distinct(b, 6)   # positions 5 + 0, ...: as if b had run another number of samples
    image = a.save_instances([0, 63, 130])
    before = b.save_state()
    count = Counts(lib, b)
    p = lambda v: C.c_void_p(v.ctypes.data)
    dst = i64([5, 6, 63])
    assert lib.fxb_load_instances(b._h, p(dst), 3, p(image), image.size) == FX_E_ARG and "positions" in b.last_error(), b.last_error()
    count.expect("positions differ: refused", 0, 0)
    assert np.array_equal(b.save_state(), before)
    # one record out of three with other positions is enough
    img_a = Image(a.save_state())
    fixed = instance_records(image, img_a.words).copy()
    fixed[:, img_a.cursors:img_a.cursors + 4] = rec_b[0, img_a.cursors:img_a.cursors + 4]
    for k in range(4):
        bad = image.copy()
        words = bad[64:].view(np.uint32).reshape(3, -1)
        words[...] = fixed
        words[2, img_a.cursors + k] ^= 1
        assert lib.fxb_load_instances(b._h, p(dst), 3, p(bad), bad.size) == FX_E_ARG
    count.expect("one position word differs: refused", 0, 0)
    assert np.array_equal(b.save_state(), before)
    ok = image.copy()
    ok[64:].view(np.uint32).reshape(3, -1)[...] = fixed
    assert b.load_instances(dst, ok) == 0
    count.expect("equal positions: loaded", 0, 1)
    rec_b[dst] = fixed
    assert np.array_equal(state_of(b), rec_b)
    # a program without delay-line instructions loads whatever the position words say
    c, d = A.Batch(N, 1, 0), A.Batch(N, 1, 0)
    for h in (c, d):
        assert h.load_text(PLAIN), h.errors()
    distinct(c, 7, same_cursors=False)
    _, rec_d = distinct(d, 9, same_cursors=False)
    assert d.load_instances([199, 0], c.save_instances([3, 64])) == 0
    rec_d[[199, 0]] = state_of(c)[[3, 64]]
    assert np.array_equal(state_of(d), rec_d)
    # promotion: a register the destination holds as one value becomes per-instance when a record has another
    s, t = A.Batch(N, 1, 0), A.Batch(N, 1, 0)
    for h in (s, t):
        assert h.load_text(PLAIN), h.errors()
        h.process_block(np.zeros((4, N), dtype=np.float32))
    assert s.set_register_i("vol", 3, 0.25) == 0
    rows = t.info("num_lane_regs")
    assert t.get_register_i("vol", 7) == 0.5
    assert t.load_instances([7, 128], s.save_instances([3, 4])) == 0
    assert t.get_register_i("vol", 7) == 0.25 and t.get_register_i("vol", 128) == 0.5
    assert t.get_register_i("vol", 8) == 0.5 and t.get_register_i("vol", 199) == 0.5, "the broadcast value of the other instances"
    assert t.info("num_lane_regs") == rows + 1, "vol has a row of its own from now on"
    # equal values promote nothing
    u = A.Batch(N, 1, 0)
    assert u.load_text(PLAIN), u.errors()
    u.process_block(np.zeros((4, N), dtype=np.float32))
    rows = u.info("num_lane_regs")
    assert u.load_instances([1], t.save_instances([9])) == 0 and u.info("num_lane_regs") == rows
    print("instances load ok")


def child_streams():
    """a copy queued behind a block on a caller's stream runs after it and in front of the next block on that stream: the stand-in's
    emulation kernel takes its time, so an unordered copy would finish first"""
    A, lib = stub_library()
    N, S = 200, 16
    b = A.Batch(N, 1, 0)
    assert b.load_text(TRAMS), b.errors()
    img, rec = distinct(b, 13)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    stream = C.c_void_p()
    assert lib.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and stream.value
    x = lib.fxb_host_alloc(N * S * 4)
    y = lib.fxb_host_alloc(N * S * 4)
    C.memset(x, 0, N * S * 4)
    lib.fxstub_set_kernel_micros(20000)
    kernels = lib.fxstub_kernels_run()
    assert lib.fxb_process_block_dev(b._h, C.c_void_p(x), C.c_void_p(y), S, stream) == 0
    b.copy_instances([0, 63], [64, 199])
    assert lib.fxb_process_block_dev(b._h, C.c_void_p(x), C.c_void_p(y), S, stream) == 0
    b.reset_instances([1])
    b.sync()
    lib.fxstub_set_kernel_micros(0)
    assert lib.fxstub_kernels_run() - kernels == 2 and lib.fxstub_inst_gathers() == 1 and lib.fxstub_inst_scatters() == 2
    got = state_of(b)
    assert np.array_equal(got[[64, 199]], got[[0, 63]])
    lib.fxb_host_free(x)
    lib.fxb_host_free(y)
    print("instances streams ok")


def child_shards():
    A, lib = stub_library()
    N = 3 * 256 + 40
    for text in (TRAMS, PLAIN):
        one, three = A.Batch(N, 1, 0), A.Batch(N, 1, devices=[0, 1, 2])
        assert [(d, f) for d, f, _ in three.shards()] == [(0, 0), (1, 320), (2, 576)], three.shards()
        for h in (one, three):
            assert h.load_text(text), h.errors()
        img, rec = distinct(one, 19)
        assert np.array_equal(distinct(three, 19)[1], rec)
        assert three.instance_words == img.words
        # inside shards, across every pair of shards, a source fanned out over all three
        src = [0, 5, 330, 600, 319, 320, 807, 576, 100, 100, 100, 400]
        dst = [1, 321, 6, 322, 577, 2, 3, 575, 101, 500, 700, 806]
        for h in (one, three):
            h.copy_instances(src, dst)
        rec[dst] = rec[src]
        assert np.array_equal(state_of(one), rec) and np.array_equal(state_of(three), rec)
        assert three.info("instance_gathers") >= 3 and three.info("instance_scatters") >= 3
        # save in an order that interleaves the shards, load into another interleaving (of both handles, from the other's image)
        order, into = [807, 0, 320, 319, 576, 575, 7], [10, 577, 11, 330, 12, 806, 331]
        images = [h.save_instances(order) for h in (one, three)]
        assert np.array_equal(images[0], images[1]) and np.array_equal(instance_records(images[0], img.words), rec[order])
        one.load_instances(into, images[1])
        three.load_instances(into, images[0])
        rec[into] = rec[order]
        assert np.array_equal(state_of(one), rec) and np.array_equal(state_of(three), rec)
        group = [0, 319, 320, 575, 576, 807]
        for h in (one, three):
            h.reset_instances(group)
        fresh = fresh_record(A, text, 64, img)
        keep = slice(img.cursors, img.cursors + 4)
        held = rec[group, keep].copy()
        rec[group] = fresh
        rec[group, keep] = held
        assert np.array_equal(state_of(one), rec) and np.array_equal(state_of(three), rec)
        # refusals go by the whole batch
        before = three.save_state()
        p = lambda v: C.c_void_p(v.ctypes.data)
        assert lib.fxb_copy_instances(three._h, p(i64([0, 400])), p(i64([700, 0])), 2) == FX_E_ARG
        assert lib.fxb_copy_instances(three._h, p(i64([0, 400])), p(i64([700, N])), 2) == FX_E_ARG
        assert lib.fxb_reset_instances(three._h, p(i64([1, 700, 1])), 3) == FX_E_ARG
        assert np.array_equal(three.save_state(), before)
    assert lib.fxstub_cross_device_errors() == 0
    print("instances shards ok")


if __name__ == "__main__":
    {"indexing": child_indexing, "consistency": child_consistency, "refusals": child_refusals, "pieces": child_pieces, "reset": child_reset, "load": child_load,
     "streams": child_streams, "shards": child_shards}[sys.argv[1]]()
