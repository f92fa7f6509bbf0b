"""fxb_load_instances_rotated without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process as tests/test_instances_stub.py does (this file
is also that child; the image helpers are that file's).  The stand-in of the kernel fx_inst_scatter_rot
(tests/hipstub/fx_instances_rot_stub.cpp) does the real move with an addressing of its own.  Every check is equality of 32-bit
patterns over the WHOLE state block: an image with chosen delay-line positions and random words goes in through fxb_load_state,
records are saved and loaded rotated, the image comes back through fxb_save_state and must equal numpy.roll applied to the records
- which also says that the four position rows and every instance outside the list keep what they held.  Refusals launch nothing
and leave the block byte-identical.  The indexing and the refusals run again as a program of their own under ASan + UBSan
(tests/hipstub/instance_rot_checks.cpp).  Parity with the emulation itself is tests/test_gpu_instances_rot.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_ARG = -3
SIZES = [1, 5, 7, 63, 64, 65, 1000]
PLAIN = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend"
# iTRAM a ring of 64, xTRAM written at offset 3: 503 slots for a line of 500, no ring
OFFSET = ("itramsize 64 \nxtramsize 500 \ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 7\n"
          "xdelay write, in, at, 3\nxdelay read, xr, at, 403\nmacs out, r1, xr, vol\nend")
WRITE_ONLY = "itramsize 8 \ninput in 0\noutput out 0\nidelay write, in, at, 0\nmacs out, in, 0, 0\nend"
LONG = ("itramsize 8192 \nxtramsize 8192 \ninput in 0\noutput out 0\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 8000\n"
        "xdelay write, in, at, 0\nxdelay read, xr, at, 8100\nmacs out, r1, xr, 0.5\nend")
SCRATCH = 64 << 20


def rings(zi, zx):
    """one write at offset 0 and one read per line: both lines are rings, both position kinds count"""
    return ("itramsize %d \nxtramsize %d \ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, %d\n"
            "xdelay write, in, at, 0\nxdelay read, xr, at, %d\nmacs out, r1, xr, vol\nend" % (zi, zx, min(3, zi - 1), min(2, zx - 1)))


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_rotation_equals_numpy_roll_on_every_word():
    run_child("rotation", "rotated rotation ok")


def test_rotated_refusals_launch_nothing_and_change_nothing():
    run_child("refusals", "rotated refusals ok")


def test_rotated_load_above_the_scratch_limit_runs_in_pieces():
    run_child("pieces", "rotated pieces ok")


def test_rotated_load_on_three_shards():
    run_child("shards", "rotated shards ok", devices=3)


def test_rotated_load_promotes_registers_and_equals_the_plain_load_at_rotation_zero():
    run_child("load", "rotated load ok")


def test_rotated_indexing_and_refusals_under_asan():
    """the same ground as a stand-alone program with the sanitizers linked in: nothing is preloaded into python"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasanrot"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "instance_rot_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "instance rotation checks ok" in r.stdout, r.stdout[-4000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
    import test_instances_stub as base
    A, lib = base.stub_library()
    for f in ("fxstub_inst_rotations", "fxstub_inst_rotation_strays"):
        getattr(lib, f).restype = C.c_long
    return base, A, lib


def handle(A, text, N, cols=64, devices=None, dane=False):
    """cols 128 / 256: the HIP tier with 2 / 4 instances per lane tiles the delay memory that wide (read at creation)"""
    for k in ("FX_KERNEL", "FX_INST_PER_LANE"):
        os.environ.pop(k, None)
    if cols != 64:
        os.environ.update(FX_KERNEL="hip", FX_INST_PER_LANE=str(cols // 64))
    b = A.Batch(N, 1, 0) if devices is None else A.Batch(N, 1, devices=devices)
    if dane:
        b.set_option(A.OPT_TRAM_DANE)
    assert b.load_text(text), b.errors()
    assert b.info("itram_slots") + b.info("xtram_slots") == 0 or b.info("inst_per_lane") == cols // 64
    return b


def sizes_of(img, zi, zx):
    """(first word, ring size) of the two lines of a record"""
    return (img.rows, zi), (img.rows + img.islots, zx)


def filled(base, A, b, text, seed, positions):
    """b with random words (NaN patterns among them) in the delay memory, the latches, the LFSR, flag and counter rows and the
    program's own state registers, and `positions` [N, 4] in the position rows, through fxb_load_state.  The rows of the literals
    stay: other words in a delay-line offset would make it per-instance and the line would stop being a ring.  Returns the image
    and its records."""
    img = base.Image(b.save_state())
    rng = np.random.default_rng(seed)
    rec = img.records()
    noise = rng.integers(0, 1 << 32, rec.shape, dtype=np.uint64).astype(np.uint32)
    noise[::7, ::5] |= 0x7FC00000                                            # quiet NaNs with payloads
    noise[3::11, 1::3] = (noise[3::11, 1::3] & 0x003FFFFF) | 0x7F800001       # signalling NaNs
    f = A.FrontEnd(1)
    assert f.load_text(text)
    names = [r[0] for r in f.registers()]
    free = [names.index(n) for n in ("r1", "xr", "a") if n in names] + list(range(img.regs, img.cursors)) + list(range(img.cursors + 4, img.words))
    rec[:, free] = noise[:, free]
    rec[:, img.cursors:img.cursors + 4] = np.asarray(positions, dtype=np.uint32)
    b.load_state(img.with_records(rec))
    assert Image_words(base, b) == img.words and np.array_equal(base.state_of(b), rec)
    return img, rec


def Image_words(base, b):
    return base.Image(b.save_state()).words


def rolled(img, rec, src, dst, lines, shifts):
    """what the block must hold after records of `src` went into `dst` with shifts [count, 2]: every word of the source but the four
    position words, the ring part of each line rolled"""
    want = rec.copy()
    for k, (s, d) in enumerate(zip(src, dst)):
        row = rec[s].copy()
        for line, (first, z) in enumerate(lines):
            row[first:first + z] = np.roll(rec[s, first:first + z], int(shifts[k][line]))
        row[img.cursors:img.cursors + 4] = rec[d, img.cursors:img.cursors + 4]
        want[d] = row
    return want


class Counts:
    """(rotations, scatters, gathers) since the last look: the stand-ins' counters and the handle's selectors must agree"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        self.b.sync()
        return (self.lib.fxstub_inst_rotations(), self.b.info("instance_rotations"), self.lib.fxstub_inst_scatters(), self.b.info("instance_scatters"),
                self.lib.fxstub_inst_gathers(), self.lib.fxstub_kernels_run())

    def expect(self, what, rotations, scatters=0, gathers=0):
        now = self.now()
        got = tuple(a - b for a, b in zip(now, self.seen))
        assert got == (rotations, rotations, scatters, scatters, gathers, 0), (what, got)
        self.seen = now


def positions_for(rng, N, zi, zx, src, dst, shifts):
    """positions [N, 4] (iTRAM write, iTRAM read, xTRAM write, xTRAM read), random per instance, with those of src[k] placed
    shifts[k] behind those of dst[k] on each line - both kinds by the same amount, as on a handle that has run"""
    pos = np.stack([rng.integers(0, zi, N), rng.integers(0, zi, N), rng.integers(0, zx, N), rng.integers(0, zx, N)], axis=1).astype(np.int64)
    for k, (s, d) in enumerate(zip(src, dst)):
        di, dx = int(shifts[k][0]), int(shifts[k][1])
        pos[s] = [(pos[d, 0] - di) % zi, (pos[d, 1] - di) % zi, (pos[d, 2] - dx) % zx, (pos[d, 3] - dx) % zx]
    return pos


def shift_set(z):
    return sorted({0, 1 % z, z - 1, z // 2})


def child_rotation():
    base, A, lib = stub_library()
    N = 300
    rng = np.random.default_rng(11)
    # destinations on both sides of the column-tile boundaries of 64, 128 and 256 columns, sources likewise
    edge_dst = [127, 128, 255, 256, 63, 64, 191, 192, 0, 299]
    edge_src = [126, 129, 254, 257, 62, 65, 190, 193, 1, 298]
    rest = [i for i in range(N) if i not in edge_dst and i not in edge_src]
    for cols in (64, 128, 256):
        for zi, zx in zip(SIZES, SIZES[1:] + SIZES[:1]):
            text = rings(zi, zx)
            b = handle(A, text, N, cols)
            assert b.info("instance_rings") == 3 and b.info("itram_slots") == zi and b.info("xtram_slots") == zx
            count = Counts(lib, b)
            for entries in (1, 64, 65):
                src = (edge_src + rest[:60])[:entries] if entries > 1 else [129]
                dst = (edge_dst + rest[60:120])[:entries] if entries > 1 else [128]
                si, sx = shift_set(zi), shift_set(zx)
                # another rotation per record, the two lines out of step with each other
                shifts = [(si[k % len(si)], sx[(k + 1 + k // len(si)) % len(sx)]) for k in range(entries)]
                pos = positions_for(rng, N, zi, zx, src, dst, shifts)
                img, rec = filled(base, A, b, text, 100 * zi + entries, pos)
                image = b.save_instances(src)
                count.expect("save", 0, 0, 1)
                assert b.load_instances_rotated(dst, image) == 0
                count.expect("rotated load", 1)
                got = base.state_of(b)
                want = rolled(img, rec, src, dst, sizes_of(img, zi, zx), shifts)
                assert np.array_equal(got, want), (cols, zi, zx, entries, np.argwhere(got != want)[:8])
            assert b.load_instances_rotated([], b.save_instances([])) == 0
            count.expect("empty", 0)
    # a line that is no ring beside one that is: the ring rotates, the other is copied as it is (and must stand at the same place)
    b = handle(A, OFFSET, 200)
    assert b.info("instance_rings") == 1 and b.info("xtram_slots") == 503
    src, dst = [0, 63, 130], [5, 64, 199]
    shifts = [(5, 0), (0, 0), (63, 0)]
    pos = positions_for(rng, 200, 64, 500, src, dst, shifts)
    img, rec = filled(base, A, b, OFFSET, 77, pos)
    assert b.load_instances_rotated(dst, b.save_instances(src)) == 0
    assert np.array_equal(base.state_of(b), rolled(img, rec, src, dst, ((img.rows, 64), (img.rows + 64, 0)), shifts))
    # a line the program only writes: the read position never moves and does not count
    b = handle(A, WRITE_ONLY, 70)
    assert b.info("instance_rings") == 1
    pos = np.zeros((70, 4), dtype=np.int64)
    pos[:, 0] = np.arange(70) % 8
    pos[:, 1] = (np.arange(70) * 3) % 8
    img, rec = filled(base, A, b, WRITE_ONLY, 78, pos)
    src, dst = [1, 2, 3], [69, 7, 64]
    shifts = [((pos[d, 0] - pos[s, 0]) % 8, 0) for s, d in zip(src, dst)]
    assert b.load_instances_rotated(dst, b.save_instances(src)) == 0
    assert np.array_equal(base.state_of(b), rolled(img, rec, src, dst, ((img.rows, 8), (img.rows + 8, 0)), shifts))
    # the DANE model: one counter per line in the write word, the read words are not compared
    b = handle(A, rings(7, 11), 70, dane=True)
    assert b.info("instance_rings") == 3
    pos = positions_for(rng, 70, 7, 11, [], [], [])
    img, rec = filled(base, A, b, rings(7, 11), 79, pos)
    src, dst = [0, 1, 65], [64, 63, 2]
    shifts = [((pos[d, 0] - pos[s, 0]) % 7, (pos[d, 2] - pos[s, 2]) % 11) for s, d in zip(src, dst)]
    assert b.load_instances_rotated(dst, b.save_instances(src)) == 0
    assert np.array_equal(base.state_of(b), rolled(img, rec, src, dst, sizes_of(img, 7, 11), shifts))
    # without delay-line instructions the call is the plain load, whatever the position words say
    c = handle(A, PLAIN, 200)
    assert c.info("instance_rings") == 0
    _, rec = base.distinct(c, 7, same_cursors=False)
    count = Counts(lib, c)
    assert c.load_instances_rotated([199, 0], c.save_instances([3, 64])) == 0
    count.expect("no delay lines: the scatter", 0, 1, 1)
    rec[[199, 0]] = rec[[3, 64]]
    assert np.array_equal(base.state_of(c), rec)
    assert lib.fxstub_inst_rotation_strays() == 0 and lib.fxstub_cross_device_errors() == 0
    print("rotated rotation ok")


def child_refusals():
    base, A, lib = stub_library()
    N = 200
    p = lambda v: C.c_void_p(v.ctypes.data if v is not None else 0)
    rng = np.random.default_rng(5)

    def words_of(image, img):
        return image[64:].view(np.uint32).reshape(-1, img.words)

    for text, zi, zx, ring_x in ((rings(64, 65), 64, 65, True), (OFFSET, 64, 500, False)):
        b = handle(A, text, N)
        src, dst = [0, 63, 130], [5, 64, 199]
        pos = positions_for(rng, N, zi, zx, src, dst, [(5, 0), (0, 0), (63, 0)])
        img, rec = filled(base, A, b, text, 31, pos)
        before = b.save_state()
        good = b.save_instances(src)
        count = Counts(lib, b)
        d3 = base.i64(dst)

        def refused(what, image, names=(), nbytes=None, lst=d3, n=3):
            rc = lib.fxb_load_instances_rotated(b._h, p(lst), n, p(image), image.size if nbytes is None else nbytes)
            assert rc == FX_E_ARG, (what, rc, b.last_error())
            for name in names:
                assert name in b.last_error(), (what, b.last_error())
            count.expect(what, 0)
            assert np.array_equal(b.save_state(), before), what

        cur = img.cursors
        for word, line in ((0, "iTRAM"), (1, "iTRAM"), (2, "xTRAM"), (3, "xTRAM")):
            bad = good.copy()
            words_of(bad, img)[2, cur + word] = (zi, zx)[word // 2]
            refused("a position word of the record at the line's size", bad, (line, "entry 2"))
            bad = good.copy()
            words_of(bad, img)[1, cur + word] = 0xFFFFFFFF
            refused("a position word of the record far outside", bad, (line, "entry 1"))
            # one kind moved alone: the write and the read position are no longer at one distance from the destination's
            bad = good.copy()
            w = words_of(bad, img)
            w[1, cur + word] = (int(w[1, cur + word]) + 1) % (zi, zx)[word // 2]
            refused("the shifts of the two kinds disagree", bad, (line, "entry 1"))
        if not ring_x:
            bad = good.copy()
            w = words_of(bad, img)
            w[0, cur + 2:cur + 4] = (w[0, cur + 2:cur + 4].astype(np.int64) + 499) % 500
            refused("a rotation on a line that is no ring", bad, ("xTRAM", "entry 0", "ring"))
        # the refusals of the plain load
        refused("truncated", good, nbytes=good.size - 4)
        refused("no header", good, nbytes=63)
        refused("another count than the image's", good, n=2)
        refused("repeated destination", good, lst=base.i64([4, 4, 6]))
        refused("beyond the batch", good, lst=base.i64([4, 5, N]))
        assert lib.fxb_load_instances_rotated(b._h, p(None), 3, p(good), good.size) == FX_E_ARG
        assert lib.fxb_load_instances_rotated(b._h, p(d3), 3, p(None), good.size) == FX_E_ARG
        whole = good.copy()
        whole[:4] = before[:4]
        refused("a whole-batch image's kind", whole)
        for at in (4, 16, 20, 24, 28, 32):
            other = good.copy()
            other[at:at + 4].view(np.int32)[0] += 1
            refused("another shape at byte %d" % at, other)
        count.expect("all refusals", 0)
        assert np.array_equal(b.save_state(), before)
        # ... and the good image still loads
        assert b.load_instances_rotated(dst, good) == 0
        count.expect("the good image", 1)
        lines = ((img.rows, zi), (img.rows + img.islots, zx if ring_x else 0))
        assert np.array_equal(base.state_of(b), rolled(img, rec, src, dst, lines, [(5, 0), (0, 0), (63, 0)]))
    assert lib.fxb_load_instances_rotated(None, p(d3), 3, p(good), good.size) == FX_E_ARG
    e = A.Batch(8, 1, 0)
    assert lib.fxb_load_instances_rotated(e._h, p(base.i64([0])), 0, p(None), 0) == -2   # FX_E_NOTREADY without a program
    assert lib.fxstub_inst_rotation_strays() == 0
    print("rotated refusals ok")


def child_pieces():
    base, A, lib = stub_library()
    N = 1100
    b = handle(A, LONG, N)
    W = b.instance_words
    per = SCRATCH // (W * 4)
    assert W > 16384 and 1000 < per < N, (W, per)
    rng = np.random.default_rng(3)
    rec = rng.integers(0, 1 << 32, (N, W), dtype=np.uint64).astype(np.uint32)
    cursors = b.info("num_registers") + 1
    rows = W - 2 * 8192
    head = base.instance_records(b.save_instances([0]), W)[0, :cursors + 4]
    rec[:, :cursors + 4] = head       # registers and positions of a handle that has processed nothing: w = r = 0 on both lines
    shifts = np.stack([np.arange(N) * 37 % 8192, np.arange(N) * 101 % 8192], axis=1)
    # record k stands `shifts[k]` behind the destination on each line
    rec[:, cursors + 0] = rec[:, cursors + 1] = (8192 - shifts[:, 0]) % 8192
    rec[:, cursors + 2] = rec[:, cursors + 3] = (8192 - shifts[:, 1]) % 8192
    image = np.empty(64 + N * W * 4, dtype=np.uint8)
    image[:64] = b.save_instances([])[:64]
    image[8:16].view(np.int64)[0] = N
    image[64:] = rec.view(np.uint8).ravel()
    count = Counts(lib, b)
    order = np.arange(N)[::-1].copy()
    assert b.load_instances_rotated(order, image) == 0
    count.expect("rotated load of 1100 records: two pieces", 2)
    got = base.state_of(b)
    for k in (0, 1, per - 1, per, per + 1, N - 1):   # both sides of the piece boundary: every piece takes ITS rotations
        inst = order[k]
        assert np.array_equal(got[inst, rows:rows + 8192], np.roll(rec[k, rows:rows + 8192], shifts[k, 0])), k
        assert np.array_equal(got[inst, rows + 8192:], np.roll(rec[k, rows + 8192:], shifts[k, 1])), k
        assert np.array_equal(got[inst, cursors + 4:rows], rec[k, cursors + 4:rows]) and not got[inst, cursors:cursors + 4].any(), k
    assert lib.fxstub_inst_rotation_strays() == 0
    print("rotated pieces ok")


def child_shards():
    base, A, lib = stub_library()
    N = 3 * 256 + 40
    rng = np.random.default_rng(23)
    zi, zx = 63, 65
    text = rings(zi, zx)
    one, three = handle(A, text, N), handle(A, text, N, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in three.shards()] == [(0, 0), (1, 320), (2, 576)], three.shards()
    # sources and destinations interleave the shards; saved from the one handle, loaded into both (and the other way round)
    src, dst = [807, 0, 320, 319, 576, 575, 7], [10, 577, 11, 330, 12, 806, 331]
    shifts = [(k * 9 % zi, (k * 5 + 1) % zx) for k in range(len(src))]
    pos = positions_for(rng, N, zi, zx, src, dst, shifts)
    img, rec = filled(base, A, one, text, 19, pos)
    assert np.array_equal(filled(base, A, three, text, 19, pos)[1], rec)
    images = [h.save_instances(src) for h in (one, three)]
    assert np.array_equal(images[0], images[1])
    assert one.load_instances_rotated(dst, images[1]) == 0 and three.load_instances_rotated(dst, images[0]) == 0
    want = rolled(img, rec, src, dst, sizes_of(img, zi, zx), shifts)
    assert np.array_equal(base.state_of(one), want) and np.array_equal(base.state_of(three), want)
    assert np.array_equal(one.save_state(), three.save_state())
    assert one.info("instance_rotations") == 1 and three.info("instance_rotations") == 3 and three.info("instance_scatters") == 0
    # a refusal on one shard: no shard changes a word
    before = three.save_state()
    bad = images[0].copy()
    bad[64:].view(np.uint32).reshape(len(src), -1)[5, img.cursors] ^= 1   # (the record for instance 806, on the last shard)
    p = lambda v: C.c_void_p(v.ctypes.data)
    assert lib.fxb_load_instances_rotated(three._h, p(base.i64(dst)), len(dst), p(bad), bad.size) == FX_E_ARG and "iTRAM" in three.last_error()
    assert lib.fxb_load_instances_rotated(three._h, p(base.i64([1, 700, 1])), 3, p(bad), bad.size) == FX_E_ARG
    assert np.array_equal(three.save_state(), before) and three.info("instance_rotations") == 3
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_inst_rotation_strays() == 0
    print("rotated shards ok")


def child_load():
    base, A, lib = stub_library()
    N = 200
    rng = np.random.default_rng(41)
    text = rings(64, 1000)
    # rotation 0 everywhere: the bytes of the plain load
    u, v = handle(A, text, N), handle(A, text, N)
    src, dst = [0, 63, 130], [5, 64, 199]
    pos = positions_for(rng, N, 64, 1000, src, dst, [(0, 0)] * 3)
    for h in (u, v):
        filled(base, A, h, text, 43, pos)
    image = u.save_instances(src)
    count = Counts(lib, u)
    assert u.load_instances(dst, image) == 0
    count.expect("plain", 0, 1)
    count = Counts(lib, v)
    assert v.load_instances_rotated(dst, image) == 0
    count.expect("rotated: the new kernel, rotation 0 included", 1, 0)
    assert np.array_equal(u.save_state(), v.save_state())
    # promotion: a register the destination holds as one value becomes per-instance when a record has another
    s, t = handle(A, text, N), handle(A, text, N)
    for h, samples in ((s, 4), (t, 9)):
        h.process_block(np.zeros((samples, N), dtype=np.float32))
    assert s.set_register_i("vol", 3, 0.25) == 0
    rows = t.info("num_lane_regs")
    assert t.get_register_i("vol", 7) == 0.5
    assert t.load_instances_rotated([7, 128], s.save_instances([3, 4])) == 0
    assert t.get_register_i("vol", 7) == 0.25 and t.get_register_i("vol", 128) == 0.5
    assert t.get_register_i("vol", 8) == 0.5 and t.get_register_i("vol", 199) == 0.5, "the broadcast value of the other instances"
    assert t.info("num_lane_regs") == rows + 1, "vol has a row of its own from now on"
    assert t.info("instance_rings") == 3, "still rings after the lowering that followed"
    w = handle(A, text, N)
    w.process_block(np.zeros((4, N), dtype=np.float32))
    rows = w.info("num_lane_regs")
    assert w.load_instances_rotated([1], t.save_instances([9])) == 0 and w.info("num_lane_regs") == rows
    print("rotated load ok")


if __name__ == "__main__":
    {"rotation": child_rotation, "refusals": child_refusals, "pieces": child_pieces, "shards": child_shards, "load": child_load}[sys.argv[1]]()
