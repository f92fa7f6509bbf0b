"""The record bank (fxb_bank_*) without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process as tests/test_instances_rot_stub.py does (this
file is also that child; the image helpers are that file's and tests/test_instances_stub.py's).  The stand-ins of the three kernels
(tests/hipstub/fx_bank_stub.cpp) do the real moves with an addressing of their own.  Every check is equality of 32-bit patterns over
the WHOLE state block: an image with chosen delay-line positions and random words goes in through fxb_load_state, records are
stored and recalled, the image comes back through fxb_save_state and must equal numpy.roll applied to the records.  What the device
refuses leaves the block byte-identical and shows in fxb_bank_status.  The indexing, the gates and the refusals run again as a
program of their own under ASan + UBSan (tests/hipstub/bank_checks.cpp).  Parity with the emulation itself is
tests/test_gpu_bank.py."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")
FX_E_ARG, FX_E_MEMORY = -3, -5
BAD_POSITION, PHASE, NO_RING = 1, 2, 3


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_store_and_recall_equal_numpy_roll_on_every_word():
    run_child("moves", "bank moves ok")


def test_the_three_gates_are_all_or_nothing():
    run_child("gates", "bank gates ok")


def test_bank_on_three_devices():
    run_child("shards", "bank shards ok", devices=3)


def test_bank_memory_is_refused_whole_and_given_back():
    run_child("memory", "bank memory ok")


def test_store_and_recall_do_not_wait_for_the_queued_block():
    run_child("queued", "bank queued ok")


def test_bank_registers_follow_the_shadow():
    run_child("registers", "bank registers ok", devices=3)


def test_bank_indexing_gates_and_refusals_under_asan():
    """the same ground as a stand-alone program with the sanitizers linked in: nothing is preloaded into python"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasanbank"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "bank_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "record bank checks ok" in r.stdout, r.stdout[-4000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def stub_library():
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
    import test_instances_rot_stub as rot
    base, A, lib = rot.stub_library()
    for f in ("fxstub_bank_gathers", "fxstub_bank_rotations", "fxstub_bank_scatters", "fxstub_bank_gated", "fxstub_bank_strays"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_bytes_in_use.restype = C.c_ulonglong
    lib.fxstub_fail_mallocs.argtypes = [C.c_long, C.c_long]
    lib.fxstub_fail_mallocs.restype = None
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    return rot, base, A, lib


class Counts:
    """(gathers, rotations, scatters) of the bank since the last look: the stand-ins' counters and the handle's selectors must
    agree, the instance kernels and the emulation must not have run"""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        self.seen = self.now()

    def now(self):
        self.b.sync()
        lib, b = self.lib, self.b
        return (lib.fxstub_bank_gathers(), b.info("bank_stores"), lib.fxstub_bank_rotations(), lib.fxstub_bank_scatters(), b.info("bank_recalls"),
                lib.fxstub_inst_rotations() + lib.fxstub_inst_scatters() + lib.fxstub_inst_gathers() + lib.fxstub_kernels_run())

    def expect(self, what, gathers=0, rotations=0, scatters=0):
        now = self.now()
        got = tuple(a - b for a, b in zip(now, self.seen))
        assert got == (gathers, gathers, rotations, scatters, scatters, 0), (what, got)
        self.seen = now


def child_moves():
    rot, base, A, lib = stub_library()
    N = 300
    rng = np.random.default_rng(17)
    edge_dst = [127, 128, 255, 256, 63, 64, 191, 192, 0, 299]
    edge_src = [126, 129, 254, 257, 62, 65, 190, 193, 1, 298]
    rest = [i for i in range(N) if i not in edge_dst and i not in edge_src]
    for cols in (64, 128, 256):
        for zi, zx in zip(rot.SIZES, rot.SIZES[1:] + rot.SIZES[:1]):
            if cols != 64 and zi not in (63, 64, 1000):
                continue   # (the wider column tiles: the ring sizes around the word tile, and the long one)
            text = rot.rings(zi, zx)
            b = rot.handle(A, text, N, cols)
            assert b.info("instance_rings") == 3
            for entries in (1, 64, 65):
                src = (edge_src + rest[:60])[:entries] if entries > 1 else [129]
                dst = (edge_dst + rest[60:120])[:entries] if entries > 1 else [128]
                si, sx = rot.shift_set(zi), rot.shift_set(zx)
                shifts = [(si[k % len(si)], sx[(k + 1 + k // len(si)) % len(sx)]) for k in range(entries)]
                pos = rot.positions_for(rng, N, zi, zx, src, dst, shifts)
                img, rec = rot.filled(base, A, b, text, 100 * zi + entries, pos)
                assert b.bank_create(entries + 2) == 0 and b.info("bank_bytes") == (entries + 2) * img.words * 4
                slots = np.arange(entries + 1, 1, -1)   # in reverse, the last slot of the bank among them
                count = Counts(lib, b)
                assert b.bank_store(slots, src) == 0
                count.expect("store", gathers=1)
                assert np.array_equal(b.bank_get(slots), b.save_instances(src)), "store then get: the bytes of save_instances"
                assert not b.bank_get([0, 1])[64:].any(), "a slot nobody stored to"
                count = Counts(lib, b)
                assert b.bank_recall(slots, dst) == 0
                count.expect("recall", rotations=1, scatters=1)
                assert b.bank_status() == (0, -1, 0)
                got = base.state_of(b)
                want = rot.rolled(img, rec, src, dst, rot.sizes_of(img, zi, zx), shifts)
                assert np.array_equal(got, want), (cols, zi, zx, entries, np.argwhere(got != want)[:8])
            assert b.bank_store([], []) == 0 and b.bank_recall([], []) == 0
    # fan-out: one slot into many destinations, each at a rotation of its own
    zi, zx = 7, 1000
    text = rot.rings(zi, zx)
    b = rot.handle(A, text, N)
    dst = list(range(3, 3 + 70))
    shifts = [(k % zi, (k * 37) % zx) for k in range(70)]
    pos = rot.positions_for(rng, N, zi, zx, [200] * 70, dst, [(0, 0)] * 70)
    for k, d in enumerate(dst):   # the one source stands still, every destination `shifts[k]` ahead of it
        pos[d] = [(pos[200, 0] + shifts[k][0]) % zi, (pos[200, 1] + shifts[k][0]) % zi, (pos[200, 2] + shifts[k][1]) % zx, (pos[200, 3] + shifts[k][1]) % zx]
    img, rec = rot.filled(base, A, b, text, 5, pos)
    assert b.bank_create(1) == 0 and b.bank_put([0], b.save_instances([200])) == 0
    assert b.bank_recall([0] * 70, dst) == 0 and b.bank_status() == (0, -1, 0)
    assert np.array_equal(base.state_of(b), rot.rolled(img, rec, [200] * 70, dst, rot.sizes_of(img, zi, zx), shifts))
    # a line that is no ring beside one that is; the DANE model; a line the program only writes
    b = rot.handle(A, rot.OFFSET, 200)
    src, dst, shifts = [0, 63, 130], [5, 64, 199], [(5, 0), (0, 0), (63, 0)]
    img, rec = rot.filled(base, A, b, rot.OFFSET, 77, rot.positions_for(rng, 200, 64, 500, src, dst, shifts))
    assert b.bank_create(3) == 0 and b.bank_store([0, 1, 2], src) == 0 and b.bank_recall([0, 1, 2], dst) == 0 and b.bank_status() == (0, -1, 0)
    assert np.array_equal(base.state_of(b), rot.rolled(img, rec, src, dst, ((img.rows, 64), (img.rows + 64, 0)), shifts))
    b = rot.handle(A, rot.rings(7, 11), 70, dane=True)
    pos = rot.positions_for(rng, 70, 7, 11, [], [], [])
    img, rec = rot.filled(base, A, b, rot.rings(7, 11), 79, pos)
    src, dst = [0, 1, 65], [64, 63, 2]
    shifts = [((pos[d, 0] - pos[s, 0]) % 7, (pos[d, 2] - pos[s, 2]) % 11) for s, d in zip(src, dst)]
    assert b.bank_create(3) == 0 and b.bank_store([2, 1, 0], src) == 0 and b.bank_recall([2, 1, 0], dst) == 0 and b.bank_status() == (0, -1, 0)
    assert np.array_equal(base.state_of(b), rot.rolled(img, rec, src, dst, rot.sizes_of(img, 7, 11), shifts))
    b = rot.handle(A, rot.WRITE_ONLY, 70)
    pos = np.zeros((70, 4), dtype=np.int64)
    pos[:, 0], pos[:, 1] = np.arange(70) % 8, (np.arange(70) * 3) % 8
    img, rec = rot.filled(base, A, b, rot.WRITE_ONLY, 78, pos)
    src, dst = [1, 2, 3], [69, 7, 64]
    shifts = [((pos[d, 0] - pos[s, 0]) % 8, 0) for s, d in zip(src, dst)]
    assert b.bank_create(3) == 0 and b.bank_store([0, 1, 2], src) == 0 and b.bank_recall([0, 1, 2], dst) == 0 and b.bank_status() == (0, -1, 0)
    assert np.array_equal(base.state_of(b), rot.rolled(img, rec, src, dst, ((img.rows, 8), (img.rows + 8, 0)), shifts))
    # without delay-line instructions: the plain scatter, no rotations kernel, whatever the position words say
    c = rot.handle(A, rot.PLAIN, 200)
    _, rec = base.distinct(c, 7, same_cursors=False)
    assert c.bank_create(2) == 0
    count = Counts(lib, c)
    assert c.bank_store([1, 0], [3, 64]) == 0 and c.bank_recall([1, 0], [199, 0]) == 0
    count.expect("no delay lines", gathers=1, rotations=0, scatters=1)
    rec[[199, 0]] = rec[[3, 64]]
    assert np.array_equal(base.state_of(c), rec)
    assert lib.fxstub_bank_strays() == 0 and lib.fxstub_cross_device_errors() == 0
    print("bank moves ok")


def child_gates():
    rot, base, A, lib = stub_library()
    N = 200
    rng = np.random.default_rng(5)
    for text, zi, zx, ring_x in ((rot.rings(64, 65), 64, 65, True), (rot.OFFSET, 64, 500, False)):
        b = rot.handle(A, text, N)
        src, dst, shifts = [0, 63, 130, 7, 9], [5, 64, 199, 100, 101], [(5, 0), (0, 0), (63, 0), (1, 0), (2, 0)]
        pos = rot.positions_for(rng, N, zi, zx, src, dst, shifts)
        img, rec = rot.filled(base, A, b, text, 31, pos)
        before = b.save_state()
        good = b.save_instances(src)
        assert b.bank_create(5) == 0
        slots = [4, 3, 2, 1, 0]
        cur, refused = img.cursors, 0

        def gated(what, image, entry, reason):
            nonlocal refused
            assert b.bank_put(slots, image) == 0
            count, gates = Counts(lib, b), lib.fxstub_bank_gated()
            assert b.bank_recall(slots, dst) == 0, "a recall the device refuses returns 0"
            count.expect(what, rotations=1, scatters=1)
            refused += 1
            assert lib.fxstub_bank_gated() == gates + 1 and b.bank_status() == (refused, entry, reason), (what, b.bank_status())
            assert np.array_equal(b.save_state(), before), what

        words = lambda image: image[64:].view(np.uint32).reshape(-1, img.words)
        for word in range(4):
            z = (zi, zx)[word // 2]
            bad = good.copy()
            words(bad)[2, cur + word] = z
            gated("a position word of the record at the line's size", bad, 2, BAD_POSITION)
            bad = good.copy()
            words(bad)[1, cur + word] = 0xFFFFFFFF
            words(bad)[3, cur + word] = z + 1
            gated("two bad records: the lowest entry", bad, 1, BAD_POSITION)
            bad = good.copy()
            words(bad)[3, cur + word] = (int(words(bad)[3, cur + word]) + 1) % z
            gated("the shifts of the two kinds disagree", bad, 3, PHASE)
        if not ring_x:
            bad = good.copy()
            words(bad)[2, cur + 2:cur + 4] = (words(bad)[2, cur + 2:cur + 4].astype(np.int64) + 499) % 500
            gated("a rotation on a line that is no ring", bad, 2, NO_RING)
        assert b.bank_status(reset=True)[0] == refused and b.bank_status() == (0, -1, 0)
        # ... and the good image still recalls
        assert b.bank_put(slots, good) == 0 and b.bank_recall(slots, dst) == 0 and b.bank_status() == (0, -1, 0)
        lines = ((img.rows, zi), (img.rows + img.islots, zx if ring_x else 0))
        assert np.array_equal(base.state_of(b), rot.rolled(img, rec, src, dst, lines, shifts))
    assert lib.fxstub_bank_strays() == 0
    print("bank gates ok")


def child_shards():
    rot, base, A, lib = stub_library()
    N = 3 * 256 + 40
    rng = np.random.default_rng(23)
    zi, zx = 63, 65
    text = rot.rings(zi, zx)
    one, three = rot.handle(A, text, N), rot.handle(A, text, N, devices=[0, 1, 2])
    assert [(d, f) for d, f, _ in three.shards()] == [(0, 0), (1, 320), (2, 576)], three.shards()
    # sources of every shard, destinations that interleave the shards: every recall of a record from another shard's instance crosses
    src, dst = [807, 0, 320, 319, 576, 575, 7], [10, 577, 11, 330, 12, 806, 331]
    slots = [6, 0, 3, 2, 5, 1, 4]
    shifts = [(k * 9 % zi, (k * 5 + 1) % zx) for k in range(len(src))]
    pos = rot.positions_for(rng, N, zi, zx, src, dst, shifts)
    # further destinations of the same records, for the calls below: each stands a shift of its own ahead of its source
    for k, (s, d) in enumerate(((807, 400), (0, 13), (320, 700), (575, 402), (0, 403))):
        di, dx = 3 + 11 * k, 60 - 7 * k
        pos[d] = [(pos[s, 0] + di) % zi, (pos[s, 1] + di) % zi, (pos[s, 2] + dx) % zx, (pos[s, 3] + dx) % zx]
    img, rec = rot.filled(base, A, one, text, 19, pos)
    assert np.array_equal(rot.filled(base, A, three, text, 19, pos)[1], rec)
    for h in (one, three):
        assert h.bank_create(8) == 0 and h.bank_store(slots, src) == 0
    assert three.info("bank_bytes") == 3 * one.info("bank_bytes") and three.info("bank_slots") == 8 and three.info("bank_stores") == 3
    assert np.array_equal(one.bank_get(slots), three.bank_get(slots)) and np.array_equal(one.bank_get(slots), one.save_instances(src))
    for h in (one, three):
        assert h.bank_recall(slots, dst) == 0 and h.bank_status() == (0, -1, 0)
    want = rot.rolled(img, rec, src, dst, rot.sizes_of(img, zi, zx), shifts)
    assert np.array_equal(base.state_of(one), want) and np.array_equal(base.state_of(three), want)
    assert one.info("bank_recalls") == 1 and three.info("bank_recalls") == 3
    # a bad record, put on every shard: the shard of its destination keeps its part, the other shards' parts run
    bad = one.bank_get([0])
    bad[64:].view(np.uint32)[img.cursors] = zi
    for h in (one, three):
        assert h.bank_put([7], bad) == 0
    before = base.state_of(three)
    call_slots, call_dst = [6, 0, 7, 3, 1], [400, 13, 401, 700, 402]    # entries 0, 2 and 4 fall to the second shard
    assert three.bank_recall(call_slots, call_dst) == 0 and three.bank_status() == (1, 2, BAD_POSITION)
    got = base.state_of(three)
    assert np.array_equal(got[320:576], before[320:576]), "the refused shard's part"
    assert one.bank_recall([0, 3], [13, 700]) == 0 and one.bank_status() == (0, -1, 0)
    assert np.array_equal(got, base.state_of(one))
    # the most recent refused call, and the lowest entry across shards
    assert three.bank_recall([7, 0, 7], [14, 403, 701]) == 0 and three.bank_status() == (3, 0, BAD_POSITION)
    assert three.bank_status(reset=True)[0] == 3 and three.bank_status() == (0, -1, 0)
    assert lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bank_strays() == 0
    print("bank shards ok")


def child_memory():
    rot, base, A, lib = stub_library()
    N = 200
    text = rot.rings(64, 1000)
    floor = lib.fxstub_bytes_in_use()
    b = rot.handle(A, text, N)
    b.process_block(np.zeros((4, N), dtype=np.float32))
    assert b.prepare(4, True) == 0   # (the builder thread is idle: no allocation of its own meets the injected failure)
    W = b.instance_words
    without = lib.fxstub_bytes_in_use()
    for nth in (0, 1):   # the cells, the slots
        lib.fxstub_fail_mallocs(nth, 1)
        rc = lib.fxb_bank_create(b._h, 9)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and b.last_error() and b.bank_slots() == 0, (nth, rc)
        assert lib.fxstub_bytes_in_use() <= without + 64, "a refused create holds no more than the cells"
    assert b.bank_create(9) == 0 and lib.fxstub_bytes_in_use() >= without + 9 * W * 4
    assert b.bank_store([8], [199]) == 0
    kept = b.bank_get([8])
    used = lib.fxstub_bytes_in_use()
    lib.fxstub_fail_mallocs(0, 1)
    rc = lib.fxb_bank_create(b._h, 50)
    lib.fxstub_fail_mallocs(-1, 0)
    assert rc == FX_E_MEMORY and b.bank_slots() == 9 and lib.fxstub_bytes_in_use() == used and np.array_equal(b.bank_get([8]), kept), "the old bank stays in force"
    assert b.bank_create(50) == 0 and b.bank_slots() == 50 and not b.bank_get([8])[64:].any(), "a larger bank keeps nothing of the old"
    with_bank = lib.fxstub_bytes_in_use()
    assert b.load_text("static zz\nmacs zz, zz, 0.5, 0.5\nend"), b.errors()
    assert b.bank_slots() == 0 and lib.fxstub_bytes_in_use() <= with_bank - 50 * W * 4 + 4 * N + 4096, "a program load frees the slots"
    one = base.i64([0])
    assert lib.fxb_bank_recall(b._h, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), 1) == FX_E_ARG and "bank" in b.last_error()
    assert b.bank_create(3) == 0 and b.bank_store([0], [1]) == 0 and b.sync() == 0
    b.close()
    assert lib.fxstub_bytes_in_use() == floor, "destroy gives everything back"
    print("bank memory ok")


def child_queued():
    """a store, and a recall, queued behind a block that takes 30 ms return long before it ends, and still run behind it (two list
    calls behind ONE block: the second waits for the first - the frame's own wait, its lists are in the staging)"""
    rot, base, A, lib = stub_library()
    N, S = 200, 16
    text = rot.rings(64, 65)
    b = rot.handle(A, text, N)
    rng = np.random.default_rng(3)
    src, dst = [0, 63], [64, 199]
    img, rec = rot.filled(base, A, b, text, 13, rot.positions_for(rng, N, 64, 65, src, dst, [(0, 0), (0, 0)]))
    assert b.bank_create(2) == 0 and b.bank_store([0, 1], src) == 0 and b.bank_recall([0, 1], dst) == 0 and b.sync() == 0   # (the staging exists)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    stream = C.c_void_p()
    assert lib.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and stream.value
    x, y = lib.fxb_host_alloc(N * S * 4), lib.fxb_host_alloc(N * S * 4)
    C.memset(x, 0, N * S * 4)
    for own in (None, stream):
        for call in (lambda: b.bank_store([0, 1], src), lambda: b.bank_recall([0, 1], dst)):
            lib.fxstub_set_kernel_micros(30000)
            kernels = lib.fxstub_kernels_run()
            t0 = time.perf_counter()
            assert lib.fxb_process_block_dev(b._h, C.c_void_p(x), C.c_void_p(y), S, own) == 0
            t1 = time.perf_counter()
            assert call() == 0
            t2 = time.perf_counter()
            ran = lib.fxstub_kernels_run() - kernels
            b.sync()
            t3 = time.perf_counter()
            lib.fxstub_set_kernel_micros(0)
            assert ran == 0 and t3 - t0 >= 0.030, "the block was still running when the call had returned"
            assert t2 - t1 < 0.010, "the call took %.1f ms of the host: it waited for the block" % ((t2 - t1) * 1e3)
        got = base.state_of(b)
        assert np.array_equal(got[dst][:, img.cursors + 4:], got[src][:, img.cursors + 4:]), "both ran, behind their blocks"
    lib.fxb_host_free(x)
    lib.fxb_host_free(y)
    print("bank queued ok")


def child_registers():
    rot, base, A, lib = stub_library()
    N = 200
    text = rot.rings(64, 1000)

    def voice():
        b = rot.handle(A, text, N)
        b.process_block(np.zeros((4, N), dtype=np.float32))
        assert b.bank_create(2) == 0
        return b, b.info("num_lane_regs")

    b, rows = voice()
    assert b.bank_store([0], [3]) == 0 and b.bank_recall([0], [7]) == 0 and b.info("num_lane_regs") == rows, "never moved: no other code"
    b, rows = voice()
    assert b.bank_store([0], [3]) == 0 and b.set_register("vol", 0.25) == 0 and b.bank_recall([0], [7]) == 0
    assert b.get_register_i("vol", 7) == 0.5 and b.get_register_i("vol", 8) == 0.25 and b.info("num_lane_regs") == rows + 1
    b, rows = voice()
    assert b.set_register_i("vol", 3, 0.75) == 0 and b.bank_store([0], [3]) == 0 and b.bank_recall([0], [7]) == 0
    assert b.get_register_i("vol", 7) == 0.75 and b.get_register_i("vol", 8) == 0.5
    b, rows = voice()   # a put knows the image's words
    image = b.save_instances([3])
    assert b.bank_put([1], image) == 0 and b.bank_recall([1], [7]) == 0 and b.info("num_lane_regs") == rows
    assert b.set_register("vol", 0.125) == 0 and b.bank_recall([1], [9]) == 0
    assert b.get_register_i("vol", 9) == 0.5 and b.get_register_i("vol", 7) == 0.125 and b.info("num_lane_regs") == rows + 1
    # three devices: a store on one shard, the shadow travels with the slot
    t = rot.handle(A, text, 3 * 256 + 40, devices=[0, 1, 2])
    t.process_block(np.zeros((4, 3 * 256 + 40), dtype=np.float32))
    rows = t.info("num_lane_regs")
    assert t.bank_create(2) == 0 and t.bank_store([1], [5]) == 0 and t.bank_recall([1], [700]) == 0 and t.info("num_lane_regs") == rows
    assert t.set_register("vol", 0.25) == 0 and t.bank_recall([1], [400]) == 0
    assert t.get_register_i("vol", 400) == 0.5 and t.get_register_i("vol", 700) == 0.25 and t.get_register_i("vol", 5) == 0.25
    print("bank registers ok")


if __name__ == "__main__":
    {"moves": child_moves, "gates": child_gates, "shards": child_shards, "memory": child_memory, "queued": child_queued, "registers": child_registers}[sys.argv[1]]()
