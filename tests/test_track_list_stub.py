"""Register tracks by list without a GPU: fxb_set_register_tracks_list on the library's host sources linked against tests/hipstub/
(`make -C fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like
tests/test_register_list_stub.py (this file is also that child).

On the translated tier the stand-ins of the two kernels (tests/hipstub/fx_tracks_stub.cpp) expand the schedules with an addressing
of their own and remember where they wrote: the expanded event rows are read back and compared with a numpy MODEL written from
the definition - the hold value everywhere, the due step's words at the listed voices from that step's event up to the same
schedule's next one.  With FX_KERNEL=hip and FX_KERNEL=asm (the tiers that cut the block) the handle is compared with a TWIN
that cuts the block itself and calls fxb_set_registers_list at the cuts - the definition in include/fx8010_amd.h "Register tracks
by list": every block word, every get_register_array row, save_state() and the counters of the code in force.  There is no
tolerance anywhere.  What the stand-in cannot show is which values a block computed with (its emulation kernel copies the input):
that is tests/test_gpu_track_list.py; here the ORDER in which the stand-in ran the launches is observed instead.  The
Python-driven cases do not run under a sanitizer: that is tests/hipstub/track_list_checks.cpp, a program of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, FX_E_MEMORY, ROOT, Pinned, same_words, stub_library  # noqa: E402
from test_bus_tap_stub import same_bits  # noqa: E402
from test_register_list_stub import SPECIALS, key_table, lists_of, ptr, register_names  # noqa: E402

FX_E_NOTREADY = -2
N = 200
# three parameters the program only reads (a filter coefficient, an output gain, a second gain), a register it writes itself
TEXT = ("input in 0\noutput out 0\ncontrol coef = 0.5\ncontrol gain = 0.25\ncontrol trim = 0.75\nstatic a\nstatic b\n"
        "macs a, a, coef, in\nmacs b, a, trim, 0.5\nmacs out, b, in, gain\nend")
# (first, period, steps) of the issue for S = 32: (3, 5, 9) runs past the block, (32, 1, 1) has nothing due, (31, 7, 2) one step inside
SHAPES = ((0, 8, 4), (0, 1, 32), (13, 1, 1), (3, 5, 9), (32, 1, 1), (31, 7, 2))


def run_child(which, marker, devices=1, kernel=None):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    if kernel:
        env["FX_KERNEL"] = kernel
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


def test_expanded_event_rows_equal_the_model_on_the_hip_stand_in():
    """every list, one and two keys, every schedule shape, S = 32 and 45, two schedules on one register, a list schedule beside a
    dense and a broadcast track; the order header copy -> hold -> scatter -> block; a list set between arming and the block"""
    run_child("rows", "track list rows ok")


@pytest.mark.parametrize("kernel", ("hip", "asm"))
def test_cut_block_tiers_equal_the_twin_on_the_hip_stand_in(kernel):
    run_child("twin", "track list twin ok", kernel=kernel)


def test_list_schedules_and_caller_streams_on_the_hip_stand_in():
    """a block on another stream in front; arming for the next block while one is queued"""
    run_child("streams", "track list streams ok")


def test_list_schedule_refusals_change_nothing_on_the_hip_stand_in():
    run_child("refusals", "track list refusals ok")


def test_list_schedule_allocation_failures_on_the_hip_stand_in():
    run_child("memory", "track list memory ok")


def test_list_schedules_and_the_code_in_force_on_the_hip_stand_in():
    """the code hash equals the dense track's; a second arming does not translate; fxb_clear_register_tracks_list"""
    run_child("code", "track list code ok")


def test_list_schedules_on_three_shards_on_the_hip_stand_in():
    run_child("shards", "track list shards ok", devices=3)


def test_list_schedule_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    """tests/hipstub/track_list_checks.cpp (csrc/Makefile `stubasantracklist`): the list, key and step shapes through the C ABI on
    exactly-sized heap blocks, the refusals and the allocation failures, on one handle and on three shards, under AddressSanitizer +
    UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded and no interpreter is involved."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasantracklist"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "track_list_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "track list checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]


# ---- the child ----------------------------------------------------------------------------------------------------------------

def track_library():
    A, lib = stub_library()
    for f in ("fxstub_track_holds", "fxstub_track_scatters", "fxstub_track_strays", "fxstub_track_hold_at", "fxstub_track_scatter_at", "fxstub_track_hold_before_scatter",
              "fxstub_reg_scatters", "fxstub_reg_strays", "fxstub_live_allocations"):
        getattr(lib, f).restype = C.c_long
    lib.fxstub_track_rows.restype = C.c_longlong
    lib.fxstub_track_rows.argtypes = [C.c_void_p, C.c_longlong]
    lib.fxstub_track_table.restype = C.c_longlong
    lib.fxstub_track_table.argtypes = [C.c_void_p, C.c_int]
    return A, lib


def raw_arm(lib, b, keys, L, v, steps, first, period, n_keys=None, count=None, table=True):
    return lib.fxb_set_register_tracks_list(b._h, key_table(keys) if table else None, len(keys) if n_keys is None else n_keys, ptr(L),
                                            (0 if L is None else L.size) if count is None else count, ptr(v), steps, first, period)


def step_values(rng, steps, n_keys, count):
    """[steps, n_keys, count] words of every magnitude; the specials walk through the first columns of every row"""
    v = (rng.standard_normal((steps, n_keys, count)) * 10.0 ** rng.integers(-8, 8, (steps, n_keys, count))).astype(np.float32)
    for q in range(steps):
        for k in range(n_keys):
            m = min(count, SPECIALS.size)
            v[q, k, :m] = np.roll(SPECIALS, q + k)[:m]
    return v


class Schedule:
    def __init__(self, keys, L, v, first, period):
        self.keys, self.L, self.v, self.first, self.period = list(keys), np.ascontiguousarray(L, dtype=np.int64), np.ascontiguousarray(v, dtype=np.float32), first, period
        self.steps = self.v.shape[0]

    def due(self, S):
        """the samples of the steps that fall inside a block of S samples"""
        return [self.first + q * self.period for q in range(self.steps) if self.first + q * self.period < S]

    def arm(self, lib, b):
        L, v = self.L.copy(), self.v.copy()
        rc = raw_arm(lib, b, self.keys, L, v, self.steps, self.first, self.period)
        L[...] = -5            # the arrays are the caller's again on return
        v[...] = np.nan
        return rc


def model_rows(schedules, S, hold):
    """per register, in the order of `hold` (name -> the row every voice holds at the head of the block): (events, rows[event][N])"""
    out = {}
    for key, held in hold.items():
        mine = [s for s in schedules if key in s.keys]
        events = sorted({t for s in mine for t in s.due(S)})
        rows = np.tile(np.asarray(held, dtype=np.float32), (len(events), 1))
        for s in mine:
            due, k = s.due(S), s.keys.index(key)
            for q, t in enumerate(due):
                lo = events.index(t)
                hi = events.index(due[q + 1]) if q + 1 < len(due) else len(events)
                rows[lo:hi, s.L] = s.v[q, k]
        out[key] = (events, rows)
    return out


def read_rows(lib):
    """the event rows the last hold filled and its table: {state row: rows[event][nPad]}"""
    tab = np.zeros(1 + 3 * 16, dtype=np.int32)
    n_pad = lib.fxstub_track_table(tab.ctypes.data, tab.size)
    total = lib.fxstub_track_rows(None, 0)
    words = np.zeros((total, n_pad), dtype=np.float32)
    assert lib.fxstub_track_rows(words.ctypes.data, words.size) == total
    assert n_pad % 256 == 0
    out = {}
    for t in range(tab[0]):
        row, first, count = (int(x) for x in tab[1 + 3 * t:4 + 3 * t])
        out[row] = words[first:first + count]
    assert sum(r.shape[0] for r in out.values()) == total, "the registers' rows tile the block"
    return out


def check_block(A, lib, b, names, schedules, S, rng, what, extra=None):
    """arm, run a block on the translated tier, compare the expanded rows with the model"""
    assert "translated" in b.tier_note(), b.tier_note()
    keys = []
    for s in schedules:
        keys += [k for k in s.keys if k not in keys]
    for s in schedules:
        assert s.arm(lib, b) == 0, (what, b.last_error())
    if extra:
        extra()
    hold = {k: b.get_register_array(k) for k in keys}
    holds, scatters, expands, ran = lib.fxstub_track_holds(), lib.fxstub_track_scatters(), b.info("track_list_expands"), lib.fxstub_kernels_run()
    x = rng.standard_normal((S, N)).astype(np.float32)
    assert same_words(b.process_block(x), x), what
    model = model_rows(schedules, S, hold)
    live = [s for s in schedules if s.due(S)]
    if not live:
        assert (lib.fxstub_track_holds(), lib.fxstub_track_scatters(), b.info("track_list_expands")) == (holds, scatters, expands), (what, "nothing due: nothing launched")
        return
    assert (lib.fxstub_track_holds(), lib.fxstub_track_scatters(), b.info("track_list_expands")) == (holds + 1, scatters + len(live), expands + 1), what
    # header copy -> hold -> scatter -> block: the scatter read its ranges from the header, ran behind the hold, and both ran
    # before this block's emulation kernel
    assert lib.fxstub_track_hold_before_scatter() == 1 and lib.fxstub_track_hold_at() == ran and lib.fxstub_track_scatter_at() == ran and lib.fxstub_kernels_run() == ran + 1, what
    got = read_rows(lib)
    assert sorted(got) == sorted(names.index(k) for k in keys if model[k][0]), (what, sorted(got))
    for k in keys:
        events, rows = model[k]
        if events:
            g = got[names.index(k)]
            assert g.shape[0] == len(events) and same_bits(g[:, :N], rows), (what, k)
    assert lib.fxstub_track_strays() == 0


def child_rows():
    A, lib = track_library()
    rng = np.random.default_rng(601)
    names = register_names(A, TEXT, 1)
    b = A.Batch(N, 1, 0)
    assert b.load_text(TEXT)
    # the parameters differ per voice before anything is armed: the hold rows are not constants
    assert b.set_register_array("coef", rng.standard_normal(N).astype(np.float32)) == 0 and b.set_register_array("gain", rng.standard_normal(N).astype(np.float32)) == 0
    b.process_block(np.zeros((8, N), dtype=np.float32))
    for S in (32, 45):
        for n_keys, L in [(1 + i % 2, L) for i, L in enumerate(lists_of(rng, N))] + [(2, np.array([N // 2], dtype=np.int64)), (1, rng.permutation(N).astype(np.int64))]:
            for first, period, steps in SHAPES:
                keys = ["coef", "gain"][:n_keys]
                s = Schedule(keys, L, step_values(rng, steps, n_keys, L.size), first, period)
                check_block(A, lib, b, names, [s], S, rng, (S, n_keys, L.size, first, period, steps))
    # two schedules on one register with disjoint lists and interleaved events; the second also names another register
    perm = rng.permutation(N).astype(np.int64)
    for S in (32, 45):
        a = Schedule(["coef"], perm[:65], step_values(rng, 4, 1, 65), 0, 8)
        c = Schedule(["gain", "coef"], perm[65:130], step_values(rng, 9, 2, 65), 3, 5)
        d = Schedule(["coef"], perm[130:131], step_values(rng, 1, 1, 1), 13, 1)
        check_block(A, lib, b, names, [a, c, d], S, rng, ("interleaved", S))
    # a list schedule, a dense per-instance track and a broadcast track on three registers, events due at the same samples
    dense = rng.standard_normal((4, N)).astype(np.float32)

    def tracks():
        assert b.set_register_track("gain", dense, 8) == 0 and b.set_register_track("trim", np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32), 8) == 0

    check_block(A, lib, b, names, [Schedule(["coef"], perm[:64], step_values(rng, 4, 1, 64), 0, 8)], 32, rng, "three kinds", extra=tracks)
    # a list set queued between arming and the block shows in the held values
    fresh = rng.standard_normal((1, 3)).astype(np.float32)
    held = []

    def list_set():
        assert b.set_registers_list(["coef"], [1, 2, N - 1], fresh) == 0
        held.append(1)

    others = np.array([5, 6, 7], dtype=np.int64)
    check_block(A, lib, b, names, [Schedule(["coef"], others, step_values(rng, 2, 1, 3), 4, 9)], 32, rng, "a list set in between", extra=list_set)
    got = read_rows(lib)[names.index("coef")]
    assert held and same_bits(got[:, [1, 2, N - 1]], np.tile(fresh, (2, 1))), "the hold read the rows behind the list set"
    b.close()
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("track list rows ok")


class Twin:
    """a handle with list schedules beside one whose blocks the test cuts itself, with fxb_set_registers_list at the cuts"""
    COUNTERS = ("xlate_builds", "num_rows", "control_rows", "kernel", "num_lane_regs", "num_uniform_regs")

    def __init__(self, A, lib, n, rng, devices=None, track=("coef", "gain", "trim")):
        self.A, self.lib, self.n, self.rng = A, lib, n, rng
        self.b = A.Batch(n, 1, devices=devices) if devices else A.Batch(n, 1, 0)
        self.t = A.Batch(n, 1, 0)
        assert self.b.load_text(TEXT) and self.t.load_text(TEXT), self.b.errors()
        self.names = register_names(A, TEXT, 1)
        # the twin's registers are trackable too (a schedule with nothing due changes nothing else): both run the same code
        one = np.zeros((1, len(track), 1), dtype=np.float32)
        for h in (self.b, self.t):
            assert raw_arm(lib, h, list(track), np.array([0], dtype=np.int64), one, 1, 1 << 20, 1) == 0, h.last_error()
            h.process_block(np.zeros((4, n), dtype=np.float32))

    def block(self, S, schedules, what, dense=None, broadcast=None):
        """dense / broadcast: (key, values, period) armed through set_register_track on the handle, written at the cuts on the twin"""
        x = self.rng.standard_normal((S, self.n)).astype(np.float32)
        scat = self.lib.fxstub_reg_scatters()
        for key, values, period in [t for t in (dense, broadcast) if t]:
            assert self.b.set_register_track(key, values, period) == 0
        for s in schedules:
            assert s.arm(self.lib, self.b) == 0, (what, self.b.last_error())
        got = self.b.process_block(x)
        assert self.b.sync() == 0
        mine = self.lib.fxstub_reg_scatters() - scat
        cuts = {0, S}
        for s in schedules:
            cuts |= set(s.due(S))
        for t in (dense, broadcast):
            if t:
                cuts |= {q * t[2] for q in range(len(t[1])) if q * t[2] < S}
        cuts = sorted(cuts)
        want = np.zeros_like(x)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if dense and lo % dense[2] == 0 and lo // dense[2] < len(dense[1]):
                assert self.t.set_register_array(dense[0], dense[1][lo // dense[2]]) == 0
            if broadcast and lo % broadcast[2] == 0 and lo // broadcast[2] < len(broadcast[1]):
                assert self.t.set_register(broadcast[0], float(broadcast[1][lo // broadcast[2]])) == 0
            for s in schedules:
                if lo in s.due(S):
                    q = (lo - s.first) // s.period
                    assert self.t.set_registers_list(s.keys, s.L, s.v[q]) == 0
            want[lo:hi] = self.t.process_block(x[lo:hi])
        assert self.t.sync() == 0
        assert same_words(got, want), what
        shards = len(self.b.shards())
        if shards == 1:
            assert mine == self.lib.fxstub_reg_scatters() - scat - mine == sum(len(s.due(S)) for s in schedules), (what, "one scatter per due step, as the twin's")
        for key in self.names:
            assert same_bits(self.b.get_register_array(key), self.t.get_register_array(key)), (what, key)
        assert (self.b.save_state() == self.t.save_state()).all(), what
        if shards == 1:
            assert [self.b.info(c) for c in self.COUNTERS] == [self.t.info(c) for c in self.COUNTERS], (what, [self.b.info(c) for c in self.COUNTERS], [self.t.info(c) for c in self.COUNTERS])
        assert self.b.info("track_list_expands") == 0, "the tiers that cut the block launch no expansion"

    def close(self):
        self.b.close()
        self.t.close()


def child_twin():
    A, lib = track_library()
    rng = np.random.default_rng(607)
    w = Twin(A, lib, N, rng)
    assert "translated" not in w.b.tier_note(), w.b.tier_note()
    for S in (32, 45):
        for i, L in enumerate(lists_of(rng, N)):
            for first, period, steps in SHAPES:
                keys = ["coef", "gain"][:1 + i % 2]
                w.block(S, [Schedule(keys, L, step_values(rng, steps, len(keys), L.size), first, period)], (S, L.size, first, period, steps))
        perm = rng.permutation(N).astype(np.int64)
        a = Schedule(["coef"], perm[:65], step_values(rng, 4, 1, 65), 0, 8)
        c = Schedule(["gain", "coef"], perm[65:130], step_values(rng, 9, 2, 65), 3, 5)
        w.block(S, [a, c], ("interleaved", S))
        w.block(S, [Schedule(["coef"], perm[:64], step_values(rng, 4, 1, 64), 0, 8)], ("three kinds", S),
                dense=("gain", rng.standard_normal((4, N)).astype(np.float32), 8), broadcast=("trim", np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32), 8))
    w.close()
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("track list twin ok")


def child_streams():
    """a slow block queued on stream A; a schedule armed and the next block queued on stream B: arming and queueing return while
    the first block still runs, the expansion runs behind it (uploadTracks keeps its host wait for the previous block), and
    arming for the block after that waits only for the expansion, not for the slow block behind it"""
    A, lib = track_library()
    pinned = Pinned(lib)
    rng = np.random.default_rng(613)
    lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.fxstub_set_kernel_micros.argtypes = [C.c_int]
    lib.fxstub_set_kernel_micros.restype = None
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert lib.hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value
    S = 32
    names = register_names(A, TEXT, 1)
    b = A.Batch(N, 1, 0)
    assert b.load_text(TEXT)
    L = np.array([0, 77, N - 1], dtype=np.int64)
    warm = Schedule(["coef"], L, step_values(rng, 4, 1, 3), 0, 8)
    assert warm.arm(lib, b) == 0 and b.prepare(S, True) == 0
    b.process_block(np.zeros((S, N), dtype=np.float32))   # (rows, code and staging exist before anything is timed)

    def fresh():
        p, o = pinned((S, 1, N)), pinned((S, 1, N))
        p[...] = rng.standard_normal((S, 1, N)).astype(np.float32)
        o[...] = -7.0
        return p, o

    def dev(bufs, stream):
        return lib.fxb_process_block_dev(b._h, ptr(bufs[0]), ptr(bufs[1]), S, stream)

    first, second, third = fresh(), fresh(), fresh()
    holds = lib.fxstub_track_holds()
    lib.fxstub_set_kernel_micros(150000)
    assert dev(first, streams[0]) == 0
    one = Schedule(["coef"], L, step_values(rng, 4, 1, 3), 0, 8)
    assert one.arm(lib, b) == 0
    assert (first[1][S - 1] == -7.0).all() and lib.fxstub_track_holds() == holds, "arming returned while the block in front was still running"
    hold = b_hold = None
    lib.fxstub_set_kernel_micros(150000)
    assert dev(second, streams[1]) == 0   # (waits on the host for the first block: uploadTracks' wait, kept)
    assert not (first[1][S - 1] == -7.0).any(), "the first block keeps what it was queued with: it had finished before the rows were rebuilt"
    two = Schedule(["gain"], L, step_values(rng, 2, 1, 3), 13, 3)
    assert two.arm(lib, b) == 0
    assert lib.fxstub_track_holds() == holds + 1 and (second[1][S - 1] == -7.0).all(), "arming for the next block waited for the expansion, not for the block"
    lib.fxstub_set_kernel_micros(150)
    assert dev(third, None) == 0 and b.sync() == 0
    assert lib.fxstub_track_holds() == holds + 2
    for bufs in (first, second, third):
        assert same_words(bufs[1], bufs[0])
    got = read_rows(lib)[names.index("gain")]
    model = model_rows([two], S, {"gain": np.full(N, 0.25, dtype=np.float32)})["gain"][1]
    assert same_bits(got[:, :N], model)
    del hold, b_hold
    pinned.free()
    b.close()
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("track list streams ok")


def child_refusals():
    A, lib = track_library()
    rng = np.random.default_rng(617)
    S = 32
    e = A.Batch(N, 1, 0)
    good_L, good_v = np.array([3, 0, N - 1], dtype=np.int64), step_values(rng, 2, 2, 3)
    assert raw_arm(lib, e, ["coef", "gain"], good_L, good_v, 2, 0, 8) == FX_E_NOTREADY
    e.close()
    w = Twin(A, lib, N, rng, track=("coef", "gain"))
    b = w.b
    big = np.zeros(1, dtype=np.int64)
    K = ["coef", "gain"]
    refused = [
        ("count < 0", FX_E_ARG, dict(count=-1)), ("n_keys < 0", FX_E_ARG, dict(n_keys=-1)), ("null keys", FX_E_ARG, dict(table=False)),
        ("a null list", FX_E_ARG, dict(L=None, count=3)), ("null values", FX_E_ARG, dict(v=None)),
        ("n_steps < 1", FX_E_ARG, dict(steps=0)), ("period < 1", FX_E_ARG, dict(period=0)), ("first < 0", FX_E_ARG, dict(first=-1)),
        ("n_steps * n_keys * count = 2^31", FX_E_ARG, dict(L=big, count=1 << 29, steps=2)),
        ("an instance of N", FX_E_ARG, dict(L=np.array([0, N, 1], dtype=np.int64))), ("an instance of -1", FX_E_ARG, dict(L=np.array([0, 1, -1], dtype=np.int64))),
        ("an instance listed twice", FX_E_ARG, dict(L=np.array([5, 9, 5], dtype=np.int64))),
        ("two keys that name one register", FX_E_ARG, dict(keys=["coef", "coef"])),
        ("a key that is no register", 1, dict(keys=["coef", "nosuch"])),
        ("a register the program writes", FX_E_ARG, dict(keys=["coef", "a"]), "'a'"),
        ("an output register", FX_E_ARG, dict(keys=["out", "gain"]), "'out'"),
        ("an input register", FX_E_ARG, dict(keys=["in", "gain"]), "'in'"),
    ]

    def state():
        return (b.info("track_list_expands"), b.info("xlate_builds"), b.info("num_rows"), lib.fxstub_track_holds(), lib.fxstub_track_scatters(), lib.fxstub_reg_scatters())

    def attempt(kw):
        return raw_arm(lib, b, kw.get("keys", K), kw.get("L", good_L), kw.get("v", good_v), kw.get("steps", 2), kw.get("first", 0), kw.get("period", 8),
                       n_keys=kw.get("n_keys"), count=kw.get("count"), table=kw.get("table", True))

    for S in (32,):
        for entry in refused:
            what, rc, kw = entry[:3]
            seen = state()
            got = attempt(kw)
            assert got == rc and b.last_error(), (what, got, b.last_error())
            assert len(entry) < 4 or entry[3] in b.last_error(), (what, b.last_error())
            assert rc != 1 or "nosuch" in b.last_error()
            assert state() == seen, what
            w.block(S, [], "nothing is armed after: " + what)   # (a block with nothing armed equals the twin's uncut block)
    assert "entry 1" in (attempt(dict(L=np.array([0, N, 1], dtype=np.int64))), b.last_error())[1], b.last_error()
    assert lib.fxb_set_register_tracks_list(None, key_table(K), 2, ptr(good_L), 3, ptr(good_v), 2, 0, 8) == FX_E_ARG and lib.fxb_clear_register_tracks_list(None) == FX_E_ARG
    # count == 0 and n_keys == 0 arm nothing
    assert raw_arm(lib, b, K, None, None, 2, 0, 8) == 0 and raw_arm(lib, b, [], good_L, None, 2, 0, 8) == 0
    w.block(S, [], "count == 0 and n_keys == 0 arm nothing")
    # a register with a schedule armed through set_register_track, and the converse; a voice named twice for one register
    assert b.set_register_track("gain", np.array([0.5, 0.25], dtype=np.float32), 8) == 0
    assert attempt({}) == FX_E_ARG and "gain" in b.last_error() and attempt(dict(keys=["coef"], v=good_v[:, :1].copy())) == 0
    with pytest.raises(RuntimeError, match="list schedules"):
        b.set_register_track("coef", np.array([0.5], dtype=np.float32), 8)
    assert attempt(dict(keys=["coef"], L=np.array([7, N - 1], dtype=np.int64), v=good_v[:, :1, :2].copy())) == FX_E_ARG and "instance %d" % (N - 1) in b.last_error()
    assert attempt(dict(keys=["trim", "coef"], L=np.array([7, 8, 9], dtype=np.int64))) == 0, "another list on the same register is fine; trim becomes trackable"
    assert b.clear_register_tracks_list() == 0
    b.process_block(np.zeros((4, N), dtype=np.float32))   # (consumes the dense track of gain)
    w.t.set_register("gain", 0.25)
    w.t.process_block(np.zeros((4, N), dtype=np.float32))
    assert same_bits(b.get_register_array("coef"), w.t.get_register_array("coef")), "cleared schedules change nothing"
    # a 65th schedule
    for i in range(64):
        assert attempt(dict(keys=["coef"], L=np.array([i], dtype=np.int64), v=good_v[:, :1, :1].copy())) == 0, i
    assert attempt(dict(keys=["coef"], L=np.array([100], dtype=np.int64), v=good_v[:, :1, :1].copy())) == FX_E_ARG and "64" in b.last_error()
    assert b.clear_register_tracks_list() == 0
    w.close()
    # a 17th register with schedules
    text = "input in 0\noutput out 0\n" + "".join("control c%d = 0.5\n" % i for i in range(17)) + "static a\n" + "".join("macs a, a, c%d, in\n" % i for i in range(17)) + "macs out, a, in, 0.5\nend"
    b = A.Batch(N, 1, 0)
    assert b.load_text(text)
    for i in range(15):
        assert raw_arm(lib, b, ["c%d" % i], good_L, good_v[:, :1].copy(), 2, 0, 8) == 0
    assert raw_arm(lib, b, ["c15", "c16"], good_L, good_v, 2, 0, 8) == FX_E_ARG and "16" in b.last_error()
    assert raw_arm(lib, b, ["c15"], good_L, good_v[:, :1].copy(), 2, 0, 8) == 0 and raw_arm(lib, b, ["c16"], good_L, good_v[:, :1].copy(), 2, 0, 8) == FX_E_ARG
    b.close()
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("track list refusals ok")


def child_memory():
    """an allocation that fails, at each allocation of the arming call (the pinned staging, the device staging, the track
    buffer): FX_E_MEMORY, nothing armed, then the same call succeeds"""
    A, lib = track_library()
    rng = np.random.default_rng(619)
    names = register_names(A, TEXT, 1)
    L = lists_of(rng, N)[3]
    failed = 0
    for nth in range(4):
        b = A.Batch(N, 1, 0)
        assert b.load_text(TEXT) and b.prepare(32, True) == 0
        b.process_block(np.zeros((32, N), dtype=np.float32))
        assert b.prepare(32, True) == 0
        s = Schedule(["coef", "gain"], L, step_values(rng, 4, 2, L.size), 0, 8)
        live, rows = lib.fxstub_live_allocations(), b.info("num_rows")
        lib.fxstub_fail_mallocs(nth, 1)
        rc = s.arm(lib, b)
        lib.fxstub_fail_mallocs(-1, 0)
        if nth < 3:
            assert rc == FX_E_MEMORY and b.last_error(), (nth, rc)
            failed += 1
            assert lib.fxstub_live_allocations() <= live + 2 and b.info("num_rows") == rows
            holds = lib.fxstub_track_holds()
            b.process_block(np.zeros((32, N), dtype=np.float32))
            assert lib.fxstub_track_holds() == holds and b.info("track_list_expands") == 0, "nothing was armed"
        else:
            assert rc == 0, "the call makes three allocations"
            b.clear_register_tracks_list()
        check_block(A, lib, b, names, [s], 32, rng, ("after an allocation failure", nth))
        b.close()
    assert failed == 3
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_cross_device_errors() == 0
    print("track list memory ok")


def child_code():
    A, lib = track_library()
    rng = np.random.default_rng(623)
    names = register_names(A, TEXT, 1)
    L = lists_of(rng, N)[2]
    x = rng.standard_normal((32, N)).astype(np.float32)
    b, d = A.Batch(N, 1, 0), A.Batch(N, 1, 0)
    assert b.load_text(TEXT) and d.load_text(TEXT)
    for h in (b, d):
        h.process_block(x)
    builds = b.info("xlate_builds") + b.info("xlate_background_builds") + b.info("code_cache_hits")
    s = Schedule(["coef", "gain"], L, step_values(rng, 4, 2, L.size), 0, 8)
    assert s.arm(lib, b) == 0
    for k in s.keys:
        assert d.set_register_track(k, rng.standard_normal((4, N)).astype(np.float32), 8) == 0
    for h in (b, d):
        h.process_block(x)
    assert b.info("xlate_code_hash") == d.info("xlate_code_hash") and b.info("xlate_code_hash") != 0, "the code of dense per-instance tracks on the same registers"
    assert b.prepare(32, True) == 0
    after = (b.info("xlate_builds"), b.info("xlate_background_builds"), b.info("code_cache_hits"))
    assert sum(after) >= builds + 1, "the first schedule made the registers trackable: other code, once"
    for i in range(3):
        check_block(A, lib, b, names, [Schedule(["gain", "coef"], L, step_values(rng, 3, 2, L.size), i, 7)], 32, rng, "a later arming")
    assert (b.info("xlate_builds"), b.info("xlate_background_builds"), b.info("code_cache_hits")) == after, "arming for a trackable register never translates again"
    # fxb_clear_register_tracks_list drops what is armed; the next arming starts over
    holds = lib.fxstub_track_holds()
    assert s.arm(lib, b) == 0 and b.clear_register_tracks_list() == 0
    b.process_block(x)
    assert lib.fxstub_track_holds() == holds and b.info("track_list_expands") == 4
    check_block(A, lib, b, names, [s], 32, rng, "after a clear")
    b.close()
    d.close()
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("track list code ok")


def child_shards():
    """three shards: a list on every shard, one wholly inside the middle shard (the others launch nothing); on the tiers that cut
    the block (FX_KERNEL is set by the second pass) against the twin; refusals in front of every shard; allocation failures"""
    A, lib = track_library()
    rng = np.random.default_rng(631)
    n, S = 3 * 256 + 40, 32
    inside = rng.permutation(np.arange(330, 400)).astype(np.int64)
    everywhere = np.concatenate([[0, n - 1], rng.permutation(np.arange(1, n - 1))[:128]]).astype(np.int64)
    b = A.Batch(n, 1, devices=[0, 1, 2])
    assert b.load_text(TEXT) and [(dv, f) for dv, f, _ in b.shards()] == [(0, 0), (1, 320), (2, 576)], b.shards()
    x = rng.standard_normal((S, n)).astype(np.float32)
    b.process_block(x)
    for L, launches in ((inside, 1), (everywhere, 3)):
        s = Schedule(["coef", "gain"], L, step_values(rng, 4, 2, L.size), 0, 8)
        seen = (b.info("track_list_expands"), lib.fxstub_track_holds(), lib.fxstub_track_scatters())
        assert s.arm(lib, b) == 0, b.last_error()
        assert same_words(b.process_block(x), x)
        assert (b.info("track_list_expands"), lib.fxstub_track_holds(), lib.fxstub_track_scatters()) == (seen[0] + launches, seen[1] + launches, seen[2] + launches), "a shard without entries launches nothing"
    # refused for the whole handle, in front of every shard
    seen = (b.info("track_list_expands"), lib.fxstub_track_holds())
    v = step_values(rng, 2, 1, 3)
    assert raw_arm(lib, b, ["coef"], np.array([0, n - 1, 0], dtype=np.int64), v, 2, 0, 8) == FX_E_ARG and raw_arm(lib, b, ["coef"], np.array([0, n, 1], dtype=np.int64), v, 2, 0, 8) == FX_E_ARG
    assert raw_arm(lib, b, ["nosuch"], np.array([0], dtype=np.int64), v, 2, 0, 8) == 1 and raw_arm(lib, b, ["a"], np.array([0, 400, 700], dtype=np.int64), v, 2, 0, 8) == FX_E_ARG
    # a voice of the last shard is named twice for one register: no shard arms
    assert raw_arm(lib, b, ["coef"], np.array([1, 400, 700], dtype=np.int64), v, 2, 0, 8) == 0
    assert raw_arm(lib, b, ["coef"], np.array([2, 401, 700], dtype=np.int64), v, 2, 0, 8) == FX_E_ARG and "instance 700" in b.last_error(), b.last_error()
    assert b.clear_register_tracks_list() == 0
    b.process_block(x)
    assert (b.info("track_list_expands"), lib.fxstub_track_holds()) == seen
    b.close()
    # an allocation that fails on whichever shard: FX_E_MEMORY and no shard has armed
    for nth in range(9):
        c = A.Batch(n, 1, devices=[0, 1, 2])
        assert c.load_text(TEXT) and c.prepare(S, True) == 0
        c.process_block(x)
        assert c.prepare(S, True) == 0
        s = Schedule(["coef"], everywhere, step_values(rng, 4, 1, everywhere.size), 0, 8)
        lib.fxstub_fail_mallocs(nth, 1)
        rc = s.arm(lib, c)
        lib.fxstub_fail_mallocs(-1, 0)
        assert rc == FX_E_MEMORY and c.last_error(), (nth, rc)
        holds = lib.fxstub_track_holds()
        c.process_block(x)
        assert lib.fxstub_track_holds() == holds and c.info("track_list_expands") == 0, "no shard has armed"
        assert s.arm(lib, c) == 0
        c.process_block(x)
        assert c.info("track_list_expands") == 3
        c.close()
    # the tiers that cut the block, against a single twin
    os.environ["FX_KERNEL"] = "asm"
    w = Twin(A, lib, n, rng, devices=[0, 1, 2])
    for L in (inside, everywhere):
        for first, period, steps in SHAPES:
            w.block(S, [Schedule(["coef", "gain"], L, step_values(rng, steps, 2, L.size), first, period)], ("shards", L.size, first, period, steps))
    w.close()
    assert lib.fxstub_track_strays() == 0 and lib.fxstub_reg_strays() == 0 and lib.fxstub_cross_device_errors() == 0 and lib.fxstub_bad_pcm_launches() == 0
    print("track list shards ok")


if __name__ == "__main__":
    {"rows": child_rows, "twin": child_twin, "streams": child_streams, "refusals": child_refusals, "memory": child_memory, "code": child_code,
     "shards": child_shards}[sys.argv[1]]()
