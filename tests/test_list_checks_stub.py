"""The one list check behind every by-list call, without a GPU: the library's host sources linked against tests/hipstub/ (`make -C
fx8010-emulator-core_amd/csrc stublib`), driven through the C ABI in a child process like tests/test_tram_list_stub.py (this file
is also that child).  One table of the public calls that take a list of instances - fxb_set_registers_list,
fxb_get_registers_list, fxb_set_register_tracks_list, fxb_set_tram_list, fxb_get_tram_list, fxb_meter_read_list (with and without
reset), fxb_meter_reset_list, fxb_bus_set_gains_list, fxb_reset_instances - is walked over the edges of the check:

  * repeats are looked up in a bitmap over the instances while (N + 63) / 64 <= 16 * count and in a sorted copy beyond: a list of
    two entries meets the bitmap on 2048 instances (32 <= 32) and the sorted copy on 2049 (33 > 32), a list of four on 4096 and
    4097.  The pair [a, a] sits on the bit and word edges of the bitmap (0, 63, 64, N - 1) and, on three shards, in the last one;
  * of several repeats both paths name the first entry in list order that repeats an earlier one - the expected entry comes from
    first_repeat() below, not from the library;
  * -1 and N at the first and at the last entry: the message names that entry;
  * the calls that only read accept [a, a] and answer the same words twice; fxb_meter_reset_list accepts it as well (its header
    entry: zeroing twice is zeroing); the sets, the read with reset and fxb_reset_instances refuse it;
  * after every refusal the state image, the meters, the gains and the launch counters are what they were;
  * fxb_set_tram_list / fxb_get_tram_list with n_words == 0: a null list is accepted, a list that is there is checked; count == 0
    returns 0 everywhere.

The same edges run under AddressSanitizer + UBSan in tests/hipstub/register_list_checks.cpp, a program of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bus_stub import CSRC, FX_E_ARG, ROOT  # noqa: E402
from test_bus_tap_stub import same_bits  # noqa: E402
from test_instances_rot_stub import handle, rings  # noqa: E402

TEXT = rings(8, 16)   # a control (`vol`), two delay lines that are rings: every call of the table has something to act on
COUNTERS = ("register_list_sets", "register_list_gets", "tram_list_sets", "tram_list_gets", "meter_list_reads", "meter_list_resets", "gain_list_sets", "instance_scatters",
            "track_list_expands")


def run_child(which, marker, devices=1):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang on this machine")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FX_")}
    subprocess.check_call(["make", "-s", "-C", CSRC, "stublib"])
    env["FX8010_AMD_LIB"] = os.path.join(CSRC, "build", "stub", "libfx8010_amd.so")
    env["FXSTUB_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("devices", (1, 3))
def test_repeat_paths_and_range_edges_of_every_list_call_on_the_hip_stand_in(devices):
    """N = 2048 (bitmap) and 2049 (sorted copy) with lists of two entries; one handle and three shards"""
    run_child("edges-%d" % devices, "list check edges ok", devices=devices)


def test_several_repeats_name_the_first_in_list_order_on_both_paths_on_the_hip_stand_in():
    """[5, 9, 9, 5] and others on 2048, 2049, 4096 (bitmap for four entries) and 4097 instances (sorted copy): one text"""
    run_child("several", "list check several ok", devices=3)


def test_tram_special_cases_and_empty_lists_on_the_hip_stand_in():
    run_child("special", "list check special ok", devices=3)


# ---- the child ----------------------------------------------------------------------------------------------------------------

def first_repeat(L):
    """the model of the rule: the first entry in list order that repeats an earlier one (None: no repeat)"""
    seen = set()
    for i, v in enumerate(L):
        if int(v) in seen:
            return i
        seen.add(int(v))
    return None


def ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


class Call:
    """one public call that takes a list: fn(lib, b, L, count) -> (rc, what it read per entry [count, ...] or None); `repeats`: the
    call accepts a repeated instance; name: what its messages begin with; twice(L, i): its text for entry i repeating an earlier one"""

    def __init__(self, what, fn, repeats, name, twice=None, outside=None):
        self.what, self.fn, self.repeats, self.name, self.twice, self.fixed_outside = what, fn, repeats, name, twice, outside

    def outside(self, i, n):
        return self.fixed_outside or "%s: entry %d of the list is outside 0..%d" % (self.name, i, n - 1)


KEYS = (C.c_char_p * 1)(b"vol")
WORDS = 3   # of a delay-line window


def room(count, *shape):
    return np.full((max(int(count), 1),) + shape, 0.25, dtype=np.float32)


def regs_set(lib, b, L, count):
    return lib.fxb_set_registers_list(b._h, KEYS, 1, ptr(L), count, ptr(room(count))), None


def regs_get(lib, b, L, count):
    out = room(count)
    return lib.fxb_get_registers_list(b._h, KEYS, 1, ptr(L), count, ptr(out)), out


def tracks_set(lib, b, L, count):
    return lib.fxb_set_register_tracks_list(b._h, KEYS, 1, ptr(L), count, ptr(room(count)), 1, 0, 1), None


def tram_set(lib, b, L, count, n_words=WORDS, values=True):
    return lib.fxb_set_tram_list(b._h, 1, ptr(L), count, 2, n_words, ptr(room(count, WORDS)) if values else None, 0), None


def tram_get(lib, b, L, count, n_words=WORDS, values=True):
    out = room(count, WORDS)
    return lib.fxb_get_tram_list(b._h, 1, ptr(L), count, 2, n_words, ptr(out) if values else None, 0), out


def meter_read(reset):
    def fn(lib, b, L, count):
        energy, peak = np.zeros(max(int(count), 1), dtype=np.float64), room(count)
        rc = lib.fxb_meter_read_list(b._h, ptr(L), count, ptr(energy), ptr(peak), None, None, reset)
        return rc, np.stack([energy.view(np.uint32).reshape(-1, 2)[:, 0].view(np.float32), energy.view(np.uint32).reshape(-1, 2)[:, 1].view(np.float32), peak], axis=1)
    return fn


def meter_reset(lib, b, L, count):
    return lib.fxb_meter_reset_list(b._h, ptr(L), count), None


def gains_set(lib, b, L, count):
    return lib.fxb_bus_set_gains_list(b._h, ptr(L), count, ptr(room(count)), 0), None


def instances_reset(lib, b, L, count):
    return lib.fxb_reset_instances(b._h, ptr(L), count), None


CALLS = [
    Call("fxb_set_registers_list", regs_set, False, "set_registers_list", lambda L, i: "set_registers_list: instance %d is listed more than once" % L[i]),
    Call("fxb_get_registers_list", regs_get, True, "get_registers_list"),
    Call("fxb_set_register_tracks_list", tracks_set, False, "set_register_tracks_list", lambda L, i: "set_register_tracks_list: instance %d is listed more than once" % L[i]),
    Call("fxb_set_tram_list", tram_set, False, "set_tram_list", lambda L, i: "set_tram_list: entry %d of the list names instance %d a second time" % (i, L[i])),
    Call("fxb_get_tram_list", tram_get, True, "get_tram_list"),
    Call("fxb_meter_read_list", meter_read(0), True, "meter_read_list"),
    Call("fxb_meter_read_list, reset", meter_read(1), False, "meter_read_list", lambda L, i: "meter_read_list: instance %d is listed more than once (reset)" % L[i]),
    Call("fxb_meter_reset_list", meter_reset, True, "meter_reset_list"),
    Call("fxb_bus_set_gains_list", gains_set, False, "bus gains by list", lambda L, i: "bus gains by list: index %d is listed more than once" % L[i]),
    Call("fxb_reset_instances", instances_reset, False, "instances", lambda L, i: "instances: a destination is listed twice", "instances: an instance number outside the batch"),
]


def library():
    import test_instances_rot_stub as rot
    _, A, lib = rot.stub_library()
    return A, lib


def voices(A, n, devices):
    """a handle with per-instance registers, delay memory, meters and gains that hold something"""
    b = handle(A, TEXT, n, devices=[0, 1, 2] if devices == 3 else None)
    rng = np.random.default_rng(n)
    assert b.meter_enable(True) == 0
    assert b.bus_set_gains(rng.uniform(0.1, 1.0, (1, n)).astype(np.float32)) == 0
    assert b.set_registers_list(["vol"], np.arange(0, n, 3), rng.uniform(0.1, 1.0, (1, len(range(0, n, 3)))).astype(np.float32)) == 0
    b.process_block(rng.standard_normal((9, n)).astype(np.float32))
    assert b.sync() == 0
    return b


def held(b):
    """everything a call of the table could have touched, as bytes, and the launch counters"""
    m = b.meter_read()
    return [b.save_state().tobytes(), b.bus_get_gains().tobytes()] + [np.ascontiguousarray(m[k]).tobytes() for k in sorted(m)] + [tuple(b.info(c) for c in COUNTERS)]


def refused(lib, b, call, L, text, before):
    L = np.asarray(L, dtype=np.int64)
    rc, _ = call.fn(lib, b, L.copy(), L.size)
    assert rc == FX_E_ARG and b.last_error() == text, (call.what, L.tolist(), rc, b.last_error(), text)
    assert held(b) == before, (call.what, L.tolist(), "a refusal changed something")


def child_edges(devices):
    A, lib = library()
    for n in (2048, 2049):
        b = voices(A, n, devices)
        last = b.shards()[-1][1]   # the first instance of the last shard (0 on one handle)
        assert (devices == 1) == (last == 0)
        edges = sorted({0, 63, 64, n - 1} | ({last, last + 63, last + 64} if devices == 3 else set()))
        start = before = held(b)
        for call in CALLS:
            for a in edges:
                L = np.array([a, a], dtype=np.int64)
                assert first_repeat(L) == 1
                if not call.repeats:
                    refused(lib, b, call, L, call.twice(L, 1), before)
                    continue
                rc, out = call.fn(lib, b, L.copy(), 2)
                assert rc == 0, (call.what, a, b.last_error())
                if out is not None:
                    assert same_bits(out[0], out[1]), (call.what, a)
                    one = call.fn(lib, b, L[:1].copy(), 1)[1]
                    assert same_bits(out[0], one[0]), (call.what, a)
                before = held(b)   # (the counters of the call that went through; the columns a list reset of the meters zeroed)
            # -1 and N at the first and at the last entry
            for bad in (-1, n):
                for at, L in ((0, [bad, 1, 2]), (2, [1, 2, bad])):
                    refused(lib, b, call, L, call.outside(at, n), before)
            # an entry outside the batch in front of a repeat: the order of the refusals
            refused(lib, b, call, [7, n, 7], call.outside(1, n), before)
        # (the reads and the list reset of the meters that went through: the reset zeroes the listed columns, nothing else moved)
        assert before[0] == start[0] and before[1] == start[1], "the calls that accept a repeat changed state or gains"
        b.close()
    assert lib.fxstub_cross_device_errors() == 0
    print("list check edges ok")


def child_several():
    A, lib = library()
    lists = [[5, 9, 9, 5], [5, 9, 5, 9], [2000, 3, 3, 2000], [1, 1, 0, 0], [63, 64, 64, 63]]
    texts = {}
    for n, devices in ((2048, 1), (2049, 1), (4096, 1), (4097, 1), (4096, 3), (4097, 3)):
        b = voices(A, n, devices)
        before = held(b)
        for call in CALLS:
            if call.repeats:
                continue
            for L in lists:
                i = first_repeat(L)
                assert i == (1 if L[0] == L[1] else 2)
                refused(lib, b, call, L, call.twice(L, i), before)
                texts.setdefault((call.what, tuple(L)), set()).add(b.last_error())
        b.close()
    assert texts and all(len(t) == 1 for t in texts.values()), texts
    print("list check several ok")


def child_special():
    A, lib = library()
    for n, devices in ((2048, 1), (2049, 3)):
        b = voices(A, n, devices)
        before = held(b)
        # count == 0 returns 0 everywhere, with or without a list, and changes nothing
        for call in CALLS:
            for L in (None, np.array([n, n], dtype=np.int64)):
                rc, _ = call.fn(lib, b, L, 0)
                assert rc == 0, (call.what, b.last_error())
        # n_words == 0 moves nothing: a null list (and null values) is accepted, a list that is there is checked like any other
        good, pair = np.array([0, n - 1], dtype=np.int64), np.array([n - 1, n - 1], dtype=np.int64)
        for fn in (tram_set, tram_get):
            assert fn(lib, b, None, 2, n_words=0, values=False)[0] == 0, b.last_error()
            assert fn(lib, b, good.copy(), 2, n_words=0, values=False)[0] == 0, b.last_error()
            name = "set_tram_list" if fn is tram_set else "get_tram_list"
            for at, L in ((0, [n, 1]), (1, [1, n]), (0, [-1, 1]), (1, [1, -1])):
                rc, _ = fn(lib, b, np.array(L, dtype=np.int64), 2, n_words=0, values=False)
                assert rc == FX_E_ARG and b.last_error() == "%s: entry %d of the list is outside 0..%d" % (name, at, n - 1), (name, L, rc, b.last_error())
        rc, _ = tram_set(lib, b, pair.copy(), 2, n_words=0, values=False)
        assert rc == FX_E_ARG and b.last_error() == "set_tram_list: entry 1 of the list names instance %d a second time" % (n - 1), (rc, b.last_error())
        assert tram_get(lib, b, pair.copy(), 2, n_words=0, values=False)[0] == 0, b.last_error()
        assert held(b) == before
        b.close()
    print("list check special ok")


if __name__ == "__main__":
    which = sys.argv[1]
    if which.startswith("edges-"):
        child_edges(int(which[6:]))
    else:
        {"several": child_several, "special": child_special}[which]()
