"""The record bank on the GPU (include/fx8010_amd.h "Record banks"): fxb_bank_store is fxb_save_instances without the host,
fxb_bank_recall is fxb_load_instances_rotated with the rotations worked out on the device.  The bar is that of
tests/test_gpu_instances.py and tests/test_gpu_instances_rot.py (whose helpers these are): equality of 32-bit patterns - with a twin
handle that goes through the host calls, with the oracle, and with a twin that made no call wherever the device refuses."""
import ctypes as C

import numpy as np
import pytest

import fx8010_programs as progs
from test_gpu_instances import (PROGRAMS, S1, S2, bits, cutoffs, handle, right_tier, run, state_registers, tier,  # noqa: F401 (tier: a fixture)
                                use_tier)
from test_gpu_instances_rot import OFFSET3, SHADOW_BOTH, SHADOW_READ, TINY, TWO_TAPS, continues_like, replay, shifts_between, unlisted_equal_the_twin

pytestmark = pytest.mark.gpu

FX_E_NOTREADY, FX_E_ARG = -2, -3
N = 200
EDGES = [0, 63, 64, 127, 128, 199]   # both sides of every wavefront boundary
# both lines rings, a control the program reads (tests/test_instances_rot_stub.py rings(64, 1000))
RINGS = ("itramsize 64 \nxtramsize 1000 \ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 3\n"
         "xdelay write, in, at, 0\nxdelay read, xr, at, 2\nmacs out, r1, xr, vol\nend")
MORE = "static zz\nmacs zz, zz, 0.5, 0.5\nend"   # a further load that succeeds: registers and instructions accumulate over loads
COUNTERS = ("bank_slots", "bank_stores", "bank_recalls", "bank_bytes", "instance_gathers", "instance_scatters", "instance_rotations")


def make(gpu, text, n, control=None, values=None, dane=False, devices=None):
    b = gpu.Batch(n, 1, 0) if devices is None else gpu.Batch(n, 1, devices=devices)
    if dane:
        b.set_option(gpu.OPT_TRAM_DANE)
    assert b.load_text(text), b.errors()
    if control:
        assert b.set_register_array(control, values) == 0
    return b


def counters(b):
    return {k: b.info(k) for k in COUNTERS}


def cursor_word(b):
    """the record word of the first of the four positions: registers, output latches, then the positions"""
    return b.info("num_registers") + b.channels


# ---- 1. store is save ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [1, 65])
@pytest.mark.parametrize("name", ["config3", "config5"])
def test_store_is_save(gpu, tier, name, n_slots):
    text, control, _ = PROGRAMS[name]
    b = handle(gpu, text(), N, control, cutoffs(N))
    run(b, progs.stimulus(N, S1))
    assert right_tier(b, tier), b.tier_note()
    assert b.bank_slots() == 0 and b.bank_create(n_slots) == 0 and b.bank_slots() == n_slots
    assert b.info("bank_slots") == n_slots and b.info("bank_bytes") == n_slots * b.instance_words * 4
    inst = EDGES if n_slots > 1 else [199]
    slots = [64, 63, 33, 2, 1, 0] if n_slots > 1 else [0]
    before = counters(b)
    assert b.bank_store(slots, inst) == 0
    got = b.bank_get(slots)
    after = counters(b)
    assert after["bank_stores"] == before["bank_stores"] + 1 and after["instance_gathers"] == before["instance_gathers"]
    assert np.array_equal(got, b.save_instances(inst)), "the bank holds other bytes than save_instances writes"
    if n_slots > 1:
        assert not b.bank_get([3, 62, 32, 34])[64:].any(), "a slot that was not stored is no longer zero"
        assert np.array_equal(b.bank_get(slots[::-1]), b.save_instances(inst[::-1]))


def test_store_is_save_for_a_record_that_is_no_multiple_of_the_tile(gpu, monkeypatch):
    use_tier(monkeypatch, "xlate")
    b = handle(gpu, TINY, 70)
    run(b, progs.stimulus(70, 23))
    assert b.instance_words % 64 != 0 and b.bank_create(70) == 0
    inst = np.arange(70)
    assert b.bank_store(inst[::-1], inst) == 0
    assert np.array_equal(b.bank_get(inst[::-1]), b.save_instances(inst))


# ---- 2. recall is the rotated load -------------------------------------------------------------------------------------------------
TWINS = {
    # name: (text, N, control, samples before the store, samples between store and recall, sources, destinations, DANE)
    "config3": (progs.config3, N, "cutoff", S1, S2, [0, 63, 130], [5, 64, 199], False),
    "config5": (progs.config5, N, "damp", S1, S2, [0, 63, 127, 128], [5, 64, 199, 126], False),
    "tiny": (lambda: TINY, 70, None, 10, 13, list(range(66)), list(range(4, 70)), False),
    "shadow_both": (lambda: SHADOW_BOTH, 130, None, 40, 50, [0, 63, 64, 129], [65, 1, 128, 62], False),
    "two_taps_dane": (lambda: TWO_TAPS, 130, None, 100, 37, [0, 63, 129], [64, 128, 1], True),
    "immediate": (progs.config3, N, "cutoff", 333, 0, [0, 63, 130], [5, 64, 199], False),
}


def twin_recall(gpu, tier, name):
    text, n, control, first, later, src, dst, dane = TWINS[name]
    text = text()
    cut = cutoffs(n) if control else None
    a, b = (make(gpu, text, n, control, cut, dane) for _ in range(2))
    x1, x2, x3 = progs.stimulus(n, first), progs.stimulus(n, max(later, 1), first_sample=first, seed=99)[:later], progs.stimulus(n, 300, first_sample=first + later, seed=7)
    assert np.array_equal(bits(run(a, x1)), bits(run(b, x1)))
    slots = np.arange(len(src))[::-1].copy()
    assert a.bank_create(len(src)) == 0 and a.bank_store(slots, src) == 0
    image = b.save_instances(src)
    if later:
        assert np.array_equal(bits(run(a, x2)), bits(run(b, x2)))
    before = counters(a)
    assert a.bank_recall(slots, dst) == 0
    assert b.load_instances_rotated(dst, image) == 0
    assert np.array_equal(a.save_state(), b.save_state()), "right after the recall"
    assert a.bank_status() == (0, -1, 0)
    after = counters(a)
    assert after["bank_recalls"] == before["bank_recalls"] + 1
    assert (after["instance_rotations"], after["instance_scatters"]) == (before["instance_rotations"], before["instance_scatters"])
    assert np.array_equal(bits(run(a, x3)), bits(run(b, x3)))
    assert right_tier(a, tier) and right_tier(b, tier), a.tier_note()
    assert np.array_equal(a.save_state(), b.save_state()), "after the last run"


@pytest.mark.parametrize("name", ["config3", "config5", "tiny", "shadow_both", "two_taps_dane"])
def test_recall_is_the_rotated_load(gpu, tier, name):
    twin_recall(gpu, tier, name)


def test_an_immediate_recall_is_rotation_zero_everywhere(gpu, monkeypatch):
    use_tier(monkeypatch, "xlate")
    twin_recall(gpu, "xlate", "immediate")


# ---- 3. against the oracle ----------------------------------------------------------------------------------------------------------
def test_undo_from_the_bank_against_the_oracle(gpu, tier):
    """the `undo` case of tests/test_gpu_instances_rot.py for config3, the bank in place of the image"""
    text, control, tram, sizes = progs.config3(), "cutoff", [(0, 1000)], (1000, 0)
    src, dst = [0, 63, 130], [5, 64, 199]
    cut = cutoffs(N)
    b, twin = handle(gpu, text, N, control, cut), handle(gpu, text, N, control, cut)
    x1, x2, x3 = progs.stimulus(N, S1), progs.stimulus(N, S2, first_sample=S1, seed=99), progs.stimulus(N, 300, first_sample=S1 + S2, seed=7)
    assert np.array_equal(bits(run(b, x1)), bits(run(twin, x1))) and right_tier(twin, tier), twin.tier_note()
    assert b.bank_create(3) == 0 and b.bank_store([2, 0, 1], src) == 0
    saved = [b.get_cursors_i(s) for s in src]
    run(b, x2)
    run(twin, x2)
    held = [b.get_cursors_i(d) for d in dst]
    assert b.bank_recall([2, 0, 1], dst) == 0
    y3, t3 = run(b, x3), run(twin, x3)
    assert b.bank_status() == (0, -1, 0)
    names = state_registers(text) + [control]
    for k, (s, d) in enumerate(zip(src, dst)):
        o, ref = replay(text, [x1[:, s], x3[:, d]], control, cut[s])
        shifts = shifts_between(saved[k], held[k], sizes)
        assert shifts[0] == 100
        continues_like(b, d, o, names, y3[:, d], ref, tram, shifts)
        assert b.get_cursors_i(d) == b.get_cursors_i(6), "the positions are those of an untouched neighbour"
    unlisted_equal_the_twin(b, twin, N, dst, y3, t3, names)


# ---- 4. fan-out from a preset -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entries", [1, 64, 65, 73])
def test_fan_out_from_a_preset(gpu, tier, entries):
    """a two-record image of another handle is put; slot 0 goes into 70 destinations over three wavefronts, slot 1 into 3"""
    text, control = progs.config3(), "cutoff"
    cut = cutoffs(N)
    a, b = handle(gpu, text, N, control, cut), handle(gpu, text, N, control, cut)
    xa, xb = progs.stimulus(N, S1), progs.stimulus(N, 700, seed=31)
    run(a, xa)
    run(b, xb)
    src = [0, 130]
    assert b.bank_create(2) == 0 and b.bank_put([0, 1], a.save_instances(src)) == 0
    dst = np.concatenate([np.arange(1, 196, 3), np.arange(2, 24, 3)])[:73]   # 65 + 8 distinct instances, 1 .. 193
    slots = np.zeros(73, dtype=np.int64)
    slots[[0, 40, 72]] = 1
    dst, slots = dst[:entries], slots[:entries]
    assert len(set(dst.tolist())) == entries and (entries < 73 or (dst.max() > 128 and dst.min() < 64))
    assert b.bank_recall(slots, dst) == 0
    x2 = progs.stimulus(N, 300, first_sample=700, seed=99)
    y2 = run(b, x2)
    assert right_tier(b, tier) and b.bank_status() == (0, -1, 0), b.tier_note()
    names = state_registers(text) + [control]
    for s, d in zip(slots, dst):
        o, ref = replay(text, [xa[:, src[s]], x2[:, d]], control, cut[src[s]])
        continues_like(b, int(d), o, names, y2[:, d], ref, [(0, 1000)], [(700 - S1) % 1000, 0])


# ---- 5. device refusals are all or nothing ------------------------------------------------------------------------------------------
def refused_then_good(gpu, b, twin, slots, dst, bad, reason):
    """the recall of `slots` into `dst` has the bad entry `bad`: nothing changes; without it the recall is the rotated load"""
    assert b.bank_status(reset=True)[0] == 0
    before = counters(b)
    assert b.bank_recall(slots, dst) == 0, "a recall the device refuses still returns 0"
    assert np.array_equal(b.save_state(), twin.save_state()), "a refused recall changed the batch"
    assert b.bank_status() == (1, bad, reason)
    assert b.info("bank_recalls") == before["bank_recalls"] + 1
    good = [k for k in range(len(dst)) if k != bad]
    gs, gd = [slots[k] for k in good], [dst[k] for k in good]
    assert b.bank_recall(gs, gd) == 0
    assert twin.load_instances_rotated(gd, b.bank_get(gs)) == 0
    assert np.array_equal(b.save_state(), twin.save_state()), "the good recall after the refused one"
    assert b.bank_status() == (1, bad, reason), "status counts nothing new"
    assert b.bank_status(reset=True)[0] == 1 and b.bank_status() == (0, -1, 0)


def test_a_record_in_another_phase_is_refused_on_the_device(gpu, tier):
    n = 130
    x = progs.stimulus(n, 90)
    b, twin = handle(gpu, SHADOW_READ, n), handle(gpu, SHADOW_READ, n)
    for h in (b, twin):
        run(h, x)
    assert right_tier(b, tier), b.tier_note()
    cur = [b.get_cursors_i(i) for i in range(n)]
    s, d = next((s, d) for s in range(n) for d in range(n) if s != d and (cur[d][0] - cur[s][0]) % 7 != (cur[d][1] - cur[s][1]) % 7)
    same = [(u, v) for u in range(n) for v in range(n) if u != v and cur[u] == cur[v] and v != d]
    (s0, d0) = same[0]
    (s2, d2) = next((u, v) for u, v in same if v != d0)
    assert b.bank_create(3) == 0 and b.bank_store([0, 1, 2], [s0, s, s2]) == 0
    refused_then_good(gpu, b, twin, [0, 1, 2], [d0, d, d2], 1, gpu.BANK_PHASE)


def test_a_rotation_on_a_line_that_is_no_ring_is_refused_on_the_device(gpu, tier):
    n = 70
    x = progs.stimulus(n, 13)
    b, twin = handle(gpu, OFFSET3, n), handle(gpu, OFFSET3, n)
    assert b.bank_create(3) == 0
    for h in (b, twin):
        run(h, x[:10])
    assert b.bank_store([1], [64]) == 0
    for h in (b, twin):
        run(h, x[10:])
    assert right_tier(b, tier), b.tier_note()
    assert b.bank_store([0, 2], [0, 5]) == 0
    refused_then_good(gpu, b, twin, [0, 1, 2], [69, 1, 20], 1, gpu.BANK_NO_RING)


def test_a_position_word_outside_the_line_is_refused_on_the_device(gpu, tier):
    n = 70
    b, twin = handle(gpu, TINY, n), handle(gpu, TINY, n)
    for h in (b, twin):
        run(h, progs.stimulus(n, 23))
    assert right_tier(b, tier), b.tier_note()
    image = b.save_instances([0, 64, 69])
    image[64:].view(np.uint32).reshape(3, -1)[1, cursor_word(b) + 2] = 11   # the xTRAM write position at Z
    assert b.bank_create(3) == 0 and b.bank_put([0, 1, 2], image) == 0
    refused_then_good(gpu, b, twin, [0, 1, 2], [1, 2, 65], 1, gpu.BANK_BAD_POSITION)


# ---- 6. host refusals ---------------------------------------------------------------------------------------------------------------
def test_host_refusals_launch_nothing_and_change_nothing(gpu):
    lib = gpu.load()
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    p = lambda v: C.c_void_p(v.ctypes.data if v is not None else 0)
    e = gpu.Batch(8, 1, 0)
    one = i64([0])
    assert lib.fxb_bank_create(e._h, 4) == FX_E_NOTREADY and lib.fxb_bank_store(e._h, p(one), p(one), 1) == FX_E_NOTREADY
    assert lib.fxb_bank_recall(e._h, p(one), p(one), 1) == FX_E_NOTREADY and e.bank_slots() == 0
    b = handle(gpu, progs.config3(), N, "cutoff", cutoffs(N))
    run(b, progs.stimulus(N, 40))
    image = b.save_instances([0, 1, 2])
    s3, l3 = i64([0, 1, 2]), i64([5, 64, 199])
    # no bank
    for rc in (lib.fxb_bank_store(b._h, p(s3), p(l3), 3), lib.fxb_bank_recall(b._h, p(s3), p(l3), 3), lib.fxb_bank_put(b._h, p(s3), 3, p(image), image.size),
               lib.fxb_bank_get(b._h, p(s3), 3, p(image), image.size), lib.fxb_bank_status(b._h, None, None, None, 0)):
        assert rc == FX_E_ARG and "bank" in b.last_error(), (rc, b.last_error())
    assert lib.fxb_bank_create(b._h, -1) == FX_E_ARG
    assert b.bank_create(4) == 0 and b.bank_store(s3, l3) == 0
    state, seen = b.save_state(), counters(b)
    other = handle(gpu, TINY, 8).save_instances([0, 1, 2])
    buf = np.empty(image.size, dtype=np.uint8)
    cases = {
        "store: count < 0": lib.fxb_bank_store(b._h, p(s3), p(l3), -1),
        "recall: count < 0": lib.fxb_bank_recall(b._h, p(s3), p(l3), -1),
        "store: null slots": lib.fxb_bank_store(b._h, None, p(l3), 3),
        "store: null list": lib.fxb_bank_store(b._h, p(s3), None, 3),
        "recall: null slots": lib.fxb_bank_recall(b._h, None, p(l3), 3),
        "recall: null list": lib.fxb_bank_recall(b._h, p(s3), None, 3),
        "put: null slots": lib.fxb_bank_put(b._h, None, 3, p(image), image.size),
        "get: null slots": lib.fxb_bank_get(b._h, None, 3, p(buf), buf.size),
        "store: slot outside": lib.fxb_bank_store(b._h, p(i64([0, 4, 2])), p(l3), 3),
        "store: slot below": lib.fxb_bank_store(b._h, p(i64([0, -1, 2])), p(l3), 3),
        "recall: slot outside": lib.fxb_bank_recall(b._h, p(i64([0, 1, 4])), p(l3), 3),
        "put: slot outside": lib.fxb_bank_put(b._h, p(i64([4, 1, 2])), 3, p(image), image.size),
        "get: slot outside": lib.fxb_bank_get(b._h, p(i64([0, 1, 4])), 3, p(buf), buf.size),
        "store: instance outside": lib.fxb_bank_store(b._h, p(s3), p(i64([5, N, 7])), 3),
        "recall: instance outside": lib.fxb_bank_recall(b._h, p(s3), p(i64([5, 64, -1])), 3),
        "store: a slot twice": lib.fxb_bank_store(b._h, p(i64([0, 1, 0])), p(l3), 3),
        "put: a slot twice": lib.fxb_bank_put(b._h, p(i64([2, 1, 2])), 3, p(image), image.size),
        "recall: a destination twice": lib.fxb_bank_recall(b._h, p(s3), p(i64([5, 64, 5])), 3),
        "get: a short buffer": lib.fxb_bank_get(b._h, p(s3), 3, p(buf), buf.size - 4),
        "get: no buffer": lib.fxb_bank_get(b._h, p(s3), 3, None, buf.size),
        "put: a truncated image": lib.fxb_bank_put(b._h, p(s3), 3, p(image), image.size - 4),
        "put: no image": lib.fxb_bank_put(b._h, p(s3), 3, None, image.size),
        "put: another count than the image's": lib.fxb_bank_put(b._h, p(s3), 2, p(image), image.size),
        "put: an image of another program": lib.fxb_bank_put(b._h, p(s3), 3, p(other), other.size),
    }
    for what, rc in cases.items():
        assert rc == FX_E_ARG, (what, rc)
    assert lib.fxb_bank_store(b._h, None, None, 0) == 0 and lib.fxb_bank_recall(b._h, None, None, 0) == 0
    assert lib.fxb_bank_put(b._h, None, 0, None, 0) == 0 and lib.fxb_bank_get(b._h, None, 0, None, 0) == 0
    assert counters(b) == seen and np.array_equal(b.save_state(), state)
    assert np.array_equal(b.bank_get(s3), b.save_instances(l3)), "the bank after the refusals"
    assert lib.fxb_bank_store(None, p(s3), p(l3), 3) == FX_E_ARG and lib.fxb_bank_slots(None) == 0


# ---- 7. stream order ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False])
def test_store_and_recall_queued_between_blocks(gpu, own_stream):
    """block, store, block, recall, block with one sync at the end equals a twin that waits after every step and goes through the host"""
    import torch

    n, S = 777, 2048
    text = progs.config3()
    cut = cutoffs(n)
    b, t = handle(gpu, text, n, "cutoff", cut), handle(gpu, text, n, "cutoff", cut)
    warm = progs.stimulus(n, 8)
    assert np.array_equal(bits(b.process_block(warm)), bits(t.process_block(warm)))
    blocks = [np.ascontiguousarray(progs.stimulus(n, S, first_sample=8 + k * S, seed=5 + k)).reshape(S, 1, n) for k in range(3)]
    stream = None if own_stream else torch.cuda.Stream()
    sp = None if own_stream else stream.cuda_stream
    d_in = [torch.from_numpy(x).to("cuda") for x in blocks]
    d_out = [torch.full((S, 1, n), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    src, dst = [0, 63, 700], [5, 64, 776]
    assert b.bank_create(3) == 0
    assert b.process_block_dev_pitched(d_in[0], d_out[0], S, stream=sp) == 0
    assert b.bank_store([0, 1, 2], src) == 0
    assert b.process_block_dev_pitched(d_in[1], d_out[1], S, stream=sp) == 0
    assert b.bank_recall([0, 1, 2], dst) == 0
    assert b.process_block_dev_pitched(d_in[2], d_out[2], S, stream=sp) == 0
    assert b.sync() == 0
    want = [t.process_block(blocks[0].reshape(S, n))]
    image = t.save_instances(src)
    want.append(t.process_block(blocks[1].reshape(S, n)))
    assert t.load_instances_rotated(dst, image) == 0
    want.append(t.process_block(blocks[2].reshape(S, n)))
    for k in range(3):
        assert np.array_equal(bits(d_out[k].cpu().numpy().reshape(S, n)), bits(want[k])), "block %d" % k
    assert np.array_equal(b.save_state(), t.save_state()) and b.bank_status() == (0, -1, 0)
    assert not np.array_equal(bits(want[2][:, 5]), bits(want[2][:, 6])), "the recalled voice matters to the words compared"


# ---- 8. shards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
def test_shards_hold_the_bank_each_and_equal_the_single_handle(gpu, shards):
    text, control = progs.config3(), "cutoff"
    cut = cutoffs(N)
    b, one = (make(gpu, text, N, control, cut, devices=dev) for dev in ([0] * shards, None))
    firsts = [f for _, f, _ in b.shards()]
    assert len(firsts) == shards and firsts[1] == 128
    x1, x2, x3 = progs.stimulus(N, 337), progs.stimulus(N, 150, first_sample=337, seed=99), progs.stimulus(N, 100, first_sample=487, seed=7)
    for h in (b, one):
        run(h, x1)
        assert h.bank_create(3) == 0 and h.bank_store([1, 0], [0, 63]) == 0
    assert b.info("bank_bytes") == shards * one.info("bank_bytes") and b.info("bank_slots") == 3
    assert np.array_equal(b.bank_get([0, 1]), one.bank_get([0, 1]))
    slots, dst = [0, 1, 0, 1], [5, 130, 199, 64]   # every shard, and 130 / 199 from a record of the first shard
    for h in (b, one):
        run(h, x2)
    for h in (b, one):
        assert h.bank_recall(slots, dst) == 0
        run(h, x3)
    assert np.array_equal(b.save_state(), one.save_state()) and b.bank_status() == (0, -1, 0)
    assert b.info("bank_recalls") == shards and one.info("bank_recalls") == 1
    # one bad entry: its shard's part is untouched, the other shards' parts run; the entry is the caller's
    image = one.bank_get([0])
    image[64:].view(np.uint32)[cursor_word(one)] = 1000   # the iTRAM write position at Z
    for h in (b, one):
        assert h.bank_put([2], image) == 0
    slots, dst = [0, 2, 1, 0], [6, 131, 198, 65]
    shard_of = lambda i: max(k for k, f in enumerate(firsts) if f <= i)
    spared = [k for k, d in enumerate(dst) if shard_of(d) != shard_of(131)]
    assert spared == ([0, 3] if shards == 2 else [0, 2, 3])
    assert b.bank_recall(slots, dst) == 0 and b.bank_status() == (1, 1, gpu.BANK_BAD_POSITION)
    assert one.bank_recall([slots[k] for k in spared], [dst[k] for k in spared]) == 0 and one.bank_status() == (0, -1, 0)
    assert np.array_equal(b.save_state(), one.save_state())


# ---- 9. registers -------------------------------------------------------------------------------------------------------------------
def test_what_the_host_knows_about_registers_follows_a_recall(gpu):
    x = progs.stimulus(N, 24)

    def voice():
        b = handle(gpu, RINGS, N)
        run(b, x[:9])
        assert b.bank_create(2) == 0
        return b, b.info("num_lane_regs")

    b, rows = voice()   # never moved: no other code
    assert b.bank_store([1], [3]) == 0
    run(b, x[9:16])
    assert b.bank_recall([1], [7]) == 0
    assert b.info("num_lane_regs") == rows and b.get_register_i("vol", 7) == 0.5
    b, rows = voice()   # a recall across a broadcast set
    assert b.bank_store([1], [3]) == 0 and b.set_register("vol", 0.25) == 0
    run(b, x[9:16])
    assert b.bank_recall([1], [7]) == 0
    assert b.get_register_i("vol", 7) == 0.5 and b.get_register_i("vol", 8) == 0.25 and b.get_register_i("vol", 199) == 0.25
    assert b.info("num_lane_regs") == rows + 1, "vol has a row of its own from now on"
    y = run(b, x[16:])
    o, ref = replay(RINGS, [x[:9, 3], x[16:, 7]])
    assert np.array_equal(bits(y[:, 7]), bits(ref)), "the recalled voice plays with the stored value"
    b, rows = voice()   # stored from a voice whose control was set per instance
    assert b.set_register_i("vol", 3, 0.75) == 0 and b.bank_store([0], [3]) == 0 and b.bank_recall([0], [7]) == 0
    assert b.get_register_i("vol", 7) == 0.75 and b.get_register_i("vol", 8) == 0.5


# ---- 10. lifetime -------------------------------------------------------------------------------------------------------------------
def test_a_program_load_drops_the_bank_and_a_new_bank_keeps_nothing(gpu):
    lib = gpu.load()
    b = handle(gpu, progs.config3(), N, "cutoff", cutoffs(N))
    run(b, progs.stimulus(N, 40))
    assert b.bank_create(2) == 0 and b.bank_store([0, 1], [5, 64]) == 0
    assert b.bank_get([0])[64:].any()
    assert b.bank_create(5) == 0 and b.bank_slots() == 5 and not b.bank_get([0, 1, 2, 3, 4])[64:].any(), "a replaced bank keeps nothing"
    words = b.instance_words
    assert b.load_text(MORE), b.errors()
    assert b.instance_words > words and b.bank_slots() == 0   # (the load's registers have rows of their own: records of another size) and b.info("bank_bytes") == 0
    one = np.zeros(1, dtype=np.int64)
    assert lib.fxb_bank_recall(b._h, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), 1) == FX_E_ARG
    assert b.bank_create(3) == 0 and b.bank_slots() == 3
    run(b, progs.stimulus(N, 23))
    assert b.bank_store([2], [199]) == 0 and np.array_equal(b.bank_get([2]), b.save_instances([199]))
    assert b.bank_create(0) == 0 and b.bank_slots() == 0
