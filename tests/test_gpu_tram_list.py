"""Delay-line windows by list on the GPU: fxb_set_tram_list / fxb_get_tram_list (kernels fx_tram_scatter / fx_tram_gather in
csrc/fx_tram.hip).  The kernels move words, so the bar everywhere is equality of 32-bit patterns: against a twin handle that
receives the same words through fxb_save_instances, an edit of its records and fxb_load_instances (the parent's only way to the
same effect), against oracle objects that were FED the words a logical set writes, for positions that differ per instance, for
delay memory tiled 128 and 256 columns wide, for staged code, for blocks queued on other streams around the sets, for the quiet
loop's head check and for a handle of two shards.  Which slot a logical index means is worked out here in numpy with `%` from
fxb_get_cursors_i (or the oracle's positions).  The host side without a GPU is tests/test_tram_list_stub.py."""
import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle
from test_gpu_bus_gain import kernel_tier, right_tier  # noqa: F401  (the fixture)
from test_gpu_instances import bits, handle, use_tier
from test_gpu_instances_rot import OPT_DANE, SHADOW_BOTH, TINY, TWO_TAPS, WRITE_IN
from test_gpu_quiet_states import ABOVE, WATCH5, config5_pair, quiet5

pytestmark = pytest.mark.gpu

FX_E_ARG = -3
LOGICAL, BROADCAST = 1, 2
N = 130   # two wavefronts and a tail of two lanes
# +0, -0, the smallest denormal, the largest (negative), +-1e30, a quiet NaN with a payload, a signalling NaN
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7149f2ca, 0xf149f2ca, 0x7fc12345, 0x7f812345], dtype=np.uint32)


def a_list(rng, n_all, n):
    """n distinct instances of 0..n_all-1 in a shuffled order, 0 and n_all - 1 among them (n == 1: n_all - 1; n >= n_all: all of them)"""
    if n >= n_all:
        return rng.permutation(n_all).astype(np.int64)
    if n == 1:
        return np.array([n_all - 1], dtype=np.int64)
    return rng.permutation(np.concatenate([[0, n_all - 1], rng.permutation(np.arange(1, n_all - 1))[:n - 2]])).astype(np.int64)


def windows_for(rng, count, n_words, step=0):
    """[count, n_words] float32: small finite values, with the special patterns walking through the words from one set to the next"""
    v = rng.uniform(-0.5, 0.5, (count, n_words)).astype(np.float32)
    flat = v.view(np.uint32)
    for i in range(count):
        for j, s in enumerate(SPECIALS):
            flat[i, (step + i + j * 3) % n_words] = s
    return v


def slots_of(positions, which, Z, first, n_words, logical, dane):
    """[count, n_words]: the slot of every window word from the definition in include/fx8010_amd.h; positions: one get_cursors_i
    answer per listed instance"""
    a = first + np.arange(n_words, dtype=np.int64)
    if not logical:
        return np.tile(a, (len(positions), 1))
    p = np.array([c[2 * which] for c in positions], dtype=np.int64)[:, None]
    return (p + 1 + a) % Z if dane else (p - 1 - a) % Z


def line_offset(h, which):
    """the first record word of a delay line: stateRows (+ iSlots)"""
    return h.info("instance_words") - h.info("xtram_slots") - (h.info("itram_slots") if which == 0 else 0)


def twin_set(t, which, L, slots, rows):
    """the same words through save_instances, an edit of the record words stateRows (+ iSlots) + slot, load_instances"""
    W = t.info("instance_words")
    image = t.save_instances(L)
    rec = image[64:].view(np.uint32).reshape(len(L), W)
    off = line_offset(t, which)
    for i in range(len(L)):
        rec[i, off + slots[i]] = bits(rows[i])
    assert t.load_instances(L, image) == 0


def set_both(b, t, which, L, first, v, logical, dane=False):
    Z = b.info("xtram_slots" if which else "itram_slots")
    slots = slots_of([t.get_cursors_i(int(i)) for i in L], which, Z, first, v.shape[-1], logical, dane)
    rows = np.tile(v, (len(L), 1)) if v.ndim == 1 else v
    assert b.set_tram_list(which, L, first, v, logical=logical) == 0, b.last_error()
    twin_set(t, which, L, slots, rows)
    return slots


def same_get(b, t, which, L, first, n_words, logical, dane, what):
    """get_tram_list in the mode asked for against get_tram_i of both handles through the numpy model; physical: word for word"""
    A = b.info("xtram_slots" if which else "itram_slots")
    got = b.get_tram_list(which, L, first, n_words, logical=logical)
    assert got.shape == (len(L), n_words)
    slots = slots_of([b.get_cursors_i(int(i)) for i in L], which, A, first, n_words, logical, dane)
    for i, inst in enumerate(L):
        mine, twin = bits(b.get_tram_i(which, int(inst), A)), bits(t.get_tram_i(which, int(inst), A))
        assert np.array_equal(bits(got[i]), mine[slots[i]]) and np.array_equal(bits(got[i]), twin[slots[i]]), (what, i, inst)


def dane_handle(gpu, text, n, dane, devices=None):
    b = gpu.Batch(n, 1, 0) if devices is None else gpu.Batch(n, 1, devices=devices)
    if dane:
        b.set_option(gpu.OPT_TRAM_DANE)
    assert b.load_text(text), b.errors()
    return b


# ---- 1. against the twin, all three tiers ------------------------------------------------------------------------------------------
CASES = [("TINY", TINY, False), ("TWO_TAPS", TWO_TAPS, False), ("TWO_TAPS-dane", TWO_TAPS, True)]


@pytest.mark.parametrize("kernel_tier", ["default", "asm", "hip"], indirect=True)
@pytest.mark.parametrize("name,text,dane", CASES, ids=[c[0] for c in CASES])
def test_window_sets_equal_the_twin_bit_for_bit(gpu, kernel_tier, name, text, dane):
    """physical and logical sets with the special patterns in front of blocks of 33, 1 and 2 samples; lists of 1, 64, 65 and N
    entries; outputs, get_tram_i of the listed instances, get_tram_list in both modes and save_state() after every block; the two
    counters count the launches.  TWO_TAPS without the DANE model writes its xTRAM at offset 3: 503 slots, no ring - physical only"""
    rng = np.random.default_rng(len(name) * 1000 + len(kernel_tier))
    b, t = dane_handle(gpu, text, N, dane), dane_handle(gpu, text, N, dane)
    x = progs.stimulus(N, 400)
    clock = 5
    assert np.array_equal(bits(b.process_block(x[:clock])), bits(t.process_block(x[:clock])))
    rings = b.info("instance_rings")
    sizes = (b.info("itram_slots"), b.info("xtram_slots"))
    assert rings == {"TINY": 3, "TWO_TAPS": 1, "TWO_TAPS-dane": 3}[name] and sizes == {"TINY": (7, 11), "TWO_TAPS": (64, 503), "TWO_TAPS-dane": (64, 500)}[name]
    sets = gets = step = 0
    for which in (0, 1):
        A = sizes[which]
        for logical in (True, False):
            if logical and not rings & (1 << which):
                with pytest.raises(RuntimeError, match="ring"):
                    b.set_tram_list(which, [0], 0, np.zeros(4, dtype=np.float32), logical=True)
                continue
            for entries in (1, 64, 65, N):
                S = (33, 1, 2)[step % 3]
                L = a_list(rng, N, entries)
                n_words = (A, min(A, 65), 1, max(A // 2, 1))[step % 4]
                first = (A - 1, A // 2, 0)[step % 3] if logical else (A - n_words, 0, (A - n_words) // 2)[step % 3]
                what = "%s %s: line %d, %s, %d entries, first %d, %d words, S %d" % (name, kernel_tier, which, "logical" if logical else "physical", entries, first, n_words, S)
                step += 1
                set_both(b, t, which, L, first, windows_for(rng, L.size, n_words, step), logical, dane)
                sets += 1
                assert b.info("tram_list_sets") == sets, what
                few = L[:3]
                for inst in few:
                    assert np.array_equal(bits(b.get_tram_i(which, int(inst), A)), bits(t.get_tram_i(which, int(inst), A))), (what, inst)
                same_get(b, t, which, few, first, n_words, logical, dane, what)
                gets += 1
                assert np.array_equal(bits(b.process_block(x[clock:clock + S])), bits(t.process_block(x[clock:clock + S]))), what
                clock += S
                assert np.array_equal(b.save_state(), t.save_state()), what
                same_get(b, t, which, L, 0, A, False, dane, what)
                gets += 1
                if rings & (1 << which):
                    same_get(b, t, which, L, A - 1, A, True, dane, what)
                    gets += 1
                assert b.info("tram_list_gets") == gets, what
    assert right_tier(b, kernel_tier) and right_tier(t, kernel_tier), b.tier_note()
    assert b.ood_flags() == t.ood_flags()
    for h in (b, t):
        h.close()


# ---- 2. against the oracle, in the reference's own words ---------------------------------------------------------------------------
ORACLE_CASES = [("WRITE_IN", WRITE_IN, 0, 16, 0, False), ("WRITE_IN-dane", WRITE_IN, 0, 16, 0, True), ("TWO_TAPS-xtram-dane", TWO_TAPS, 1, 500, 3, True)]


@pytest.mark.parametrize("S0", [16, 37, 100])
@pytest.mark.parametrize("name,text,which,Z,tap,dane", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_a_logical_set_is_what_the_oracle_was_fed(gpu, monkeypatch, name, text, which, Z, tap, dane, S0):
    """one oracle object per listed instance.  Handle and oracles get the same samples first (S0 - Z of them for the line of 16; S0
    for the line of 500, which is longer than every S0 - the set then stands S0 + Z samples in), so that the wrap lies at
    different places.  Then the oracle gets a window u, reversed, as its last Z inputs while the handle gets Z zeros.  Then
    set_tram_list(logical) of u on the handle - the write tap at position `tap` stored its newest word at age `tap` - and from
    there outputs, delay memory, positions and registers agree bit for bit over 3 Z further samples, run in four blocks.  The oracle's
    out-of-domain flags stay 0.
    WRITE_IN: outputs over the Z samples of the feed agree already - the words are not read yet.  TWO_TAPS (its xTRAM is written at
    position 3: a ring under the DANE model only) cannot have that: its output hears the input through the iTRAM, 7 and 19 samples
    later, so the feed itself sounds, and what the oracle heard also sits in its iTRAM and in the register w.  The handle gets
    those from the oracle object - the logical window of the iTRAM by list, w by fxb_set_registers_list (that window is cut from
    the oracle's memory with the formula under test: it only keeps the outputs comparable, the test is not about it).  What the
    test rests on is the line `which`: u as the test drew it, compared with the oracle's memory right behind the set and then,
    with the registers that read it, after Z / 10, Z / 2, 9 Z / 10 and 3 Z samples."""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    rng = np.random.default_rng(S0 * 7 + Z)
    prefix = S0 - Z if Z <= S0 else S0
    b = dane_handle(gpu, text, N, dane)
    assert b.info("instance_rings") & (1 << which)
    L = np.array([129, 0, 64, 63, 128, 65], dtype=np.int64)
    x1, x3 = progs.stimulus(N, max(prefix, 1))[:prefix], progs.stimulus(N, 3 * Z, first_sample=1000, seed=5)
    u = windows_for(rng, L.size, Z, S0)
    feed = np.zeros((Z, N), dtype=np.float32)
    if prefix:
        b.process_block(x1)
    y2 = b.process_block(feed)
    oracles = []
    for k, inst in enumerate(L):
        o = Oracle(1)
        if dane:
            o.set_option(OPT_DANE)
        assert o.load_text(text), o.errors()
        if prefix:
            o.process_block(np.ascontiguousarray(x1[:, inst]))
        r2 = o.process_block(np.ascontiguousarray(u[k][::-1]))
        if text is WRITE_IN:
            assert np.array_equal(bits(y2[:, inst]), bits(r2)), (inst, "the words are not read yet")
        oracles.append(o)
    assert b.set_tram_list(which, L, tap, u, logical=True) == 0, b.last_error()
    assert b.info("tram_list_sets") == 1
    if text is TWO_TAPS:
        heard = np.stack([bits(o.tram(0, 64))[(o.cursors()[0] + 1 + np.arange(64)) % 64].view(np.float32) for o in oracles])
        assert b.set_tram_list(0, L, 0, heard, logical=True) == 0, b.last_error()
        w = np.array([o.get_register_bits("w") for o in oracles], dtype=np.uint32).view(np.float32)
        assert b.set_registers_list(["w"], L, w[None, :]) == 0, b.last_error()
    names = [w.split()[1] for w in text.split("\n") if w.startswith("static ")] + ["out", "ccr"]
    # right behind the set, before any block: the line of every listed instance is the oracle's, word for word, and so are the
    # positions - a window one slot off, or no write at all, stops here.  (The registers wait for the first sample: TWO_TAPS'
    # xr still holds the zero the handle read last.)
    for inst, o in zip(L, oracles):
        assert np.array_equal(bits(b.get_tram_i(which, int(inst), Z)), bits(o.tram(which, Z))), (inst, "right behind the set")
        assert np.array_equal(bits(b.get_tram_list(which, [int(inst)], tap, Z, logical=True)[0]), bits(u[list(L).index(inst)])), inst
        assert b.get_cursors_i(int(inst)) == o.cursors(), inst
    # x3 in four blocks: after Z / 10, Z / 2 and 9 Z / 10 samples words of u are still in the ring and being read (TWO_TAPS reads
    # its xTRAM 400 samples behind the write tap into xr), after 3 Z none is left
    cuts = [0, max(Z // 10, 1), Z // 2, 9 * Z // 10, 3 * Z]
    y3 = []
    for lo, hi in zip(cuts, cuts[1:]):
        y = b.process_block(np.ascontiguousarray(x3[lo:hi]))
        y3.append(y)
        for k, (inst, o) in enumerate(zip(L, oracles)):
            r3 = o.process_block(np.ascontiguousarray(x3[lo:hi, inst]))
            if text is TWO_TAPS and hi < 400:   # (the read tap is 400 samples behind the write tap: what xr holds is a word of this instance's u)
                assert b.get_register_bits_i("xr", int(inst)) in set(bits(u[k]).tolist()), (inst, hi)
            assert np.array_equal(bits(y[:, inst]), bits(r3)), (inst, lo, np.argwhere(bits(y[:, inst]) != bits(r3))[:4].tolist())
            assert np.array_equal(bits(b.get_tram_i(which, int(inst), Z)), bits(o.tram(which, Z))), (inst, hi)
            assert b.get_cursors_i(int(inst)) == o.cursors(), (inst, hi)
            for r in names:
                assert b.get_register_bits_i(r, int(inst)) == o.get_register_bits(r), (inst, hi, r)
            assert o.ood_flags() == 0
    y3 = np.concatenate(y3, axis=0)
    # an instance the list did not name heard the zeros
    o = Oracle(1)
    if dane:
        o.set_option(OPT_DANE)
    assert o.load_text(text)
    for part in ([x1[:, 1]] if prefix else []) + [feed[:, 1], x3[:, 1]]:
        ref = o.process_block(np.ascontiguousarray(part))
    assert np.array_equal(bits(y3[:, 1]), bits(ref)) and b.ood_flags() == 0
    b.close()


def test_the_reference_model_refuses_a_logical_window_on_a_line_written_at_an_offset(gpu):
    b = dane_handle(gpu, TWO_TAPS, N, False)
    assert b.info("instance_rings") == 1
    with pytest.raises(RuntimeError, match="xTRAM"):
        b.get_tram_list(1, [0], 0, 4, logical=True)
    assert b.info("tram_list_gets") == 0
    b.close()


# ---- 3. positions that differ per instance, 5. staged code --------------------------------------------------------------------------
def against_the_oracles(gpu, text, Z, S, lanes, tier_ok):
    """after S samples: the logical get of every instance equals the numpy model on its OWN positions and delay memory, and
    for `lanes` the model on the oracle's; then the line of those lanes is overwritten slot by slot and put back with a logical
    set of the oracle's window, newest word first - words land where each lane's ring stands - and the handle continues like the
    oracles: outputs, delay memory, positions, registers"""
    x = progs.stimulus(N, S + 40)
    b = handle(gpu, text, N)
    b.process_block(x[:S])
    assert tier_ok(b), b.tier_note()
    every = np.arange(N, dtype=np.int64)
    got = b.get_tram_list(0, every, 0, Z, logical=True)
    cur = [b.get_cursors_i(i) for i in range(N)]
    for i in range(N):
        assert np.array_equal(bits(got[i]), bits(b.get_tram_i(0, i, Z))[(cur[i][0] - 1 - np.arange(Z)) % Z]), i
    oracles, windows = {}, []
    for inst in lanes:
        o = Oracle(1)
        assert o.load_text(text), o.errors()
        o.process_block(np.ascontiguousarray(x[:S, inst]))
        assert o.cursors() == cur[inst], inst
        windows.append(bits(o.tram(0, Z))[(o.cursors()[0] - 1 - np.arange(Z)) % Z].view(np.float32))
        assert np.array_equal(bits(got[inst]), bits(windows[-1])), inst
        oracles[inst] = o
    L = np.array(lanes, dtype=np.int64)
    assert b.set_tram_list(0, L, 0, np.full(Z, np.float32(0.123))) == 0
    assert all((bits(b.get_tram_i(0, int(i), Z)) == bits(np.float32(0.123))).all() for i in L)
    assert b.set_tram_list(0, L, 0, np.stack(windows), logical=True) == 0
    y = b.process_block(x[S:])
    names = [w.split()[1] for w in text.split("\n") if w.startswith("static ") and w.split()[1] != "noise"] + ["out", "ccr"]
    for inst, o in oracles.items():
        ref = o.process_block(np.ascontiguousarray(x[S:, inst]))
        assert np.array_equal(bits(y[:, inst]), bits(ref)), inst
        assert np.array_equal(bits(b.get_tram_i(0, inst, Z)), bits(o.tram(0, Z))) and b.get_cursors_i(inst) == o.cursors(), inst
        for r in names:
            assert b.get_register_bits_i(r, inst) == o.get_register_bits(r), (inst, r)
    return b, cur


@pytest.mark.parametrize("tier", ["hip", "xlate"])
def test_positions_that_differ_per_instance(gpu, monkeypatch, tier):
    """delay instructions in a SKIP shadow taken by the sign of the input: lanes of one wavefront stand at different positions"""
    use_tier(monkeypatch, tier)
    b, cur = against_the_oracles(gpu, SHADOW_BOTH, 7, 90, [0, 1, 5, 62, 63, 64, 65, 128, 129], lambda h: h.info("kernel") == 0 if tier == "hip" else h.info("kernel") != 0)
    assert len({c[0] for c in cur[:64]}) > 1, "the positions differ inside the first wavefront"
    b.close()


def test_staged_code_keeps_the_position_rows_current(gpu, monkeypatch):
    """the program of test_gpu_stages.test_delay_lines_noise_skip_and_tables_in_stages in four stages (the delay line and the noise
    stay in stage 0): a logical get and a logical set behind a block, against the oracle"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES_TUNE", "FX_STAGES_GROUP"):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setenv("FX_STAGES", "4")
    text = ("itramsize 11 \ninput in 0\noutput out 0\ncontrol k = 0.25\nstatic noise\nstatic rd\nstatic a\nstatic t\nstatic u\nstatic w\n"
            + "".join("static s%d\n" % i for i in range(10))
            + "idelay read, rd, at, 0\nmacs a, in, rd, 0.5\nmacs a, a, noise, 0.125\nidelay write, a, at, 0\n"
            + "".join("interp s%d, s%d, k, %s\nmacs t, s%d, a, 0.05\n" % (i, i, "a" if i == 0 else "t", i) for i in range(4))
            + "macs u, t, 0, 0\nskip ccr, ccr, 6, 2\nmacs t, t, 0.5, 0.5\nmacs out, out, t, 0.1\nlog w, u, 3, 0\nexp u, w, 5, 0\n"
            + "".join("interp s%d, s%d, k, %s\nmacs t, s%d, u, 0.05\n" % (i, i, "t", i) for i in range(4, 10))
            + "macs out, out, t, 0.5\nend")
    b, _ = against_the_oracles(gpu, text, 11, 27, [0, 63, 64, 129], lambda h: h.info("kernel") >= 9)
    assert b.info("waves_per_wg") >= 2 and b.ood_flags() == 0
    b.close()


# ---- 4. several instances per lane --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["hip2", "hip4"])
def test_windows_on_the_hip_tier_with_several_instances_per_lane(gpu, monkeypatch, lanes):
    """delay memory tiled in 128 / 256 columns, N = 777: lists on both sides of the column-tile boundaries, and a shuffled 300"""
    use_tier(monkeypatch, lanes)
    n = 777
    rng = np.random.default_rng(int(lanes[3:]))
    b, t = handle(gpu, TINY, n), handle(gpu, TINY, n)
    x = progs.stimulus(n, 60)
    for h in (b, t):
        h.process_block(x[:9])
    assert b.info("inst_per_lane") == int(lanes[3:]) and b.info("kernel") == 0
    edges = np.array([127, 128, 255, 256, 63, 64, 511, 512, 0, 776, 767, 768], dtype=np.int64)
    clock = 9
    for step, (which, L, logical) in enumerate(((0, edges, True), (1, edges[::-1].copy(), False), (1, a_list(rng, n, 300), True), (0, a_list(rng, n, n), False))):
        A = (7, 11)[which]
        n_words = (A, 5, A, 3)[step]
        first = (A - 2, 6, 0, 4)[step]
        set_both(b, t, which, L, first, windows_for(rng, L.size, n_words, step), logical)
        same_get(b, t, which, L[:70], first, n_words, logical, False, (lanes, step))
        assert np.array_equal(bits(b.process_block(x[clock:clock + 7])), bits(t.process_block(x[clock:clock + 7]))), step
        clock += 7
        assert np.array_equal(b.save_state(), t.save_state()), step
    for h in (b, t):
        h.close()


# ---- 6. ordering -------------------------------------------------------------------------------------------------------------------
def test_window_sets_between_blocks_on_other_streams(gpu, monkeypatch):
    """a block on stream A, a window set, a block on stream B, another set, a block on the handle's own stream, fxb_sync once: each
    block sees exactly the sets queued before it (TWO_TAPS reads its iTRAM 7 and 19 samples back: a window shows in the output
    at once).  S = 4096 at N = 777: the first block is still running when the set is queued.  Then a set followed by
    copy_instances of a written voice: the copy carries the written words"""
    import torch

    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    n, S = 777, 4096
    rng = np.random.default_rng(61)
    b, t = handle(gpu, TWO_TAPS, n), handle(gpu, TWO_TAPS, n)
    warm = progs.stimulus(n, 8)
    assert np.array_equal(bits(b.process_block(warm)), bits(t.process_block(warm)))
    blocks = [np.ascontiguousarray(progs.stimulus(n, S, first_sample=8 + k * S, seed=k).reshape(S, 1, n)) for k in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = [torch.from_numpy(x).to("cuda") for x in blocks]
    d_out = [torch.full((S, 1, n), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    L1, L2 = a_list(rng, n, 257), a_list(rng, n, 65)
    v1, v2 = windows_for(rng, L1.size, 64, 0), windows_for(rng, L2.size, 40, 3)
    assert b.process_block_dev_pitched(d_in[0], d_out[0], S, stream=streams[0].cuda_stream) == 0
    assert b.set_tram_list(0, L1, 0, v1, logical=True) == 0
    assert b.process_block_dev_pitched(d_in[1], d_out[1], S, stream=streams[1].cuda_stream) == 0
    assert b.set_tram_list(0, L2, 50, v2, logical=True) == 0
    assert b.process_block_dev_pitched(d_in[2], d_out[2], S) == 0
    assert b.sync() == 0
    want = [t.process_block(blocks[0][:, 0])]
    twin_set(t, 0, L1, slots_of([t.get_cursors_i(int(i)) for i in L1], 0, 64, 0, 64, True, False), v1)
    want.append(t.process_block(blocks[1][:, 0]))
    twin_set(t, 0, L2, slots_of([t.get_cursors_i(int(i)) for i in L2], 0, 64, 50, 40, True, False), v2)
    want.append(t.process_block(blocks[2][:, 0]))
    for k in range(3):
        assert np.array_equal(bits(d_out[k].cpu().numpy()[:, 0]), bits(want[k])), "block %d: the windows queued before it, and no other" % k
    plain = handle(gpu, TWO_TAPS, n)
    plain.process_block(warm)
    plain.process_block(blocks[0][:, 0])
    assert not np.array_equal(bits(plain.process_block(blocks[1][:, 0])[:64, L1]), bits(want[1][:64, L1])), "the windows matter to the words compared"
    assert np.array_equal(b.save_state(), t.save_state()) and b.info("tram_list_sets") == 2
    # a set followed by a copy of a written voice
    src, dst = int(L2[0]), int(np.setdiff1d(np.arange(n), L2)[0])
    v3 = windows_for(rng, L2.size, 500, 1)
    assert b.set_tram_list(1, L2, 0, v3) == 0
    b.copy_instances([src], [dst])
    assert np.array_equal(bits(b.get_tram_i(1, dst, 503))[:500], bits(v3[0])) and np.array_equal(bits(b.get_tram_list(1, [dst, src], 0, 500)), bits(v3[[0, 0]]))
    for h in (b, t, plain):
        h.close()


# ---- 7. the quiet loop -------------------------------------------------------------------------------------------------------------
def test_written_words_send_a_wavefront_out_of_the_quiet_loop(gpu, monkeypatch):
    """config5 with its quiet loop in force: 1.5, the next float above the bound of the read rows (0.25) and a NaN are written, one
    after the other, into the slots the four leading delay reads of lane 70 fill in the next sample (the slots on both sides of
    its read position).  The twin gets the same words through save_instances / load_instances.  Outputs, the state image and
    FXB_INFO_XLATE_QUIET_LEFT equal the twin's, and the head check catches the row each time: wavefront 1 leaves, as for loaded
    records"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES", "FX_XLATE_PRIO"):
        monkeypatch.delenv(env, raising=False)
    b, w = config5_pair(gpu)
    t, _ = config5_pair(gpu)
    x = quiet5(24, watched=WATCH5, level=0.2)
    _, left = w.run(b, x, "before the sets")
    t.process_block(x)
    assert b.info("xlate_quiet") == 1 and left == 0 and b.info("xlate_quiet_left") == 0 and t.info("xlate_quiet_left") == 0
    Z = 8192
    assert b.info("xtram_slots") == Z and b.info("instance_rings") == 2
    lane = np.array([70], dtype=np.int64)
    bound = max([bd for _, bd in w.reads] or [0.25])
    assert bound == 0.25 and np.float32(ABOVE) > np.float32(bound), w.reads
    for k, value in enumerate((np.float32(1.5), np.float32(ABOVE), np.float32(np.nan))):
        r = b.get_cursors_i(70)[3]
        assert r == t.get_cursors_i(70)[3] and 16 <= r < Z - 16, r
        v = np.full((1, 17), value, dtype=np.float32)
        assert b.set_tram_list(1, lane, r - 8, v) == 0
        twin_set(t, 1, lane, np.arange(r - 8, r + 9)[None, :], v)
        xk = quiet5(6, seed=k + 1, watched=WATCH5, level=0.2)
        yb, yt = b.process_block(xk), t.process_block(xk)
        assert np.array_equal(bits(yb), bits(yt)), k
        assert b.info("xlate_quiet_left") == t.info("xlate_quiet_left") == 1, (k, b.info("xlate_quiet_left"), t.info("xlate_quiet_left"))
        assert np.array_equal(b.save_state(), t.save_state()), k
        assert b.info("xlate_quiet") == 1
        # back to silence in that lane: its line and its registers as a fresh voice
        for h in (b, t):
            h.reset_instances(lane)
            h.process_block(quiet5(24, seed=10 + k, watched=WATCH5, level=0.2))
        assert np.array_equal(b.save_state(), t.save_state()) and b.info("xlate_quiet_left") == t.info("xlate_quiet_left"), k
    assert b.info("tram_list_sets") == 3
    for h in (b, t):
        h.close()


# ---- 8. two shards on one GPU -------------------------------------------------------------------------------------------------------
def test_two_shards_on_one_gpu_equal_the_single_handle(gpu, monkeypatch):
    """devices = [0, 0]: a list across the boundary and one wholly inside the last shard, physical and logical; every refusal
    leaves both shards unchanged"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    n, S = 64 * 10 + 17, 33
    rng = np.random.default_rng(n)
    one = handle(gpu, TINY, n)
    many = handle(gpu, TINY, n, devices=[0, 0])
    (_, _, _), (_, first, count) = many.shards()
    x = progs.stimulus(n, 8 * S)
    for h in (many, one):
        h.process_block(x[:5])
    inside = (first + rng.permutation(count)[:65]).astype(np.int64)
    across = np.concatenate([np.arange(first - 40, first + 40), [0, n - 1]]).astype(np.int64)
    rng.shuffle(across)
    clock = 5
    for step, (which, L, logical) in enumerate(((0, across, True), (1, across, False), (1, inside, True), (0, inside[:1], False), (1, a_list(rng, n, n), True))):
        A = (7, 11)[which]
        n_words, at = (A, 4, A, 2, 6)[step], (5, 7, 10, 3, 0)[step]
        v = windows_for(rng, L.size, n_words, step)
        before = many.info("tram_list_sets")
        for h in (many, one):
            assert h.set_tram_list(which, L, at, v, logical=logical) == 0, h.last_error()
        launched = many.info("tram_list_sets") - before
        assert launched == (1 if L is inside or L.size == 1 else 2), "a shard without an entry launches nothing"
        assert np.array_equal(bits(many.get_tram_list(which, L, at, n_words, logical=logical)), bits(v)), step
        assert np.array_equal(bits(many.get_tram_list(which, L, 0, A, logical=True)), bits(one.get_tram_list(which, L, 0, A, logical=True))), step
        assert np.array_equal(bits(many.process_block(x[clock:clock + S])), bits(one.process_block(x[clock:clock + S]))), step
        clock += S
        assert np.array_equal(many.save_state(), one.save_state()), step
    image, seen = many.save_state(), (many.info("tram_list_sets"), many.info("tram_list_gets"))
    v = windows_for(rng, across.size, 7, 0)
    out = np.zeros_like(v)
    lib, p = many._lib, lambda a: a.ctypes.data  # noqa: E731
    twice = across.copy()
    twice[-1] = twice[0]
    beyond = across.copy()
    beyond[3] = n
    for what, rc in (("an instance listed twice", lib.fxb_set_tram_list(many._h, 0, p(twice), twice.size, 0, 7, p(v), 0)),
                     ("an instance of N", lib.fxb_set_tram_list(many._h, 0, p(beyond), beyond.size, 0, 7, p(v), LOGICAL)),
                     ("an instance of N, get", lib.fxb_get_tram_list(many._h, 0, p(beyond), beyond.size, 0, 7, p(out), 0)),
                     ("one word past the slots", lib.fxb_set_tram_list(many._h, 0, p(across), across.size, 1, 7, p(v), 0)),
                     ("first = Z", lib.fxb_set_tram_list(many._h, 0, p(across), across.size, 7, 1, p(v), LOGICAL)),
                     ("n_words = Z + 1", lib.fxb_set_tram_list(many._h, 0, p(across), across.size, 0, 8, p(v), LOGICAL)),
                     ("which = 2", lib.fxb_set_tram_list(many._h, 2, p(across), across.size, 0, 7, p(v), 0)),
                     ("an unknown flag", lib.fxb_set_tram_list(many._h, 0, p(across), across.size, 0, 7, p(v), 8)),
                     ("broadcast on a get", lib.fxb_get_tram_list(many._h, 0, p(across), across.size, 0, 7, p(out), BROADCAST)),
                     ("null values", lib.fxb_set_tram_list(many._h, 0, p(across), across.size, 0, 7, None, 0)),
                     # n_words == 0 moves no word, but a list that is given is checked all the same ("once the other arguments have
                     # been checked"): tools/fuzz_voices.py seeds 3, 4 and 10 found these three accepted
                     ("an instance listed twice, n_words = 0", lib.fxb_set_tram_list(many._h, 1, p(twice), twice.size, 11, 0, p(v), 0)),
                     ("an instance of N, n_words = 0", lib.fxb_set_tram_list(many._h, 1, p(beyond), beyond.size, 0, 0, None, 0)),
                     ("an instance of N, n_words = 0, get", lib.fxb_get_tram_list(many._h, 0, p(beyond), beyond.size, 3, 0, p(out), 0))):
        assert rc == FX_E_ARG and many.last_error(), (what, rc)
        assert (many.info("tram_list_sets"), many.info("tram_list_gets")) == seen and not out.any(), what
    # ... and without a list there is nothing to check: no word moves, on any shard
    for what, rc in (("n_words = 0, no list, set", lib.fxb_set_tram_list(many._h, 0, None, 5, 7, 0, None, 0)),
                     ("n_words = 0, no list, get", lib.fxb_get_tram_list(many._h, 1, None, 5, 0, 0, None, 0)),
                     ("n_words = 0, a good list", lib.fxb_set_tram_list(many._h, 0, p(across), across.size, 7, 0, None, 0))):
        assert rc == 0, (what, rc, many.last_error())
        assert (many.info("tram_list_sets"), many.info("tram_list_gets")) == seen, what
    assert np.array_equal(many.save_state(), image) and np.array_equal(many.save_state(), one.save_state())
    for h in (many, one):
        h.close()
