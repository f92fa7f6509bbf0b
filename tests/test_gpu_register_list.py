"""Register calls by list on the GPU: fxb_set_registers_list / fxb_get_registers_list (kernels fx_reg_scatter / fx_reg_gather in
csrc/fx_registers.hip).  The kernels move words, so the bar everywhere is equality of 32-bit patterns: against a twin handle that
receives the same writes through fxb_set_register_i / fxb_set_register_array (the definition of the set), against oracle objects
that get setRegisterValue on the listed instances, for blocks queued on other streams around the sets, for the quiet loop's head
check and for a handle of two shards.  The host's bookkeeping without a GPU is tests/test_register_list_stub.py."""
import numpy as np
import pytest

import fx8010_programs as progs
from pyoracle import Oracle
from test_gpu_bus import bits, group_input, handles, program, register_names
from test_gpu_bus_gain import kernel_tier, right_tier  # noqa: F401  (the fixture)
from test_gpu_instances import cutoffs, equals_oracle, handle, state_registers
from test_gpu_quiet_states import WATCH5, config5_pair, quiet5

pytestmark = pytest.mark.gpu

# +0, -0, the smallest denormal, the largest (negative), +-1e30, a quiet NaN with a payload
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7149f2ca, 0xf149f2ca, 0x7fc12345], dtype=np.uint32).view(np.float32)


def a_list(rng, N, n):
    """n distinct instances of 0..N-1 in a shuffled order, 0 and N - 1 among them (n == 1: N - 1; n >= N: all of them)"""
    if n >= N:
        return rng.permutation(N).astype(np.int64)
    if n == 1:
        return np.array([N - 1], dtype=np.int64)
    return rng.permutation(np.concatenate([[0, N - 1], rng.permutation(np.arange(1, N - 1))[:n - 2]])).astype(np.int64)


def values_for(rng, n_keys, count, step):
    """[n_keys, count] filter settings in (0, 1) with the specials walking through the columns from one set to the next"""
    v = rng.uniform(0.02, 0.98, (n_keys, count)).astype(np.float32)
    for k in range(n_keys):
        for j, s in enumerate(SPECIALS):
            v[k, (step + k + j * 3) % count] = s
    return v


def twin_write(t, keys, L, v):
    """the same writes through the calls the definition names: word by word for the short lists, whole rows for the others"""
    for k, key in enumerate(keys):
        if L.size <= 2:
            for i, inst in enumerate(L):
                assert t.set_register_i(key, int(inst), float(v[k, i])) == 0   # (a Python float carries a quiet NaN's payload)
        else:
            row = t.get_register_array(key)
            row[L] = v[k]
            assert t.set_register_array(key, row) == 0


def same_get(b, t, keys, L, what):
    """get_registers_list against the rows of both handles, and against get_register_i of both on a few entries of every key"""
    got = b.get_registers_list(keys, L)
    assert got.shape == (len(keys), L.size)
    few = sorted({0, L.size // 2, L.size - 1})
    for k, key in enumerate(keys):
        assert np.array_equal(bits(got[k]), bits(t.get_register_array(key))[L]) and np.array_equal(bits(got[k]), bits(b.get_register_array(key))[L]), (what, key)
        for i in few:
            assert bits(got[k, i]) == b.get_register_bits_i(key, int(L[i])) == t.get_register_bits_i(key, int(L[i])), (what, key, i)


GRID = [("default", 5, 1), ("default", 65, 2), ("default", 200, 1), ("default", 777, 2), ("hip", 777, 2), ("asm", 777, 2)]


@pytest.mark.parametrize("kernel_tier,N,channels", GRID, indirect=["kernel_tier"], ids=["%s-N%d-C%d" % g for g in GRID])
def test_list_sets_equal_the_twin_bit_for_bit(gpu, kernel_tier, N, channels):
    """blocks of 33, 1 and 2 samples with a list set in front of each: lists of 1, 64, 65, 257 and N entries (0 and N - 1 among
    them from two entries on) with one key, two keys and every register of the program; the twin gets the same writes through
    set_register_i / set_register_array; get after every set, outputs and the whole state image after every block"""
    rng = np.random.default_rng(9000 * N + channels)
    text = program("config3", channels)
    names = register_names(gpu, text, channels)
    b, t = handles(gpu, text, N, channels, 2)
    key_sets = (["cutoff"], ["fb", "s7"], names)
    sizes = (1, 64, 65, 257, N)
    clock, sets = 0, 0
    for step in range(15):
        S, n, keys = (33, 1, 2)[step % 3], min(sizes[step % 5], N), key_sets[(step + step // 3) % 3]
        what = "step %d: S %d, %d entries, %d keys" % (step, S, n, len(keys))
        L = a_list(rng, N, n)
        v = values_for(rng, len(keys), L.size, step)
        assert b.set_registers_list(keys, L, v) == 0, b.last_error()
        twin_write(t, keys, L, v)
        sets += 1
        assert b.info("register_list_sets") == sets, what
        same_get(b, t, keys, L, what)
        x = group_input(N, S, channels, clock)
        clock += S
        assert np.array_equal(bits(b.process_block(x)), bits(t.process_block(x))), what
        assert np.array_equal(b.save_state(), t.save_state()), what
    assert right_tier(b, kernel_tier) and right_tier(t, kernel_tier), b.tier_note()
    assert b.ood_flags() == t.ood_flags() and b.info("register_list_gets") == 15
    same_get(b, t, names, np.arange(N, dtype=np.int64), "every word at the end")
    for h in (b, t):
        h.close()


def test_list_set_against_the_oracle(gpu, monkeypatch):
    """config3, N = 130, the translated tier: instances on both sides of every wavefront boundary get a new cutoff and feedback by
    list between two runs; each continues exactly like a reference object that got setRegisterValue at that point, and an instance
    the list did not name like one that did not"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    text = progs.config3()
    N, S1, S2 = 130, 1037, 500
    cut = cutoffs(N)
    b = handle(gpu, text, N, "cutoff", cut)
    x1, x2 = progs.stimulus(N, S1), progs.stimulus(N, S2, first_sample=S1, seed=99)
    b.process_block(x1)
    assert b.info("kernel") >= 9, b.tier_note()
    L = np.array([129, 0, 64, 63, 127, 128], dtype=np.int64)
    v = np.array([[0.9, 0.07, 0.5, 0.33, 0.61, 0.2], [0.1, 0.7, -0.0, 0.45, 0.25, 0.6]], dtype=np.float32)
    assert b.set_registers_list(["cutoff", "fb"], L, v) == 0
    y2 = b.process_block(x2)
    names = state_registers(text)
    written = {int(i): (float(v[0, k]), float(v[1, k])) for k, i in enumerate(L)}
    for inst in list(written) + [1, 65]:
        o = Oracle(1)
        assert o.load_text(text), o.errors()
        o.set_register("cutoff", float(cut[inst]))
        o.process_block(np.ascontiguousarray(x1[:, inst]))
        if inst in written:
            o.set_register("cutoff", written[inst][0])
            o.set_register("fb", written[inst][1])
        ref = o.process_block(np.ascontiguousarray(x2[:, inst]))
        equals_oracle(b, inst, o, names, y2[:, inst], ref, [(0, 1000)])
    assert b.info("register_list_sets") == 1 and b.ood_flags() == 0
    b.close()


def test_list_sets_between_blocks_on_other_streams(gpu):
    """a block on stream A, a list set, a block on stream B, another list set, a block on the handle's own stream, fxb_sync once:
    each block has the values it was queued with.  S = 4096 at N = 777: the first block is still running when the set is queued"""
    import torch

    text = progs.config3()
    N, S = 777, 4096
    rng = np.random.default_rng(97)
    b, t = handles(gpu, text, N, 1, 2)
    keys = ["cutoff", "fb"]
    first = rng.uniform(0.05, 0.95, (2, N)).astype(np.float32)
    for h in (b, t):   # (rows and code for per-instance values of both registers exist before anything is queued)
        for k, key in enumerate(keys):
            assert h.set_register_array(key, first[k]) == 0
    warm = group_input(N, 8, 1, 0)
    assert np.array_equal(bits(b.process_block(warm)), bits(t.process_block(warm)))
    blocks = [group_input(N, S, 1, 8 + k * S) for k in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = [torch.from_numpy(x).to("cuda") for x in blocks]
    d_out = [torch.full((S, 1, N), -7.0, dtype=torch.float32, device="cuda") for _ in blocks]
    torch.cuda.synchronize()
    L1, L2 = a_list(rng, N, 257), a_list(rng, N, 65)
    v1, v2 = values_for(rng, 2, L1.size, 0), values_for(rng, 2, L2.size, 5)
    assert b.process_block_dev_pitched(d_in[0], d_out[0], S, stream=streams[0].cuda_stream) == 0
    assert b.set_registers_list(keys, L1, v1) == 0
    assert b.process_block_dev_pitched(d_in[1], d_out[1], S, stream=streams[1].cuda_stream) == 0
    assert b.set_registers_list(keys, L2, v2) == 0
    assert b.process_block_dev_pitched(d_in[2], d_out[2], S) == 0
    assert b.sync() == 0
    want = [t.process_block(blocks[0])]
    twin_write(t, keys, L1, v1)
    want.append(t.process_block(blocks[1]))
    twin_write(t, keys, L2, v2)
    want.append(t.process_block(blocks[2]))
    for k in range(3):
        assert np.array_equal(bits(d_out[k].cpu().numpy()), bits(want[k])), "block %d: the register values it was queued with" % k
    assert not np.array_equal(bits(want[0][-1]), bits(t.process_block(blocks[0])[-1])), "the values matter to the words compared"
    same_get(b, t, keys, np.arange(N, dtype=np.int64), "after the streams")
    assert b.info("register_list_sets") == 2
    for h in (b, t):
        h.close()


def test_list_set_that_sends_wavefronts_out_of_the_quiet_loop(gpu, monkeypatch):
    """config5 with its quiet loop: one list set puts two checked rows of three lanes in three wavefronts above their bound (0.25)
    and inside [-1, 1]; the same writes go to the oracles; the three wavefronts enter the loop and leave it at sample 0"""
    for env in ("FX_KERNEL", "FX_INST_PER_LANE", "FX_STAGES"):
        monkeypatch.delenv(env, raising=False)
    b, w = config5_pair(gpu)
    _, left = w.run(b, quiet5(24, watched=WATCH5, level=0.2), "before the set")
    assert b.info("xlate_quiet") == 1 and left == 0 and b.info("xlate_quiet_left") == 0
    lanes, regs = np.array([128, 63, 70], dtype=np.int64), ["y3", "y7"]
    v = np.array([[0.5, -0.75, 0.3], [-0.5, 0.26, 1.0]], dtype=np.float32)
    assert b.set_registers_list(regs, lanes, v) == 0
    for k, r in enumerate(regs):
        for i, lane in enumerate(lanes):
            w.set(int(lane), r, float(v[k, i]))
    _, left = w.run(b, quiet5(24, seed=1, watched=WATCH5, level=0.2), "after the set")
    assert b.info("xlate_quiet") == 1
    assert left == 3 and b.info("xlate_quiet_left") == 3, (left, b.info("xlate_quiet_left"))
    w.state(b, "after the set")
    _, left = w.run(b, quiet5(24, seed=2, watched=WATCH5, level=0.2), "the block after")
    assert b.info("xlate_quiet_left") == left
    w.state(b, "the block after")
    b.close()


def test_two_shards_on_one_gpu_equal_the_single_handle(gpu):
    """devices = [0, 0]: a list wholly inside the last shard, lists on both, every register; outputs, gets and the state image"""
    N, ch, S = 64 * 10 + 17, 2, 33
    text = program("config3", ch)
    names = register_names(gpu, text, ch)
    rng = np.random.default_rng(N)
    (one,) = handles(gpu, text, N, ch, 1)
    many = gpu.Batch(N, ch, devices=[0, 0])
    assert many.load_text(text), many.errors()
    assert many.set_register_array("cutoff", cutoffs(N)) == 0
    (_, _, _), (_, first, count) = many.shards()
    inside = (first + rng.permutation(count)[:65]).astype(np.int64)
    sets = 0
    for step, (keys, L) in enumerate(((["cutoff"], inside), (["fb", "s7"], a_list(rng, N, 130)), (names, a_list(rng, N, N)), (["cutoff", "fb"], inside[:1]))):
        v = values_for(rng, len(keys), L.size, step)
        before = many.info("register_list_sets")
        for h in (many, one):
            assert h.set_registers_list(keys, L, v) == 0, h.last_error()
        launched = many.info("register_list_sets") - before
        assert launched == (1 if L is inside or L.size == 1 else 2), "a shard without an entry launches nothing"
        sets += 1
        same_get(many, one, keys, L, "step %d" % step)
        x = group_input(N, S, ch, step * S)
        assert np.array_equal(bits(many.process_block(x)), bits(one.process_block(x))), step
        assert np.array_equal(many.save_state(), one.save_state()), step
    assert one.info("register_list_sets") == sets
    for h in (many, one):
        h.close()
