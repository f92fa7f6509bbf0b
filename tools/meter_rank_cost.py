#!/usr/bin/env python3
"""What a meter rank costs (fxb_meter_rank_level, kernels fx_rank_hist / fx_rank_count / fx_rank_scan / fx_rank_emit) beside the way
to the same answer without it: fxb_meter_read_level of every row of every instance, then numpy on the host - the channel maximum,
numpy.argpartition for the k-th value, the ties at it taken by instance number, a sort of the k.

One process, one GPU, one handle: 524 288 instances, 2 channels, a pass-through program, meters and level meters on, one 32-sample
block of voices at random levels (a quarter of them silent, so that ties at the k-th value are the rule for the quietest).  The
two ways by turns, --repeats times each after --warmup rounds, on the caller's clock (us): median and p99, for k = 64 and 4 096,
the K quietest voices by envelope.  Both ways must give the same list, word for word: that is asserted before anything is timed.

    python tools/meter_rank_cost.py [--repeats 200] [--warmup 20] [--out profiles/meter_rank_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "fx8010-emulator-core_amd", "python"),):
    if p not in sys.path:
        sys.path.insert(0, p)

N, CHANNELS, S = 524288, 2, 32
KS = (64, 4096)
PASS_THROUGH = "input in 0\ninput in1 1\noutput out 0\noutput out1 1\nmacs out, in, 0, 0\nmacs out1, in1, 0, 0\nend"   # what goes in comes out
PASSES, CHUNK = 8, 256   # kMeterRankPasses, kMeterSelectChunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import fx8010_amd as A

    b = A.Batch(N, CHANNELS, 0)
    assert b.load_text(PASS_THROUGH), b.errors()
    assert b.meter_enable() == 0 and b.meter_set_level(0.999, 0.05) == 0
    rng = np.random.default_rng(N)
    level = (0.05 + 0.9 * rng.random((CHANNELS, N))).astype(np.float32)
    level[:, rng.random(N) < 0.25] = 0.0
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0).astype(np.float32)
    b.process_block(np.ascontiguousarray(sign[:, None, None] * level[None, :, :]))
    lib, h, vp = b._lib, b._h, C.c_void_p
    rows = {"level": np.empty((CHANNELS, N), dtype=np.float32), "quiet": np.empty((CHANNELS, N), dtype=np.uint32)}
    lst, val = np.empty(max(KS), dtype=np.int64), np.empty(max(KS), dtype=np.float64)
    host = {}

    def rank(k):
        return lib.fxb_meter_rank_level(h, A.LEVEL_ENVELOPE, k, C.c_double(-np.inf), 0, N, vp(lst.ctypes.data), vp(val.ctypes.data), 0)

    def read_and_sort(k):
        assert lib.fxb_meter_read_level(h, vp(rows["level"].ctypes.data), vp(rows["quiet"].ctypes.data), 0) == 0
        V = rows["level"].max(axis=0)
        part = np.argpartition(V, k - 1)[:k]
        kth = V[part].max()
        below = part[V[part] < kth]
        equal = np.nonzero(V == kth)[0][:k - below.size]   # the ties at the k-th value go to the smaller instance numbers
        take = np.concatenate([below, equal])
        host["list"] = take[np.lexsort((take, V[take]))]

    for k in KS:
        assert rank(k) == N
        read_and_sort(k)
        assert np.array_equal(lst[:k], host["list"]), "both ways give the same list (k = %d)" % k
    launches = b.info("meter_level_ranks")
    calls = {}
    for k in KS:
        calls["rank k=%d" % k] = lambda k=k: rank(k)
        calls["read + numpy k=%d" % k] = lambda k=k: read_and_sort(k)
    times = {name: [] for name in calls}
    for turn in range(args.warmup + args.repeats):
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            if turn >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e6)
    assert b.info("meter_level_ranks") == launches + len(KS) * (args.warmup + args.repeats)
    b.close()

    chunks = (N + CHUNK - 1) // CHUNK
    lines = ["%d instances, %d channels, a pass-through program, meters and level meters on (release 0.999, floor 0.05), one %d-sample block; %s" % (N, CHANNELS, S, time.strftime("%Y-%m-%d")),
             "the K quietest voices by envelope: fxb_meter_rank_level(FXB_LEVEL_ENVELOPE, k) over the whole range beside fxb_meter_read_level of both rows",
             "[%d][%d] + numpy (channel maximum, argpartition, the ties at the k-th value by instance number, a sort of the k); both give the same list." % (CHANNELS, N),
             "the caller's clock in us, by turns, %d repeats each after %d warm-up rounds: median / p99" % (args.repeats, args.warmup), "",
             "%-8s %21s %21s %12s %24s %24s" % ("k", "rank", "read + numpy", "rank / read", "rank: bytes over PCIe", "read: bytes over PCIe")]
    ok = True
    for k in KS:
        r, p = times["rank k=%d" % k], times["read + numpy k=%d" % k]
        mr, mp = statistics.median(r), statistics.median(p)
        ok = ok and mr < mp
        lines.append("%-8d %10.1f / %8.1f %10.1f / %8.1f %12.3f %24d %24d" % (k, mr, float(np.percentile(r, 99)), mp, float(np.percentile(p, 99)), mr / mp, 16 * k + 32, 8 * CHANNELS * N))
    lines += ["", "a rank is %d kernel launches behind one memset whatever N, k and the data are (%d of fx_rank_hist over %d chunks, fx_rank_count, fx_rank_scan," % (PASSES + 3, PASSES, chunks),
              "fx_rank_emit), one copy of 4 words + 16 k bytes and one wait.",
              "the condition - the rank call's median below the other way's at both k - %s." % ("holds" if ok else "DOES NOT HOLD")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
