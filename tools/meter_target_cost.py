#!/usr/bin/env python3
"""What the target meters cost (fxb_meter_set_target, kernels fx_meter_target / fx_match_count / fx_match_emit / fx_meter_best)
beside what there was before them: fx_meter on the same blocks with no target set, and fxb_meter_read_match of both rows with a
numpy argmin over the groups on the host.

One process, one GPU.
  The kernels: a child process under rocprofv3, in a run of its own with nothing else traced -
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o target -- python tools/meter_target_cost.py --child
  config5 at 524 288 instances, meters on, bus blocks of 32 samples with K = 64 and both flags (the shape of
  profiles/bus_meter_kernel_stats.csv), --blocks of them (200) in each of three phases: no target (fx_meter: the yardstick, in
  the same trace), a target with group = 64, a target with group = 1 (both 32 samples long, with LOOP).
  The queries: handles at 131 072, 524 288 and 2 097 152 instances of the smallest program, one 32-sample block against a
  target with group = 64; by turns, --repeats times each, median and p99 on the caller's clock (us):
      fxb_meter_best(FXB_MATCH_ERROR, 64)                     beside fxb_meter_read_match of both rows + numpy (reshape, argmin)
      fxb_meter_select_match(FXB_MATCH_ERROR, t, BELOW) with M = 64 and 4 096, cap = N

    python tools/meter_target_cost.py [--repeats 200] [--blocks 200] [--out profiles/meter_target.txt] [--no-trace]
"""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "fx8010-emulator-core_amd", "python"),):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = (131072, 524288, 2097152)
TRACE_N, TRACE_S, TRACE_K = 524288, 32, 64


def child(args):
    """three phases of args.blocks bus blocks: no target, group = 64, group = 1; the trace is read by kernel name"""
    import numpy as np

    import fx8010_amd as A
    import fx8010_programs as progs

    n, S, K = TRACE_N, TRACE_S, TRACE_K
    b = A.Batch(n, 1, 0)
    assert b.load_text(progs.config5()), b.errors()
    assert b.meter_enable() == 0
    xg = progs.stimulus(n // K, S).reshape(S, 1, n // K)
    rng = np.random.default_rng(1)
    for group in (None, 64, 1):
        if group:
            assert b.meter_set_target((rng.standard_normal((S, 1, n // group)) * 0.2).astype(np.float32), group, loop=True) == 0
        for _ in range(args.blocks):
            b.process_block_bus(xg, K, True, True)
        b.sync()
    assert b.info("meter_launches") == args.blocks and b.info("meter_target_launches") == 2 * args.blocks
    b.close()
    print("CHILD ok", flush=True)


def traced(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "target", "--", sys.executable, os.path.abspath(__file__), "--child", "--blocks", str(args.blocks)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.timeout)
        if r.returncode != 0 or "CHILD ok" not in r.stdout:
            return ["the profiled run failed (%d): %s" % (r.returncode, r.stdout[-600:].replace("\n", " | "))]
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return ["rocprofv3 wrote no kernel trace"]
        rows = list(csv.DictReader(open(traces[0])))
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))

    def times(word):
        return [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows if word in row["Kernel_Name"]]

    # (the plain meter kernel's name is a prefix of the other's: fx_meter(MeterArgs) against fx_meter_target(MeterTargetArgs))
    target = times("fx_meter_target(")
    plain = times("fx_meter(")
    B = args.blocks
    if len(plain) != B or len(target) != 2 * B:
        return ["expected %d launches of fx_meter and %d of fx_meter_target, the trace has %d and %d" % (B, 2 * B, len(plain), len(target))]
    mean = statistics.mean
    m0, m64, m1 = mean(plain), mean(target[:B]), mean(target[B:])
    # bytes per column and block: S output words; the target words a wavefront fetches; the accumulators read and written
    y = TRACE_S * 4
    b0, b64, b1 = y + 2 * 20, y + TRACE_S * 4 / 64 + 2 * 36, y + TRACE_S * 4 + 2 * 36
    return ["kernel means in us from one rocprofv3 --kernel-trace --stats run of its own: config5, %d instances, bus blocks of %d samples, K = %d, both flags, %d blocks per phase" % (TRACE_N, TRACE_S, TRACE_K, B),
            "%-34s %10s %12s %18s" % ("kernel", "mean us", "x fx_meter", "bytes per column"),
            "%-34s %10.2f %12s %18.0f" % ("fx_meter (no target, same trace)", m0, "1.00", b0),
            "%-34s %10.2f %12.2f %18.0f   (byte ratio %.2f)" % ("fx_meter_target, group = 64", m64, m64 / m0, b64, b64 / b0),
            "%-34s %10.2f %12.2f %18.0f   (byte ratio %.2f)" % ("fx_meter_target, group = 1", m1, m1 / m0, b1, b1 / b0)]


def wall(n, repeats):
    import numpy as np

    import fx8010_amd as A
    import fx8010_programs as progs

    S, K = 32, 64
    b = A.Batch(n, 1, 0)
    assert b.load_text(progs.config1_shipped()), b.errors()
    assert b.meter_enable() == 0
    rng = np.random.default_rng(n)
    assert b.meter_set_target((rng.standard_normal((S, 1, n // K)) * 0.2).astype(np.float32), K) == 0
    # per-instance levels: the error of every instance differs
    x = (rng.standard_normal((S, 1, n)) * 0.2).astype(np.float32)
    b.process_block(x)
    lib, h, vp = b._lib, b._h, C.c_void_p
    G = n // K
    err, cross = np.empty((1, n)), np.empty((1, n))
    winner, value = np.empty(G, dtype=np.int64), np.empty(G)
    buf = np.empty(n, dtype=np.int64)
    assert lib.fxb_meter_read_match(h, vp(err.ctypes.data), vp(cross.ctypes.data), 0) == 0
    order = np.sort(err[0])
    cases = {"64": float(order[64]), "4096": float(order[4096])}   # BELOW: strictly smaller - M of them (no two alike here)
    host = {}

    def scan():
        v = err[0].reshape(G, K)
        k = v.argmin(axis=1)
        host["winner"], host["value"] = np.arange(G) * K + k, v[np.arange(G), k]

    calls = {"best": lambda: lib.fxb_meter_best(h, 0, K, vp(winner.ctypes.data), vp(value.ctypes.data), 0),
             "read both rows": lambda: lib.fxb_meter_read_match(h, vp(err.ctypes.data), vp(cross.ctypes.data), 0), "host argmin": scan}
    for name, t in cases.items():
        calls["select M=" + name] = lambda t=t: lib.fxb_meter_select_match(h, 0, C.c_double(t), 0, n, vp(buf.ctypes.data), n, 1)
    # the device's answers against the host's, once, before anything is timed
    assert calls["best"]() == 0
    scan()
    assert np.array_equal(winner, host["winner"]) and np.array_equal(value.view(np.uint64), host["value"].view(np.uint64)), n
    for name in cases:
        m = calls["select M=" + name]()
        assert m == int(name) and np.array_equal(buf[:m], np.nonzero(err[0] < cases[name])[0]), (n, name, m)
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e6)
    b.close()
    return {k: (statistics.median(v), float(np.percentile(v, 99))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=400.0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = ["one channel, the smallest program (config1_shipped), meters on, a target with group = 64, one 32-sample block; %s" % time.strftime("%Y-%m-%d"),
             "the caller's clock in us, by turns, %d repeats each: median / p99.  best: fxb_meter_best(FXB_MATCH_ERROR, 64); select: fxb_meter_select_match(FXB_MATCH_ERROR, t, BELOW), cap = N." % args.repeats,
             "the way without them: fxb_meter_read_match of both rows [1][N] each + numpy (reshape to [G][64], argmin, take)", ""]
    fmt = "%-10s %19s | %19s %19s %10s | %19s %19s"
    lines.append(fmt % ("instances", "best", "read both rows", "host argmin", "read+scan", "select M=64", "select M=4096"))
    pair = lambda v: "%8.1f / %8.1f" % v  # noqa: E731
    for n in SIZES:
        t = wall(n, args.repeats)
        lines.append(fmt % (n, pair(t["best"]), pair(t["read both rows"]), pair(t["host argmin"]), "%.1f" % (t["read both rows"][0] + t["host argmin"][0]), pair(t["select M=64"]), pair(t["select M=4096"])))
    if not args.no_trace:
        lines += [""] + traced(args)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
