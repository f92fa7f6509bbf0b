#!/usr/bin/env python3
"""What the tone meters cost (fxb_meter_set_tones, kernels fx_meter_tone<K> / fx_tone_count / fx_tone_emit / fx_rank_*) beside
what there was before them: fx_meter on the same blocks, and fxb_meter_read_tones of the power with numpy on the host.

One process, one GPU.
  The kernels: a child process under rocprofv3, in a run of its own with nothing else traced -
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tone -- python tools/meter_tone_cost.py --child
  config5 at 524 288 instances, meters on, bus blocks of 32 samples with K = 64 and both flags (the setting of
  profiles/meter_level.txt), --blocks of them (200) in each of three phases: 1, 4 and 8 tones.  fx_meter runs in front of every
  tone launch: the yardstick, in the same trace.  The byte count predicts (128 + 32 tones) / 168 of fx_meter's time: a column
  reads 32 output words (128 bytes) and reads and writes 16 bytes per tone, fx_meter 128 + 2 x 20.
  The queries: handles at 131 072, 524 288 and 2 097 152 instances of a pass-through program, four tones, one 64-sample block
  in which 64 voices (and 4 096) carry an on-bin sine; by turns, --repeats times each, median and p99 on the caller's clock (us):
      fxb_meter_select_tone(0, t) with M = 64 and 4 096, cap = N;  fxb_meter_rank_tone(0, 64, LARGEST)
      beside fxb_meter_read_tones of the power [4][1][N] + numpy (compare, nonzero / argpartition)

    python tools/meter_tone_cost.py [--repeats 200] [--blocks 200] [--out profiles/meter_tone.txt] [--no-trace]
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
TONES = (1, 4, 8)
PASS_THROUGH = "input in 0\noutput out 0\nmacs out, in, 0, 0\nend"


def coeff(k, n):
    import math
    return 2.0 * math.cos(2.0 * math.pi * k / n)


def child(args):
    """a phase of args.blocks bus blocks per tone count; the trace is read by kernel name"""
    import fx8010_amd as A
    import fx8010_programs as progs

    n, S, K = TRACE_N, TRACE_S, TRACE_K
    b = A.Batch(n, 1, 0)
    assert b.load_text(progs.config5()), b.errors()
    assert b.meter_enable() == 0
    xg = progs.stimulus(n // K, S).reshape(S, 1, n // K)
    for tones in TONES:
        assert b.meter_set_tones([coeff(k + 1, 32) for k in range(tones)]) == 0
        for _ in range(args.blocks):
            b.process_block_bus(xg, K, True, True)
        b.sync()
    assert b.info("meter_launches") == len(TONES) * args.blocks == b.info("meter_tone_launches")
    b.close()
    print("CHILD ok", flush=True)


def traced(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "tone", "--", sys.executable, os.path.abspath(__file__), "--child", "--blocks", str(args.blocks)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.timeout)
        if r.returncode != 0 or "CHILD ok" not in r.stdout:
            return ["the profiled run failed (%d): %s" % (r.returncode, r.stdout[-600:].replace("\n", " | "))]
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return ["rocprofv3 wrote no kernel trace"]
        rows = list(csv.DictReader(open(traces[0])))

    def times(word):
        return [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows if word in row["Kernel_Name"]]

    B = args.blocks
    meter = times("fx_meter(")
    tone = {k: times("fx_meter_tone<%d>" % k) for k in TONES}
    if len(meter) != len(TONES) * B or any(len(v) != B for v in tone.values()):
        names = sorted({row["Kernel_Name"][:60] for row in rows if "fx_meter" in row["Kernel_Name"]})
        return ["expected %d launches of fx_meter and %d of each tone kernel, the trace has %d and %s; names: %s" % (len(TONES) * B, B, len(meter), {k: len(v) for k, v in tone.items()}, names)]
    m = statistics.mean(meter)
    out = ["kernel means in us from one rocprofv3 --kernel-trace --stats run of its own: config5, %d instances, bus blocks of %d samples, K = %d, both flags, %d blocks per phase" % (TRACE_N, TRACE_S, TRACE_K, B),
           "%-32s %10s %12s %18s %12s" % ("kernel", "mean us", "x fx_meter", "bytes per column", "byte ratio"),
           "%-32s %10.2f %12s %18d %12s" % ("fx_meter (same trace)", m, "1.00", TRACE_S * 4 + 40, "1.00")]
    for k in TONES:
        t = statistics.mean(tone[k])
        out.append("%-32s %10.2f %12.2f %18d %12.2f" % ("fx_meter_tone<%d>" % k, t, t / m, TRACE_S * 4 + 32 * k, (TRACE_S * 4 + 32 * k) / (TRACE_S * 4 + 40.0)))
    return out


def wall(n, repeats):
    import numpy as np

    import fx8010_amd as A

    S, bins = 64, (4, 8, 12, 16)
    coeffs = [coeff(k, S) for k in bins]
    b = A.Batch(n, 1, 0)
    assert b.load_text(PASS_THROUGH), b.errors()
    assert b.meter_enable() == 0 and b.meter_set_tones(coeffs) == 0
    # 64 voices carry bin 4 at amplitude 0.5, 4 032 more at 0.25; every other voice carries bin 8
    rng = np.random.default_rng(n)
    t = np.arange(S, dtype=np.float64)[:, None]
    own = rng.permutation(n)[:4096]
    amp = np.full(n, 0.3)
    k = np.full(n, 8.0)
    k[own] = 4.0
    amp[own] = 0.25
    amp[own[:64]] = 0.5
    x = (amp[None, :] * np.sin(2 * np.pi * k[None, :] * t / S + 0.3)).astype(np.float32).reshape(S, 1, n)
    b.process_block(x)
    lib, h, vp = b._lib, b._h, C.c_void_p
    power = np.empty((4, 1, n), dtype=np.float64)
    buf = np.empty(n, dtype=np.int64)
    val = np.empty(64, dtype=np.float64)
    assert lib.fxb_meter_read_tones(h, None, None, vp(power.ctypes.data), 0) == 0
    cases = {"64": 200.0, "4096": 32.0}   # (0.5 * 32)^2 = 256, (0.25 * 32)^2 = 64
    host = {}

    def scan(thr):
        host["list"] = np.nonzero(power[0, 0] >= thr)[0]

    def top():
        v = power[0, 0]
        part = np.argpartition(-v, 64)[:64]
        host["top"] = part[np.lexsort((part, -v[part]))]

    calls = {"read power": lambda: lib.fxb_meter_read_tones(h, None, None, vp(power.ctypes.data), 0)}
    for name, thr in cases.items():
        calls["select M=" + name] = lambda thr=thr: lib.fxb_meter_select_tone(h, 0, C.c_double(thr), 0, n, vp(buf.ctypes.data), n, 0)
        calls["host scan M=" + name] = lambda thr=thr: scan(thr)
    calls["rank k=64"] = lambda: lib.fxb_meter_rank_tone(h, 0, 64, C.c_double(-np.inf), 0, n, vp(buf.ctypes.data), vp(val.ctypes.data), 2)
    calls["host top 64"] = top
    # the device's answers against the host's, once, before anything is timed
    for name in cases:
        m = calls["select M=" + name]()
        scan(cases[name])
        assert m == int(name) and np.array_equal(buf[:m], host["list"]), (n, name, m)
    assert calls["rank k=64"]() == n and set(buf[:64].tolist()) == set(own[:64].tolist())
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
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = ["one channel, a pass-through program, meters and four tone meters on (bins 4, 8, 12, 16 of 64), one 64-sample block; %s" % time.strftime("%Y-%m-%d"),
             "the caller's clock in us, by turns, %d repeats each: median / p99.  select: fxb_meter_select_tone(0, t), cap = N; rank: fxb_meter_rank_tone(0, 64, LARGEST)." % args.repeats,
             "the way without them: fxb_meter_read_tones of the power [4][1][N] + numpy (compare, nonzero; argpartition and a sort of 64)", ""]
    fmt = "%-10s %19s %19s %19s | %21s %19s %19s %19s"
    lines.append(fmt % ("instances", "select M=64", "select M=4096", "rank k=64", "read power", "host scan M=64", "host scan M=4096", "host top 64"))
    pair = lambda v: "%8.1f / %8.1f" % v  # noqa: E731
    for n in args.sizes:
        t = wall(n, args.repeats)
        lines.append(fmt % (n, pair(t["select M=64"]), pair(t["select M=4096"]), pair(t["rank k=64"]), pair(t["read power"]), pair(t["host scan M=64"]), pair(t["host scan M=4096"]), pair(t["host top 64"])))
    if not args.no_trace:
        lines += [""] + traced(args)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
