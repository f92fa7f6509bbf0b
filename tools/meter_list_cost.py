#!/usr/bin/env python3
"""What a meter query by list costs (fxb_meter_select / fxb_meter_read_list / fxb_meter_reset_list, kernels fx_meter_count /
fx_meter_scan / fx_meter_emit / fx_meter_gather / fx_meter_zero) beside the only way there was before them: fxb_meter_read of the
row the question needs, and a scan of it on the host.

One process, one GPU.  Handles at 131 072, 458 752 and 2 097 152 instances, two channels, the smallest program (config1_shipped,
one MACS per channel), meters on; one 8-sample block whose levels put 64 voices above 0.85, 4 096 above 0.7 and every second
above 0.5, none above 0.95.  By turns, --repeats times each, median and p99 on the caller's clock (us):
  fxb_meter_select(FXB_METER_PEAK, t) with M = 0, 64, 4 096 and N / 2, the list taken with cap = N
  fxb_meter_read of the peak row alone, and the host scan of it (numpy: max over the channels, compare, nonzero) - apart
  fxb_meter_read_list of 64 voices               beside fxb_meter_read of the four rows
  fxb_meter_reset_list of 64 voices + fxb_sync   beside fxb_meter_read(NULL ..., reset = 1)
The kernels' means come from a child process under rocprofv3, in a run of its own with nothing else traced:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o meter -- python tools/meter_list_cost.py --child

    python tools/meter_list_cost.py [--repeats 200] [--out profiles/meter_list.txt] [--no-trace]
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

SIZES = (131072, 458752, 2097152)
CASES = ((0.95, "0"), (0.85, "64"), (0.7, "4096"), (0.5, "N/2"))   # thresholds on the peak, and the M they give
PEAK = 1
CHILD_REPEATS = 50


def handle(n):
    import numpy as np

    import fx8010_amd as A
    import fx8010_programs as progs

    text = progs.config1_shipped()
    assert text.endswith("macs out_l, 0, in_l, volume\nend")
    text = text[:-3].replace("macs out_l", "input in_r 1\noutput out_r 1\nmacs out_l", 1) + "macs out_r, 0, in_r, volume\nend"
    b = A.Batch(n, 2, 0)
    assert b.load_text(text), b.errors()
    assert b.meter_enable() == 0
    level = np.where(np.arange(n) % 2 == 0, 0.6, 0.3)
    loud = np.random.default_rng(n).permutation(n)[:4096]
    level[loud] = 0.8
    level[loud[:64]] = 0.9
    x = np.empty((8, 2, n), dtype=np.float32)
    x[:, 0, :] = level
    x[:, 1, :] = 0.5 * level
    x[1::2] *= -1
    b.process_block(x)
    want = {"0": 0, "64": 64, "4096": 4096, "N/2": int((level >= 0.5).sum())}
    return np, A, b, want


def child(args):
    """every size, every case CHILD_REPEATS times; then the list read and the list reset as often: the trace is read by position"""
    for n in SIZES:
        np, A, b, want = handle(n)
        buf = np.empty(n, dtype=np.int64)
        for t, name in CASES:
            for _ in range(CHILD_REPEATS):
                m = b._lib.fxb_meter_select(b._h, PEAK, C.c_double(t), 0, n, C.c_void_p(buf.ctypes.data), n, 0)
                assert m == want[name], (n, t, m)
        L = np.random.default_rng(1).permutation(n)[:64].astype(np.int64)
        for _ in range(CHILD_REPEATS):
            b.meter_read_list(L)
        for _ in range(CHILD_REPEATS):
            b.meter_reset_list(L)
            b.sync()
        b.close()
    print("CHILD ok", flush=True)


def wall(n, repeats):
    np, A, b, want = handle(n)
    lib, h = b._lib, b._h
    buf = np.empty(n, dtype=np.int64)
    row = np.empty((2, n), dtype=np.float32)
    full = {"energy": np.empty((2, n), dtype=np.float64), "peak": np.empty((2, n), dtype=np.float32), "full_scale": np.empty((2, n), dtype=np.uint32), "nonfinite": np.empty((2, n), dtype=np.uint32)}
    L = np.random.default_rng(1).permutation(n)[:64].astype(np.int64)
    out64 = [np.empty((2, 64), dtype=full[k].dtype) for k in ("energy", "peak", "full_scale", "nonfinite")]
    vp = C.c_void_p
    found = {}

    def select(t):
        return lib.fxb_meter_select(h, PEAK, C.c_double(t), 0, n, vp(buf.ctypes.data), n, 0)

    def read_row():
        return lib.fxb_meter_read(h, None, vp(row.ctypes.data), None, None, 0)

    def scan(t):
        found["host"] = np.nonzero(row.max(axis=0) >= np.float32(t))[0]

    calls = {}
    for t, name in CASES:
        calls["select M=" + name] = lambda t=t: select(t)
        calls["host scan M=" + name] = lambda t=t: scan(t)
    calls["read one row"] = read_row
    calls["read_list 64"] = lambda: lib.fxb_meter_read_list(h, vp(L.ctypes.data), 64, *[vp(o.ctypes.data) for o in out64], 0)
    calls["read four rows"] = lambda: lib.fxb_meter_read(h, *[vp(full[k].ctypes.data) for k in ("energy", "peak", "full_scale", "nonfinite")], 0)
    # the device's list against the host's, once, before anything is timed
    read_row()
    for t, name in CASES:
        m = select(t)
        scan(t)
        assert m == want[name] == found["host"].size and np.array_equal(buf[:m], found["host"]), (n, name, m)
    times = {k: [] for k in calls}
    for f in calls.values():
        f()
    for _ in range(repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e6)
    # the two resets last: they zero what the selects look at
    resets = {"reset_list 64 + sync": lambda: (lib.fxb_meter_reset_list(h, vp(L.ctypes.data), 64), lib.fxb_sync(h)), "read(NULL, reset=1)": lambda: lib.fxb_meter_read(h, None, None, None, None, 1)}
    for k, f in resets.items():
        f()
        times[k] = []
    for _ in range(repeats):
        for k, f in resets.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e6)
    b.close()
    return {k: (statistics.median(v), float(np.percentile(v, 99))) for k, v in times.items()}, want


def traced(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "meter", "--", sys.executable, os.path.abspath(__file__), "--child"]
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

    R = CHILD_REPEATS
    count, scan, emit, gather, zero = (times(w) for w in ("fx_meter_count", "fx_meter_scan", "fx_meter_emit", "fx_meter_gather", "fx_meter_zero"))
    # (M = 0 still emits: cap > 0; every select is three launches)
    expect = len(SIZES) * len(CASES) * R
    if (len(count), len(scan), len(emit)) != (expect,) * 3 or len(gather) != len(SIZES) * R or len(zero) != len(SIZES) * R:
        return ["expected %d launches of each select kernel and %d of the list kernels, the trace has %d / %d / %d and %d / %d" % (expect, len(SIZES) * R, len(count), len(scan), len(emit), len(gather), len(zero))]
    lines = ["kernel means in us from one rocprofv3 --kernel-trace --stats run of its own, %d launches each" % R,
             "%-10s %-6s %14s %14s %14s %10s" % ("instances", "M", "fx_meter_count", "fx_meter_scan", "fx_meter_emit", "sum")]
    mean = statistics.mean
    for i, n in enumerate(SIZES):
        for j, (_, name) in enumerate(CASES):
            at = (i * len(CASES) + j) * R
            c, s, e = mean(count[at:at + R]), mean(scan[at:at + R]), mean(emit[at:at + R])
            lines.append("%-10d %-6s %14.2f %14.2f %14.2f %10.2f" % (n, name, c, s, e, c + s + e))
    lines += ["", "%-10s %16s %14s" % ("instances", "fx_meter_gather", "fx_meter_zero")]
    for i, n in enumerate(SIZES):
        lines.append("%-10d %16.2f %14.2f" % (n, mean(gather[i * R:(i + 1) * R]), mean(zero[i * R:(i + 1) * R])))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=400.0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = ["two channels, the smallest program (config1_shipped, one MACS per channel), meters on, one 8-sample block; %s" % time.strftime("%Y-%m-%d"),
             "the caller's clock in us, by turns, %d repeats each: median / p99.  select: fxb_meter_select(FXB_METER_PEAK, t), cap = N." % args.repeats,
             "the way without it: fxb_meter_read of the peak row alone [2][N] + the host scan (numpy max over the channels, >=, nonzero)", ""]
    fmt = "%-10s %-6s %19s | %19s %19s %10s"
    lines.append(fmt % ("instances", "M", "select", "read one row", "host scan", "read+scan"))
    rest = []
    for n in SIZES:
        t, want = wall(n, args.repeats)
        pair = lambda v: "%8.1f / %8.1f" % v  # noqa: E731
        for _, name in CASES:
            lines.append(fmt % (n, name if name != "N/2" else str(want[name]), pair(t["select M=" + name]), pair(t["read one row"]), pair(t["host scan M=" + name]),
                                "%.1f" % (t["read one row"][0] + t["host scan M=" + name][0])))
        rest.append("%-10d %19s %19s | %21s %21s" % (n, pair(t["read_list 64"]), pair(t["read four rows"]), pair(t["reset_list 64 + sync"]), pair(t["read(NULL, reset=1)"])))
    lines += ["", "%-10s %19s %19s | %21s %21s" % ("instances", "read_list of 64", "read four rows", "reset_list 64 + sync", "read(NULL.., reset=1)")] + rest
    if not args.no_trace:
        lines += [""] + traced(args)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
