#!/usr/bin/env python3
"""What the level meters cost (fxb_meter_set_level, kernels fx_meter_level / fx_meter_target_level / fx_level_count / fx_level_emit)
beside what there was before them: fx_meter and fx_meter_target on the same blocks with the mode off, and fxb_meter_read_level of
the quiet row with a numpy compare on the host.

One process, one GPU.
  The kernels: a child process under rocprofv3, in a run of its own with nothing else traced -
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o level -- python tools/meter_level_cost.py --child
  config5 at 524 288 instances, meters on, bus blocks of 32 samples with K = 64 and both flags (the setting of
  profiles/meter_target.txt), --blocks of them (200) in each of four phases: fx_meter (the yardstick, in the same trace),
  fx_meter_level, fx_meter_target (group = 64, 32 samples, LOOP), fx_meter_target_level.
  The queries: handles at 131 072, 524 288 and 2 097 152 instances of a pass-through program, voices that fall silent at different
  samples of one 32-sample block; by turns, --repeats times each, median and p99 on the caller's clock (us):
      fxb_meter_select_level(FXB_LEVEL_QUIET, t) with M = 64 and 4 096, cap = N
      beside fxb_meter_read_level of the quiet row [1][N] + numpy (compare, nonzero)

    python tools/meter_level_cost.py [--repeats 200] [--blocks 200] [--out profiles/meter_level.txt] [--no-trace]
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
PASS_THROUGH = "input in 0\noutput out 0\nmacs out, in, 0, 0\nend"   # what goes in comes out: a silent input is a silent voice


def child(args):
    """four phases of args.blocks bus blocks: plain, level, target, target + level; the trace is read by kernel name"""
    import numpy as np

    import fx8010_amd as A
    import fx8010_programs as progs

    n, S, K = TRACE_N, TRACE_S, TRACE_K
    b = A.Batch(n, 1, 0)
    assert b.load_text(progs.config5()), b.errors()
    assert b.meter_enable() == 0
    xg = progs.stimulus(n // K, S).reshape(S, 1, n // K)
    rng = np.random.default_rng(1)
    for target, level in ((False, False), (False, True), (True, False), (True, True)):
        if target:
            assert b.meter_set_target((rng.standard_normal((S, 1, n // 64)) * 0.2).astype(np.float32), 64, loop=True) == 0
        if level:
            assert b.meter_set_level(np.float32(np.exp(-1.0 / (0.3 * 48000.0))), 1e-4) == 0
        else:
            assert b.meter_clear_level() == 0
        for _ in range(args.blocks):
            b.process_block_bus(xg, K, True, True)
        b.sync()
    assert b.info("meter_launches") == 2 * args.blocks and b.info("meter_target_launches") == 2 * args.blocks and b.info("meter_level_launches") == 2 * args.blocks
    b.close()
    print("CHILD ok", flush=True)


def traced(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "level", "--", sys.executable, os.path.abspath(__file__), "--child", "--blocks", str(args.blocks)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.timeout)
        if r.returncode != 0 or "CHILD ok" not in r.stdout:
            return ["the profiled run failed (%d): %s" % (r.returncode, r.stdout[-600:].replace("\n", " | "))]
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return ["rocprofv3 wrote no kernel trace"]
        rows = list(csv.DictReader(open(traces[0])))

    def times(word):
        return [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows if word in row["Kernel_Name"]]

    # (a kernel's name is a prefix of the next one's: the opening bracket of the argument list tells them apart)
    t = {k: times(k + "(") for k in ("fx_meter", "fx_meter_level", "fx_meter_target", "fx_meter_target_level")}
    B = args.blocks
    if any(len(v) != B for v in t.values()):
        return ["expected %d launches of each of the four meter kernels, the trace has %s" % (B, {k: len(v) for k, v in t.items()})]
    m = {k: statistics.mean(v) for k, v in t.items()}
    # bytes per column and block: S output words; the target words a wavefront fetches; the accumulators read and written
    y = TRACE_S * 4
    tw = TRACE_S * 4 / 64
    bytes_ = {"fx_meter": y + 2 * 20, "fx_meter_level": y + 2 * 28, "fx_meter_target": y + tw + 2 * 36, "fx_meter_target_level": y + tw + 2 * 44}
    out = ["kernel means in us from one rocprofv3 --kernel-trace --stats run of its own: config5, %d instances, bus blocks of %d samples, K = %d, both flags, %d blocks per phase" % (TRACE_N, TRACE_S, TRACE_K, B),
           "%-40s %10s %14s %18s" % ("kernel", "mean us", "x its sibling", "bytes per column")]
    for k, sibling in (("fx_meter", None), ("fx_meter_level", "fx_meter"), ("fx_meter_target", None), ("fx_meter_target_level", "fx_meter_target")):
        if sibling:
            out.append("%-40s %10.2f %14.2f %18.0f   (byte ratio %.2f)" % (k, m[k], m[k] / m[sibling], bytes_[k], bytes_[k] / bytes_[sibling]))
        else:
            out.append("%-40s %10.2f %14s %18.0f" % (k + (" (same trace)" if k == "fx_meter" else ", group = 64"), m[k], "1.00", bytes_[k]))
    return out


def wall(n, repeats):
    import numpy as np

    import fx8010_amd as A

    S = 32
    b = A.Batch(n, 1, 0)
    assert b.load_text(PASS_THROUGH), b.errors()
    assert b.meter_enable() == 0 and b.meter_set_level(0.999, 0.05) == 0
    # 64 voices silent for the whole block, 4 032 more for its second half, the others sound throughout
    rng = np.random.default_rng(n)
    x = (0.1 + 0.2 * rng.random((S, 1, n))).astype(np.float32)
    silent = rng.permutation(n)[:4096]
    x[:, 0, silent[:64]] = 0.0
    x[S // 2:, 0, silent[64:]] = 0.0
    b.process_block(x)
    lib, h, vp = b._lib, b._h, C.c_void_p
    quiet = np.empty((1, n), dtype=np.uint32)
    buf = np.empty(n, dtype=np.int64)
    assert lib.fxb_meter_read_level(h, None, vp(quiet.ctypes.data), 0) == 0
    cases = {"64": float(S), "4096": float(S // 2)}   # quiet for at least t samples: M voices
    host = {}

    def scan(t):
        host["list"] = np.nonzero(quiet[0] >= t)[0]

    calls = {"read quiet row": lambda: lib.fxb_meter_read_level(h, None, vp(quiet.ctypes.data), 0)}
    for name, t in cases.items():
        calls["select M=" + name] = lambda t=t: lib.fxb_meter_select_level(h, 1, C.c_double(t), 0, n, vp(buf.ctypes.data), n, 0)
        calls["host scan M=" + name] = lambda t=t: scan(t)
    # the device's answers against the host's, once, before anything is timed
    for name in cases:
        m = calls["select M=" + name]()
        scan(cases[name])
        assert m == int(name) and np.array_equal(buf[:m], host["list"]), (n, name, m)
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
    lines = ["one channel, a pass-through program, meters and level meters on (release 0.999, floor 0.05), one 32-sample block; %s" % time.strftime("%Y-%m-%d"),
             "the caller's clock in us, by turns, %d repeats each: median / p99.  select: fxb_meter_select_level(FXB_LEVEL_QUIET, t), cap = N." % args.repeats,
             "the way without it: fxb_meter_read_level of the quiet row [1][N] + numpy (compare, nonzero)", ""]
    fmt = "%-10s %19s %19s | %19s %19s %19s %10s"
    lines.append(fmt % ("instances", "select M=64", "select M=4096", "read quiet row", "host scan M=64", "host scan M=4096", "read+scan"))
    pair = lambda v: "%8.1f / %8.1f" % v  # noqa: E731
    for n in SIZES:
        t = wall(n, args.repeats)
        lines.append(fmt % (n, pair(t["select M=64"]), pair(t["select M=4096"]), pair(t["read quiet row"]), pair(t["host scan M=64"]), pair(t["host scan M=4096"]),
                            "%.1f" % (t["read quiet row"][0] + t["host scan M=4096"][0])))
    if not args.no_trace:
        lines += [""] + traced(args)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
