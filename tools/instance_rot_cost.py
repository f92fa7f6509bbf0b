#!/usr/bin/env python3
"""The kernel time of fx_inst_scatter_rot beside fx_inst_scatter: 30 config5 records into one list of one handle, by the plain load
(fx_inst_scatter), by the rotated load at the same positions (rotation 0) and, 1 025 samples later, by the rotated load at rotation
4 100 (config5 makes four delay writes per sample on its 8 192-slot line) - the plain load is refused there.

Kernel times cannot be taken from outside (the calls run on the handle's own stream), so the work runs in a child process under
rocprofv3, in a run of its own with nothing else traced:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rot -- python tools/instance_rot_cost.py --child

and this program reads DIR/**/rot_kernel_trace.csv: the launches of each kernel in order, the first --repeats of the rotating one
at rotation 0, the rest at 4 100; median, minimum and maximum of End_Timestamp - Start_Timestamp.

    python tools/instance_rot_cost.py [--instances 4096] [--repeats 20] [--out profiles/instance_rot.txt]
"""
import argparse
import csv
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

RECORDS, WARM, LATER = 30, 64, 1025


def child(args):
    import numpy as np

    import fx8010_amd as A
    import fx8010_programs as progs

    n = args.instances
    b = A.Batch(n, 1, 0)
    assert b.load_text(progs.config5()), b.errors()
    x = progs.stimulus(n, WARM + LATER)
    b.process_block(np.ascontiguousarray(x[:WARM]))
    src, dst = np.arange(RECORDS) * 7, n // 2 + np.arange(RECORDS) * 5
    image = b.save_instances(src)
    saved = b.get_cursors_i(int(src[0]))
    for _ in range(args.repeats):
        assert b.load_instances(dst, image) == 0
    for _ in range(args.repeats):
        assert b.load_instances_rotated(dst, image) == 0
    for at in range(WARM, WARM + LATER, 256):
        b.process_block(np.ascontiguousarray(x[at:min(at + 256, WARM + LATER)]))
    held = b.get_cursors_i(int(dst[0]))
    for _ in range(args.repeats):
        assert b.load_instances_rotated(dst, image) == 0
    assert (b.info("instance_scatters"), b.info("instance_rotations")) == (args.repeats, 2 * args.repeats)
    print("CHILD words %d kernel %d rotation %d" % (b.instance_words, b.info("kernel"), (held[2] - saved[2]) % 8192), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "rot", "--", sys.executable, os.path.abspath(__file__),
               "--child", "--instances", str(args.instances), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.timeout)
        note = [line for line in r.stdout.splitlines() if line.startswith("CHILD ")]
        if r.returncode != 0 or not note:
            sys.exit("the profiled run failed (%d):\n%s" % (r.returncode, r.stdout[-3000:]))
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            sys.exit("rocprofv3 wrote no kernel trace:\n" + r.stdout[-3000:])
        rows = list(csv.DictReader(open(traces[0])))
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))

    def times(wanted):
        return [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows if wanted(row["Kernel_Name"])]

    plain = times(lambda name: "fx_inst_scatter" in name and "fx_inst_scatter_rot" not in name)
    rot = times(lambda name: "fx_inst_scatter_rot" in name)
    if len(plain) != args.repeats or len(rot) != 2 * args.repeats:
        sys.exit("expected %d + %d launches, the trace has %d + %d" % (args.repeats, 2 * args.repeats, len(plain), len(rot)))
    token = note[0].split()   # CHILD words W kernel K rotation D
    words, kernel, rotation = token[2], token[4], token[6]
    lines = ["config5, %d instances, %d records of W = %s words (%d bytes each) into one list; kernel tier %s; %s" %
             (args.instances, RECORDS, words, int(words) * 4, kernel, time.strftime("%Y-%m-%d")),
             "kernel times in us from one rocprofv3 --kernel-trace --stats run of its own, %d launches each" % args.repeats,
             "",
             "%-22s %-10s %10s %10s %10s" % ("kernel", "rotation", "median", "min", "max")]
    for name, d, part in (("fx_inst_scatter", "-", plain), ("fx_inst_scatter_rot", "0", rot[:args.repeats]), ("fx_inst_scatter_rot", rotation, rot[args.repeats:])):
        lines.append("%-22s %-10s %10.2f %10.2f %10.2f" % (name, d, statistics.median(part), min(part), max(part)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
