#!/usr/bin/env python3
"""What a delay-line window by list costs (fxb_set_tram_list / fxb_get_tram_list, kernels fx_tram_scatter / fx_tram_gather): config5
on the translated tier, xTRAM windows of 256 and 8 192 words, lists of 1, 64 and 4 096 voices, scattered and consecutive, logical
and physical.

Two views, two runs:
  the caller's clock  around the call and fxb_sync (median of --repeats), beside the parent's only ways to the same effect - the
                      fxb_save_instances / edit / fxb_load_instances round trip of the same voices and, for the get, `count` calls
                      of fxb_get_tram_i - and a device-to-device copy of the same bytes (hipMemcpy on the null stream, then a wait for it);
  the kernel's time   from a child process under rocprofv3, in a run of its own with nothing else traced
                          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tram -- python tools/tram_list_cost.py --child
                      fx_tram_scatter / fx_tram_gather beside fx_inst_scatter (fxb_load_instances) on the same lists.

    python tools/tram_list_cost.py [--instances 262144] [--repeats 20] [--out profiles/tram_list.txt] [--no-trace]
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

WARM = 64
VOICES, WORDS = (1, 64, 4096), (256, 8192)


def cases(n):
    """(voices, words, 'scattered' | 'consecutive', logical) in the order both runs walk them"""
    for voices in VOICES:
        if voices > n:
            continue
        for words in WORDS:
            for shape in ("scattered", "consecutive"):
                for logical in (False, True):
                    yield voices, words, shape, logical


def first_of(words):
    """windows begin at word 100, the whole line at word 0"""
    return 100 if words < 8192 else 0


def list_of(np, n, voices, shape):
    if shape == "consecutive":
        return (min(n // 3, n - voices) + np.arange(voices)).astype(np.int64)
    return np.random.default_rng(voices).permutation(n)[:voices].astype(np.int64)


def handle(args):
    import numpy as np

    import fx8010_amd as A
    import fx8010_programs as progs

    b = A.Batch(args.instances, 1, 0)
    assert b.load_text(progs.config5()), b.errors()
    b.process_block(np.ascontiguousarray(progs.stimulus(args.instances, WARM)))
    assert b.info("xtram_slots") == 8192 and b.info("instance_rings") & 2
    return np, b


def child(args):
    """every case --repeats times, one kernel per call; then fxb_load_instances of the same lists"""
    np, b = handle(args)
    n = args.instances
    for voices, words, shape, logical in cases(n):
        L = list_of(np, n, voices, shape)
        v = np.zeros((voices, words), dtype=np.float32)
        first = first_of(words)
        for _ in range(args.repeats):
            assert b.set_tram_list(1, L, first, v, logical=logical) == 0
        for _ in range(args.repeats):
            b.get_tram_list(1, L, first, words, logical=logical)
    loads = []
    for voices in VOICES:
        if voices > n:
            continue
        for shape in ("scattered", "consecutive"):
            L = list_of(np, n, voices, shape)
            image = b.save_instances(L)
            before = b.info("instance_scatters")
            for _ in range(args.repeats):
                assert b.load_instances(L, image) == 0
            loads.append((b.info("instance_scatters") - before) // args.repeats)
    b.sync()
    print("CHILD kernel %d words %d pieces %s" % (b.info("kernel"), b.instance_words, ",".join(str(k) for k in loads)), flush=True)


def wall(np, b, args):
    """the caller's clock, in us: median of --repeats"""
    n = args.instances
    lines = ["%-6s %-6s %-12s %-9s %10s %10s %14s %14s %10s" % ("voices", "words", "list", "mode", "set+sync", "get", "save/edit/load", "get_tram_i x n", "d2d copy")]
    # a device-to-device copy of the same bytes, through the HIP runtime the library is linked against
    import ctypes as C
    hip = b._lib
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    biggest = max(v_ * w_ for v_, w_, _, _ in cases(n)) * 4
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_src), biggest) == 0 and hip.hipMalloc(C.byref(d_dst), biggest) == 0

    def median(f, repeats=args.repeats):
        out = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(out)

    W = b.instance_words
    off = W - 8192
    for voices, words, shape, logical in cases(n):
        L = list_of(np, n, voices, shape)
        v = np.random.default_rng(1).uniform(-0.1, 0.1, (voices, words)).astype(np.float32)
        first = first_of(words)
        b.set_tram_list(1, L, first, v, logical=logical)   # (staging exists before anything is timed)
        b.sync()
        t_set = median(lambda: (b.set_tram_list(1, L, first, v, logical=logical), b.sync()))
        t_get = median(lambda: b.get_tram_list(1, L, first, words, logical=logical))
        few = max(2, args.repeats // 4)

        def round_trip():
            image = b.save_instances(L)
            rec = image[64:].view(np.uint32).reshape(voices, W)
            if logical:
                for i in range(voices):
                    p = b.get_cursors_i(int(L[i]))[2]
                    rec[i, off + (p - 1 - first - np.arange(words)) % 8192] = v[i].view(np.uint32)
            else:
                rec[:, off + first:off + first + words] = v.view(np.uint32)
            b.load_instances(L, image)
            b.sync()

        timed_trip = not (logical and voices > 64)   # (a get_cursors_i per voice: minutes at 4 096)
        if timed_trip:
            round_trip()   # (its buffers exist before anything is timed, as for the set)
        b.get_tram_i(1, int(L[0]), 8192)
        t_trip = median(round_trip, few) if timed_trip else float("nan")
        t_single = median(lambda: [b.get_tram_i(1, int(i), 8192) for i in L[:64]], few) * (voices / min(voices, 64))
        t_copy = median(lambda: (hip.hipMemcpy(d_dst, d_src, voices * words * 4, 3), hip.hipStreamSynchronize(None)))
        lines.append("%-6d %-6d %-12s %-9s %10.1f %10.1f %14.1f %14.1f %10.1f" % (voices, words, shape, "logical" if logical else "physical", t_set, t_get, t_trip, t_single, t_copy))
    hip.hipFree(d_src)
    hip.hipFree(d_dst)
    return lines


def traced(args):
    """kernel times in us from the child's trace: {case: (scatter median, gather median)}, and fx_inst_scatter per load"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "tram", "--", sys.executable, os.path.abspath(__file__),
               "--child", "--instances", str(args.instances), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.timeout)
        note = [line for line in r.stdout.splitlines() if line.startswith("CHILD ")]
        if r.returncode != 0 or not note:
            return ["the profiled run failed (%d): %s" % (r.returncode, r.stdout[-600:].replace("\n", " | "))]
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return ["rocprofv3 wrote no kernel trace"]
        rows = list(csv.DictReader(open(traces[0])))
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))

    def times(wanted):
        return [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows if wanted(row["Kernel_Name"])]

    scatter, gather = times(lambda name: "fx_tram_scatter" in name), times(lambda name: "fx_tram_gather" in name)
    inst = times(lambda name: "fx_inst_scatter" in name and "fx_inst_scatter_rot" not in name)
    R = args.repeats
    all_cases = list(cases(args.instances))
    # (a call whose windows exceed the 64 MiB of staging runs in pieces: its time is the sum of their kernels)
    parts = [-(-voices // max((64 << 20) // (words * 4), 1)) for voices, words, _, _ in all_cases]
    if len(scatter) != R * sum(parts) or len(gather) != R * sum(parts):
        return ["expected %d launches of each kernel, the trace has %d and %d" % (R * sum(parts), len(scatter), len(gather))]
    token = note[0].split()   # CHILD kernel K words W pieces a,b,...
    pieces = [int(k) for k in token[6].split(",")]
    lines = ["kernel times in us from one rocprofv3 --kernel-trace --stats run of its own, %d launches each (median, min - max); kernel tier %s" % (R, token[2]),
             "%-6s %-6s %-12s %-9s %26s %26s" % ("voices", "words", "list", "mode", "fx_tram_scatter", "fx_tram_gather")]
    at = 0
    for k, (voices, words, shape, logical) in enumerate(all_cases):
        per = parts[k]
        s = [sum(scatter[at + c * per:at + (c + 1) * per]) for c in range(R)]
        g = [sum(gather[at + c * per:at + (c + 1) * per]) for c in range(R)]
        at += per * R
        lines.append("%-6d %-6d %-12s %-9s %10.2f (%6.2f - %6.2f) %10.2f (%6.2f - %6.2f)" % (voices, words, shape, "logical" if logical else "physical",
                                                                                     statistics.median(s), min(s), max(s), statistics.median(g), min(g), max(g)))
    lines += ["", "fx_inst_scatter on the same lists (fxb_load_instances: whole records of %s words; per call, the sum of its pieces)" % token[4]]
    at, k = 0, 0
    for voices in VOICES:
        if voices > args.instances:
            continue
        for shape in ("scattered", "consecutive"):
            per = pieces[k]
            calls = [sum(inst[at + c * per:at + (c + 1) * per]) for c in range(R)]
            at += per * R
            k += 1
            lines.append("%-6d %-6s %-12s %-9s %10.2f (%6.2f - %6.2f)  %d piece(s)" % (voices, "record", shape, "-", statistics.median(calls), min(calls), max(calls), per))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=500.0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    np, b = handle(args)
    lines = ["config5, %d instances, kernel tier %d, xTRAM windows from word 100 (the whole line: from word 0); %s" % (args.instances, b.info("kernel"), time.strftime("%Y-%m-%d")),
             "the caller's clock in us around the call (the set with fxb_sync), median of %d; the round trip and the single calls: of %d" % (args.repeats, max(2, args.repeats // 4)), ""]
    lines += wall(np, b, args)
    b.close()
    if not args.no_trace:
        lines += [""] + traced(args)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
