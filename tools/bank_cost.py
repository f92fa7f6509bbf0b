#!/usr/bin/env python3
"""What a recall costs: config5 at 262 144 instances, 1, 64 and 1 024 voices taking a whole state behind a queued block - from the
record bank (fxb_bank_recall) and, beside it, through fxb_load_instances_rotated from a pinned image, the only way without a bank.

Per size and path, medians of --repeats, the two paths alternating inside one run:

  total   the caller's clock from the call to the return of fxb_sync, a 32-sample block queued in front on the handle's stream
          (the block's own time is in both figures: the rotated load waits for it inside the call, the recall behind it);
  host    the caller's clock inside the call alone: what the call holds the caller for.

The records of both paths are the same voices' (stored and saved after the same block), the destinations are scattered over the
batch and alike in both; what crosses PCIe is computed from the shapes: the recall sends two 64-bit words per entry, the rotated
load fetches the four position rows of the whole batch and sends every record.  fxb_bank_status must have counted no refusal.

The GPU work runs in a child process under a time limit of its own (--timeout).

    python tools/bank_cost.py [--instances 262144] [--out profiles/bank_recall.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK = 32


def child(args):
    import numpy as np
    import torch   # (before the library: see tests/conftest.py)
    import fx8010_amd as A
    import fx8010_programs as progs

    lib = A.load()
    N = args.instances
    b = A.Batch(N, 1, 0)
    if not b.load_text(progs.CONFIGS["config5"]()):
        raise RuntimeError("load failed: %s" % b.errors())
    x = torch.from_numpy(progs.stimulus(N, BLOCK)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()

    def block():
        rc = lib.fxb_process_block_dev(b._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), BLOCK, None)
        if rc != 0:
            raise RuntimeError("block failed (%d): %s" % (rc, b.last_error()))

    b.prepare(BLOCK, True)
    for _ in range(20):
        block()
    b.sync()
    W = b.instance_words
    sizes = [n for n in (1, 64, 1024) if 2 * n <= N]
    b.bank_create(max(sizes))
    rng = np.random.default_rng(11)
    result = {"program": "config5", "instances": N, "instance_words": W, "record_bytes": W * 4, "block_samples": BLOCK, "repeats": args.repeats,
              "kernel": b.info("kernel"), "date": time.strftime("%Y-%m-%d"), "unit": "us", "sizes": []}
    for n in sizes:
        pick = rng.choice(N, 2 * n, replace=False).astype(np.int64)
        src, dst = np.sort(pick[:n]), np.sort(pick[n:])
        slots = np.arange(n, dtype=np.int64)
        b.bank_store(slots, src)
        nbytes = b.instance_image_size(n)
        pinned = lib.fxb_host_alloc(nbytes)
        if not pinned:
            raise RuntimeError("no pinned image")
        if lib.fxb_save_instances(b._h, C.c_void_p(src.ctypes.data), n, C.c_void_p(pinned), nbytes) != 0:
            raise RuntimeError("save failed: %s" % b.last_error())
        calls = {
            "bank_recall": lambda: lib.fxb_bank_recall(b._h, C.c_void_p(slots.ctypes.data), C.c_void_p(dst.ctypes.data), n),
            "load_instances_rotated": lambda: lib.fxb_load_instances_rotated(b._h, C.c_void_p(dst.ctypes.data), n, C.c_void_p(pinned), nbytes),
        }
        times = {k: {"total": [], "host": []} for k in calls}
        for rep in range(args.repeats + 3):   # (the first three turns warm both paths up: staging, scratch, code)
            for name, call in calls.items():
                b.sync()
                block()
                t0 = time.perf_counter_ns()
                rc = call()
                t1 = time.perf_counter_ns()
                b.sync()
                t2 = time.perf_counter_ns()
                if rc != 0:
                    raise RuntimeError("%s failed (%d): %s" % (name, rc, b.last_error()))
                if rep >= 3:
                    times[name]["total"].append((t2 - t0) * 1e-3)
                    times[name]["host"].append((t1 - t0) * 1e-3)
        lib.fxb_host_free(C.c_void_p(pinned))
        row = {"voices": n,
               "pcie_bytes": {"bank_recall": 16 * n, "load_instances_rotated": 16 * N + n * W * 4 + 16 * n}}
        for name in calls:
            for clock in ("total", "host"):
                v = sorted(times[name][clock])
                row["%s_%s_us" % (name, clock)] = round(statistics.median(v), 1)
                row["%s_%s_quartiles_us" % (name, clock)] = [round(v[len(v) // 4], 1), round(v[(3 * len(v)) // 4], 1)]
        result["sizes"].append(row)
    refused, entry, reason = b.bank_status()
    if refused:
        raise RuntimeError("the device refused %d recall(s): entry %d, reason %d - the bank figures are those of a gate, not of a recall" % (refused, entry, reason))
    # the block alone, for scale
    t = []
    for _ in range(args.repeats):
        b.sync()
        t0 = time.perf_counter_ns()
        block()
        b.sync()
        t.append((time.perf_counter_ns() - t0) * 1e-3)
    result["block_alone_us"] = round(statistics.median(t), 1)
    result["launches"] = {k: b.info(k) for k in ("bank_stores", "bank_recalls", "instance_rotations")}
    text = json.dumps(result, indent=1) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--instances", str(args.instances), "--repeats", str(args.repeats)]
    if args.out:
        cmd += ["--out", args.out]
    r = subprocess.run(cmd, timeout=args.timeout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
