#!/usr/bin/env python3
"""What the per-instance state calls cost: config5 at 262 144 instances, fxb_copy_instances / fxb_reset_instances /
fxb_save_instances over lists of 1, 64 and 4 096 instances, scattered and consecutive.

The calls run on the handle's own stream, ordered behind the blocks queued so far and in front of the later ones, so a GPU event
pair cannot be put around their kernels alone from outside.  Two clocks instead:

  gpu    GPU events on the caller's stream around  block, call, block  minus the same around  block, block  (1-sample blocks;
         median of --repeats): what the call adds to a stream of blocks, kernels and list upload included;
  host   the caller's clock around the call and fxb_sync, after an fxb_sync: launch latency included (save is synchronous by
         itself: its device-to-host copy is in the figure).

Yardsticks: for the consecutive lists a device-to-device copy of the same bytes, GPU events (a copy reads and writes every word
once; fxb_copy_instances moves every word twice, into the scratch and out of it); fxb_save_state + fxb_load_state of the whole
batch, the only way to reach one instance's state without these calls (host clock; --whole-batch 0 skips it: the image of the
default workload is 8 GiB); and the real-time figure: a reset of 64 voices queued between two 32-sample blocks, beside the
666.667 us budget of a block.

The GPU work runs in a child process under a time limit of its own (--timeout).

    python tools/instance_ops_cost.py [--instances 262144] [--out profiles/instance_ops.txt]
"""
import argparse
import ctypes as C
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

BUDGET_US = 666.667


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
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    x = torch.from_numpy(progs.stimulus(N, 32)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()

    def block(samples):
        rc = lib.fxb_process_block_dev(b._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), samples, sp)
        if rc != 0:
            raise RuntimeError("block failed (%d): %s" % (rc, b.last_error()))

    for s in (32, 1):
        b.prepare(s, True)
        for _ in range(20):
            block(s)
    b.sync()
    W = b.instance_words
    rows = ["config5, %d instances, record W = %d words (%d bytes); kernel tier %d; %s" % (N, W, W * 4, b.info("kernel"), time.strftime("%Y-%m-%d")),
            "times in us, median of %d; gpu = (block, call, block) - (block, block) by GPU events, host = call + fxb_sync on the caller's clock" % args.repeats, ""]

    def gpu_pair(samples, call):
        """median GPU time of block, call(), block on the caller's stream"""
        t = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.sync()
            e0.record(stream)
            block(samples)
            if call:
                call()
            block(samples)
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(t)

    def host_clock(call, synchronous=False):
        t = []
        for _ in range(args.repeats):
            b.sync()
            t0 = time.perf_counter_ns()
            call()
            if not synchronous:
                b.sync()
            t.append((time.perf_counter_ns() - t0) * 1e-3)
        return statistics.median(t)

    def dtod(nbytes):
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        t = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                dst.copy_(src)
                e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(t)

    rng = np.random.default_rng(11)
    half = N // 2
    base = gpu_pair(1, None)
    rows.append("%-8s %-12s %6s %12s %12s %14s %12s" % ("call", "list", "count", "gpu us", "host us", "DtoD copy us", "bytes"))
    for count in (1, 64, 4096):
        if count > half:
            continue
        for shape in ("scattered", "consecutive"):
            if shape == "scattered":
                src = np.sort(rng.choice(half, count, replace=False)).astype(np.int64)
                dst = (half + np.sort(rng.choice(N - half, count, replace=False))).astype(np.int64)
            else:
                src = np.arange(1000, 1000 + count, dtype=np.int64) % half
                dst = half + src
            nbytes = count * W * 4
            copy_us = dtod(nbytes) if shape == "consecutive" else None
            image = np.empty(b.instance_image_size(count), dtype=np.uint8)
            calls = {
                "copy": lambda: b.copy_instances(src, dst),
                "reset": lambda: b.reset_instances(dst),
                "save": lambda: lib.fxb_save_instances(b._h, C.c_void_p(src.ctypes.data), count, C.c_void_p(image.ctypes.data), image.size),
            }
            for name in ("copy", "reset", "save"):
                gpu = None if name == "save" else gpu_pair(1, calls[name]) - base
                host = host_clock(calls[name], synchronous=name == "save")
                rows.append("%-8s %-12s %6d %12s %12.1f %14s %12d" % (name, shape, count, "-" if gpu is None else "%.1f" % gpu, host,
                                                                      "-" if copy_us is None else "%.1f" % copy_us, nbytes))
    rows.append("")
    voices = np.sort(rng.choice(N, min(64, N), replace=False)).astype(np.int64)
    plain = gpu_pair(32, None)
    with_reset = gpu_pair(32, lambda: b.reset_instances(voices))
    rows.append("real time: two 32-sample blocks %.1f us, with a reset of %d voices queued between them %.1f us: +%.1f us beside the %.3f us budget of a block"
                % (plain, voices.size, with_reset, with_reset - plain, BUDGET_US))
    if args.whole_batch:
        b.sync()
        t0 = time.perf_counter()
        image = b.save_state()
        t1 = time.perf_counter()
        b.load_state(image)
        t2 = time.perf_counter()
        rows.append("whole batch (the parent commit's only way): fxb_save_state %.2f s + fxb_load_state %.2f s for an image of %.2f GiB"
                    % (t1 - t0, t2 - t1, image.size / 2.0 ** 30))
    rows.append("launches: %d fx_inst_gather, %d fx_inst_scatter" % (b.info("instance_gathers"), b.info("instance_scatters")))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--whole-batch", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--instances", str(args.instances), "--repeats", str(args.repeats), "--whole-batch", str(args.whole_batch)]
    if args.out:
        cmd += ["--out", args.out]
    r = subprocess.run(cmd, timeout=args.timeout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
