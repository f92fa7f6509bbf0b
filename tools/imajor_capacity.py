#!/usr/bin/env python3
"""What instance-major blocks cost a real-time host that holds one stream per instance: 32-sample blocks of config5 from pinned
host buffers, three paths by turns in stretches in ONE process on ONE build.

  plain   fxb_process_block in place on buffers that are ALREADY [sample][channel][instance] - the floor: a caller with
          per-instance streams cannot get there without a transposition;
  imajor  fxb_process_block_imajor in place on pinned per-instance streams [instance][sample]: a gather and a scatter kernel around
          the unchanged emulation launch read and write the streams over PCIe;
  host    what such a caller does today: numpy copyto on transposed views into and out of a pinned [sample][instance] buffer
          around the plain call (the fastest means at hand in this process: one strided copy each way on one thread).

1. Side by side at --instances: median, p99, p99.9 of each path; the last block of the imajor and host paths must be, word for
   word, the plain path's transposed.
2. Capacity: the instance count goes up for the imajor path; the largest count whose p99.9 block time (and every smaller count's)
   stays inside 666.667 us.  The last block of every row is compared with a plain handle's replay of the run.
3. `--trace-run`: nothing is timed; --trace-blocks device-entry blocks of --trace-samples samples at --trace-instances run on
   device memory, each followed by a device-to-device hipMemcpyAsync of the bytes one of the two kernels moves one way - the
   program to put behind `rocprofv3 --kernel-trace --memory-copy-trace --stats ... --` in a run of its own, without counters.
   `--kernel-stats FILE.csv [--copy-stats FILE.csv]` reads the tables that run wrote: the two kernels' time per launch, their
   achieved bytes/s (every word read once and written once) and the same for the copy, the yardstick.

Every path slides the control `decay` like the reference's harness does (realtime_capacity.py).

    python tools/imajor_capacity.py [--blocks 3000] [--json profiles/imajor_realtime.json] [--out profiles/imajor_realtime.txt]
"""
import argparse
import csv
import ctypes as C
import gc
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import realtime_capacity as rt   # (sets the import paths of the binding and the oracle)

BLOCK, BUDGET_US, SLIDER, SLIDER_EVERY, RING = rt.BLOCK, rt.BUDGET_US, rt.SLIDER, rt.SLIDER_EVERY, rt.RING


class Path:
    """one handle and its pinned buffers; block() is one synchronous call on the caller's clock.  kind: plain / imajor / host"""

    def __init__(self, A, progs, n, kind):
        import numpy as np
        self.np, self.A, self.n, self.kind, self.lib = np, A, n, kind, A.load()
        self.b = A.Batch(n, 1, 0)
        if not self.b.load_text(progs.CONFIGS["config5"]()):
            raise RuntimeError("load failed: %s" % self.b.errors())
        wide = kind != "imajor"   # the pinned buffers the library sees: [sample][instance], or the streams [instance][sample]
        self.pin_in = A.HostBuffer((BLOCK, n) if wide else (n, BLOCK))
        self.pin_out = A.HostBuffer((BLOCK, n) if wide else (n, BLOCK))
        self.ring = []
        for k in range(RING):
            x = progs.stimulus(n, BLOCK, first_sample=k * BLOCK)   # [sample][instance]
            if kind == "plain":
                h = A.HostBuffer((BLOCK, n))
                h.array[...] = x
            elif kind == "imajor":
                h = A.HostBuffer((n, BLOCK))
                h.array[...] = x.T
            else:
                h = np.ascontiguousarray(x.T)   # the caller's own streams, in its own memory
            self.ring.append(h)
        self.streams_out = np.empty((n, BLOCK), dtype=np.float32) if kind == "host" else None
        ptr = lambda h: C.c_void_p(h.array.ctypes.data)
        self.xp = [ptr(h) for h in self.ring] if kind != "host" else None
        self.ip, self.yp = ptr(self.pin_in), ptr(self.pin_out)
        self.b.prepare(BLOCK, True)
        self.k = 0
        self.times = []

    def block(self):
        k, h, np = self.k, self.b._h, self.np
        if k % SLIDER_EVERY == 0:
            assert self.lib.fxb_set_register(h, b"decay", C.c_float(SLIDER[(k // SLIDER_EVERY) % len(SLIDER)])) == 0
        if self.kind == "plain":
            rc = self.lib.fxb_process_block_pitched(h, self.xp[k % RING], self.yp, BLOCK, self.n)
        elif self.kind == "imajor":
            rc = self.lib.fxb_process_block_imajor(h, self.xp[k % RING], self.yp, BLOCK, 0, 0)
        else:
            np.copyto(self.pin_in.array, self.ring[k % RING].T)
            rc = self.lib.fxb_process_block_pitched(h, self.ip, self.yp, BLOCK, self.n)
            np.copyto(self.streams_out, self.pin_out.array.T)
        if rc != 0:
            raise RuntimeError("block %d failed (%d): %s" % (k, rc, self.b.last_error()))
        self.k = k + 1

    def last_streams(self):
        """the last block's output as [instance][sample]"""
        return {"plain": lambda: self.np.ascontiguousarray(self.pin_out.array.T), "imajor": lambda: self.pin_out.array, "host": lambda: self.streams_out}[self.kind]()

    def stretch(self, blocks, timed=True):
        for _ in range(blocks):
            t0 = time.perf_counter_ns()
            self.block()
            if timed:
                self.times.append((time.perf_counter_ns() - t0) * 1e-3)

    def close(self):
        self.b.close()
        for h in self.ring + [self.pin_in, self.pin_out]:
            if hasattr(h, "close"):
                h.close()


def same_words(a, b):
    import numpy as np
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


def side_by_side(A, progs, n, blocks, warm, stretch, log):
    paths = [(kind, Path(A, progs, n, kind)) for kind in ("plain", "imajor", "host")]
    for _, p in paths:
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    start = {kind: (p.b.info("host_staged_blocks"), p.b.info("host_inplace_blocks")) for kind, p in paths}
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for _, p in paths:   # by turns: what else happens on the host and the device meets all three
                p.stretch(stretch)
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "stretch_blocks": stretch, "pcie_bytes_each_way_per_block": BLOCK * n * 4}
    floor = paths[0][1].last_streams()
    for kind, p in paths:
        r = rt.percentiles(p.times)
        r.update({"host_staged_blocks_in_timed_region": p.b.info("host_staged_blocks") - start[kind][0],
                  "host_inplace_blocks_in_timed_region": p.b.info("host_inplace_blocks") - start[kind][1],
                  "kernel_us_last": round(p.b.last_kernel_ms() * 1e3, 1), "last_block_equals_plain_transposed": same_words(p.last_streams(), floor)})
        out[kind] = r
        log("%-6s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  emulation kernel %6.1f us  last block %s" % (
            kind, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["p999_us"] <= BUDGET_US else "over budget",
            r["kernel_us_last"], "equal" if r["last_block_equals_plain_transposed"] else "DIFFERS"))
    for _, p in paths:
        p.close()
    return out


def imajor_row(A, progs, n, blocks, warm, log):
    """one count of the sweep; after the timed region a plain handle replays every block of the run (same PCM, same slider
    schedule, untimed) and the imajor path's LAST block must be, word for word, the plain one's transposed"""
    p = Path(A, progs, n, "imajor")
    p.stretch(warm, timed=False)
    p.b.prepare(BLOCK, True)
    gc.collect()
    gc.disable()
    try:
        p.stretch(blocks)
    finally:
        gc.enable()
    r = rt.percentiles(p.times)
    r.update({"instances": n, "mode": "imajor", "within_budget_p999": r["p999_us"] <= BUDGET_US, "kernel_us_last": round(p.b.last_kernel_ms() * 1e3, 1),
              "host_inplace_blocks": p.b.info("host_inplace_blocks"), "host_staged_blocks": p.b.info("host_staged_blocks")})
    plain = Path(A, progs, n, "plain")
    plain.stretch(p.k, timed=False)
    picks = sorted({0, 63, 64, n // 2, n - 1})
    ok = same_words(p.last_streams(), plain.last_streams()) and all(p.b.instruction_counter_i(i) == plain.b.instruction_counter_i(i) for i in picks)
    r.update({"parity_ok": ok, "parity": "last of %d blocks against a plain handle's replay of the run, transposed; instruction counters of %d instances" % (p.k, len(picks))})
    log("imajor N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  parity %s" % (n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"],
        "REAL TIME" if r["within_budget_p999"] else "over budget", "ok" if ok else "MISMATCH"))
    plain.close()
    p.close()
    return r


def samples_per_launch(n, samples):
    """a block above the 64 MiB scratch runs in consecutive sample ranges (mono): the samples of one of them"""
    most = max((64 << 20) // (n * 4), 1)
    pieces = -(-samples // most)
    return -(-samples // pieces)


def trace_run(torch, A, progs, n, samples, blocks):
    """device-entry blocks in place on one device tensor, each followed by a device-to-device copy of one kernel's bytes one way"""
    b = A.Batch(n, 1, 0)
    if not b.load_text(progs.CONFIGS["config5"]()):
        raise RuntimeError("load failed: %s" % b.errors())
    d = torch.zeros((n, samples, 1), dtype=torch.float32, device="cuda")
    piece = samples_per_launch(n, samples)   # the copy matches one piece
    src = torch.zeros((n * piece,), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    b.prepare(min(samples, 32), True)
    for _ in range(blocks):
        b.process_block_imajor_dev(d, d, samples)
        dst.copy_(src, non_blocking=True)
    b.sync()
    torch.cuda.synchronize()
    print("traced %d blocks of %d samples x %d instances; copy of %d bytes per block" % (blocks, samples, n, n * piece * 4), flush=True)
    b.close()


def kernel_rates(kernel_csv, copy_csv, n, samples):
    """per launch: ns and achieved TB/s (bytes read + bytes written) of the gather, the scatter and the copy"""
    piece = samples_per_launch(n, samples)
    moved = 2 * n * piece * 4
    out = {"instances": n, "samples": samples, "samples_per_launch": piece, "bytes_read_plus_written_per_launch": moved, "kernels": {}}
    for path in (kernel_csv, copy_csv):
        if not path:
            continue
        for r in csv.DictReader(open(path)):
            name = r["Name"]
            for key in ("fx_imajor_gather", "fx_imajor_scatter", "fx_bus_expand", "fx_bus_mix", "fx_meter", "DEVICE_TO_DEVICE", "copyBuffer"):
                if key in name:
                    avg = float(r["AverageNs"])
                    out["kernels"][name[:100]] = {"calls": int(r["Calls"]), "average_ns": round(avg, 1), "achieved_TBps": round(moved / avg / 1e3, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--stretch", type=int, default=250, help="blocks of one path before the next takes its turn")
    ap.add_argument("--instances", type=int, default=131072)
    ap.add_argument("--sweep", default="65536,98304,131072,147456,163840,180224")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-instances", type=int, default=524288)
    ap.add_argument("--trace-samples", type=int, default=32)
    ap.add_argument("--trace-blocks", type=int, default=200)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--copy-stats", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--out", default="", help="keep the lines in this text file")
    args = ap.parse_args()
    import torch  # first: its HIP runtime is the one the library binds to

    import fx8010_amd as A
    import fx8010_programs as progs
    lines = []

    def log(s):
        lines.append(s)
        print(s, flush=True)
    if args.trace_run:
        trace_run(torch, A, progs, args.trace_instances, args.trace_samples, args.trace_blocks)
        return 0
    if args.kernel_stats:
        print(json.dumps(kernel_rates(args.kernel_stats, args.copy_stats, args.trace_instances, args.trace_samples), indent=1))
        return 0
    out = {"what": "32-sample blocks of config5 at 48 kHz against %.3f us, pinned host buffers, call -> output in host memory on the caller's clock; plain: "
                   "fxb_process_block in place on [sample][instance]; imajor: fxb_process_block_imajor in place on [instance][sample] streams; host: numpy "
                   "copyto on transposed views into and out of a pinned [sample][instance] buffer around the plain call" % BUDGET_US,
           "gpu": torch.cuda.get_device_name(0), "budget_us": round(BUDGET_US, 3), "blocks_per_point": args.blocks, "warmup_blocks": args.warmup}
    log("%s; %d blocks per point after %d warm-up blocks, stretches of %d; %s" % (out["what"], args.blocks, args.warmup, args.stretch, out["gpu"]))
    out["side_by_side"] = side_by_side(A, progs, args.instances, args.blocks, args.warmup, args.stretch, log)
    rows = [imajor_row(A, progs, int(v), args.blocks, args.warmup, log) for v in args.sweep.split(",") if v]
    out["imajor_rows"], out["capacity_imajor"] = rows, rt.capacity(rows)
    log("largest N within %.3f us at p99.9 on per-instance streams in place: %s" % (BUDGET_US, out["capacity_imajor"]))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ok = all(out["side_by_side"][k]["last_block_equals_plain_transposed"] for k in ("imajor", "host")) and all(r["parity_ok"] for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
