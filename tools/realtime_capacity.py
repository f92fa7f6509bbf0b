#!/usr/bin/env python3
"""How many emulated FX8010s does one MI355X carry in REAL TIME - measured the way the reference measures itself.

The reference's only timing idea (source/main.cpp:99-155, include/FX8010.h:37-38): one AUDIOBLOCKSIZE = 32-sample block at
48 kHz must be done within 666.667 us, while a slider moves (main.cpp:107-114: setRegisterValue("volume", ...) with the values
0.1 / 0.25 / 0.5 / 1.0).  Here: program = config5 (the 512-instruction reverb of BASELINE configs[4], 8192-sample xTRAM), N
instances per block call, PCM **host-fed from pinned buffers** through fxb_process_block (copy in, kernel, copy out, done when
the output is in host memory), after fxb_prepare; the declared control `decay` takes the harness's four values in turn, a new
one every 8th block (a fill of one register row - no code is generated in the timed region: checked).  Per N: median / p99 /
p99.9 / max of the block time, the kernel's own time, the PCIe rate, and whether p99.9 <= 666.667 us; the answer is the
largest such N.  The same with device-resident PCM (fxb_process_block_dev + fxb_sync per block: what a host that already has
its audio on the GPU pays).  After the timed region the device's LAST block is compared bit for bit with the CPU oracle, which
replays every block of the run for sampled instances (same PCM, same slider schedule).

    python tools/realtime_capacity.py [--blocks 5000] [--instances 4096,...] [--json profiles/r05_realtime.json]

--register-list: instead of the sweep, what per-instance register writes in front of every block cost - no writes,
fxb_set_registers_list, fxb_set_register_array and fxb_set_register_i by turns in one process (register_paths;
profiles/register_list_realtime.txt).

    python tools/realtime_capacity.py --track-list [--blocks 3000] [--register-instances 131072,458752] [--track-out FILE]
    python tools/realtime_capacity.py --register-list [--blocks 3000] [--register-instances 131072,458752] [--register-out FILE]
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fx8010-emulator-core_amd", "python"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK = 32                      # AUDIOBLOCKSIZE, /root/reference/include/FX8010.h:38
SAMPLERATE = 48000              # /root/reference/include/FX8010.h:37
BUDGET_US = BLOCK / SAMPLERATE * 1e6   # 666.667 us: "Erlaubtes Zeitfenster ohne Dropouts", source/main.cpp:155
SLIDER = (0.1, 0.25, 0.5, 1.0)  # source/main.cpp:80
SLIDER_EVERY = int(os.environ.get("FX_RT_SLIDER_EVERY", "8"))   # a new value every 8th block (the environment can slow the slider down: a slider that
                                # rests longer than 8192 sample periods cools down and is folded into the code again, on the builder thread)
RING = 8                        # distinct PCM blocks, fed in turn


def percentiles(us):
    import numpy as np
    a = np.sort(np.asarray(us, dtype=np.float64))
    pick = lambda q: float(a[min(len(a) - 1, int(np.ceil(q * len(a))) - 1)])
    return {"median_us": round(pick(0.5), 1), "p99_us": round(pick(0.99), 1), "p999_us": round(pick(0.999), 1), "max_us": round(float(a[-1]), 1),
            "mean_us": round(float(a.mean()), 1), "blocks": int(len(a)), "over_budget": int((a > BUDGET_US).sum())}


def measure(torch, A, progs, n, blocks, warm, mode, check=4, config="config5", control="decay", shards=1):
    """one N, one mode ("host": pinned host PCM through fxb_process_block; "device": resident PCM, launch + sync per block).
    shards > 1 (host mode): the handle is made of that many shards ON THE SAME GPU (fxb_create_on_devices with the ordinal
    repeated): each shard has its own host thread and stream and works on its own columns of the caller's pinned [S][N] buffers in
    place (before row-pitched PCM: copied its columns in and out, staged)."""
    import numpy as np
    from pyoracle import Oracle

    text = progs.CONFIGS[config]()
    lib = A.load()
    b = A.Batch(n, 1, 0) if shards <= 1 else A.Batch(n, 1, devices=[0] * shards)
    if not b.load_text(text):
        raise RuntimeError("load failed: %s" % b.errors())
    ring = [progs.stimulus(n, BLOCK, first_sample=k * BLOCK) for k in range(RING)]
    if mode == "host":
        xin = [torch.empty((BLOCK, n), dtype=torch.float32).pin_memory() for _ in range(RING)]
        for t, r in zip(xin, ring):
            t.numpy()[...] = r
        yout = torch.empty((BLOCK, n), dtype=torch.float32).pin_memory()
        xp = [C.cast(t.data_ptr(), C.POINTER(C.c_float)) for t in xin]
        yp = C.cast(yout.data_ptr(), C.POINTER(C.c_float))
    else:
        xin = [torch.from_numpy(r).cuda() for r in ring]
        yout = torch.empty((BLOCK, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        xp = [C.c_void_p(t.data_ptr()) for t in xin]
        yp = C.c_void_p(yout.data_ptr())
    h = b._h
    b.prepare(BLOCK, True)                       # the code for 32-sample blocks (and the variant with the controls in rows) before the stream starts
    key = control.encode()

    def block(k):
        if k % SLIDER_EVERY == 0:
            rc = lib.fxb_set_register(h, key, C.c_float(SLIDER[(k // SLIDER_EVERY) % len(SLIDER)]))
            assert rc == 0, rc
        if mode == "host":
            rc = lib.fxb_process_block(h, xp[k % RING], yp, BLOCK)
        else:
            rc = lib.fxb_process_block_dev(h, xp[k % RING], yp, BLOCK, None)
            rc = rc or lib.fxb_sync(h)
        if rc != 0:
            raise RuntimeError("block %d failed (%d): %s" % (k, rc, b.last_error()))

    for k in range(warm):                        # first control touch, the tuner's trials, clocks
        block(k)
    b.prepare(BLOCK, True)
    builds0 = (b.info("xlate_builds"), b.info("xlate_background_builds"))
    times, kernel = [], []
    gc.collect()
    gc.disable()
    try:
        t_start = time.perf_counter()
        for k in range(warm, warm + blocks):
            t0 = time.perf_counter_ns()
            block(k)                             # (the slider write of every 8th block is inside the block's time: it is the caller's)
            times.append((time.perf_counter_ns() - t0) * 1e-3)
            if k % 64 == 0:
                kernel.append(b.last_kernel_ms() * 1e3)
        wall = time.perf_counter() - t_start
    finally:
        gc.enable()
    builds1 = (b.info("xlate_builds"), b.info("xlate_background_builds"))
    total = warm + blocks
    y_last = (yout.numpy() if mode == "host" else yout.cpu().numpy()).copy()
    # parity: the oracle replays every block of the run for sampled instances
    picks = sorted(set([0, min(63, n - 1), n // 2, n - 1]))[:check]
    ok = True
    for inst in picks:
        o = Oracle(1)
        assert o.load_text(text)
        ref = None
        cols = [np.ascontiguousarray(r[:, inst]) for r in ring]
        for k in range(total):
            if k % SLIDER_EVERY == 0:
                o.set_register(control, SLIDER[(k // SLIDER_EVERY) % len(SLIDER)])
            ref = o.process_block(cols[k % RING])
        ok = ok and bool(np.array_equal(ref.view(np.uint32), np.ascontiguousarray(y_last[:, inst]).view(np.uint32)))
        ok = ok and b.instruction_counter_i(inst) == o.instruction_counter()
    res = percentiles(times)
    kk = sorted(v for v in kernel if v > 0)
    # what the slider costs: the blocks that start with a control write beside the others
    moved = [t for k, t in zip(range(warm, total), times) if k % SLIDER_EVERY == 0]
    plain = [t for k, t in zip(range(warm, total), times) if k % SLIDER_EVERY != 0]
    if moved and plain:
        pm, pp = percentiles(moved), percentiles(plain)
        res.update({"control_blocks": {"median_us": pm["median_us"], "p99_us": pm["p99_us"], "max_us": pm["max_us"], "blocks": pm["blocks"]},
                    "other_blocks": {"median_us": pp["median_us"], "p99_us": pp["p99_us"], "p999_us": pp["p999_us"], "max_us": pp["max_us"], "blocks": pp["blocks"]}})
    res.update({
        "instances": n, "mode": mode, "shards_on_the_gpu": shards, "budget_us": round(BUDGET_US, 3), "within_budget_p999": res["p999_us"] <= BUDGET_US,
        "kernel_us_median": round(kk[len(kk) // 2], 1) if kk else None,
        "pcie_GBps_each_way_at_median": round(BLOCK * n * 4 / (res["median_us"] * 1e-6) / 1e9, 2) if mode == "host" else None,
        "realtime_factor_at_median": round(BUDGET_US / res["median_us"], 2),
        "emulated_mips_sustained": round(progs.count_instructions(text) * BLOCK * n * blocks / wall / 1e6, 1),
        "translations_in_timed_region": [builds1[0] - builds0[0], builds1[1] - builds0[1]],
        "tier": b.tier_note(), "parity_instances": len(picks), "parity_ok": ok, "blocks_replayed_by_oracle": total,
        # host blocks by route, summed over the shards (FXB_INFO_HOST_STAGED_BLOCKS / _INPLACE_BLOCKS): 0 staged on pinned buffers
        "host_staged_blocks": b.info("host_staged_blocks"), "host_inplace_blocks": b.info("host_inplace_blocks"),
    })
    b.close()
    del xin, yout
    if mode == "device":
        torch.cuda.empty_cache()
    return res


def capacity(rows):
    """largest N such that it AND every smaller N measured keep their p99.9 block time within the budget (None when even the
    smallest does not): a lucky row above a failing one does not count"""
    best = None
    for r in sorted(rows, key=lambda r: r["instances"]):
        if not (r["within_budget_p999"] and r["parity_ok"]):
            break
        best = r["instances"]
    return best


def run(torch, A, progs, instances, blocks, warm, modes=("host", "device"), log=None, shards=1):
    out = {"what": "32-sample blocks at 48 kHz against %.3f us (the reference's own real-time measure, source/main.cpp:99-155); program config5 (512 instructions, "
                   "8192-sample xTRAM); control `decay` takes 0.1 / 0.25 / 0.5 / 1.0 in turn, one step every 8th block; times are call -> output in host memory "
                   "(host mode, pinned buffers) or call -> fxb_sync (device mode), on the caller's clock" % BUDGET_US,
           "budget_us": round(BUDGET_US, 3), "block_samples": BLOCK, "blocks_per_point": blocks, "warmup_blocks": warm, "rows": []}
    for mode in modes:
        for n in instances:
            r = measure(torch, A, progs, n, blocks, warm, mode, shards=shards if mode == "host" else 1)
            out["rows"].append(r)
            if log:
                log(("%d shards " % shards if shards > 1 and mode == "host" else "") + "%-6s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  kernel %6.1f us  %s  parity %s" % (
                    mode, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], r["kernel_us_median"] or -1,
                    "REAL TIME" if r["within_budget_p999"] else "over budget", "ok" if r["parity_ok"] else "MISMATCH")
                    + ("  staged %d in place %d" % (r["host_staged_blocks"], r["host_inplace_blocks"]) if mode == "host" else "")
                    + ("  (blocks that move the slider: median %.1f, the others %.1f, p99.9 %.1f)" % (
                        r["control_blocks"]["median_us"], r["other_blocks"]["median_us"], r["other_blocks"]["p999_us"]) if "control_blocks" in r else ""))
        out["capacity_%s_fed" % mode] = capacity([r for r in out["rows"] if r["mode"] == mode])
    return out


REGISTER_KEYS = ("damp", "decay", "diff", "u")   # config5: its three declared controls and a state register
REGISTER_LIST, REGISTER_SINGLES = 1024, 64


def register_paths(torch, A, progs, n, blocks, warm, stretch, log, clock=lambda: None, only=None):
    """--register-list: 32-sample blocks of config5 from pinned host buffers, four handles by turns in stretches in one process:
    no register writes; fxb_set_registers_list of 1 024 instances x 4 registers in front of every block; fxb_set_register_array of
    the same 4 registers; fxb_set_register_i for 64 x 4 values (the smaller count: a call waits for the queued blocks and copies
    four bytes).  The writes are inside the block's time.  All four handles hold per-instance values of the four registers from
    the start, so all four run the same code (a handle whose controls are folded into the code runs faster code: that would be
    another comparison).  only: the one path of a profiler run."""
    import numpy as np

    text = progs.config5()
    lib = A.load()
    names = ("none", "list %d" % REGISTER_LIST, "array", "single %d" % REGISTER_SINGLES)
    paths = []
    rng = np.random.default_rng(5)
    keys = (C.c_char_p * len(REGISTER_KEYS))(*[k.encode() for k in REGISTER_KEYS])
    ring = [progs.stimulus(n, BLOCK, first_sample=k * BLOCK) for k in range(RING)]
    xin = [torch.empty((BLOCK, n), dtype=torch.float32).pin_memory() for _ in range(RING)]
    for t, r in zip(xin, ring):
        t.numpy()[...] = r
    xp = [C.cast(t.data_ptr(), C.POINTER(C.c_float)) for t in xin]
    for name in names:
        if only and name.split()[0] != only:
            continue
        b = A.Batch(n, 1, 0)
        if not b.load_text(text):
            raise RuntimeError("load failed: %s" % b.errors())
        rows = rng.uniform(0.1, 0.4, (len(REGISTER_KEYS), n)).astype(np.float32)
        rows[3] *= np.float32(0.01)
        for k, key in enumerate(REGISTER_KEYS):
            assert b.set_register_array(key, rows[k]) == 0
        b.prepare(BLOCK, True)
        yout = torch.empty((BLOCK, n), dtype=torch.float32).pin_memory()
        # the moved voices: spread over the instances, other ones in every block of a ring of lists
        lists = [np.ascontiguousarray(rng.permutation(n)[:REGISTER_LIST].astype(np.int64)) for _ in range(RING)]
        values = [np.ascontiguousarray(rows[:, L]) for L in lists]
        paths.append({"name": name, "b": b, "rows": rows, "yout": yout, "yp": C.cast(yout.data_ptr(), C.POINTER(C.c_float)), "lists": lists, "values": values, "times": [], "clocks": [], "k": 0})

    def block(p, timed):
        b, k, h = p["b"], p["k"], p["b"]._h
        p["k"] += 1
        L, v = p["lists"][k % RING], p["values"][k % RING]
        t0 = time.perf_counter_ns()
        kind = p["name"].split()[0]
        if kind == "list":
            rc = lib.fxb_set_registers_list(h, keys, len(REGISTER_KEYS), C.c_void_p(L.ctypes.data), REGISTER_LIST, C.c_void_p(v.ctypes.data))
            assert rc == 0, (rc, b.last_error())
        elif kind == "array":
            for j, key in enumerate(REGISTER_KEYS):
                rc = lib.fxb_set_register_array(h, key.encode(), C.c_void_p(p["rows"][j].ctypes.data))
                assert rc == 0, rc
        elif kind == "single":
            for j, key in enumerate(REGISTER_KEYS):
                name = key.encode()
                for i in range(REGISTER_SINGLES):
                    lib.fxb_set_register_i(h, name, int(L[i]), C.c_float(float(v[j, i])))
        rc = lib.fxb_process_block(h, xp[k % RING], p["yp"], BLOCK)
        if rc != 0:
            raise RuntimeError("block %d failed (%d): %s" % (k, rc, b.last_error()))
        if timed:
            p["times"].append((time.perf_counter_ns() - t0) * 1e-3)

    for p in paths:
        for _ in range(warm):
            block(p, False)
        p["b"].prepare(BLOCK, True)
        p["builds"] = (p["b"].info("xlate_builds"), p["b"].info("xlate_background_builds"))
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for p in paths:   # by turns: what else happens on the host and the device meets all of them
                for _ in range(stretch):
                    block(p, True)
                p["clocks"].append(clock())   # (one reading right behind the stretch's last block, outside every timed block)
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "rows": []}
    for p in paths:
        b = p["b"]
        r = percentiles(p["times"])
        mhz = [c for c in p["clocks"] if c]
        r.update({"path": p["name"], "instances": n, "within_budget_p999": r["p999_us"] <= BUDGET_US, "shader_clock_mhz_behind_a_stretch": round(sum(mhz) / len(mhz), 1) if mhz else None,
                  "register_list_sets": b.info("register_list_sets"), "tier": b.tier_note(),
                  "translations_in_timed_region": [b.info("xlate_builds") - p["builds"][0], b.info("xlate_background_builds") - p["builds"][1]]})
        out["rows"].append(r)
        log("%-11s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  %d list sets  translations in the timed region %s  shader clock %s MHz" % (
            p["name"], n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["within_budget_p999"] else "over budget", r["register_list_sets"],
            r["translations_in_timed_region"], r["shader_clock_mhz_behind_a_stretch"]))
        b.close()
    return out


TRACK_KEY, TRACK_LIST, TRACK_STEPS, TRACK_PERIOD = "decay", 1024, 4, 8


def track_paths(torch, A, progs, n, blocks, warm, stretch, log, only=None):
    """--track-list: 32-sample blocks of config5 from pinned host buffers, four handles by turns in stretches in one process: no
    schedule; a list schedule of 1 024 voices x 1 register x 4 steps (period 8) armed in front of every block; the same schedule
    as a dense per_instance track (fxb_set_register_track, 4 x N floats - the rows are ready-made: the host's work of knowing
    every voice's value is not in the timed region); the block cut in four with fxb_set_registers_list at the cuts.  The arming
    is inside the block's time.  All four handles have the register trackable from the start, so all four run the same code.
    only: the one path of a profiler run."""
    import numpy as np

    text = progs.config5()
    lib = A.load()
    names = ("none", "list %d" % TRACK_LIST, "dense", "cut")
    paths = []
    rng = np.random.default_rng(7)
    keys = (C.c_char_p * 1)(TRACK_KEY.encode())
    ring = [progs.stimulus(n, BLOCK, first_sample=k * BLOCK) for k in range(RING)]
    xin = [torch.empty((BLOCK, n), dtype=torch.float32).pin_memory() for _ in range(RING)]
    for t, r in zip(xin, ring):
        t.numpy()[...] = r
    piece = BLOCK // TRACK_STEPS
    assert piece == TRACK_PERIOD
    for name in names:
        if only and name.split()[0] != only:
            continue
        b = A.Batch(n, 1, 0)
        if not b.load_text(text):
            raise RuntimeError("load failed: %s" % b.errors())
        row = rng.uniform(0.1, 0.4, n).astype(np.float32)
        assert b.set_register_array(TRACK_KEY, row) == 0
        # trackable from the start: a schedule with nothing due inside any block
        assert b.set_register_tracks_list([TRACK_KEY], [0], np.zeros((1, 1, 1), dtype=np.float32), first=1 << 20) == 0
        b.process_block(ring[0])
        b.prepare(BLOCK, True)
        b.prepare(piece, True)
        yout = torch.empty((BLOCK, n), dtype=torch.float32).pin_memory()
        lists = [np.ascontiguousarray(rng.permutation(n)[:TRACK_LIST].astype(np.int64)) for _ in range(RING)]
        values = [np.ascontiguousarray(rng.uniform(0.1, 0.4, (TRACK_STEPS, 1, TRACK_LIST)).astype(np.float32)) for _ in range(RING)]
        dense = None
        if name == "dense":
            dense = []
            for L, v in zip(lists, values):
                d = np.tile(row, (TRACK_STEPS, 1))
                d[:, L] = v[:, 0, :]
                dense.append(np.ascontiguousarray(d))
        paths.append({"name": name, "b": b, "yout": yout, "lists": lists, "values": values, "dense": dense, "times": [], "k": 0})

    def fptr(t, sample=0):
        return C.cast(t.data_ptr() + sample * n * 4, C.POINTER(C.c_float))

    def block(p, timed):
        b, k, h = p["b"], p["k"], p["b"]._h
        p["k"] += 1
        L, v = p["lists"][k % RING], p["values"][k % RING]
        x, y = xin[k % RING], p["yout"]
        t0 = time.perf_counter_ns()
        kind = p["name"].split()[0]
        if kind == "cut":
            for q in range(TRACK_STEPS):
                rc = lib.fxb_set_registers_list(h, keys, 1, C.c_void_p(L.ctypes.data), TRACK_LIST, C.c_void_p(v[q].ctypes.data))
                assert rc == 0, (rc, b.last_error())
                rc = lib.fxb_process_block(h, fptr(x, q * piece), fptr(y, q * piece), piece)
                assert rc == 0, (rc, b.last_error())
        else:
            if kind == "list":
                rc = lib.fxb_set_register_tracks_list(h, keys, 1, C.c_void_p(L.ctypes.data), TRACK_LIST, C.c_void_p(v.ctypes.data), TRACK_STEPS, 0, TRACK_PERIOD)
                assert rc == 0, (rc, b.last_error())
            elif kind == "dense":
                rc = lib.fxb_set_register_track(h, TRACK_KEY.encode(), C.c_void_p(p["dense"][k % RING].ctypes.data), TRACK_STEPS, TRACK_PERIOD, 1)
                assert rc == 0, (rc, b.last_error())
            rc = lib.fxb_process_block(h, fptr(x), fptr(y), BLOCK)
            if rc != 0:
                raise RuntimeError("block %d failed (%d): %s" % (k, rc, b.last_error()))
        if timed:
            p["times"].append((time.perf_counter_ns() - t0) * 1e-3)

    for p in paths:
        for _ in range(warm):
            block(p, False)
        p["b"].prepare(BLOCK, True)
        p["builds"] = (p["b"].info("xlate_builds"), p["b"].info("xlate_background_builds"))
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for p in paths:
                for _ in range(stretch):
                    block(p, True)
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "rows": []}
    for p in paths:
        b = p["b"]
        r = percentiles(p["times"])
        r.update({"path": p["name"], "instances": n, "within_budget_p999": r["p999_us"] <= BUDGET_US, "track_list_expands": b.info("track_list_expands"), "tier": b.tier_note(),
                  "code_hash": b.info("xlate_code_hash"), "translations_in_timed_region": [b.info("xlate_builds") - p["builds"][0], b.info("xlate_background_builds") - p["builds"][1]]})
        out["rows"].append(r)
        log("%-10s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  %d expansions  translations in the timed region %s  code %016x" % (
            p["name"], n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["within_budget_p999"] else "over budget", r["track_list_expands"],
            r["translations_in_timed_region"], r["code_hash"] & 0xffffffffffffffff))
        b.close()
    return out


def track_main(args, torch, A, progs):
    lines = []

    def keep(s):
        print(s, flush=True)
        lines.append(s)

    if args.trace_run:   # under rocprofv3 --kernel-trace --stats: the list path alone, a run of its own
        track_paths(torch, A, progs, args.trace_instances, 200, 50, 200, keep, only="list")
        return
    keep("32-sample blocks of config5 (pinned host buffers, fxb_process_block) against %.3f us: no schedule; fxb_set_register_tracks_list of %d voices x 1 register (%s) x %d steps, "
         "period %d; the same schedule through fxb_set_register_track(per_instance = 1); the block cut in %d with fxb_set_registers_list at the cuts - armed in front of every "
         "block, inside the timed region, by turns in stretches of %d blocks in one process, %d blocks per point after %d warm-up blocks; the register is trackable on all "
         "four handles; %s" % (BUDGET_US, TRACK_LIST, TRACK_KEY, TRACK_STEPS, TRACK_PERIOD, TRACK_STEPS, args.stretch, args.blocks, args.warmup, torch.cuda.get_device_name(0)))
    out = [track_paths(torch, A, progs, n, args.blocks, args.warmup, args.stretch, keep) for n in [int(v) for v in args.register_instances.split(",") if v]]
    for point in out:
        med = {r["path"].split()[0]: r["median_us"] for r in point["rows"]}
        keep("           N=%7d  median over no schedule: list %+.1f us, dense %+.1f us, cut %+.1f us" % (point["instances"], med["list"] - med["none"], med["dense"] - med["none"], med["cut"] - med["none"]))
    if args.track_out:
        with open(args.track_out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


def register_main(args, torch, A, progs):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bus_capacity import shader_clock_reader
    lines = []

    def keep(s):
        print(s, flush=True)
        lines.append(s)

    if args.trace_run:   # under rocprofv3 --kernel-trace --stats: the list path alone, a run of its own
        register_paths(torch, A, progs, args.trace_instances, 200, 50, 200, keep, only="list")
        return
    keep("32-sample blocks of config5 (pinned host buffers, fxb_process_block) against %.3f us: no register writes; fxb_set_registers_list of %d instances x %d registers "
         "(%s); fxb_set_register_array of the same registers; fxb_set_register_i for %d x %d values - in front of every block, inside the timed region, by turns in stretches "
         "of %d blocks in one process, %d blocks per point after %d warm-up blocks; %s" % (
             BUDGET_US, REGISTER_LIST, len(REGISTER_KEYS), ", ".join(REGISTER_KEYS), REGISTER_SINGLES, len(REGISTER_KEYS), args.stretch, args.blocks, args.warmup,
             torch.cuda.get_device_name(0)))
    out = [register_paths(torch, A, progs, n, args.blocks, args.warmup, args.stretch, keep, shader_clock_reader(torch)) for n in [int(v) for v in args.register_instances.split(",") if v]]
    for point in out:
        med = {r["path"].split()[0]: r["median_us"] for r in point["rows"]}
        keep("            N=%7d  median over no writes: list %+.1f us, array %+.1f us, single %+.1f us" % (point["instances"], med["list"] - med["none"], med["array"] - med["none"], med["single"] - med["none"]))
    if args.register_out:
        with open(args.register_out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--register-list", action="store_true", help="the four register-write paths by turns (register_paths) instead of the capacity sweep")
    ap.add_argument("--track-list", action="store_true", help="no schedule / list schedule / dense per-instance track / cut block by turns (track_paths) instead of the capacity sweep")
    ap.add_argument("--track-out", default="", help="keep the lines of --track-list in this text file")
    ap.add_argument("--register-instances", default="131072,458752")
    ap.add_argument("--register-out", default="", help="keep the lines of --register-list in this text file")
    ap.add_argument("--stretch", type=int, default=250, help="--register-list: blocks of one path before the next takes its turn")
    ap.add_argument("--trace-run", action="store_true", help="--register-list: 200 blocks of the list path alone, for a profiler run of its own")
    ap.add_argument("--trace-instances", type=int, default=458752)
    ap.add_argument("--blocks", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--instances", default="4096,16384,65536,98304,131072,147456,163840,180224,196608")
    ap.add_argument("--device-instances", default="", help="instance counts of the device-resident rows (default: 4096 ... 589824)")
    ap.add_argument("--shards", default="1", help="host-fed rows: shards on the one GPU, e.g. 1,4 (every value is a sweep of its own)")
    ap.add_argument("--no-device", action="store_true", help="skip the device-resident rows")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch  # first: its HIP runtime is the one the library binds to

    import fx8010_amd as A
    import fx8010_programs as progs
    if args.register_list:
        return register_main(args, torch, A, progs)
    if args.track_list:
        return track_main(args, torch, A, progs)
    inst = [int(v) for v in args.instances.split(",") if v]
    dev_inst = [int(v) for v in args.device_instances.split(",") if v] or [4096, 65536, 131072, 262144, 393216, 458752, 524288, 557056, 589824]
    log = lambda s: print(s, flush=True)
    out = None
    for k in [int(v) for v in args.shards.split(",") if v]:
        part = run(torch, A, progs, inst, args.blocks, args.warmup, ("host",), log, shards=k)
        part["capacity_host_fed_by_shards"] = {str(k): part["capacity_host_fed"]}
        if out is None:
            out = part
        else:
            out["rows"] += part["rows"]
            out["capacity_host_fed_by_shards"][str(k)] = part["capacity_host_fed"]
            out["capacity_host_fed"] = max([v for v in out["capacity_host_fed_by_shards"].values() if v] or [None], key=lambda v: v or 0)
    out["capacity_device_fed"] = None
    if not args.no_device:
        dev = run(torch, A, progs, dev_inst, args.blocks, args.warmup, ("device",), log)
        out["rows"] += dev["rows"]
        out["capacity_device_fed"] = dev["capacity_device_fed"]
    out["gpu"] = torch.cuda.get_device_name(0)
    print("largest N within %.3f us at p99.9: host-fed %s, device-resident PCM %s" % (BUDGET_US, out["capacity_host_fed"], out["capacity_device_fed"]))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
