#!/usr/bin/env python3
"""What a group bus buys a real-time host: 32-sample blocks of config5 from pinned host buffers, the plain in-place
fxb_process_block ([32][N] in and out over PCIe) beside fxb_process_block_bus with a shared input and a mixed output per group
of 64 instances ([32][N / 64] in and out over PCIe; an expand and a mix kernel around the unchanged emulation launch).

1. The condition: at 131 072 instances, stretches of blocks of the two paths take turns in ONE process on ONE build; the bus
   path's median block time must not exceed the plain path's.  It moves 1/64 of the PCIe bytes and adds two passes over the
   16.8 MB per-instance block in device memory: if it is slower, the bus kernels are at fault.  The exit status is 1 then.
2. Capacity: the instance count goes up for the bus path; the largest count whose p99.9 block time (and every smaller count's)
   stays inside 666.667 us is reported beside the plain path's, measured by tools/realtime_capacity.py's own routine.
3. `--trace-run`: nothing is timed, a stretch of bus blocks at --trace-instances runs - the program to put behind
   `rocprofv3 --kernel-trace --stats ... --` in a run of its own, without counters.  `--kernel-stats FILE.csv` then reads the
   table that run wrote: the expand and mix kernels' share of device time, and their achieved bytes/s (the bytes the two must
   move, from the shapes) against the 6.3 TB/s an MI355X's HBM gives a streaming kernel.

4. `--meter`: what the output meters (fxb_meter_enable) cost a real-time host.  At every count of --meter-instances two bus
   handles, meters off and meters on, take turns in stretches in ONE process; median and p99.9 of both are reported with the
   shader clock behind their stretches (`--meter-out FILE.txt` keeps the lines).  Their outputs must stay equal word for word.
   With `--trace-run --meter` the traced stretch runs with meters on, and `--kernel-stats` then also reports the meter kernel
   beside the mix kernel, which reads the same per-instance block.

5. `--gains`: what the per-instance mix gains (fxb_bus_set_gains) cost a real-time host.  At every count of --gain-instances three
   bus handles take turns in stretches in ONE process: gains off (the plain mix kernel), static gains, and a ramp on every block
   (a set with ramp = 1 in front of every block, inside the timed region: it is what a mixer host with moving faders pays).
   Median and p99.9 of the three are reported (`--gains-out FILE.txt` keeps the lines).  Before anything is timed, gains of 1.0f
   must give the words of gains off.  With `--trace-run --gains` the traced run is the same three handles by turns, 200 blocks
   each, and `--kernel-stats` reports fx_bus_mix_gain (static and ramping) beside fx_bus_mix.

6. `--taps T`: what bus taps (fxb_bus_set_taps, fxb_process_block_bus_tap) cost a real-time host.  At every count of
   --tap-instances two bus handles, untapped and with T instances tapped into a pinned [32][T] side, take turns in stretches in
   ONE process; median and p99.9 of both are reported (`--taps-out FILE.txt` keeps the lines).  Before anything is timed the tap
   words must be the plain path's columns, and the two mixes must stay equal word for word.  With `--trace-run --taps T` the
   traced stretch runs tapped and with meters on - fx_meter, which reads the whole per-instance block, is the yardstick in the same
   trace - and `--kernel-stats` then reports fx_bus_tap beside it.

7. `--sends A`: what bus sends (fxb_bus_set_sends, fxb_process_block_bus_aux) cost a real-time host.  Every instance is a member
   of each of A aux buses (ascending lists, weights of their own), delivered to a pinned [32][A] side.  At every count of
   --send-instances two bus handles, without sends and with them, take turns in stretches in ONE process; median and p99.9 of
   both are reported (`--sends-out FILE.txt` keeps the lines).  Before anything is timed the aux words must be the definition of
   include/fx8010_amd.h applied to the plain path's output, and the two mixes must stay equal word for word.  With `--trace-run
   --gains --sends A` the traced stretch is 200 blocks of one handle with static bus gains and the sends - fx_bus_mix_gain, which
   moves 8 bytes per member where the sends move 12, is the yardstick in the same trace - and `--kernel-stats` then reports
   fx_bus_send_chunks and fx_bus_send_fold beside it.

9. `--gains --gains-list K`: a fourth path beside "gains off / static / ramping": a list set of K faders with ramp = 1
   (fxb_bus_set_gains_list) in front of every block, inside the timed region - the K faders are spread over the instances and
   alternate between two levels.  It is what a mixer host pays that moves K faders where "ramping" re-sends all N.  With
   `--trace-run --gains --gains-list K` the traced run is the four handles by turns; fx_gain_scatter then stands beside
   fx_bus_mix_gain in the table.  `--sends A --send-gains-list K` is the same for the send gains: a third path, sends with a list
   set of K entries (fxb_bus_set_send_gains_list, ramp = 1) in front of every block.

Every path slides the control `decay` like the reference's harness does (realtime_capacity.py); before anything is timed the bus
path's output is compared word for word with the summation order include/fx8010_amd.h fixes, applied to the plain path's output.

    python tools/bus_capacity.py [--blocks 4000] [--json profiles/bus_realtime.json] [--kernel-stats bus_kernel_stats.csv]
8. `--feeds F`: what bus feeds (fxb_bus_set_feeds, fxb_process_block_bus_feed) cost against the shared input they generalise.
   F = 1 is the map n / group, unweighted - the words of FXB_BUS_SHARED_IN, checked before anything is timed -, F >= 2 a CSR
   structure of F weighted entries per instance.  At each of --feed-instances a handle with the shared input and one with feeds
   take turns in stretches in ONE process; median and p99.9 of both are reported (`--feeds-out FILE.txt` keeps the lines).  With
   `--trace-run --feeds F` the traced stretch is 200 blocks of each handle: fx_bus_expand, which writes the same bytes, is the
   yardstick of fx_bus_feed in the same trace.
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
GROUP = 64
HBM_ACHIEVABLE_BPS = 6.3e12


def mix_model(y, K):
    """[..., N] -> [..., G] in the order include/fx8010_amd.h fixes (K <= 64 here: one member per lane, then the tree)"""
    import numpy as np
    N = y.shape[-1]
    assert K <= 64 and N % K == 0
    p = np.zeros(y.shape[:-1] + (N // K, 64), dtype=np.float32)
    p[..., :K] = p[..., :K] + y.reshape(y.shape[:-1] + (N // K, K))
    for step in (32, 16, 8, 4, 2, 1):
        p[..., :step] = p[..., :step] + p[..., step:2 * step]
    return p[..., 0]


def tree_model(v):
    """[..., L] -> [...]: T of include/fx8010_amd.h "Bus sends" (64 partial sums over j ascending, then the shuffle-down tree)"""
    import numpy as np
    L = v.shape[-1]
    p = np.zeros(v.shape[:-1] + (64,), dtype=np.float32)
    for j in range(-(-L // 64)):
        w = min(64, L - j * 64)
        p[..., :w] = p[..., :w] + v[..., j * 64:j * 64 + w]
    for step in (32, 16, 8, 4, 2, 1):
        p[..., :step] = p[..., :step] + p[..., step:2 * step]
    return p[..., 0]


def send_all_model(y, w):
    """y [S, 1, n], w [A, n] (static weights, none of them zero) -> [S, 1, A]: every instance on each bus, ascending"""
    import numpy as np
    n = y.shape[-1]
    assert n % 1024 == 0 and n > 1024
    term = (w[None, :, :] * y[:, 0, None, :]).astype(np.float32)                       # [S, A, n]
    chunks = tree_model(term.reshape(term.shape[:2] + (n // 1024, 1024)))             # [S, A, Q]
    return np.ascontiguousarray(tree_model(chunks)[:, None, :])


class Path:
    """one handle and its pinned buffers; block(k) is one synchronous call on the caller's clock"""

    def __init__(self, A, progs, n, bus, meter=False, gains=None, taps=0, sends=0, feeds=0, gains_list=0, send_gains_list=0):
        import numpy as np
        self.A, self.n, self.bus, self.lib = A, n, bus, A.load()
        self.b = A.Batch(n, 1, 0)
        if not self.b.load_text(progs.CONFIGS["config5"]()):
            raise RuntimeError("load failed: %s" % self.b.errors())
        self.width = self.b.bus_groups(GROUP) if bus else n
        self.ring = [A.HostBuffer((BLOCK, 1, self.width)) for _ in range(RING)]
        for k, h in enumerate(self.ring):
            g = progs.stimulus(self.b.bus_groups(GROUP), BLOCK, first_sample=k * BLOCK)
            h.array[:, 0, :] = g if bus else np.repeat(g, GROUP, axis=1)[:, :n]
        self.out = A.HostBuffer((BLOCK, 1, self.width))
        self.xp = [C.c_void_p(h.array.ctypes.data) for h in self.ring]
        self.yp = C.c_void_p(self.out.array.ctypes.data)
        if meter:
            self.b.meter_enable()
        # gains: None = off, "static" = set once, "ramp" = a set with ramp = 1 in front of every block, between two sets of levels,
        # "list" = a list set of gains_list faders with ramp = 1 in front of every block, the faders between the same two levels
        self.gains = gains
        if gains:
            level = (0.25 + 0.75 * (progs.stimulus(n, 1, seed=99)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32)
            self.levels = [np.ascontiguousarray(level.reshape(1, n)), np.ascontiguousarray((np.float32(1.25) - level).reshape(1, n))]
            self.lp = [C.c_void_p(g.ctypes.data) for g in self.levels]
            self.b.bus_set_gains(self.levels[0])
            if gains == "list":
                self.fader, self.fader_levels, self.fp = self.fader_list(n, gains_list, self.levels)
        # taps: T instances spread over the batch (the first and the last among them), delivered to a pinned [BLOCK][T] side
        self.taps, self.tap_list, self.tp = taps, None, None
        if taps:
            self.tap_list = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(5).integers(0, n, max(taps - 2, 0))]))[:taps].astype(np.int64)
            while self.tap_list.size < taps:   # (draws that met: top up with repeats)
                self.tap_list = np.concatenate([self.tap_list, self.tap_list[:taps - self.tap_list.size]])
            self.tap_list = np.ascontiguousarray(np.random.default_rng(6).permutation(self.tap_list))
            self.b.bus_set_taps(self.tap_list)
            self.tap_out = A.HostBuffer((BLOCK, 1, taps))
            self.tp = C.c_void_p(self.tap_out.array.ctypes.data)
        # sends: every instance on each of `sends` aux buses, ascending, bus a with weights of its own; a pinned [BLOCK][sends] side
        self.sends, self.ap = sends, None
        if sends:
            base = (0.25 + 0.75 * (progs.stimulus(n, 1, seed=77)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32)
            self.send_gains = np.ascontiguousarray(np.stack([np.roll(base, 17 * a) for a in range(sends)]))   # [A, n] = [1][E]
            self.b.bus_set_sends(np.arange(sends + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int64), sends), self.send_gains.reshape(1, -1))
            self.aux_out = A.HostBuffer((BLOCK, 1, sends))
            self.ap = C.c_void_p(self.aux_out.array.ctypes.data)
            self.send_gains_list = send_gains_list
            if send_gains_list:
                flat = np.ascontiguousarray(self.send_gains.reshape(1, -1))
                self.send_fader, self.send_fader_levels, self.sfp = self.fader_list(flat.shape[1], send_gains_list, [flat, np.ascontiguousarray(np.float32(1.25) - flat)])
        # feeds: the input block [BLOCK][G] is the source block.  1: the map n / GROUP, unweighted - the words of the shared input;
        # F >= 2: CSR, every instance hears F columns (its own group's first) with weights of its own
        self.feeds = feeds
        if feeds:
            G = self.width
            own = np.arange(n, dtype=np.int64) // GROUP
            if feeds == 1:
                self.b.bus_set_feeds(G, np.arange(n + 1, dtype=np.int64), own)
            else:
                src = np.ascontiguousarray(np.stack([(own + 7 * k) % G for k in range(feeds)], axis=1).reshape(-1))
                w = (0.25 + 0.75 * (progs.stimulus(n * feeds, 1, seed=55)[0] * np.float32(0.5) + np.float32(0.5))).astype(np.float32) / np.float32(feeds)
                self.feed_sources, self.feed_gains = src, np.ascontiguousarray(w.reshape(1, -1))
                self.b.bus_set_feeds(G, np.arange(n + 1, dtype=np.int64) * feeds, src, self.feed_gains)
        self.b.prepare(BLOCK, True)
        self.k = 0
        self.times = []

    @staticmethod
    def fader_list(width, count, levels):
        """`count` indices spread over 0..width-1, their columns of the two sets of levels, and the pointers of all three"""
        import numpy as np
        if not 0 < count <= width:
            raise RuntimeError("a list of %d faders out of %d" % (count, width))
        idx = np.ascontiguousarray((np.arange(count, dtype=np.int64) * width) // count)
        vals = [np.ascontiguousarray(level[:, idx]) for level in levels]
        return idx, vals, [C.c_void_p(idx.ctypes.data)] + [C.c_void_p(v.ctypes.data) for v in vals]

    def block(self):
        k, h = self.k, self.b._h
        if k % SLIDER_EVERY == 0:
            assert self.lib.fxb_set_register(h, b"decay", C.c_float(SLIDER[(k // SLIDER_EVERY) % len(SLIDER)])) == 0
        if self.gains == "ramp" and self.lib.fxb_bus_set_gains(h, self.lp[(k + 1) % 2], 1) != 0:
            raise RuntimeError("set_gains in front of block %d failed: %s" % (k, self.b.last_error()))
        if self.gains == "list" and self.lib.fxb_bus_set_gains_list(h, self.fp[0], self.fader.size, self.fp[1 + (k + 1) % 2], 1) != 0:
            raise RuntimeError("set_gains_list in front of block %d failed: %s" % (k, self.b.last_error()))
        if self.sends and self.send_gains_list and self.lib.fxb_bus_set_send_gains_list(h, self.sfp[0], self.send_fader.size, self.sfp[1 + (k + 1) % 2], 1) != 0:
            raise RuntimeError("set_send_gains_list in front of block %d failed: %s" % (k, self.b.last_error()))
        if self.feeds:
            rc = self.lib.fxb_process_block_bus_feed(h, self.xp[k % RING], self.yp, None, None, BLOCK, GROUP, 2)
        elif self.sends:
            rc = self.lib.fxb_process_block_bus_aux(h, self.xp[k % RING], self.yp, self.tp, self.ap, BLOCK, GROUP, 3)
        elif self.taps:
            rc = self.lib.fxb_process_block_bus_tap(h, self.xp[k % RING], self.yp, self.tp, BLOCK, GROUP, 3)
        elif self.bus:
            rc = self.lib.fxb_process_block_bus(h, self.xp[k % RING], self.yp, BLOCK, GROUP, 3)
        else:
            rc = self.lib.fxb_process_block_pitched(h, self.xp[k % RING], self.yp, BLOCK, self.n)
        if rc != 0:
            raise RuntimeError("block %d failed (%d): %s" % (k, rc, self.b.last_error()))
        self.k = k + 1

    def stretch(self, blocks, timed=True):
        for _ in range(blocks):
            t0 = time.perf_counter_ns()
            self.block()
            if timed:
                self.times.append((time.perf_counter_ns() - t0) * 1e-3)

    def close(self):
        self.b.close()
        for h in self.ring + [self.out] + ([self.tap_out] if self.taps else []) + ([self.aux_out] if self.sends else []):
            h.close()


def check_words(A, progs, n):
    """two blocks on fresh handles: the bus path's words are the model's, applied to the plain path's"""
    import numpy as np
    plain, bus = Path(A, progs, n, False), Path(A, progs, n, True)
    for _ in range(2):
        plain.block()
        bus.block()
        want, got = mix_model(plain.out.array, GROUP), bus.out.array
        nan = np.isnan(want)
        if not ((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()):
            raise RuntimeError("the bus path's output differs from the model of the plain path's at %d instances" % n)
    plain.close()
    bus.close()


def shader_clock_reader(torch):
    """-> a function that reads the shader clock of device 0 in MHz from the amdgpu hwmon file of its PCI address (None where
    that file cannot be found: the clock is extra information)"""
    import glob
    path = None
    try:
        p = torch.cuda.get_device_properties(0)
        bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        for d in glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*" % bdf):
            if os.path.exists(os.path.join(d, "freq1_input")):
                path = os.path.join(d, "freq1_input")
    except Exception:
        pass

    def read():
        try:
            with open(path) as fh:
                return float(fh.read().strip()) / 1e6 or None
        except Exception:
            return None
    return read


def side_by_side(A, progs, n, blocks, warm, stretch, log, clock=lambda: None):
    plain, bus = Path(A, progs, n, False), Path(A, progs, n, True)
    clocks = {"plain": [], "bus": []}
    for p in (plain, bus):
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    staged0 = [p.b.info("host_staged_blocks") for p in (plain, bus)]
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for name, p in (("plain", plain), ("bus", bus)):   # by turns: what else happens on the host and the device meets both
                p.stretch(stretch)
                clocks[name].append(clock())   # (one reading right behind the stretch's last block, outside every timed block)
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "group": GROUP, "stretch_blocks": stretch}
    for name, p, s0 in (("plain", plain, staged0[0]), ("bus", bus, staged0[1])):
        r = rt.percentiles(p.times)
        half = len(p.times) // 2
        r.update({"median_us_first_half": rt.percentiles(p.times[:half])["median_us"], "median_us_second_half": rt.percentiles(p.times[half:])["median_us"],
                  "pcie_bytes_each_way_per_block": BLOCK * p.width * 4, "host_staged_blocks_in_timed_region": p.b.info("host_staged_blocks") - s0,
                  "kernel_us_last": round(p.b.last_kernel_ms() * 1e3, 1), "tier": p.b.tier_note()})
        mhz = [c for c in clocks[name] if c]
        r["shader_clock_mhz_behind_a_stretch"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        out[name] = r
        log("%-5s N=%7d  median %7.1f (halves %7.1f / %7.1f)  p99 %7.1f  p99.9 %7.1f  max %8.1f us  emulation kernel %6.1f us" % (
            name, n, r["median_us"], r["median_us_first_half"], r["median_us_second_half"], r["p99_us"], r["p999_us"], r["max_us"], r["kernel_us_last"]))
    out["condition_bus_median_not_above_plain_median"] = out["bus"]["median_us"] <= out["plain"]["median_us"]
    plain.close()
    bus.close()
    return out


def meter_side_by_side(A, progs, n, blocks, warm, stretch, log, clock=lambda: None):
    """bus blocks with meters off and on by turns, in stretches, in one process"""
    import numpy as np
    off, on = Path(A, progs, n, True), Path(A, progs, n, True, meter=True)
    clocks = {"meters off": [], "meters on": []}
    for p in (off, on):
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    launches0 = on.b.info("meter_launches")
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for name, p in (("meters off", off), ("meters on", on)):
                p.stretch(stretch)
                clocks[name].append(clock())
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "group": GROUP, "stretch_blocks": stretch}
    for name, p in (("meters off", off), ("meters on", on)):
        r = rt.percentiles(p.times)
        r.update({"kernel_us_last": round(p.b.last_kernel_ms() * 1e3, 1), "blocks": len(p.times)})
        mhz = [c for c in clocks[name] if c]
        r["shader_clock_mhz_behind_a_stretch"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        out[name] = r
        log("%-10s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  launch(es) behind the last block %6.1f us  shader clock %s MHz" % (
            name, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["p999_us"] <= BUDGET_US else "over budget",
            r["kernel_us_last"], r["shader_clock_mhz_behind_a_stretch"]))
    # the two have heard the same blocks: same words out, and one meter launch per block
    same = off.k == on.k and np.array_equal(off.out.array.view(np.uint32), on.out.array.view(np.uint32))
    meters = on.b.meter_read()
    out["outputs_equal"] = bool(same)
    out["meter_launches_in_timed_region"] = on.b.info("meter_launches") - launches0
    out["meter_samples"] = on.b.meter_samples()
    log("           N=%7d  outputs of the two %s; %d meter launches for %d timed blocks; %d sample periods metered, %d instances with energy > 0, %d non-finite words" % (
        n, "equal" if same else "DIFFER", out["meter_launches_in_timed_region"], len(on.times), out["meter_samples"],
        int((meters["energy"] > 0).sum()), int(meters["nonfinite"].sum(dtype=np.uint64))))
    off.close()
    on.close()
    return out


GAIN_MODES = (("gains off", None), ("static", "static"), ("ramping", "ramp"))


def gain_modes(gains_list):
    return GAIN_MODES + ((("list %d" % gains_list, "list"),) if gains_list else ())


def gains_side_by_side(A, progs, n, blocks, warm, stretch, log, clock=lambda: None, gains_list=0):
    """bus blocks with gains off, static gains and a ramp on every block by turns, in stretches, in one process; gains_list: and,
    as a fourth path, a list set of that many faders with ramp = 1 on every block"""
    import numpy as np
    # gains of 1.0f give the words of gains off
    off, ones = Path(A, progs, n, True), Path(A, progs, n, True, gains="static")
    ones.b.bus_set_gains(np.ones((1, n), dtype=np.float32))
    for _ in range(2):
        off.block()
        ones.block()
        want, got = off.out.array, ones.out.array
        nan = np.isnan(want)
        if not ((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()):
            raise RuntimeError("gains of 1.0f differ from gains off at %d instances" % n)
    off.close()
    ones.close()
    paths = [(name, Path(A, progs, n, True, gains=mode, gains_list=gains_list)) for name, mode in gain_modes(gains_list)]
    clocks = {name: [] for name, _ in paths}
    for _, p in paths:
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for name, p in paths:
                p.stretch(stretch)
                clocks[name].append(clock())
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "group": GROUP, "stretch_blocks": stretch}
    for name, p in paths:
        r = rt.percentiles(p.times)
        r.update({"blocks": len(p.times), "bus_gain_blocks": p.b.info("bus_gain_blocks"), "gain_list_sets": p.b.info("gain_list_sets")})
        mhz = [c for c in clocks[name] if c]
        r["shader_clock_mhz_behind_a_stretch"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        out[name] = r
        log("%-9s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  %d blocks mixed with gains  shader clock %s MHz" % (
            name, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["p999_us"] <= BUDGET_US else "over budget",
            r["bus_gain_blocks"], r["shader_clock_mhz_behind_a_stretch"]))
        p.close()
    return out


def taps_side_by_side(A, progs, n, taps, blocks, warm, stretch, log, clock=lambda: None):
    """bus blocks untapped and with `taps` instances tapped by turns, in stretches, in one process"""
    import numpy as np
    # the tap words are the plain path's columns, the mix is the untapped one's
    plain, off, on = Path(A, progs, n, False), Path(A, progs, n, True), Path(A, progs, n, True, taps=taps)
    for _ in range(2):
        for p in (plain, off, on):
            p.block()
        if not np.array_equal(on.tap_out.array.view(np.uint32), plain.out.array[:, :, on.tap_list].view(np.uint32)):
            raise RuntimeError("the taps differ from the plain path's columns at %d instances" % n)
        if not np.array_equal(on.out.array.view(np.uint32), off.out.array.view(np.uint32)):
            raise RuntimeError("the tapped handle's mix differs from the untapped one's at %d instances" % n)
    plain.close()
    paths = [("untapped", off), ("%d taps" % taps, on)]
    clocks = {name: [] for name, _ in paths}
    for _, p in paths:
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for name, p in paths:
                p.stretch(stretch)
                clocks[name].append(clock())
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "group": GROUP, "taps": taps, "stretch_blocks": stretch}
    for name, p in paths:
        r = rt.percentiles(p.times)
        r.update({"blocks": len(p.times), "bus_tap_blocks": p.b.info("bus_tap_blocks")})
        mhz = [c for c in clocks[name] if c]
        r["shader_clock_mhz_behind_a_stretch"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        out[name] = r
        log("%-10s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  %d tapped blocks  shader clock %s MHz" % (
            name, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["p999_us"] <= BUDGET_US else "over budget",
            r["bus_tap_blocks"], r["shader_clock_mhz_behind_a_stretch"]))
    same = off.k == on.k and np.array_equal(off.out.array.view(np.uint32), on.out.array.view(np.uint32))
    out["outputs_equal"] = bool(same)
    out["median_difference_us"] = round(out["%d taps" % taps]["median_us"] - out["untapped"]["median_us"], 1)
    log("           N=%7d  mixes of the two %s; median with taps - median without: %+.1f us" % (n, "equal" if same else "DIFFER", out["median_difference_us"]))
    off.close()
    on.close()
    return out


def sends_side_by_side(A, progs, n, sends, blocks, warm, stretch, log, clock=lambda: None, send_gains_list=0):
    """bus blocks without sends and with every instance on each of `sends` aux buses by turns, in stretches, in one process;
    send_gains_list: and, as a third path, the sends with a list set of that many send gains with ramp = 1 on every block"""
    import numpy as np
    # the aux words are the definition over the plain path's output, the mix is the one of the handle without sends
    plain, off, on = Path(A, progs, n, False), Path(A, progs, n, True), Path(A, progs, n, True, sends=sends)
    for _ in range(2):
        for p in (plain, off, on):
            p.block()
        if not np.array_equal(on.aux_out.array.view(np.uint32), send_all_model(plain.out.array, on.send_gains).view(np.uint32)):
            raise RuntimeError("the aux buses differ from the definition applied to the plain path's output at %d instances" % n)
        if not np.array_equal(on.out.array.view(np.uint32), off.out.array.view(np.uint32)):
            raise RuntimeError("the mix of the handle with sends differs from the one without at %d instances" % n)
    plain.close()
    paths = [("no sends", off), ("%d sends" % sends, on)]
    if send_gains_list:
        paths.append(("list %d" % send_gains_list, Path(A, progs, n, True, sends=sends, send_gains_list=send_gains_list)))
    clocks = {name: [] for name, _ in paths}
    for _, p in paths:
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for name, p in paths:
                p.stretch(stretch)
                clocks[name].append(clock())
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "group": GROUP, "sends": sends, "stretch_blocks": stretch}
    for name, p in paths:
        r = rt.percentiles(p.times)
        r.update({"blocks": len(p.times), "bus_send_blocks": p.b.info("bus_send_blocks")})
        mhz = [c for c in clocks[name] if c]
        r["shader_clock_mhz_behind_a_stretch"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        out[name] = r
        log("%-10s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  %d blocks with sends  shader clock %s MHz" % (
            name, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["p999_us"] <= BUDGET_US else "over budget",
            r["bus_send_blocks"], r["shader_clock_mhz_behind_a_stretch"]))
    same = off.k == on.k and np.array_equal(off.out.array.view(np.uint32), on.out.array.view(np.uint32))
    out["outputs_equal"] = bool(same)
    out["median_difference_us"] = round(out["%d sends" % sends]["median_us"] - out["no sends"]["median_us"], 1)
    log("           N=%7d  mixes of the two %s; median with sends - median without: %+.1f us" % (n, "equal" if same else "DIFFER", out["median_difference_us"]))
    for _, p in paths:
        p.close()
    return out


def feeds_side_by_side(A, progs, n, feeds, blocks, warm, stretch, log, clock=lambda: None):
    """bus blocks with FXB_BUS_SHARED_IN and with feeds (1: the map n / GROUP, unweighted; F >= 2: CSR, F weighted entries per
    instance) by turns, in stretches, in one process"""
    import numpy as np
    shared, fed = Path(A, progs, n, True), Path(A, progs, n, True, feeds=feeds)
    for _ in range(2):
        shared.block()
        fed.block()
        # the map is the shared input, word for word
        if feeds == 1 and not np.array_equal(fed.out.array.view(np.uint32), shared.out.array.view(np.uint32)):
            raise RuntimeError("the mix of the handle with the map n / %d differs from the shared input's at %d instances" % (GROUP, n))
    paths = [("shared in", shared), ("feeds F=%d" % feeds, fed)]
    clocks = {name: [] for name, _ in paths}
    for _, p in paths:
        p.stretch(warm, timed=False)
        p.b.prepare(BLOCK, True)
    gc.collect()
    gc.disable()
    try:
        done = 0
        while done < blocks:
            for name, p in paths:
                p.stretch(stretch)
                clocks[name].append(clock())
            done += stretch
    finally:
        gc.enable()
    out = {"instances": n, "group": GROUP, "feeds": feeds, "stretch_blocks": stretch}
    for name, p in paths:
        r = rt.percentiles(p.times)
        r.update({"blocks": len(p.times), "bus_feed_blocks": p.b.info("bus_feed_blocks")})
        mhz = [c for c in clocks[name] if c]
        r["shader_clock_mhz_behind_a_stretch"] = round(sum(mhz) / len(mhz), 1) if mhz else None
        out[name] = r
        log("%-10s N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  %d feed blocks  shader clock %s MHz" % (
            name, n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"], "REAL TIME" if r["p999_us"] <= BUDGET_US else "over budget",
            r["bus_feed_blocks"], r["shader_clock_mhz_behind_a_stretch"]))
    same = feeds != 1 or (shared.k == fed.k and np.array_equal(shared.out.array.view(np.uint32), fed.out.array.view(np.uint32)))
    out["outputs_equal"] = bool(same)
    out["median_difference_us"] = round(out["feeds F=%d" % feeds]["median_us"] - out["shared in"]["median_us"], 1)
    log("           N=%7d  mixes of the two %s; median with feeds - median with the shared input: %+.1f us" % (
        n, ("equal" if same else "DIFFER") if feeds == 1 else "not compared (another input)", out["median_difference_us"]))
    shared.close()
    fed.close()
    return out


def bus_row(A, progs, n, blocks, warm, log):
    """one count of the sweep.  parity_ok is a comparison: after the timed region a plain handle at the same count replays every
    block of the run (same PCM, same slider schedule, untimed), and the bus path's LAST block must be, word for word, the
    summation order applied to the plain path's last block; the instruction counters of sampled instances must agree too."""
    import numpy as np
    p = Path(A, progs, n, True)
    p.stretch(warm, timed=False)
    p.b.prepare(BLOCK, True)
    gc.collect()
    gc.disable()
    try:
        p.stretch(blocks)
    finally:
        gc.enable()
    r = rt.percentiles(p.times)
    r.update({"instances": n, "mode": "bus", "group": GROUP, "within_budget_p999": r["p999_us"] <= BUDGET_US,
              "kernel_us_last": round(p.b.last_kernel_ms() * 1e3, 1), "host_inplace_blocks": p.b.info("host_inplace_blocks"), "host_staged_blocks": p.b.info("host_staged_blocks")})
    plain = Path(A, progs, n, False)
    plain.stretch(p.k, timed=False)
    want, got = mix_model(plain.out.array, GROUP), p.out.array
    nan = np.isnan(want)
    ok = bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())
    picks = sorted({0, 63, 64, n // 2, n - 1})
    ok = ok and all(p.b.instruction_counter_i(i) == plain.b.instruction_counter_i(i) for i in picks)
    r.update({"parity_ok": ok, "parity": "last of %d blocks against the summation order applied to a plain handle's replay of the run; instruction counters of %d instances" % (p.k, len(picks))})
    log("bus   N=%7d  median %7.1f  p99 %7.1f  p99.9 %7.1f  max %8.1f us  %s  parity %s" % (n, r["median_us"], r["p99_us"], r["p999_us"], r["max_us"],
        "REAL TIME" if r["within_budget_p999"] else "over budget", "ok" if ok else "MISMATCH"))
    plain.close()
    p.close()
    return r


def kernel_shares(path, n, taps=0, sends=0):
    """the --stats table of a `--trace-run` under rocprofv3: share of device time and achieved bytes/s of the two bus kernels"""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    groups = -(-n // GROUP)
    # what to look for in a kernel's demangled name -> bytes read + written per launch (the meter: the block, and its 20-byte
    # accumulators in and out; the weighted mix: the block, and one or two gain rows of n words that the rows of a block share).
    # The plain kernels are matched up to their "(" so that fx_bus_mix does not also match fx_bus_mix_gain<...>: this relies on the
    # full demangled signature that rocprofv3 writes; a table with truncated names ("fx_bus_mix" alone) would match nothing here.
    mix = BLOCK * (n + groups) * 4
    need = {"fx_bus_expand": ("fx_bus_expand(", BLOCK * (groups + n) * 4), "fx_bus_mix": ("fx_bus_mix(", mix), "fx_meter": ("fx_meter", BLOCK * n * 4 + 2 * 20 * n),
            "fx_bus_mix_gain<false>": ("fx_bus_mix_gain<false>", mix + n * 4), "fx_bus_mix_gain<true>": ("fx_bus_mix_gain<true>", mix + 2 * n * 4)}
    if taps:   # (the tapped words in and out, and the list)
        need["fx_bus_tap"] = ("fx_bus_tap", 2 * BLOCK * taps * 4 + taps * 4)
    if sends:   # (per entry: the scratch word, the index and the gain word; the chunk sums out, and in again with the aux words out)
        chunks = sends * -(-n // 1024)
        need["fx_bus_send_chunks"] = ("fx_bus_send_chunks", sends * n * (BLOCK * 4 + 8) + BLOCK * chunks * 4)
        need["fx_bus_send_fold"] = ("fx_bus_send_fold", BLOCK * (chunks + sends) * 4)
    out = {"instances": n, "device_time_ns": total, "kernels": {}}
    for r in rows:
        for key, (match, bytes_) in need.items():
            if match in r["Name"]:
                avg = float(r["AverageNs"])
                out["kernels"][key] = {"calls": int(r["Calls"]), "average_ns": round(avg, 1), "share_of_device_time": round(float(r["TotalDurationNs"]) / total, 4),
                                       "bytes_per_launch": bytes_, "achieved_TBps": round(bytes_ / avg / 1e3, 3),
                                       "share_of_achievable_hbm": round(bytes_ / (avg * 1e-9) / HBM_ACHIEVABLE_BPS, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--stretch", type=int, default=250, help="blocks of one path before the other takes its turn")
    ap.add_argument("--instances", type=int, default=131072)
    ap.add_argument("--sweep", default="131072,196608,262144,327680,393216,458752,524288")
    ap.add_argument("--plain-sweep", default="65536,98304,131072,147456,163840,180224")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-instances", type=int, default=524288)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--meter", action="store_true", help="bus blocks with output meters off and on by turns (with --trace-run: meters on)")
    ap.add_argument("--meter-instances", default="131072,458752")
    ap.add_argument("--meter-out", default="", help="keep the lines of --meter in this text file")
    ap.add_argument("--gains", action="store_true", help="bus blocks with gains off, static gains and a ramp on every block by turns (with --trace-run: the same three)")
    ap.add_argument("--gain-instances", default="131072,458752")
    ap.add_argument("--gains-list", type=int, default=0, help="with --gains: a fourth path, a list set of this many faders with ramp = 1 in front of every block")
    ap.add_argument("--gains-out", default="", help="keep the lines of --gains in this text file")
    ap.add_argument("--taps", type=int, default=0, help="bus blocks untapped and with this many instances tapped by turns (with --trace-run: tapped, meters on)")
    ap.add_argument("--tap-instances", default="131072,458752")
    ap.add_argument("--taps-out", default="", help="keep the lines of --taps in this text file")
    ap.add_argument("--sends", type=int, default=0, help="bus blocks without sends and with every instance on each of this many aux buses by turns "
                    "(with --trace-run --gains: one handle with static bus gains and the sends)")
    ap.add_argument("--send-instances", default="131072,458752")
    ap.add_argument("--send-gains-list", type=int, default=0, help="with --sends: a third path, a list set of this many send gains with ramp = 1 in front of every block")
    ap.add_argument("--sends-out", default="", help="keep the lines of --sends in this text file")
    ap.add_argument("--feeds", type=int, default=0, help="bus blocks with the shared input and with feeds by turns: 1 = the map n / group, unweighted; F >= 2 = CSR with F "
                    "weighted entries per instance (with --trace-run: 200 blocks of a handle with the shared input, 200 of one with the map and, for F >= 2, 200 of the CSR one)")
    ap.add_argument("--feed-instances", default="131072,458752")
    ap.add_argument("--feeds-out", default="", help="keep the lines of --feeds in this text file")
    args = ap.parse_args()
    import torch  # first: its HIP runtime is the one the library binds to

    import fx8010_amd as A
    import fx8010_programs as progs
    log = lambda s: print(s, flush=True)
    if args.trace_run and args.feeds:
        # fx_bus_expand of the first handle is the yardstick of fx_bus_feed (map) of the second in the same trace
        for feeds in (0, 1) + ((args.feeds,) if args.feeds >= 2 else ()):
            p = Path(A, progs, args.trace_instances, True, feeds=feeds)
            p.stretch(200, timed=False)
            p.close()
        return 0
    if args.feeds:
        lines = []

        def keep(s):
            lines.append(s)
            log(s)
        keep("32-sample bus blocks of config5 (mixed output per %d instances, pinned host buffers) against %.3f us, with the shared input (FXB_BUS_SHARED_IN) and with "
             "feeds (fxb_process_block_bus_feed, F = %d) by turns in stretches of %d blocks in one process, %d blocks per point after %d warm-up blocks; %s" % (
                 GROUP, BUDGET_US, args.feeds, args.stretch, args.blocks, args.warmup, torch.cuda.get_device_name(0)))
        rows = [feeds_side_by_side(A, progs, int(v), args.feeds, args.blocks, args.warmup, args.stretch, keep, shader_clock_reader(torch)) for v in args.feed_instances.split(",") if v]
        if args.feeds_out:
            with open(args.feeds_out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        if args.json:
            with open(args.json, "w") as fh:
                json.dump({"feed_rows": rows}, fh, indent=1)
        return 0 if all(r["outputs_equal"] for r in rows) else 1
    if args.trace_run and args.sends:
        p = Path(A, progs, args.trace_instances, True, gains="static" if args.gains else None, sends=args.sends, send_gains_list=args.send_gains_list)
        p.stretch(200, timed=False)
        p.close()
        return 0
    if args.sends:
        lines = []

        def keep(s):
            lines.append(s)
            log(s)
        keep("32-sample bus blocks of config5 (shared input and mixed output per %d instances, pinned host buffers) against %.3f us, without sends and with "
             "every instance on each of %d aux buses delivered to a pinned side (fxb_process_block_bus_aux) by turns in stretches of %d blocks in one process, "
             "%d blocks per point after %d warm-up blocks; %s" % (GROUP, BUDGET_US, args.sends, args.stretch, args.blocks, args.warmup, torch.cuda.get_device_name(0)))
        if args.send_gains_list:
            keep("and, as a third path, the sends with a list set of %d send gains with ramp = 1 (fxb_bus_set_send_gains_list) inside the timed region" % args.send_gains_list)
        rows = [sends_side_by_side(A, progs, int(v), args.sends, args.blocks, args.warmup, args.stretch, keep, shader_clock_reader(torch), args.send_gains_list)
                for v in args.send_instances.split(",") if v]
        if args.kernel_stats:
            keep(json.dumps(kernel_shares(args.kernel_stats, args.trace_instances, sends=args.sends)))
        if args.sends_out:
            with open(args.sends_out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        if args.json:
            with open(args.json, "w") as fh:
                json.dump({"send_rows": rows}, fh, indent=1)
        return 0 if all(r["outputs_equal"] for r in rows) else 1
    if args.trace_run and args.gains:
        paths = [Path(A, progs, args.trace_instances, True, gains=mode, gains_list=args.gains_list) for _, mode in gain_modes(args.gains_list)]
        for _ in range(4):
            for p in paths:
                p.stretch(50, timed=False)
        for p in paths:
            p.close()
        return 0
    if args.gains:
        lines = []

        def keep(s):
            lines.append(s)
            log(s)
        keep("32-sample bus blocks of config5 (shared input and mixed output per %d instances, pinned host buffers) against %.3f us: gains off, static "
             "gains, and a ramp on every block (fxb_bus_set_gains with ramp = 1 inside the timed region), by turns in stretches of %d blocks in one "
             "process, %d blocks per point after %d warm-up blocks; %s" % (GROUP, BUDGET_US, args.stretch, args.blocks, args.warmup, torch.cuda.get_device_name(0)))
        if args.gains_list:
            keep("and, as a fourth path, a list set of %d faders with ramp = 1 (fxb_bus_set_gains_list) in front of every block, inside the timed region" % args.gains_list)
        rows = [gains_side_by_side(A, progs, int(v), args.blocks, args.warmup, args.stretch, keep, shader_clock_reader(torch), args.gains_list) for v in args.gain_instances.split(",") if v]
        if args.kernel_stats:
            keep(json.dumps(kernel_shares(args.kernel_stats, args.trace_instances)))
        if args.gains_out:
            with open(args.gains_out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        if args.json:
            with open(args.json, "w") as fh:
                json.dump({"gain_rows": rows}, fh, indent=1)
        return 0
    if args.taps and not args.trace_run:
        lines = []

        def keep(s):
            lines.append(s)
            log(s)
        keep("32-sample bus blocks of config5 (shared input and mixed output per %d instances, pinned host buffers) against %.3f us, untapped and with %d "
             "instances tapped into a pinned side (fxb_process_block_bus_tap) by turns in stretches of %d blocks in one process, %d blocks per point after "
             "%d warm-up blocks; %s" % (GROUP, BUDGET_US, args.taps, args.stretch, args.blocks, args.warmup, torch.cuda.get_device_name(0)))
        rows = [taps_side_by_side(A, progs, int(v), args.taps, args.blocks, args.warmup, args.stretch, keep, shader_clock_reader(torch)) for v in args.tap_instances.split(",") if v]
        if args.kernel_stats:
            keep(json.dumps(kernel_shares(args.kernel_stats, args.trace_instances, args.taps)))
        if args.taps_out:
            with open(args.taps_out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        if args.json:
            with open(args.json, "w") as fh:
                json.dump({"tap_rows": rows}, fh, indent=1)
        return 0 if all(r["outputs_equal"] for r in rows) else 1
    if args.trace_run:
        p = Path(A, progs, args.trace_instances, True, meter=args.meter or args.taps > 0, taps=args.taps)
        p.stretch(200, timed=False)
        p.close()
        return 0
    if args.meter:
        lines = []

        def keep(s):
            lines.append(s)
            log(s)
        keep("32-sample bus blocks of config5 (shared input and mixed output per %d instances, pinned host buffers) against %.3f us, output meters off and on "
             "by turns in stretches of %d blocks in one process, %d blocks per point after %d warm-up blocks; %s" % (
                 GROUP, BUDGET_US, args.stretch, args.blocks, args.warmup, torch.cuda.get_device_name(0)))
        rows = [meter_side_by_side(A, progs, int(v), args.blocks, args.warmup, args.stretch, keep, shader_clock_reader(torch)) for v in args.meter_instances.split(",") if v]
        if args.kernel_stats:
            keep(json.dumps(kernel_shares(args.kernel_stats, args.trace_instances)))
        if args.meter_out:
            with open(args.meter_out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        if args.json:
            with open(args.json, "w") as fh:
                json.dump({"meter_rows": rows}, fh, indent=1)
        return 0 if all(r["outputs_equal"] for r in rows) else 1
    out = {"what": "32-sample blocks of config5 at 48 kHz against %.3f us, pinned host buffers, call -> output in host memory on the caller's clock; plain: "
                   "fxb_process_block in place; bus: fxb_process_block_bus, shared input and mixed output per %d instances" % (BUDGET_US, GROUP),
           "gpu": torch.cuda.get_device_name(0), "budget_us": round(BUDGET_US, 3), "blocks_per_point": args.blocks, "warmup_blocks": args.warmup}
    check_words(A, progs, args.instances)
    out["side_by_side"] = side_by_side(A, progs, args.instances, args.blocks, args.warmup, args.stretch, log, shader_clock_reader(torch))
    rows = [bus_row(A, progs, int(v), args.blocks, args.warmup, log) for v in args.sweep.split(",") if v]
    out["bus_rows"], out["capacity_bus"] = rows, rt.capacity(rows)
    plain = rt.run(torch, A, progs, [int(v) for v in args.plain_sweep.split(",") if v], args.blocks, args.warmup, ("host",), log)
    out["plain_rows"], out["capacity_plain"] = plain["rows"], plain["capacity_host_fed"]
    if args.kernel_stats:
        out["device_time"] = kernel_shares(args.kernel_stats, args.trace_instances)
    log("largest N within %.3f us at p99.9: bus %s, plain %s; bus median <= plain median at %d: %s" % (
        BUDGET_US, out["capacity_bus"], out["capacity_plain"], args.instances, out["side_by_side"]["condition_bus_median_not_above_plain_median"]))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0 if out["side_by_side"]["condition_bus_median_not_above_plain_median"] and all(r["parity_ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
