#!/usr/bin/env python3
"""How often do the quiet loop's sum groups (fx_xlate.hpp SumGroup) really repair?  One handle of `--instances` instances of a
bench.py configuration (default: the 1/8 shard of the headline workload, 262 144 instances of config5), `--blocks` blocks of
`--samples` samples of the benchmark's stimulus - enough blocks for the delay line to be full - and after every launch
FXB_INFO_XLATE_QUIET_REPAIRS and FXB_INFO_XLATE_QUIET_LEFT of that launch.  Prints one JSON line.

    python tools/quiet_repairs.py [--config config5] [--instances 262144] [--samples 4096] [--blocks 4]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fx8010-emulator-core_amd", "python"))

import numpy as np  # noqa: E402

import fx8010_amd  # noqa: E402
import fx8010_programs as progs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config5")
    ap.add_argument("--instances", type=int, default=262144)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=4)
    a = ap.parse_args()
    b = fx8010_amd.Batch(a.instances, 1, 0)
    if not b.load_text(progs.CONFIGS[a.config]()):
        raise SystemExit("load failed: %s" % b.errors())
    # the benchmark's stimulus: one block, the same for every launch, as bench.py feeds it
    x = progs.stimulus(a.instances, a.samples)
    launches = []
    for k in range(a.blocks):
        b.process_block(x)
        launches.append({"block": k, "quiet_repairs": int(b.info("xlate_quiet_repairs")), "quiet_left": int(b.info("xlate_quiet_left")),
                         "kernel_ms": round(float(b.last_kernel_ms()), 4)})
    waves = (a.instances + 63) // 64
    groups = int(b.info("xlate_sum_groups"))
    out = {"config": a.config, "instances": a.instances, "samples": a.samples, "wavefronts": waves, "quiet": int(b.info("xlate_quiet")),
           "sum_groups": groups, "sum_links": int(b.info("xlate_sum_links")), "code_hash": "%016x" % int(b.info("xlate_code_hash")),
           "group_tests_per_launch": waves * groups * max(a.samples - 1, 0), "launches": launches, "tier": b.tier_note()}
    print(json.dumps(out))
    b.close()


if __name__ == "__main__":
    main()
