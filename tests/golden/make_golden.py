#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the UNMODIFIED reference.

Runs only where /root/reference exists (the build container): it drives oracle/_ref/libfxref.so
— the reference's own sources compiled by oracle/Makefile — through its public API and writes
small JSON fixtures (program text written for this repo, input bits, output bits, final register
bits, instruction counter, error/control/meta lists).  No reference source is stored.

    python tests/golden/make_golden.py        # rewrites tests/golden/*.json
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "fx8010-emulator-core_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fx8010_programs as progs  # noqa: E402
import multichannel_programs as mc  # noqa: E402
from pyoracle import Oracle, Reference  # noqa: E402

HDR = "static a\nstatic b\ninput in 0\noutput out 0\nstatic noise\nstatic rd\ncontrol vol = 0.5\n"


def hexbits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tobytes().hex()


def run_case(name, text, x, regs=("ccr",), channels=1, sets=None):
    """sets: {sample_index: [(register, value), ...]} applied before that sample (slider schedule)."""
    r = Reference(channels)
    ok = r.load_text(text)
    case = {"name": name, "program": text, "channels": channels, "load_ok": bool(ok), "errors": r.errors(),
            "controls": r.controls(), "meta": r.meta()}
    if ok:
        x = np.ascontiguousarray(x, dtype=np.float32)
        if sets:
            outs = []
            cuts = sorted(set([0] + list(sets.keys()) + [x.shape[0]]))
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                for reg, val in sets.get(lo, []):
                    r.set_register(reg, val)
                outs.append(r.process_block(x[lo:hi]))
            y = np.concatenate(outs, axis=0)
            case["sets"] = {str(k): v for k, v in sets.items()}
        else:
            y = r.process_block(x)
        case.update({"input": hexbits(x), "output": hexbits(y), "shape": list(x.shape),
                     "counter": r.instruction_counter(), "registers": {k: r.get_register_bits(k) for k in regs}})
    return case


def ramp32():
    return np.array([i / 16.0 for i in range(-16, 16)], dtype=np.float32)


def ramp_ext():
    return np.array([i / 16.0 for i in range(-16, 16)] + [1.0, -1.0, 0.0, -0.0, 1e-39, -1e-39, 0.999999, -0.999999] * 2, dtype=np.float32)


OPCODE_PROGRAMS = {
    "macs": "macs out, in, vol, 0.75", "macsn": "macsn out, in, vol, 0.75", "macints": "macints out, in, in, 2",
    "acc3": "acc3 out, in, vol, 0.25", "macw": "macw out, in, 1.5, 1.0", "macwn": "macwn out, in, 1.5, in",
    "macintw": "macintw out, in, 1.5, 1.0", "macw_ccr_as_a": "macw out, ccr, 1.5, in", "macmv": "macmv out, in, 0.5, 0.5",
    "andxor_and": "macs a, 0, in, 100\nandxor out, a, 15, 0", "andxor_xor": "macw a, 0, in, 100\nandxor out, a, 16777215, 5",
    "andxor_generic": "macw a, 0, in, 100\nandxor out, a, 12, 3", "andxor_literals": "andxor out, 7, 5, 2",
    "tstneg": "tstneg out, in, 0.25, 0", "tstneg_overflow": "tstneg out, in, 1.0, 0", "limit": "limit out, in, 0.5, 0.25",
    "limitn": "limitn out, in, 0.5, 0.25", "log3": "log a, in, 3, 0\nmacs out, 0, a, 1.0", "log0": "log a, in, 0, 0\nmacs out, 0, a, 1.0",
    "log31": "log a, in, 31, 1\nmacs out, 0, a, 1.0", "exp7": "exp a, in, 7, 0\nmacs out, 0, a, 1.0", "exp0": "exp a, in, 0, 0\nmacs out, 0, a, 1.0",
    "exp_unclamped_r": "exp out, in, 2, 0", "interp": "interp out, out, 0.1, in", "interp_literals": "interp out, -0.25, vol, 0.25",
    "highpass": "interp a, a, 0.1, in\nmacsn out, in, a, 1", "skip_neg": "macs a, in, 0, 0\nskip ccr, ccr, 6, 1\nmacs out, 0, in, 1.0",
    "skip_zero": "macs a, in, 0, 0\nskip ccr, ccr, 8, 2\nmacs out, 0, in, 1.0\nmacs out, out, 0.5, 0.5",
    "skip_sat": "macs a, in, in, 1.0\nskip ccr, ccr, 16, 1\nmacs out, 0, a, 0.5",
    "skip_negative_count": "macs a, in, 0, 0\nskip ccr, ccr, 6, -3\nmacs out, 0, in, 1.0\nmacs b, out, 0.5, 0.5",
    "skip_never": "macs a, in, 0, 0\nskip ccr, ccr, 384, 1\nmacs out, 0, in, 1.0", "ccr_as_operand": "macs a, in, 0, 0\nmacs out, 0, ccr, 0.03125",
    "noise": "macs out, 0, noise, 1.0", "noise_twice": "macs a, 0, noise, 0.5\nmacs out, a, noise, 0.5",
    "literal_as_r": "macs 0.5, in, 0.5, 0.5\nmacs out, 0, 0.5, 1.0", "write_ccr_directly": "macs ccr, in, 0, 0\nmacs out, 0, ccr, 0.03125",
    "out_read_back": "macs out, out, in, 0.1", "idelay_nop_r": "idelay a, in, at, 0\nmacs out, 0, in, 1.0",
    "latch_on_skip": "macs out, 0, in, 1.0\nmacs out, out, 0.5, 0.5\nskip out, ccr, 2, 0",
    "skip_over_end": "macs a, in, 0, 0\nmacs out, out, 0.125, 0.5\nskip ccr, ccr, 6, 2\nmacs b, in, 0.5, 0.5",
    # END in the middle: the for-loop of process() finishes its pass, so the instructions behind it still run (and count),
    # FX8010.cpp:1033-1043
    "end_in_the_middle": "macs a, in, 0.5, 0.5\nend\nmacs out, a, in, 0.25\nmacs b, out, 0.5, 0.5",
    "end_twice_then_skip": "macs a, in, 0, 0\nend\nskip ccr, ccr, 6, 1\nmacs out, 0, in, 1.0\nend\nmacs b, out, in, 0.5",
    # the logicOps branches (FX8010.cpp:330-360) not covered above: Y == ~X (OR), Y == 0xFFFFFF with another X (NAND);
    # X == 0xFFFFFFF is not a float (it reads back as 0x10000000), so the NOT branch cannot be reached: generic result
    "andxor_or": "macw a, 0, in, 100\nandxor out, a, 12, -13", "andxor_nand": "macw a, 0, in, 100\nandxor out, a, 12, 16777215",
    "andxor_not_unreachable": "macw a, 0, in, 100\nandxor out, a, 268435455, 16777215",
    "andxor_or_from_registers": "macw a, 0, in, 100\nmacw b, -1, a, -1\nandxor out, 5, a, b",
    # LOG / EXP of a uniform operand (a literal, a control): the result is one constant - the device tiers fold it on the host
    # (fx_asm.cpp encodeAsmStream) - inside the table, at both ends of it (x == 1.0 reads table entry [idx + 1] times 0), with the
    # CCR it sets read as an operand and consumed by a SKIP
    "log_uniform": "log a, 0.5, 3, 0\nmacs out, in, a, 0.5", "exp_uniform_minus_one": "exp a, -1.0, 7, 0\nmacs out, in, a, 0.5",
    "log_uniform_one_then_skip": "log a, 1.0, 31, 0\nskip ccr, ccr, 16, 1\nmacs out, 0, in, 1.0\nmacs b, out, 0.5, 0.5",
    "log_uniform_zero_then_skip": "log a, 0, 3, 0\nskip ccr, ccr, 8, 2\nmacs out, 0, in, 1.0\nmacs b, out, 0.5, 0.5\nmacs out, out, a, 0.25",
    "exp_uniform_ccr_operand": "exp a, 0.25, 2, 0\nmacs out, in, ccr, 0.03125", "log_of_a_control": "log a, vol, 5, 0\nmacs out, in, a, 0.5",
    "exp_uniform_negative_skip": "exp a, -0.375, 3, 0\nskip ccr, ccr, 6, 1\nmacs out, 0, in, 1.0\nmacs b, a, 0.5, 0.5",
}

# loader corpus: each entry is a whole program text; only load status / error list / lists are pinned
PARSER_CORPUS = [
    "static a\nend", "static a\nend\n", "static a\nend\n\n", "static a\nend ", "static a\nEND", "static a ; c\nend ; x",
    "static a12.5\nmacs a1, a1, 0, 0\nend", "static 12.5\nmacs 1, 1, 0, 0\nend", "static a = 0.5\nend", "static a=.5\nend",
    "static a = -0.5\nend", "static a 1.\nend", "static a b\nend", "static a, 3\nend", "static a = , = 7\nend", "statics a\nend",
    "static\nend", "static a\nstatic a\nend", "static ccr\nend", "control v = 1.0\ncontrol v = 2.0\nend", "input i 0\nend",
    "input i 1\nend", "input i 0.9\nend", "output o 3\nend", "input i\nmacs i, i, i, i\nend", "temp t\nconst c 2\nmacs t, c, c, c\nend",
    "itramsize 100 \nend", "itramsize 100\nend", "itramsize 100  \nend", "itramsize 100\t\nend", "xtramsize 5 \nxtramsize 7 \nend",
    "itramsize 9000 \nitramsize 10 \nend", "xtramsize 2000000 \nxtramsize 1 \nend", " itramsize 4 \nend",
    "static a\nmacs a,a,a,a\nend", "static a\nmacs a , a , a , a \nend", "static a\nmacs a a, a, a\nend", "static a\nmacs a, a, a\nend",
    "static a\nmacs a, a, a, a, a\nend", "static a\nmacs a, b, a, a\nend", "static a\nmacsa, a, a, a\nend", "static a\nmacsn a, 1, -2.5, 3.\nend",
    "static a\nmacsn a, 1, -2.5, .3\nend", "static a\nmacs a, 1e3, 0, 0\nend", "static a\nmacs a, --1, 0, 0\nend", "static a\nmacs a, 1.2.3, 0, 0\nend",
    "static a\nfoo a, a, a, a\nend", "static a\n  MACS A, A, 0.5, A\nend", "static a\nlog a, a, 3, 0\nexp a, a, 7, 0\ninterp a, a, a, a\nend",
    "static a\nskip a, a, a, a\nandxor a, a, a, a\ntstneg a, a, a, a\nlimit a, a, a, a\nlimitn a, a, a, a\nend",
    "static a\nmacw a, a, a, a\nmacwn a, a, a, a\nmacints a, a, a, a\nmacintw a, a, a, a\nacc3 a, a, a, a\nmacmv a, a, a, a\nend",
    "static a\nidelay read, a, at, 0\nidelay write, a, at, 0\nxdelay read, a, at, 0\nxdelay write, a, at, 0\nend",
    'name "x"\nend', 'name "x" \nend', 'name  "a b c"\nend', 'name ""\nend', 'name "x\nend', 'names "x"\nend', 'guid "1-2"\ncomment "HeLLo"\nend',
    'name "a;b"\nend', 'name "one"\nname "two"\nend', "end", "\n", "end\nstatic a\nend", "static a\nmacs a, 0, 0, 0\nend\nmacs a, 1, 1, 1\nend",
    # (an empty file is left out: the reference itself crashes on it — lines.back() on an empty vector)
    "static noise\noutput o 0\nmacs o, 0, noise, 1.0\nend", "input noise 0\noutput o 0\nmacs o, 0, noise, 1.0\nend",
    "static a\r\nend\r\n", "static a\n\tmacs\ta,\ta,\ta,\ta\nend", "static a_b9\nstatic _x\nmacs a_b9, _x, 0, 0\nend", "static a.b\nend",
    "static a\nmacs a, a.b, 0, 0\nend", "static a\nmacs a, -a, 0, 0\nend", "static a\nmacs a, 0, 0, 0 end",
]


# the harness's slider schedule on two channels: both controls move, each input is heard through the other's channel as well
STEREO_SLIDER = ("input l 0\ninput r 1\noutput ol 0\noutput or 1\ncontrol vol = 0.5\ncontrol pan = 0.25\nstatic t\n"
                 "macs t, r, l, vol\nmacs ol, l, r, pan\nmacs or, t, vol, r\nmacs ol, ol, t, pan\nend")


def main():
    if not Reference.available():
        raise SystemExit("oracle/_ref/libfxref.so missing: run `make -C oracle ref` in the build container")
    out = {}

    # 1. one case per opcode / feature over the harness ramp plus edge values
    x = ramp_ext()
    out["opcodes.json"] = [run_case(k, HDR + v + "\nend", x, regs=("a", "b", "out", "ccr", "in")) for k, v in sorted(OPCODE_PROGRAMS.items())]

    # 2. known answers quoted in SURVEY.md §8(a)
    out["known_answers.json"] = [
        run_case("interp_step", HDR + "interp out, out, 0.1, in\nend", np.ones(6, np.float32), regs=("out", "ccr")),
        run_case("log3_ramp32", HDR + "log a, in, 3, 0\nmacs out, 0, a, 1.0\nend", ramp32(), regs=("a", "ccr")),
        run_case("noise_first6", HDR + "macs out, 0, noise, 1.0\nend", np.zeros(6, np.float32), regs=("noise",)),
        run_case("tstneg_overflow", HDR + "tstneg out, in, 1.0, 0\nend", ramp32(), regs=("out",)),
        run_case("macw", HDR + "macw out, in, 1.5, 1.0\nend", ramp32(), regs=("out", "ccr")),
        run_case("skip_sign", HDR + "macs a, in, 0, 0\nskip ccr, ccr, 6, 1\nmacs out, 0, in, 1.0\nend", ramp32(), regs=("out", "ccr")),
        run_case("delay5", "itramsize 5 \n" + HDR + "idelay read, rd, at, 0\nidelay write, in, at, 0\nmacs out, 0, rd, 1.0\nend", ramp32(), regs=("rd",)),
    ]

    # 3. the harness's slider schedule (main.cpp:80,103-122) on the shipped program shape
    sets = {0: [("volume", 0.1)], 8: [("volume", 0.25)], 16: [("volume", 0.5)], 24: [("volume", 1.0)]}
    out["slider.json"] = [run_case("slider_shipped", progs.config1_shipped(), ramp32(), regs=("volume", "filter_cutoff", "in_l", "out_l", "ccr"), sets=sets),
                          run_case("logtube", progs.config1_logtube(), ramp32(), regs=("a", "out_l", "ccr"))]

    # 4. LOG/EXP tables: every exponent at the 64 knots and midpoints (pins the LUT bits that reach an output)
    knots = (-1.0 + np.arange(64, dtype=np.float64) * (2.0 / 63.0)).astype(np.float32)
    mids = (knots[:-1].astype(np.float64) + 1.0 / 63.0).astype(np.float32)
    xs = np.concatenate([knots, mids, np.array([1.0], np.float32)])
    lut = []
    for op in ("log", "exp"):
        for e in range(32):
            lut.append(run_case("%s%d" % (op, e), HDR + "%s out, in, %d, 0\nend" % (op, e), xs, regs=("out",)))
    for c in lut:  # the input is the same for all 64 cases: keep it once
        del c["program"]
    out["lut_probe.json"] = {"input": hexbits(xs), "cases": [{"name": c["name"], "output": c["output"]} for c in lut]}

    # 5. feedback delay over Dirac + noise, 3000 samples
    fb = "itramsize 1000 \n" + HDR + "idelay read, rd, at, 0\nmacs a, in, rd, 0.5\nmacs a, a, noise, 0.01\nidelay write, a, at, 0\nmacs out, 0, a, 1.0\nend"
    dirac = np.zeros(3000, np.float32)
    dirac[0] = 1.0
    out["feedback_delay.json"] = [run_case("feedback_1000", fb, dirac, regs=("rd", "a", "ccr"))]

    # 6. the benchmark programs, a few instances of the synthetic PCM
    cfg = []
    for name in ("config2", "config3", "config4", "config5"):
        text = progs.CONFIGS[name]()
        for inst in (0, 1, 4095):
            x = progs.stimulus(1, 384, first_instance=inst)[:, 0].copy()
            c = run_case("%s_inst%d" % (name, inst), text, x, regs=("ccr", "out"))
            del c["program"]  # regenerated from fx8010_programs at test time
            c["config"] = name
            c["instance"] = inst
            cfg.append(c)
    out["configs.json"] = cfg

    # 6a. the delay-line programs past the first read-back.  The cursors advance per executed TRAM instruction
    # (FX8010.cpp:909-967): config5's four reads + four writes per sample bring the first written word back at sample 2048
    # of its 8192-slot line, config3's read / write pair at sample 1000 (and again at 2000).  2304 samples cover both; the
    # input is the synthetic PCM (regenerated at test time, pinned here by its SHA-256), the output is stored.
    import hashlib
    longc = []
    for name in ("config3", "config5"):
        text = progs.CONFIGS[name]()
        for inst in (0, 4095):
            x = progs.stimulus(1, 2304, first_instance=inst)[:, 0].copy()
            c = run_case("%s_long_inst%d" % (name, inst), text, x, regs=("ccr", "out", "rd", "a", "t") if name == "config3" else ("ccr", "out", "m", "u", "v", "d0", "d3", "w3"))
            del c["program"]
            c["input_sha256"] = hashlib.sha256(bytes.fromhex(c.pop("input"))).hexdigest()
            c["config"] = name
            c["instance"] = inst
            longc.append(c)
    out["configs_long.json"] = longc

    # 6a'. the program shapes the stage planner is calibrated and tested with (twelve parallel chains: 13-row packets; a delay
    # line with feedback and noise, SKIP shadows and LOG / EXP pairs): small batches run them as pipelines of stages, and these
    # are the reference's own words for them
    probe = []
    for name in ("wide12", "mixed_stages"):
        text = progs.PROBE_PROGRAMS[name]()
        for inst in (0, 777):
            x = progs.stimulus(1, 384, first_instance=inst)[:, 0].copy()
            c = run_case("%s_inst%d" % (name, inst), text, x, regs=("ccr", "out"))
            del c["program"]
            c["config"] = name
            c["instance"] = inst
            probe.append(c)
    out["configs_probe.json"] = probe

    # 6b. non-finite values: what the x86 build of the reference does with NaN (either sign, payloads, signalling) and
    # Inf coming in through the PCM input, with NaNs made by the arithmetic itself (Inf * 0, Inf - Inf: the x86 default
    # NaN is NEGATIVE, 0xFFC00000), through saturating and non-saturating instructions, TRAM and the fp64 path
    def f32(bits):
        return np.array(bits, dtype=np.uint32).view(np.float32)
    nf = f32([0x3f800000, 0x7fc00000, 0x3f000000, 0xffc00000, 0x3e800000, 0x7fc12345, 0xbf000000, 0x7f812345, 0x3f400000, 0xff9abcde,
              0x7f800000, 0xbe800000, 0xff800000, 0x00000000, 0x80000000, 0x3f800000, 0x7f800000, 0x7f800000, 0xff800000, 0x3dcccccd,
              0x7fffffff, 0x3f000000, 0xffffffff, 0x3f000000])
    NONFINITE = {
        "macs": "macs out, in, vol, 0.75", "macs_times_zero": "macs out, 0, in, 0", "macsn_self": "macsn out, in, in, 1.0",
        "macs_product_of_input": "macs out, 0.5, in, in", "acc3": "acc3 out, in, in, 0.25", "acc3_cancel": "macsn a, 0, in, 1.0\nacc3 out, in, a, 0.25",
        "interp_state": "interp out, out, 0.1, in", "interp_operands": "interp out, in, vol, in", "interp_per_lane_x": "interp out, 0.5, in, 0.25",
        "macw": "macw out, in, 1.5, 1.0", "macwn": "macwn out, in, 1.5, in", "macintw": "macintw out, in, 1.5, 1.0", "macmv": "macmv out, in, 0.5, 0.5",
        "limit": "limit out, in, 0.5, 0.25", "limitn": "limitn out, in, 0.5, 0.25", "limit_nan_y": "limit out, 0.5, 0.25, in", "tstneg": "tstneg out, in, 0.25, 0",
        "tstneg_x": "tstneg out, 0.5, in, 0", "andxor": "andxor out, in, 15, 3", "skip_on_nan": "macs a, in, 0, 0\nskip ccr, ccr, 0, 1\nmacs out, 0, 0.5, 0.5",
        "delay": "idelay read, rd, at, 0\nidelay write, in, at, 0\nmacs out, rd, 0.5, 0.5", "feedback": "macs a, a, in, 0.5\nmacs out, 0, a, 1.0",
        "chain": "macs a, in, vol, 0.75\nmacsn b, a, in, 0.5\nacc3 out, a, b, in",
    }
    out["nonfinite.json"] = [run_case(k, "itramsize 3 \n" + HDR + v + "\nend", nf, regs=("a", "b", "out", "ccr", "in", "rd")) for k, v in sorted(NONFINITE.items())]

    # 6c. two or three NaN operands at once: which payload the x86 build hands on (SSE returns its FIRST operand's NaN, and
    # which operand is first is the compiler's choice per expression) - pins the operand priority of every arithmetic opcode
    import struct

    def nanf(bits):
        return struct.unpack("<f", struct.pack("<I", bits))[0]
    PAY = {"a": 0x7fc00aaa, "b": 0xffc00bbb, "c": 0x7fc00ccc}
    coll = []
    for op in ("macs", "macsn", "macints", "acc3", "interp", "macw", "macwn", "macintw", "macmv", "limit", "limitn", "tstneg"):
        for mask in range(1, 8):
            who = [r for k, r in enumerate("abc") if mask & (1 << k)]
            sets = {0: [(r, nanf(PAY[r])) for r in who]}
            text = "static a = 0.5\nstatic b = 0.25\nstatic c = 0.125\ninput in 0\noutput out 0\n%s out, a, b, c\nend" % op
            c = run_case("%s_%s" % (op, "".join(who)), text, np.array([0.5, 0.25], np.float32), regs=("out", "ccr", "a", "b", "c"), sets=sets)
            c["sets_bits"] = {"0": [(r, PAY[r]) for r in who]}
            coll.append(c)
    out["nan_collisions.json"] = coll

    # 6d. two to four channels (tests/multichannel_programs.py): the directed programs of the input-refresh rule, 16 generated
    # programs that the restatement reports inside the parity domain, the slider schedule on a stereo program, and the loader's
    # answer to an input index beyond the last channel.  96 samples, one stimulus stream per channel.
    multi = []
    for name, (ch, text, regs) in sorted(mc.DIRECTED.items()):
        multi.append(run_case(name, text, mc.stimulus(progs, 1, 96, ch)[:, :, 0], regs=regs, channels=ch))
    seed = 0
    while sum(c["name"].startswith("generated") for c in multi) < 16:
        ch, text, regs = mc.generated(seed)
        x = mc.stimulus(progs, 1, 96, ch, seed=seed)[:, :, 0].copy()
        o = Oracle(ch)
        assert o.load_text(text)
        o.process_block(x)
        if o.ood_flags() == 0:
            multi.append(run_case("generated%d" % seed, text, x, regs=regs, channels=ch))
        seed += 1
    sets = {0: [("vol", 0.1), ("pan", 0.75)], 24: [("vol", 0.25)], 48: [("vol", 0.5), ("pan", -0.5)], 72: [("vol", 1.0)]}
    multi.append(run_case("slider_stereo", STEREO_SLIDER, mc.stimulus(progs, 1, 96, 2, seed=77)[:, :, 0], channels=2, sets=sets,
                          regs=("vol", "pan", "l", "r", "t", "ol", "or", "ccr")))
    for ch in (2, 4):
        multi.append(run_case("input_index_beyond_%d_channels" % ch, "input a 0\ninput b %d\noutput o 0\nmacs o, a, b, 0.5\nend" % ch,
                              np.zeros((4, ch), np.float32), channels=ch))
    out["multichannel.json"] = multi

    # 7. loader corpus
    corpus = []
    for i, text in enumerate(PARSER_CORPUS):
        r = Reference(1)
        ok = r.load_text(text)
        corpus.append({"program": text, "load_ok": bool(ok), "errors": r.errors(), "controls": r.controls(), "meta": r.meta(), "ready": r.ready()})
    out["parser_corpus.json"] = corpus

    for fn, data in out.items():
        with open(os.path.join(HERE, fn), "w") as fh:
            json.dump(data, fh, indent=0, separators=(",", ":"))
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
