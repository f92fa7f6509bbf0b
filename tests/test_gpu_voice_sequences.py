"""Call sequences over the by-list state operations against the oracle (tools/fuzz_voices.py): random programs, then
fxb_set_registers_list / _get_, fxb_copy_instances, fxb_reset_instances, fxb_save_instances, fxb_load_instances,
fxb_load_instances_rotated, fxb_set_tram_list / _get_ in any order between blocks, register writes, tracks and list schedules -
every output, register, position, delay-memory word, LFSR word and counter of the tracked instances bit for bit against a voice
model made of oracle objects, and every call the header refuses refused with nothing changed.  The tests of each of these calls
(test_gpu_instances.py, _instances_rot, _register_list, _tram_list, _track_list) apply it once or twice to a hand-written program
and compare with a twin handle; what only a sequence finds - a per-instance write while a register is folded, a copy in front of a
block that adopts cached code, a reset behind a list set, a logical window behind a rotated load - is here.
tests/test_voice_sequences_model.py asserts, without a GPU, what these seed ranges cover.  Also the slice of tools/fuzz_api.py
that the suite lacked.

Sizes: N out of 1, 63, 64, 65, 130, 200 and blocks of at most 40 samples - where lane, wavefront and tile edges sit; no benchmark
shape.  Every case takes one to two seconds on an MI355X (the figures measured per case stand in the docstrings)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

# tier -> environment (everything else that starts with FX_ is cleared)
TIERS = {
    "default": {},
    "asm": {"FX_KERNEL": "asm"},
    "hip": {"FX_KERNEL": "hip"},
    "hip_2_per_lane": {"FX_KERNEL": "hip", "FX_INST_PER_LANE": "2"},
    "two_shards": {"FX_FUZZ_SHARDS": "2"},
}
CASES = [("main", t) for t in TIERS] + [("wild", "default"), ("dane", "default"), ("dane", "asm"), ("staged", "default"), ("staged", "two_shards")]


def ran_staged_code(cover, count):
    """the staged range must not pass green on plain code: FXB_INFO_WAVES_PER_WG behind every device block (cover["staged_blocks"])"""
    sb = cover["staged_blocks"]
    assert sb["kernels"] and all(k >= 9 for k in sb["kernels"]), sb                # staged blocks ran translated code
    assert sb["sequences"] == count, sb                                            # every sequence ran at least one staged block
    assert sb["plain"][1] > sb["plain"][0], sb                                     # among blocks that armed no schedule, staged ones outnumber the others
    assert sb["scheduled"][1] == 0 and sb["scheduled"][0] > 0, sb                  # a block with a track or a list schedule runs one wavefront per workgroup


def set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("FX_")]:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("slice_name, tier", CASES, ids=["%s-%s" % c for c in CASES])
def test_voice_sequences(gpu, slice_name, tier, monkeypatch):
    """20 sequences of 36 steps per case, every bit compared equal, and the same range once more with the model alone (half a
    second).  Measured on an MI355X, seconds per case: main-default 2.13, main-asm 1.62, main-hip 1.68, main-hip_2_per_lane 1.67,
    main-two_shards 1.85, wild-default 1.53, dane-default 1.63, dane-asm 1.53 (about 65 ms per sequence on the device: 20 is what
    a second buys, 12 is the floor).
    The staged range (generator 4 under FX_STAGES=4) also asserts that it ran staged code: ran_staged_code().  Measured:
    staged-default 1.16 s, staged-two_shards 1.34 s; of the 151 device blocks that armed no schedule 114 ran staged (all on kernel
    13) and 37 one wavefront per workgroup - behind their handle's first schedule, which ends staged code for that handle
     -, the 31 blocks with a schedule one wavefront per workgroup, 20 of 20 sequences ran a staged block."""
    import fuzz_voices
    first, count, env = fuzz_voices.SLICES[slice_name]
    assert count >= 12
    set_env(monkeypatch, dict(env, **TIERS[tier]))
    cover = fuzz_voices.new_cover(stages=True)
    bad = [s for s in range(first, first + count) if not fuzz_voices.run(s, cover=cover)]
    assert bad == [], bad
    assert cover["loaded"] == count and cover["left_domain"] * 10 <= count, cover
    # these ARE the sequences whose coverage tests/test_voice_sequences_model.py asserts: the model alone, run over the same range,
    # stands at the same place of the random stream in front of every step and counts the same calls, accepted and refused
    alone = fuzz_voices.new_cover()
    assert all(fuzz_voices.run(s, device=False, cover=alone) for s in range(first, first + count))
    device_only = ("kernels", "sharded_handles", "staged_blocks")
    assert {k: v for k, v in cover.items() if k not in device_only} == {k: v for k, v in alone.items() if k not in device_only}
    if tier == "two_shards":
        assert cover["sharded_handles"] >= 5, cover      # (N of 1, 63 and 64 is one wavefront: one batch)
    else:
        assert cover["sharded_handles"] == 0, cover
    # the tier asked for is the tier that ran (FXB_INFO_KERNEL: 0 HIP C++, 1..8 the interpreter, 9..15 translated code)
    kernels = cover["kernels"]
    if tier.startswith("hip"):
        assert set(kernels) == {0}, kernels
    elif tier == "asm":
        assert kernels and all(1 <= k <= 8 for k in kernels), kernels
    else:
        assert sum(v for k, v in kernels.items() if k >= 9) * 2 > sum(kernels.values()), kernels
    print("staged blocks:", cover["staged_blocks"], "kernels:", kernels)
    if slice_name == "staged":
        ran_staged_code(cover, count)


# switch -> what a report that notices THAT aspect says (the state reads name what differs; the list gets name themselves)
ASPECT = {
    "copy_drops_lfsr": ("LFSR",),
    "reset_zeroes_positions": ("POSITIONS",),
    "reset_uses_initial_not_last_broadcast": ("REGISTER", "get_registers_list"),
    "logical_window_off_by_one": ("get_tram_list", "iTRAM [", "xTRAM ["),
    "rotated_load_unrotated": ("get_tram_list", "iTRAM [", "xTRAM ["),
    "list_set_skips_last_entry": ("REGISTER", "get_registers_list"),
}


@pytest.mark.parametrize("switch", sorted(ASPECT))
def test_a_wrong_model_is_noticed(gpu, switch, monkeypatch, capsys):
    """FX_FUZZ_BREAK makes the MODEL wrong in one respect; the main range on the default tier must report a mismatch - else the
    sequences are blind there.  A comparison that fails in python: nothing on the device is provoked.  Measured on an MI355X: 0.96 to
    1.29 s per switch (the whole range runs, so that the message shows how many sequences notice)."""
    import fuzz_voices
    assert switch in fuzz_voices.BREAKS
    first, count, env = fuzz_voices.SLICES["main"]
    set_env(monkeypatch, dict(env, FX_FUZZ_BREAK=switch))
    noticed = [s for s in range(first, first + count) if not fuzz_voices.run(s, cover=fuzz_voices.new_cover())]
    assert noticed, switch
    reports = [line for line in capsys.readouterr().out.split("\n") if line.startswith("MISMATCH")]
    assert len(reports) == len(noticed)
    # noticed in its own aspect, not through whatever the wrong state upsets later (a load refused, a block that differs)
    assert [r for r in reports if any(word in r for word in ASPECT[switch])], reports


def test_a_wrong_model_is_noticed_between_staged_blocks(gpu, monkeypatch, capsys):
    """the position rows live in stage 0 of staged code: a model whose reset zeroes them (FX_FUZZ_BREAK=reset_zeroes_positions)
    must be reported on the staged range too, in its own aspect - and the range must have run staged code while it was.
    Measured on an MI355X: 0.74 s; 7 of the 20 sequences notice; 104 staged and 31 other blocks without a
    schedule, 26 with one."""
    import fuzz_voices
    first, count, env = fuzz_voices.SLICES["staged"]
    set_env(monkeypatch, dict(env, FX_FUZZ_BREAK="reset_zeroes_positions"))
    cover = fuzz_voices.new_cover(stages=True)
    noticed = [s for s in range(first, first + count) if not fuzz_voices.run(s, cover=cover)]
    assert noticed
    reports = [line for line in capsys.readouterr().out.split("\n") if line.startswith("MISMATCH")]
    assert len(reports) == len(noticed)
    assert [r for r in reports if any(word in r for word in ASPECT["reset_zeroes_positions"])], reports
    print("noticed by", len(noticed), "sequences; staged blocks:", cover["staged_blocks"])
    ran_staged_code(cover, count)


@pytest.mark.parametrize("mode, env", [("default", {}), ("asm", {"FX_KERNEL": "asm"}), ("hip", {"FX_KERNEL": "hip"}), ("two_shards", {"FX_FUZZ_SHARDS": "2"}),
                                       ("panel", {"FX_FUZZ_PANEL": "1"}), ("wild", {"FX_FUZZ_WILD": "1"})])
def test_api_fuzz_slice(gpu, mode, env, monkeypatch):
    """tools/fuzz_api.py, 24 sequences per mode: the fuzzer that found the product-cache, stream-change and schedule-overwrite
    defects (docs/history.md section 2) had no slice in the suite.  Measured on an MI355X, seconds per mode: default 0.99, asm 0.76,
    hip 0.76, two_shards 1.08, panel 0.90, wild 0.90."""
    import fuzz_api
    set_env(monkeypatch, env)
    monkeypatch.setattr(fuzz_api, "WILD", mode == "wild")       # (read from the environment when the module was imported)
    monkeypatch.setattr(fuzz_api, "PANEL", mode == "panel")
    monkeypatch.setattr(fuzz_api, "PINNED", False)
    monkeypatch.setattr(fuzz_api, "NOCOMPARE", False)
    monkeypatch.setitem(fuzz_api.STATS, "loaded", 0)
    monkeypatch.setattr(sys, "argv", ["fuzz_api.py", "4200", "24"])
    assert fuzz_api.main() == 0
    assert fuzz_api.STATS["loaded"] == 24
