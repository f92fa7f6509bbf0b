"""The three programs of the staged-route tests and the registers those tests name: texts and names only (no library, no device).
Shared by test_staged_route_programs.py - which asserts without a GPU that the planner cuts them and that the named registers are
stored by different stages - and test_gpu_staged_routes.py, which runs them on the device between by-list calls, on the bus and
instance-major routes and under the meters.

config2: mono, `cutoff` is read by the INTERP of every stage.  mixed_stages(3): a delay line with feedback and noise (both live in
stage 0), a SKIP with its shadow and a LOG / EXP pair per section; `k` is read in every stage.  generated_chain(1): three channels,
inputs read late, outputs written in different stages."""
import fx8010_programs as progs
import multichannel_programs as mc


def _chain():
    channels, text, regs = mc.generated_chain(1)
    assert channels == 3
    return text


def _log_control():
    text = progs.mixed_stages(3).replace("control k = 0.25", "control k = 0.25\ncontrol e = 3", 1).replace("log w, u, 3, 0", "log w, u, e, 0")
    assert text.count("log w, u, e, 0") == 3
    return text


# name -> (channels, text, the state registers the GPU tests compare by name, the control every stage reads)
PROGRAMS = {
    "config2": (1, progs.config2(), ("t", "s0", "s7", "s15", "s22", "s30", "out"), "cutoff"),
    "mixed": (1, progs.mixed_stages(3), ("rd", "a", "t", "u", "w", "s0", "s3", "s9", "s14", "s19", "s25", "s29", "out"), "k"),
    "chain3": (3, _chain(), ("t", "s0", "s10", "s20", "s30", "s40", "o0", "o1", "o2"), "cutoff"),
    # mixed_stages(3) with the table number of its LOGs in a control: a value that shapes the code itself, so a write to it cannot
    # become a row - the library interprets for a few blocks (the translation is deferred) and then translates, and cuts, again
    "mixed_e": (1, _log_control(), ("rd", "a", "t", "u", "w", "s0", "s3", "s9", "s14", "s19", "s25", "s29", "out"), "k"),
}

# stages the front end cuts them into when 2, 4 and 8 are asked (tests/test_staged_route_programs.py asserts these)
CUTS = {"config2": (2, 4, 8), "mixed": (1, 2, 3), "chain3": (2, 4, 8), "mixed_e": (1, 2, 3)}

# programs the DEFAULT policy runs as staged code at 200 instances in blocks of a few dozen samples (measured on an MI355X; for
# mixed_stages(3) the planner's costs put its two stages above the plain program there)
DEFAULT_POLICY_STAGES = ("config2", "chain3")
