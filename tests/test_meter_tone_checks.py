"""tests/hipstub/tone_meter_checks.cpp (csrc/Makefile `stubasanmetertone`): the tone meters through the C ABI with tone rows, lists,
gathered rows, select lists and rank lists and values on exactly-sized heap blocks - one, two and four channels, one, three and
eight tones, lists with repeats and with one entry per shard - the refusals and the allocation failures, on one handle and on three
shards, under AddressSanitizer + UBSan + LeakSanitizer.  The program links the sanitizer runtime itself: nothing is preloaded and no
interpreter is involved.  This file only builds it, runs it and asks for its marker line."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc")


def test_tone_meter_indexing_and_refusals_under_asan_in_a_program_of_its_own():
    subprocess.check_call(["make", "-s", "-j6", "-C", CSRC, "stubasanmetertone"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "stubasan", "tone_meter_checks")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "tone meter checks ok" in r.stdout, r.stdout[-6000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-6000:]
