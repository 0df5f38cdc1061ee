"""The pool's wake-up protocols (spf_amd/csrc/spf_wake.hpp: the group tree of the by-handle waiters, the chunk words of the
host-pointer waiters) under forced interleavings: tests/cpp/wake_protocol.cpp parks the completing thread at every test point of
`wake_tree`, runs a late waiter meanwhile, and requires every sleeper back.  No GPU test can pin a window of a few stores; this
program is the proof that no wake-up is lost.  tools/wake_protocol.sh builds it twice with the system g++, plain and with
ThreadSanitizer; both run here as child processes (nothing is loaded into python).  The program cannot hang: it caps every
scenario at 2 s, wakes everything itself and exits 1."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the program enumerates: every (test point, late slot with a child group) of n in {9, 16, 17, 72, 73} = 4 + 4 + 12 + 144 +
# 180 = 344, times {tickets, values} in the group under test, times {late waiter runs through, held behind its last look}
N_EXHAUSTIVE = 344 * 4
N_SAMPLED = 84      # 585: 5 late slots, 4096: 7, up to 8 test points each (duplicates dropped)
N_ABANDONED = 55    # (1 + 1 + 2 + 8 + 9 + 5) parents x {run through, parked behind the first wake} + 3 value-only crowds
N_LATE = 9
N_CHUNK_PLANS = 407
N_CHUNK_SLEEPER_RUNS = 8
NAMED = "n=72 stop=store[0] late_slot=0"


@pytest.fixture(scope="module")
def binaries():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "wake_protocol.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return {v: os.path.join(ROOT, "tools", "bin", name) for v, name in (("plain", "wake_protocol"), ("tsan", "wake_protocol_tsan"))}


@pytest.mark.parametrize("variant", ["plain", "tsan"])
def test_every_sleeper_returns_under_forced_interleavings(binaries, variant):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:exitcode=66")
    r = subprocess.run([binaries[variant]], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    out = r.stdout
    assert f"forced: {N_EXHAUSTIVE} exhaustive + {N_SAMPLED} sampled scenarios, 0 failed" in out, out
    assert f"variants: {N_ABANDONED} abandoned or value-only + {N_LATE} late-arrival scenarios, 0 failed" in out, out
    assert f"chunks: {N_CHUNK_PLANS} plans against the slot loop + {N_CHUNK_SLEEPER_RUNS} sleeper runs, 0 failed" in out, out
    assert "stress: 300 rounds of 64 threads, 0 failed" in out, out
    # the conditions bite: the ascending store order leaves all eight sleepers of group 1 asleep in the scenario it was found in
    reported = [line for line in out.splitlines() if line.startswith("mutant reported")]
    assert len(reported) == 1 and NAMED in reported[0] and "8 of 8 sleepers of group 1" in reported[0], out
    assert "FAILED" not in out and out.rstrip().endswith("wake_protocol ok"), out
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]


def test_the_mutant_as_the_function_under_test_fails_and_names_the_scenario(binaries):
    r = subprocess.run([binaries["plain"], "--mutant"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAILED forced (mutant: ascending stores): " + NAMED in r.stdout, r.stdout
    assert "wake_protocol ok" not in r.stdout
