"""Every destroy order of the ABI's handles, on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer + LeakSanitizer.

include/spf_hip.h ("Lifetimes"): a child keeps its parent alive, the destroy functions may be called in any order.  The modes
of tools/fuzz_host.cpp (the same instrumented build as tests/test_asan_host.py: tools/asan_host.sh rebuilds it only when
stale) make contexts and groups by hand, without a device, hang graphs, jobs, jobs filed under a merged entry and graphs on
borrowed member contexts off them and destroy everything in the listed orders and in random ones; after every step
`spf_live_objects` must equal a model that knows the rule only.  A parent freed under a child is a heap-use-after-free
report, a parent nobody freed a LeakSanitizer report.  profiles/r22_lifetimes.md holds the reports of the same program on the
tree before the rule existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")

# the scenarios the mode must run, one line each (tools/fuzz_host.cpp, lifetime_scenarios)
SCENARIOS = ["context, graph: graph first", "context, graph: context first", "group, job: job first", "group, job: group first",
             "group, two jobs: group, job 0, job 1", "group, two jobs: group, job 1, job 0", "group, two jobs: job 0, group, job 1",
             "group, two jobs: job 0, job 1, group", "group, two jobs: job 1, group, job 0", "group, two jobs: job 1, job 0, group",
             "merged entry: its job first", "merged entry: the group first", "merged entry: the other job of the entry first",
             "borrowed member context: graph, then group, then graph"]


@pytest.fixture(scope="module")
def fuzz_binary():
    # (builds on first use, and when a source is newer: the whole translation unit)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_host.sh"), "0"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(ROOT, "tools", "bin", "fuzz_host")


def _clean(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_every_listed_destroy_order_is_safe_and_leaves_nothing(fuzz_binary):
    r = subprocess.run([fuzz_binary, "--lifetimes"], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SANITIZERS))
    _clean(r)
    lines = [l for l in r.stdout.splitlines() if l.startswith("lifetimes ") and l.endswith(": ok")]
    assert [l.split(": ", 1)[1][:-len(": ok")] for l in lines] == SCENARIOS, r.stdout
    assert f"lifetimes: {len(SCENARIOS)} scenarios" in r.stdout and "no sanitizer report" in r.stdout


def test_random_forests_in_random_destroy_orders(fuzz_binary):
    # (200000 forests: ~13 s under the sanitizers, profiles/r22_lifetimes.md)
    r = subprocess.run([fuzz_binary, "--lifetimes-random", "200000", "20261019"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **SANITIZERS))
    _clean(r)
    assert "lifetimes-random: 200000 forests" in r.stdout and "no sanitizer report" in r.stdout


def test_the_sanitizer_sees_a_parent_freed_under_its_child(fuzz_binary):
    """a group freed past its reference count and then its job destroyed: the instrumented build must report the read"""
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:exitcode=66:detect_leaks=0")
    r = subprocess.run([fuzz_binary, "--selftest-lifetime"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "heap-use-after-free" in r.stderr, r.stdout + r.stderr[-2000:]
    assert "group_forget_graph" in r.stderr and "no report" not in r.stdout
