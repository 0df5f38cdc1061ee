"""The segment plan of the launches whose parameter is per item (spf_amd/csrc/spf_each_plan.hpp: the grouping by parameter, the
runs padded to whole workgroups, the per-workgroup and per-unit tables, the output permutation), on the CPU.
tests/cpp/each_plan.cpp is a stand-alone program built from the HIP-free header alone with the system g++ and AddressSanitizer +
UndefinedBehaviorSanitizer, and run as a child process (nothing is loaded into python).  For 1, 2 and 4 units per workgroup it
checks by brute force: every item owns exactly one unit and one distinct output row and the permutation is a bijection; all units
of a workgroup carry one parameter; a padding unit duplicates an item of its own workgroup and owns no output; the workgroup
count is the sum over runs of ceil(run / units per workgroup)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("each_plan") / "each_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "each_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_every_check_passes_without_a_sanitizer_report(output):
    assert "FAILED" not in output and output.rstrip().endswith("each_plan ok"), output[-3000:]


@pytest.mark.parametrize("line", ["no item: 0 items ok", "one item: 1 items ok", "all items equal: 13 items ok",
                                  "all items distinct: 11 items ok", "one run of exactly a workgroup: 4 items ok",
                                  "a run of exactly a workgroup between two ragged ones: 13 items ok",
                                  "runs of 1, 3 and 5, interleaved: 9 items ok", "parameters at the top of 64 bits: 5 items ok"])
def test_each_named_case_was_planned_and_checked(output, line):
    assert line in output.splitlines(), output[-3000:]


def test_every_small_assignment_and_the_random_cases(output):
    lines = output.splitlines()
    assert "exhaustive: 97655 assignments ok" in lines, output[-3000:]  # 5 + 5^2 + .. + 5^7
    assert "random: 4000 cases ok" in lines, output[-3000:]
