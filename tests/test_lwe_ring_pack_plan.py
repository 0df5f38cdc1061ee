"""The launch plan of ring packing (spf_amd/csrc/spf_lwe_ring_pack_plan.hpp: the slices of a call under the scratch cap, a launch per
tree level and one for the tail, the rows every unit reads and writes), on the CPU.  tests/cpp/lwe_ring_pack_plan.cpp is a
stand-alone program built from the HIP-free header alone with the system g++ and AddressSanitizer + UndefinedBehaviorSanitizer, and
run as a child process (nothing is loaded into python).  It replays every launch on a model of the memory, by brute force over
B <= 9, every p <= 64 and caps from one output's worth upward: operands are leaves or rows an earlier launch of the same slice wrote
and nothing overwrote; results and operands of a launch are disjoint; the scratch stays within the cap and within what
spf_lwe_ring_pack_scratch_words reports; every output row is written exactly once, by the last launch of its slice; rounds and X
amounts are the definition's; the launch count is m + 1, m for p = N, 2 for p = 1."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lwe_ring_pack_plan") / "lwe_ring_pack_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "lwe_ring_pack_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_every_check_passes_without_a_sanitizer_report(output):
    assert "FAILED" not in output and output.rstrip().endswith("lwe_ring_pack_plan ok"), output[-3000:]


def test_the_whole_grid_of_calls_was_planned_and_replayed(output):
    m = re.search(r"^calls: (\d+) planned and replayed$", output, flags=re.M)
    assert m and int(m.group(1)) > 3000, output[-3000:]
    m = re.search(r"^checks: (\d+)$", output, flags=re.M)
    assert m and int(m.group(1)) > 1_000_000, output[-3000:]


def test_the_slice_loop_stands_in_the_plan_header_only():
    """tests/test_launch_slice_cases.py claims every `at +=` / `m0 +=` loop of spf_hip.hip for its table: ring packing's loop over
    slices is the plan's, which this file and the GPU tests hold"""
    with open(os.path.join(ROOT, "spf_amd", "csrc", "spf_hip.hip")) as f:
        src = f.read()
    body = src[src.index("ring packing: LWE / GLWE leaves into one GLWE"):src.index("one launch over items with a parameter each")]
    assert "spf_ring_pack::plan(" in body and "plan_slice(0, B, p, N)" in body
    assert not re.search(r"\b(at|m0)\s*\+=", body)
    with open(os.path.join(ROOT, "spf_amd", "csrc", "spf_lwe_ring_pack_plan.hpp")) as f:
        plan = f.read()
    assert "hip_runtime" not in plan and "__global__" not in plan and "__device__" not in plan
