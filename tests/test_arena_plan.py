"""The arena planner of the gate graphs (spf_amd/csrc/spf_arena_plan.hpp: rows are handed on once the level of their last reader
has passed) on the CPU.  tests/cpp/arena_plan.cpp is a stand-alone program built from the HIP-free header alone with the system
g++ and AddressSanitizer + UndefinedBehaviorSanitizer, and run as a child process (nothing is loaded into python).  It checks by
brute force that no two rows alive at the same level share a byte, that every group is one contiguous 256-aligned block, that
peak live bytes <= arena <= the layout without reuse, and that the layout is deterministic: on 300 seeded random group lists and
on the group lists of the three circuits the memory figures are quoted for, recorded here with `spf_amd.mux_circuits`."""
import os
import subprocess

import pytest

import spf_amd
from tests import arena_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arena_plan") / "arena_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "arena_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout and r.stdout.rstrip().endswith("arena_plan ok"), r.stdout[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_random_group_lists_never_share_a_live_byte(program):
    out = _run([program])
    assert "random: 300 lists" in out and ", 0 failed" in out, out


@pytest.mark.parametrize("name", ["add32", "mul8", "mul32"])
def test_circuit_arena_is_within_its_bound(program, tmp_path, name):
    P = spf_amd.DEFAULT_128
    rec = arena_cases.record(name, P)
    base, groups = arena_cases.group_list(rec, P)
    path = str(tmp_path / f"{name}.groups")
    arena_cases.write_group_list(path, base, groups)
    num, den = arena_cases.BOUNDS[name]
    out = _run([program, path, str(num), str(den)])
    print(out)
    # the program's values_bytes is the one computed from the node kinds
    assert f"values_bytes {arena_cases.values_bytes(rec, P)}," in out, out
