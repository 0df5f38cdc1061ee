"""The GLWE keyswitch, automorphism and trace nodes (`spf_graph_add_glwe_keyswitch` / `_automorphism` / `_trace`, kinds 70, 71, 72)
in the planner of the gate graphs (spf_amd/csrc/spf_graph_plan.hpp), on the CPU.  tests/cpp/glwe_keyswitch_graph_plan.cpp is a
stand-alone program built from the HIP-free header alone with the system g++ and AddressSanitizer + UndefinedBehaviorSanitizer,
and run as a child process (nothing is loaded into python).  On hand-made and on small seeded random graphs it checks by brute
force: every new node in exactly one group, a group uniform in (level, kind, parameter), in place exactly when the operands lie
consecutively, the table row equal to the operand offsets in order, the output rows disjoint from every operand row of the group,
has_glwe_ks, append shifting the operands, and that a graph without the kinds keeps its plan when new nodes are stacked on it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glwe_keyswitch_graph_plan") / "glwe_keyswitch_graph_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "glwe_keyswitch_graph_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_every_check_passes_without_a_sanitizer_report(output):
    assert "FAILED" not in output and output.rstrip().endswith("glwe_keyswitch_graph_plan ok"), output[-3000:]


@pytest.mark.parametrize("line,groups", [("in place: an XOR group under the three modes", 3), ("in place: the same at 3072-byte GLWEs", 3),
                                         ("table: an XOR group the other way round", 1), ("in place: inputs of 256 bytes", 1),
                                         ("table: inputs of 128 bytes are padded apart", 1), ("in place: one lone operand", 1),
                                         ("table: a duplicated operand", 1), ("grouping: two slots, two rounds, another level", 5),
                                         ("chains: every kind reads the one before", 4), ("no new node", 0),
                                         ("append: two graphs' keyswitches of one slot are one group", 3)])
def test_each_hand_made_graph_was_planned_and_checked(output, line, groups):
    assert f"{line}: {groups} groups ok" in output.splitlines(), output[-3000:]


def test_random_graphs_reach_both_forms(output):
    assert "random graphs: 120 graphs ok" in output.splitlines(), output[-3000:]


def test_graphs_without_the_kinds_plan_as_before(output):
    lines = [l for l in output.splitlines() if l.startswith("unchanged below: ")]
    assert len(lines) == 1 and lines[0].endswith(" graphs ok"), output[-3000:]


def test_append_shifts_the_operands(output):
    assert "append shifts the operands ok" in output.splitlines()
