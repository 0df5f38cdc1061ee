"""The polynomial linear nodes (`spf_graph_add_glwe_poly_linear`) in the planner of the gate graphs
(spf_amd/csrc/spf_graph_plan.hpp), on the CPU.  tests/cpp/glwe_poly_graph_plan.cpp is a stand-alone program built from the
HIP-free header alone with the system g++ and AddressSanitizer + UndefinedBehaviorSanitizer, and run as a child process (nothing
is loaded into python).  It builds hand-made graphs that mix the new kind with inputs, XOR, pack, unpack and LWE layers, and checks
by brute force: the key, layer-major members, in place exactly when the layers * K rows are consecutive, the table row equal to the
operand offsets in order, outputs [layers][M] consecutive, has_glwe_poly, append shifting the lists, and that two calls with
another slot, M or K on one level are different groups."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glwe_poly_graph_plan") / "glwe_poly_graph_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "glwe_poly_graph_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_every_check_passes_without_a_sanitizer_report(output):
    assert "FAILED" not in output and output.rstrip().endswith("glwe_poly_graph_plan ok"), output[-3000:]


@pytest.mark.parametrize("line,groups", [("in place: an XOR group, a previous layer", 2), ("in place: the same at 3072-byte GLWEs", 2),
                                         ("in place: a pack group", 1), ("in place: two layers, lists one behind the other", 1),
                                         ("table: two layers, lists the other way round", 1),
                                         ("in place: inputs of 256 bytes, slot 63, M = 4096", 1), ("table: inputs of 128 bytes are padded apart", 1),
                                         ("in place: one lone row", 1), ("table: two lone rows out of order", 1),
                                         ("scattered: two layers of a key, three foreign keys, another level", 5),
                                         ("scattered: the same at 3072-byte GLWEs", 5),
                                         ("scattered: two unpacks of a layer's rows, out of order", 1), ("no polynomial linear node", 0),
                                         ("append: two graphs' layers of one key are one group", 2)])
def test_each_graph_was_planned_and_checked(output, line, groups):
    assert f"{line}: {groups} groups ok" in output.splitlines(), output[-3000:]


def test_append_shifts_the_lists(output):
    assert "append shifts the lists ok" in output.splitlines()
