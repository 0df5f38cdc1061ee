"""`FheCircuit::lwe_linear` of the C++ host mirror (include/spf_evaluation.hpp) from native code:
tests/cpp/lwe_linear_graph_parity.cpp, built and run as tests/test_gpu_pbs_graph_cpp.py builds its program."""
import os
import subprocess

import pytest

import spf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_layer_table_layer_table_in_one_graph_matches_the_dev_calls(tmp_path):
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "lwe_linear_graph_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lwe_linear_graph_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
