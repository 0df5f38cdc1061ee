"""`Evaluation::blind_rotation` of the C++ host mirror (include/spf_evaluation.hpp) from native code: tests/cpp/
blind_rotation_parity.cpp, built and run as tests/test_gpu_cpp_host.py builds its program."""
import os
import subprocess

import pytest

import oracle as O
import spf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_blind_rotation_matches_the_c_call_and_the_oracle(tmp_path):
    libdir = os.path.dirname(spf_amd.lib_path())
    oracle_so = O.library_path()
    exe = tmp_path / "blind_rotation_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "cpp", "blind_rotation_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", oracle_so,
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.dirname(oracle_so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
