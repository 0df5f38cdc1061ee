"""`Evaluation::lwe_linear` of the C++ host mirror (include/spf_evaluation.hpp) from native code: tests/cpp/lwe_linear_parity.cpp,
built and run as tests/test_gpu_cpp_host.py builds its program.  The weights, the bias, the inputs and the expected words
(tests/lwe_linear_cases.py's linear_ref) are written here."""
import os
import subprocess

import numpy as np
import pytest

import spf_amd
from tests import lwe_linear_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_lwe_linear_matches_the_reference_words(tmp_path):
    M, K, B, W = 130, 5, 3, 10                    # the program's context has lwe_dimension = 9
    w = LC.class_weights(0xC4, M, K, 3)
    bias = np.random.default_rng([0xC5]).integers(0, 1 << 64, M, dtype=np.uint64)
    lwes = LC.uniform_inputs(0xC6, B, K, W)
    want = LC.linear_ref(lwes, w, bias)
    for name, a in (("weights", w.view(np.uint64)), ("bias", bias), ("lwes", lwes), ("want", want)):
        np.ascontiguousarray(a, dtype="<u8").tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "lwe_linear_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lwe_linear_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(M), str(K), str(B)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
