"""`Evaluation::glwe_poly_linear` of the C++ host mirror (include/spf_evaluation.hpp) from native code:
tests/cpp/glwe_poly_linear_parity.cpp, built and run as tests/test_gpu_lwe_linear_cpp.py builds its program.  The CSR matrix, the
bias, the inputs and the expected words (tests/glwe_poly_cases.py's poly_linear_ref) are written here."""
import os
import subprocess

import numpy as np
import pytest

import spf_amd
from tests import glwe_poly_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_glwe_poly_linear_matches_the_reference_words(tmp_path):
    M, K, B, k1, N = GC.row_tile() + 1, 3, 2, 2, 2048             # the program's context is DEFAULT_128 with a short LWE side
    off, exp, coef = GC.csr(GC.random_polys(0xC4, M, K, N, terms=3, cls="seams", empty_every=4), M, K)
    bias = GC.random_bias(0xC5, M, N)
    glwes = GC.uniform_inputs(0xC6, B, K, k1, N)
    want = GC.poly_linear_ref(glwes, (off, exp, coef), M, K, bias)
    for name, a, dt in (("offsets", off, "<u4"), ("exponents", exp, "<u4"), ("coefficients", coef.view(np.uint64), "<u8"), ("bias", bias, "<u8"),
                        ("glwes", glwes, "<u8"), ("want", want, "<u8")):
        np.ascontiguousarray(a, dtype=dt).tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "glwe_poly_linear_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "glwe_poly_linear_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(M), str(K), str(B), str(exp.size)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
