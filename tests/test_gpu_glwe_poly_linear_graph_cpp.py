"""`FheCircuit::glwe_poly_linear` of the C++ host mirror (include/spf_evaluation.hpp) from native code:
tests/cpp/glwe_poly_linear_graph_parity.cpp, built and run as tests/test_gpu_glwe_poly_linear_cpp.py builds its program.  One
scattered layer (inputs out of order, one repeated) and one in-place layer (the first layer's rows); the CSR matrices, the bias,
the inputs and the expected words (tests/glwe_poly_cases.py's poly_linear_ref) are written here."""
import os
import subprocess

import numpy as np
import pytest

import spf_amd
from tests import glwe_poly_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_layers_in_one_graph_match_the_reference_words(tmp_path):
    M1, K, M2, k1, N = GC.row_tile() + 1, 3, 2, 2, 2048               # the program's context is DEFAULT_128 with a short LWE side
    picks = [2, 0, 2]
    a = GC.csr(GC.random_polys(0xC7, M1, K, N, terms=3, cls="seams", empty_every=4), M1, K)
    b = GC.csr(GC.random_polys(0xC8, M2, M1, N, terms=2, cls="mixed"), M2, M1)
    assert not GC.is_constants_only(b)
    bias = GC.random_bias(0xC9, M1, N)
    glwes = GC.uniform_inputs(0xCA, 1, K, k1, N)[0]
    want_a = GC.poly_linear_ref(glwes[picks][None], a, M1, K, bias)
    want_b = GC.poly_linear_ref(want_a, b, M2, M1)
    files = [("a_offsets", a[0], "<u4"), ("a_exponents", a[1], "<u4"), ("a_coefficients", a[2].view(np.uint64), "<u8"), ("a_bias", bias, "<u8"),
             ("b_offsets", b[0], "<u4"), ("b_exponents", b[1], "<u4"), ("b_coefficients", b[2].view(np.uint64), "<u8"),
             ("glwes", glwes, "<u8"), ("want_a", want_a, "<u8"), ("want_b", want_b, "<u8")]
    for name, arr, dt in files:
        np.ascontiguousarray(arr, dtype=dt).tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "glwe_poly_linear_graph_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "glwe_poly_linear_graph_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(M1), str(K), str(M2), str(a[1].size), str(b[1].size)] + [str(i) for i in picks],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
