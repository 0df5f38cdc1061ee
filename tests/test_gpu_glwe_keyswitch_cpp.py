"""`Evaluation::keyswitch_glwe_to_glwe`, `glwe_automorphism` and `trace` of the C++ host mirror (include/spf_evaluation.hpp) from
native code: tests/cpp/glwe_keyswitch_parity.cpp, built and run as tests/test_gpu_glwe_poly_linear_cpp.py builds its program.  The
keys, the GLWEs and the expected words (the oracle's, tests/glwe_keyswitch_cases.py) are written here."""
import os
import subprocess

import numpy as np
import pytest

import spf_amd
from tests import glwe_keyswitch_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 10


@pytest.mark.gpu
def test_cpp_glwe_keyswitch_and_trace_match_the_oracles_words(tmp_path):
    c = KC.case("default128_6x7")                 # the program's context is DEFAULT_128 with a short LWE side
    P, B = c.P, KC.ITEMS
    files = {"ak": c.hk.ak, "ksk": c.ksk, "glwes": c.x, "want_keyswitch": KC.oracle_keyswitch(P, c.x, c.ksk_fft),
             "want_round": KC.oracle_round(c, c.x, ROUND), "want_trace": KC.oracle_traces(c.name)}
    for name, a in files.items():
        np.ascontiguousarray(a, dtype="<u8").tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "glwe_keyswitch_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "glwe_keyswitch_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(B), str(P.tr_radix_log), str(P.tr_count), str(ROUND)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
