"""`FheCircuit::glwe_keyswitch`, `glwe_automorphism` and `glwe_trace` of the C++ host mirror (include/spf_evaluation.hpp) from
native code: tests/cpp/glwe_keyswitch_graph_parity.cpp, built and run as tests/test_gpu_glwe_keyswitch_cpp.py builds its program.
The three nodes over inputs out of order with a repeat, and a trace of the keyswitched rows where they lie; the same graph through
the C calls.  The keys, the GLWEs and the expected words (the oracle's, tests/glwe_keyswitch_graph_cases.py) are written here."""
import os
import subprocess

import numpy as np
import pytest

import spf_amd
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 3
PICKS = [4, 0, 2, 0, 1]


@pytest.mark.gpu
def test_cpp_nodes_match_the_c_calls_and_the_oracles_words(tmp_path):
    c = KC.case(G.TUNED)                          # the program's context is DEFAULT_128 with a short LWE side
    P, B = c.P, KC.ITEMS
    x = c.x[PICKS]
    switched = KC.oracle_keyswitch(P, x, c.ksk_fft)
    files = {"ak": c.hk.ak, "ksk": c.ksk, "glwes": c.x, "want_keyswitch": switched, "want_round": KC.oracle_round(c, x, ROUND),
             "want_trace": KC.oracle_traces(c.name)[PICKS], "want_chain": np.stack([G.oracle_trace(c, g) for g in switched])}
    for name, a in files.items():
        np.ascontiguousarray(a, dtype="<u8").tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "glwe_keyswitch_graph_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "glwe_keyswitch_graph_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(B), str(P.tr_radix_log), str(P.tr_count), str(ROUND)] + [str(i) for i in PICKS],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
