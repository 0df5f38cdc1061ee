"""`Evaluation::private_functional_keyswitch` of the C++ host mirror (include/spf_evaluation.hpp) from native code: tests/cpp/
private_functional_keyswitch_parity.cpp, built and run as tests/test_gpu_cpp_host.py builds its program.  The keys, the inputs
and the expected words (tests/pfks_cases.py's pfks_ref) are written here."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import pfks_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_private_functional_keyswitch_matches_the_reference_words(tmp_path):
    P = O.DEFAULT_128
    n_keys, n, p, log, count, B = 2, 5, 3, 17, 2, 3
    keys, lwes = PC.uniform_case(0xC3, P.N, P.k, n, p, log, count, B, n_keys)
    want = np.stack([PC.pfks_ref(lwes, keys[q], log, count) for q in range(n_keys)])
    for name, a in (("keys", keys), ("lwes", lwes), ("want", want)):
        np.ascontiguousarray(a, dtype="<u8").tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "private_functional_keyswitch_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "private_functional_keyswitch_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(n_keys), str(n), str(p), str(log), str(count), str(B)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
