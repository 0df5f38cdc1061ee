"""`Evaluation::public_functional_keyswitch` of the C++ host mirror (include/spf_evaluation.hpp) from native code: tests/cpp/
public_functional_keyswitch_parity.cpp, built and run as tests/test_gpu_cpp_host.py builds its program.  The key, the inputs and
the expected words (tests/pufks_cases.py's pufks_oracle) are written here."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import pufks_cases as PC
from tests.polyref_cases import key_fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_public_functional_keyswitch_matches_the_oracles_words(tmp_path):
    P = O.DEFAULT_128
    n, log, count, p, B = 5, 4, 8, 33, 3
    rng = np.random.default_rng([0xC3, n, count, p, B])
    key = rng.integers(0, 1 << 64, (n, count, P.k + 1, P.N), dtype=np.uint64)
    lwes = rng.integers(0, 1 << 64, (B, p, n + 1), dtype=np.uint64)
    keyf = key_fft(key)
    want = np.stack([PC.pufks_oracle(x, keyf, P.N, P.k, log, count) for x in lwes])
    for name, a in (("key", key), ("lwes", lwes), ("want", want)):
        np.ascontiguousarray(a, dtype="<u8").tofile(tmp_path / f"{name}.bin")
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "public_functional_keyswitch_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "public_functional_keyswitch_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(n), str(log), str(count), str(p), str(B)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
