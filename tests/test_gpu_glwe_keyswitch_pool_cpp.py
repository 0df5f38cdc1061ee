"""`PooledEvaluation::keyswitch_glwe_to_glwe`, `glwe_automorphism` and `trace` of the C++ host mirror (include/spf_evaluation.hpp)
from native code: tests/cpp/glwe_keyswitch_pool_parity.cpp, built and run as tests/test_gpu_glwe_keyswitch_graph_cpp.py builds its
program.  On the generic N = 16 context, in pushed mode: scattered operands through the rows kernel, and a chain on pending
operands behind one wait.  The keys, the GLWEs and the expected words (the oracle's, tests/glwe_keyswitch_cases.py) are written
here."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 3


@pytest.mark.gpu
def test_cpp_pool_by_handle_matches_the_oracles_words(tmp_path):
    c = KC.case("N16")
    P, B = c.P, KC.ITEMS
    second = KC.second_key(c)
    ones = KC.all_ones_glwe(c)
    rotated = O.glwe_mul_xn(ones.reshape(-1), 2 * P.N - 3, P.N, P.k)
    traced = G.oracle_trace(c, rotated)
    k0 = KC.oracle_keyswitch(P, traced, c.ksk_fft)
    files = {"ak": c.hk.ak, "ksk0": c.ksk, "ksk1": second[0], "glwes": c.x, "ones": ones,
             "want_keyswitch": KC.oracle_keyswitch(P, c.x, c.ksk_fft), "want_round": KC.oracle_round(c, c.x, ROUND),
             "want_trace": KC.oracle_traces(c.name), "want_chain_trace": traced,
             "want_chain_extract": O.sample_extract(traced.reshape(-1), 0, P.N, P.k), "want_chain_k0": k0,
             "want_chain_k1": KC.oracle_keyswitch(P, k0, second[1])}
    for name, a in files.items():
        np.ascontiguousarray(a, dtype="<u8").tofile(tmp_path / f"{name}.bin")
    KC.check_can_trace(c, traced, "the driver's own chain")
    ep = G.engine_params(P)
    fields = [ep.lwe_dimension, ep.polynomial_degree, ep.glwe_size, ep.pbs_radix_log, ep.pbs_radix_count, ep.cbs_radix_log, ep.cbs_radix_count,
              ep.ks_radix_log, ep.ks_radix_count, ep.tr_radix_log, ep.tr_radix_count, ep.ss_radix_log, ep.ss_radix_count]
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path / "glwe_keyswitch_pool_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "glwe_keyswitch_pool_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), str(tmp_path), str(B), str(ROUND)] + [str(int(f)) for f in fields], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout and "MISMATCH" not in r.stdout, r.stdout
