"""What a load of plaintext polynomial weights decides before a device is touched (spf_amd/csrc/spf_glwe_poly_plan.hpp: the CSR
checks, the classification of a slot, the device image) on the CPU.  tests/cpp/glwe_poly_plan.cpp is a stand-alone program built
from the HIP-free header alone with the system g++ and AddressSanitizer + UndefinedBehaviorSanitizer, and run as a child process
(nothing is loaded into python): every rejection with its message, the term cap read from the last offset alone, and 400 seeded
random descriptions with mutated offsets and exponents through the validator and the packer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glwe_poly_plan") / "glwe_poly_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "glwe_poly_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_every_check_passes_without_a_sanitizer_report(output):
    assert "FAILED" not in output and output.rstrip().endswith("glwe_poly_plan ok"), output[-3000:]


@pytest.mark.parametrize("line", ["slot 64", "null offsets", "null exponents with terms", "null coefficients with terms", "M = 0", "K = 0",
                                  "M above SPF_GLWE_POLY_MAX_ROWS", "M * K above 2^22", "offsets that do not start at 0",
                                  "offsets that decrease", "read from the last offset alone", "an exponent = N",
                                  "a slot is constants-only iff every exponent is 0", "duplicate constants add"])
def test_each_rejection_and_rule_was_exercised(output, line):
    hits = [l for l in output.splitlines() if l.startswith(line) or l.strip().startswith(line) or line in l]
    assert hits and all(l.rstrip().endswith(" ok") for l in hits), (line, hits)


def test_random_descriptions_and_their_mutations(output):
    assert "random: 400 descriptions, 400 legal" in output and ", 0 failed" in output, output[-1000:]
    refused = int(output.split(" mutations refused")[0].rsplit(" ", 1)[1])
    assert refused >= 200, refused
