"""The public functional keyswitch (`public_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/public_functional_keyswitch.rs:
74-148) without a GPU: the oracle's composition against exact integer arithmetic (tier A), what the operation means on the exact
chain with an honest key, and the entry points' argument checks and bindings.  The GPU side is
tests/test_gpu_public_functional_keyswitch.py; figures: profiles/r18_public_functional_keyswitch.md."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spf_amd
from spf_amd import _ffi
from tests import pufks_cases as PC
from tests.polyref_cases import check_tier_a, key_fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["spf_load_public_functional_keyswitch_key_std", "spf_public_functional_keyswitch_batch",
               "spf_public_functional_keyswitch_enqueue", "spf_last_public_functional_keyswitch_kernel",
               "spf_group_load_public_functional_keyswitch_key_std", "spf_group_public_functional_keyswitch_batch"]


@pytest.mark.parametrize("shape", PC.TIER_A, ids=PC.tier_a_name)
def test_oracle_composition_against_exact_arithmetic(shape):
    N, k, n, count, log, p, _ = shape
    c, lwes, exact, nump = PC.tier_a_case(shape)
    got = PC.pufks_oracle(lwes, key_fft(c.key), N, k, log, count)
    check_tier_a(c, [got], [exact], [nump], "oracle")


@pytest.mark.parametrize("shape", PC.MEANING, ids=lambda s: f"N{s[0]}k{s[1]}-n{s[2]}-{s[3]}x{s[4]}")
def test_exact_chain_with_an_honest_key_holds_message_j_at_coefficient_j(shape):
    N, k, n, count, log = shape
    lwe_sk, glwe_sk, key = PC.meaning_keys(shape)
    for p in (1, 33, N):
        lwes = PC.meaning_lwes(shape, p)
        PC.check_meaning(PC.pufks_exact(lwes, key, log, count), lwes, lwe_sk, glwe_sk, count, log, "exact")


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _ffi.load_library()
    N = spf_amd.DEFAULT_128.polynomial_degree
    x = np.zeros(8, dtype=np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    # a null context or group is refused whatever else is given: wrong n_words, radix_log * radix_count >= 64, null pointers
    for key, n_words, n, log, count in [(p, 8, 1, 4, 4), (p, 7, 1, 4, 4), (p, 8, 1, 8, 8), (p, 8, 0, 4, 4), (None, 8, 1, 4, 4)]:
        assert lib.spf_load_public_functional_keyswitch_key_std(None, key, n_words, n, log, count) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_group_load_public_functional_keyswitch_key_std(None, key, n_words, n, log, count) == 1
        assert b"null" in lib.spf_last_error(None)
    for B, cnt, a, b in [(1, 1, p, p), (0, 1, p, p), (1, 0, p, p), (1, N + 1, p, p), (1 << 40, 2, p, p), (1, 1, None, p), (1, 1, p, None)]:
        assert lib.spf_public_functional_keyswitch_batch(None, B, cnt, a, b) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_public_functional_keyswitch_enqueue(None, None, B, cnt, a, b) == 1
        assert lib.spf_group_public_functional_keyswitch_batch(None, B, cnt, a, b) == 1
        assert b"null" in lib.spf_last_error(None)
    assert lib.spf_last_public_functional_keyswitch_kernel(None) == b""


def test_new_symbols_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "spf_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "spf_hip.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {s[0] for s in _ffi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in bound, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert "`" + name + "`" in integration, name
    assert not re.search(r"spf_public_functional_keyswitch\w*_dev\(", header)   # (the `_dev` table of tests/stream_cases.py is closed)
    for method in ("load_public_functional_keyswitch_key_std", "public_functional_keyswitch", "public_functional_keyswitch_enqueue",
                   "last_public_functional_keyswitch_kernel"):
        assert callable(getattr(spf_amd.Engine, method)), method
        assert callable(getattr(spf_amd.Group, method)), method
    mirror = open(os.path.join(ROOT, "include", "spf_evaluation.hpp")).read()
    assert "public_functional_keyswitch(" in mirror
