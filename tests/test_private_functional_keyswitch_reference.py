"""The private functional keyswitch (`private_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/private_functional_keyswitch.rs:
107-142) on the CPU: tests/pfks_cases.py's `pfks_ref` is held to a literal Python-integer restatement of the reference's loop, its
meaning is checked with honest keys built as `generate_private_functional_keyswitch_key` builds them, and the binding declares
every entry point the header does."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import pfks_cases as PC
from tests import poly_ref as R
from tests.decomp_ref import M64

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = [
    "spf_load_private_functional_keyswitch_keys_std", "spf_private_functional_keyswitch_batch",
    "spf_private_functional_keyswitch_enqueue", "spf_apply_pfks_on_ggsw_components_batch",
    "spf_apply_pfks_on_ggsw_components_enqueue", "spf_circuit_bootstrap_via_pfks_batch", "spf_circuit_bootstrap_via_pfks_enqueue",
    "spf_last_private_functional_keyswitch_kernel", "spf_group_load_private_functional_keyswitch_keys_std",
    "spf_group_private_functional_keyswitch_batch", "spf_group_circuit_bootstrap_via_pfks_batch",
]


# ---- pfks_ref against the literal loop --------------------------------------------------------------------------------------

@pytest.mark.parametrize("log,count", PC.RADICES)
def test_pfks_ref_is_the_references_loop(log, count):
    """tiny shapes (N 4, k 1 and N 2, k 2), every radix class, extreme words among the inputs, planted words in the key"""
    for N, k, n, p in [(4, 1, 2, 1), (2, 2, 1, 3)]:
        key, lwes = PC.uniform_case(1, N, k, n, p, log, count, 2)
        key = key[0]
        ext_key, ext_lwes = PC.extreme_case(2, N, k, n, p, log, count, 2)
        key.reshape(-1)[1:1 + len(PC.PLANTED)] = PC.PLANTED
        lwes[1] = ext_lwes[1]
        for kk, xx in ((key, lwes), (ext_key, ext_lwes)):
            got = PC.pfks_ref(xx, kk, log, count)
            for b in range(xx.shape[0]):
                want = PC.pfks_literal(xx[b], kk, log, count)
                assert [int(v) for v in got[b]] == want, (log, count, N, k, n, p, b)
            assert np.array_equal(PC.pfks_ref(xx[0], kk, log, count), got[0])


def test_extreme_case_holds_every_extreme_word():
    from tests.decomp_ref import extreme_words
    for log, count in PC.RADICES:
        key, lwes = PC.extreme_case(3, 8, 1, 5, 3, log, count, 2)
        assert set(extreme_words(log, count)) <= {int(v) for v in lwes.reshape(-1)}
        assert set(PC.PLANTED) <= {int(v) for v in key.reshape(-1)}


def test_limb_form_reproduces_the_digits():
    """what the matrix-core path relies on: a digit of up to 23 bits is the sum of U balanced int8 limbs"""
    for log in range(1, 24):
        U = 1 if log <= 8 else -(-(log + 1) // 8)
        assert U <= 3
        for d in {-(1 << (log - 1)), (1 << (log - 1)) - 1, 0, -1, 1, 127, 128, -128, -129} | set(
                int(v) for v in np.random.default_rng(log).integers(-(1 << (log - 1)), 1 << (log - 1), 64)):
            if not -(1 << (log - 1)) <= d < (1 << (log - 1)):
                continue
            rest, limbs = d, []
            for _ in range(U):
                e = ((rest + 128) & 0xff) - 128
                limbs.append(e)
                rest = (rest - e) >> 8
            assert rest == 0 and all(-128 <= e <= 127 for e in limbs), (log, d, limbs)
            assert sum(e << (8 * u) for u, e in enumerate(limbs)) == d
    # 16 bits do not fit two balanced limbs: 32767 = -1 + 256 * 128
    assert ((32767 + 128) & 0xff) - 128 == -1 and (32767 + 1) >> 8 == 128


def limb_form(lwes, key, log, count):
    """the matrix-core path's arithmetic on Python integers, for one output: U balanced int8 limbs per digit, the key words as eight
    byte planes stored as byte - 128, int32-sized plane sums, the 128 * rowsum correction, a shift of 8 (t + u) bits, skipped
    from 64 on, everything else mod 2^64"""
    from tests.decomp_ref import digits_array
    p, rows = lwes.shape
    w = key.shape[3] * key.shape[4]
    d = [int(v) for v in digits_array(lwes, log, count).reshape(-1)]
    rev = key[:, :, ::-1].reshape(p * rows * count, w)
    U = 1 if log <= 8 else -(-(log + 1) // 8)
    total = [0] * w
    for u in range(U):
        e = [((v + 128) & 0xff) - 128 for v in d]
        d = [(v - x) >> 8 for v, x in zip(d, e)]
        rowsum = sum(e)
        for t in range(8):
            if 8 * (t + u) >= 64:
                continue
            for c in range(w):
                acc = sum(x * (((int(rev[i, c]) >> (8 * t)) & 0xff) - 128) for i, x in enumerate(e))
                assert -(1 << 31) <= acc < (1 << 31)
                total[c] = (total[c] + ((acc + 128 * rowsum) << (8 * (t + u)))) & M64
    assert not any(d)
    return [(-v) & M64 for v in total]


@pytest.mark.parametrize("log,count", [(lg, c) for lg, c in PC.RADICES if lg <= 23])
def test_limb_and_plane_form_reproduces_the_reference_sum(log, count):
    for seed, make in ((4, PC.extreme_case), (5, lambda *a: tuple(x[0] if i == 0 else x for i, x in enumerate(PC.uniform_case(*a))))):
        key, lwes = make(seed, 4, 1, 3, 2, log, count, 2)
        want = PC.pfks_ref(lwes, key, log, count)
        for b in range(2):
            assert limb_form(lwes[b], key, log, count) == [int(v) for v in want[b]], (log, count, seed, b)


# ---- meaning with honest keys -----------------------------------------------------------------------------------------------

MEANING = [(16, 1, 5, 3, 4, 3), (16, 2, 4, 2, 9, 2), (8, 1, 3, 4, 17, 2)]   # N, k, n, p, log, count


@pytest.mark.parametrize("shape", MEANING)
def test_map_message_z_to_coefficient_z(shape):
    N, k, n, p, log, count = shape
    rng = np.random.default_rng([0xD2, N, k, n, p, log, count])
    lwe_sk, glwe_sk = R.binary_key(rng, n), R.binary_key(rng, k * N)
    key = PC.honest_key(rng, lwe_sk, glwe_sk, N, p, log, count, PC.map_message_to_coefficient(N))
    lwes = rng.integers(0, 1 << 64, (4, p, n + 1), dtype=np.uint64)
    out = PC.pfks_ref(lwes, key, log, count).reshape(4, k + 1, N)
    ph = R.glwe_phase(out, glwe_sk)
    lo, hi = PC.meaning_bounds(n, p, count, log)
    d = R.torus_distance(ph[:, :p], PC.lwe_phases(lwes, lwe_sk))
    rest = R.torus_distance(ph[:, p:], np.zeros_like(ph[:, p:]))
    print(f"pfks map 1 {shape}: max 2^{np.log2(max(d.max(), 2.0 ** -80)):.2f} (bound 2^{np.log2(lo):.2f}); beyond p max "
          f"2^{np.log2(max(rest.max(), 2.0 ** -80)):.2f} (bound 2^{np.log2(hi):.2f})")
    assert d.max() <= lo and rest.max() <= hi


@pytest.mark.parametrize("constant_mask", [False, True])
@pytest.mark.parametrize("shape", [(16, 2, 11, 3), (8, 1, 17, 2)])
def test_the_two_maps_of_the_circuit_bootstrap_keys(shape, constant_mask):
    """key r < k multiplies the phase by -S_r, key k puts it at coefficient 0; from_dimension = k N as in the circuit bootstrap"""
    N, k, log, count = shape
    n = k * N
    rng = np.random.default_rng([0xD3, N, k, log, count, int(constant_mask)])
    lwe_sk, glwe_sk = R.binary_key(rng, n), R.binary_key(rng, k * N)
    keys = PC.cbs_pfks_keys(rng, lwe_sk, glwe_sk, N, log, count, constant_mask)
    assert keys.shape == (k + 1, 1, n + 1, count, k + 1, N)
    lwes = rng.integers(0, 1 << 64, (3, 1, n + 1), dtype=np.uint64)
    phases = PC.lwe_phases(lwes, lwe_sk)[:, 0]
    lo, hi = PC.meaning_bounds(n, 1, count, log)
    sk = np.asarray(glwe_sk, dtype=np.uint64).reshape(k, N)
    for r in range(k + 1):
        out = PC.pfks_ref(lwes, keys[r], log, count).reshape(3, k + 1, N)
        ph = R.glwe_phase(out, glwe_sk)
        if r < k:
            want = (np.uint64(0) - phases)[:, None] * sk[r][None, :]
            assert R.torus_distance(ph, want).max() <= lo, (shape, r)
        else:
            assert R.torus_distance(ph[:, 0], phases).max() <= lo, (shape, r)
            assert R.torus_distance(ph[:, 1:], np.zeros_like(ph[:, 1:])).max() <= hi, (shape, r)


# ---- the binding and the documents ------------------------------------------------------------------------------------------

def test_binding_header_rust_block_and_index_name_every_new_symbol():
    from spf_amd import _ffi
    declared = {s[0] for s in _ffi.SYMBOLS}
    header = (ROOT / "include" / "spf_hip.h").read_text()
    rust = (ROOT / "include" / "spf_hip.rs").read_text()
    index = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert re.search(r"\b" + name + r"\(", header), name
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert "`" + name + "`" in index, name
    in_header = set(re.findall(r"\b(spf_[a-z0-9_]*(?:private_functional_keyswitch|pfks)[a-z0-9_]*)\(", header))
    assert in_header == set(NEW_SYMBOLS)


def test_engine_has_the_methods():
    import spf_amd
    for m in ("load_private_functional_keyswitch_keys_std", "private_functional_keyswitch", "apply_pfks_on_ggsw_components",
              "circuit_bootstrap_via_pfks", "private_functional_keyswitch_enqueue", "apply_pfks_on_ggsw_components_enqueue",
              "circuit_bootstrap_via_pfks_enqueue", "last_private_functional_keyswitch_kernel"):
        assert callable(getattr(spf_amd.Engine, m)), m
