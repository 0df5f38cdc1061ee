"""`generate_bivariate_lut` (sunscreen_tfhe ops/bootstrapping/programmable_bootstrapping.rs:413-452) and
`BivariateLookupTable::trivial_from_fn` (entities/bivariate_lookup_table.rs:36-90) on the product side, host only.

The reference is a composition of existing oracle calls: the bivariate map expanded to the univariate table
U[x] = f((x >> p) mod 2^p, x mod 2^p) over x < 2^(p + c) (`bivariate_function`, :413-430), then
`generate_lut(N, [U], p + c)` as the trivial GLWE."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import _ffi

SHAPES = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3)]
PARAMS = [(O.DEFAULT_128, spf_amd.DEFAULT_128),
          (O.DEFAULT_128.replace(N=128), spf_amd.DEFAULT_128.replace(polynomial_degree=128))]


def _maps(p: int):
    m = 1 << p
    table = np.random.default_rng(0xB1 + p).integers(0, m, size=(m, m), dtype=np.uint64)
    return {"xor": lambda l, r: l ^ r, "add": lambda l, r: (l + r) % m, "and": lambda l, r: l & r,
            "random": lambda l, r: int(table[l, r])}


def _oracle_lut(f, p: int, c: int, OP):
    m = 1 << p
    return O.trivial_lut_glwe(O.generate_lut(OP.N, [lambda x: f((x >> p) & (m - 1), x & (m - 1))], p + c), OP)


def _table_of(lut: np.ndarray, bits: int, N: int, k: int = 1) -> np.ndarray:
    """U back from a one-map LUT: input x's box is centred on body coefficient x * N / 2^bits (spf_generate_lut)"""
    body = lut[k * N:]
    stride = N >> bits
    return np.array([int(body[x * stride]) >> (64 - bits) for x in range(1 << bits)], dtype=np.uint64)


@pytest.mark.parametrize("OP,EP", PARAMS, ids=["N2048", "N128"])
@pytest.mark.parametrize("p,c", SHAPES)
def test_bivariate_lut_equals_the_oracle_composition(OP, EP, p, c):
    for name, f in _maps(p).items():
        got = spf_amd.generate_bivariate_lut(f, p, c, EP)
        assert np.array_equal(got, _oracle_lut(f, p, c, OP)), (name, p, c)
        # the table form: table[l][r] = f(l, r), 2^p x 2^p or flat
        m = 1 << p
        table = np.array([[f(l, r) for r in range(m)] for l in range(m)], dtype=np.uint64)
        assert np.array_equal(spf_amd.generate_bivariate_lut(table, p, c, EP), got), name
        assert np.array_equal(spf_amd.generate_bivariate_lut(table.reshape(-1), p, c, EP), got), name


def test_carry_bits_above_2p_drop_the_high_part_of_the_left_operand():
    """c > p: the left operand is taken mod 2^p (`bivariate_function`: lhs = (input / modulus) % modulus)"""
    p, c = 1, 3
    U = _table_of(spf_amd.generate_bivariate_lut(lambda l, r: l & (1 - r), p, c), p + c, spf_amd.DEFAULT_128.polynomial_degree)
    assert U.tolist() == [(x >> 1 & 1) & (1 - (x & 1)) for x in range(16)]
    assert U[0b0110] == U[0b0010] == 1 and U[0b1111] == 0


def test_reference_can_decompose_bivariate_map_replayed():
    """programmable_bootstrapping.rs:906-923 on the expanded table: at p = 2, input left * 4 + right decomposes to
    map(left, right) (the reference's loop runs left, right over 0..plaintext_bits; the whole square is checked too)."""
    p, modulus = 2, 4
    fmap = lambda l, r: (l + r) % 2  # noqa: E731  (bivariate_test_function)
    U = _table_of(spf_amd.generate_bivariate_lut(fmap, p, p), 2 * p, spf_amd.DEFAULT_128.polynomial_degree)
    for left in range(p):
        for right in range(p):
            assert U[left * modulus + right] == fmap(left, right)
    for left in range(modulus):
        for right in range(modulus):
            assert U[left * modulus + right] == fmap(left, right)


def test_bivariate_lut_rejections():
    ok = lambda l, r: l ^ r  # noqa: E731
    for p, c in [(2, 1), (0, 1), (0, 0)]:                        # p > c, p = 0
        with pytest.raises(spf_amd.SpfError) as e:
            spf_amd.generate_bivariate_lut(ok, p, c)
        assert e.value.status == 1
    with pytest.raises(spf_amd.SpfError) as e:                 # f(l, r) >= 2^p
        spf_amd.generate_bivariate_lut(lambda l, r: l + r, 2, 2)
    assert e.value.status == 1 and "2^plaintext_bits" in str(e.value)
    with pytest.raises(spf_amd.SpfError) as e:                 # 2^(p + c) > N
        spf_amd.generate_bivariate_lut(ok, 3, 5, spf_amd.DEFAULT_128.replace(polynomial_degree=128))
    assert e.value.status == 1
    with pytest.raises(spf_amd.SpfError):                      # a table of the wrong size
        spf_amd.generate_bivariate_lut(np.zeros(8, dtype=np.uint64), 2, 2)
    # null pointers, straight through the C ABI
    lib = spf_amd.load_library()
    cp = _ffi._cparams(spf_amd.DEFAULT_128)
    table = np.zeros(4, dtype=np.uint64)
    out = np.empty(spf_amd.DEFAULT_128.glwe_words, dtype=np.uint64)
    assert lib.spf_generate_bivariate_lut(None, _ffi._ptr(table), 1, 1, _ffi._ptr(out)) == 1
    assert lib.spf_generate_bivariate_lut(C.byref(cp), None, 1, 1, _ffi._ptr(out)) == 1
    assert lib.spf_generate_bivariate_lut(C.byref(cp), _ffi._ptr(table), 1, 1, None) == 1
    assert lib.spf_generate_bivariate_lut(C.byref(cp), _ffi._ptr(table), 1, 0xFFFFFFFF, _ffi._ptr(out)) == 1
    assert lib.spf_generate_bivariate_lut(C.byref(cp), _ffi._ptr(table), 1, 1, _ffi._ptr(out)) == 0


def test_bivariate_entry_points_validate_without_a_device():
    """the PBS entry points refuse a null context / group before anything else"""
    lib = spf_amd.load_library()
    assert lib.spf_pbs_bivariate_batch(None, 1, None, None, None, 0, 1, None) == 1
    assert lib.spf_pbs_bivariate_dev(None, None, 1, None, None, None, 0, 1, None) == 1
    assert lib.spf_group_pbs_bivariate_batch(None, 1, None, None, None, 0, 1, None) == 1
