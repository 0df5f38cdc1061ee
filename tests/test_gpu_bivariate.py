"""`programmable_bootstrap_bivariate` (sunscreen_tfhe ops/bootstrapping/programmable_bootstrapping.rs:575-621) on the GPU.

The reference packs left * 2^p + right (`scalar_mul_ciphertext_mad` into a cleared LWE, then `add_lwe_inplace`, :603-610)
and bootstraps the packed input univariately.  So every output here must be word-equal to the univariate bootstrap of the
input packed in numpy (uint64 wraps), both on the GPU (`pbs_univariate`, itself pinned against the oracle) and in the
oracle (`pbs_univariate` / `bench_generalized_pbs` + `sample_extract`).  Encryptions check the function too: the
reference's `can_bootstrap_with_bivariate_map` (:791-904) replayed at its own small parameters, and decryptions at
DEFAULT_128.
"""
import os

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests.test_gpu_generic import TEST1
from tests.util import dev_bootstrap, keyset, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu

HOST_THREADS = max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def full():
    ks = keyset(0x5EED0001, 637)
    eng = spf_amd.Engine(to_engine_params(ks.params))
    eng.load_bootstrap_key(ks.bsk_fft)
    eng.load_keyswitch_key(ks.ksk)
    return ks, eng


def pack(left, right, p: int) -> np.ndarray:
    return np.asarray(left, dtype=np.uint64) * np.uint64(1 << p) + np.asarray(right, dtype=np.uint64)


def oracle_bivariate(packed, lut, ks) -> np.ndarray:
    """generalized PBS (0, 0) on host threads, then sample_extract(., 0)"""
    P = ks.params
    _, glwe = O.bench_generalized_pbs(packed, lut, ks.bsk_fft, P, HOST_THREADS)
    return np.stack([O.sample_extract(g, 0, P.N, P.k) for g in glwe])


def bivariate_dev(eng, left, right, lut, p):
    """ONE launch through spf_pbs_bivariate_dev on the default stream"""
    P = eng.params
    B = left.shape[0]
    out = np.empty((B, P.lwe1_words), dtype=np.uint64)
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        ptr = eng.device_alloc(a.nbytes)
        bufs.append(ptr)
        eng.device_upload(ptr, a)
        return ptr

    try:
        d_l = up(left)
        d_r = up(right)
        d_lut = up(lut)
        d_out = eng.device_alloc(out.nbytes)
        bufs.append(d_out)
        eng.pbs_bivariate_dev(None, B, d_l, d_r, d_lut, 0 if lut.ndim == 1 else P.glwe_words, p, d_out)
        eng.device_download(None, out, d_out)
    finally:
        for ptr in bufs:
            eng.device_free(ptr)
    return out


def decode_with_carry(d: int, p: int, c: int) -> int:
    """`decrypt_lwe_with_carry` (high_level.rs:586-611) after the raw decryption"""
    round_bit = (d >> (64 - p - c - 1)) & 1
    return ((d >> (64 - p - c)) + round_bit) & ((1 << p) - 1)


def test_bivariate_4096_default128_every_ciphertext(full):
    ks, eng = full
    B, p = 4096, 2
    left, right = random_lwe_batch(0xB1F0, B, 637), random_lwe_batch(0xB1F1, B, 637)
    lut = spf_amd.generate_bivariate_lut(lambda l, r: (l + 3 * r) % 4, p, p)
    got = eng.pbs_bivariate(left, right, lut, p)
    kernel = eng.last_blind_rotate_kernel()
    packed = pack(left, right, p)
    exp = oracle_bivariate(packed, lut, ks)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} ciphertexts differ from the oracle, first {bad[:8]}"
    assert np.array_equal(got, eng.pbs_univariate(packed, lut))
    assert eng.last_blind_rotate_kernel() == kernel


@pytest.mark.parametrize("B", [200, 512])
def test_bivariate_shapes_shared_and_per_ciphertext_luts(full, B):
    ks, eng = full
    P = eng.params
    p, c = 1, 2
    left, right = random_lwe_batch(0xB200 + B, B, 637), random_lwe_batch(0xB300 + B, B, 637)
    packed = pack(left, right, p)
    lut = spf_amd.generate_bivariate_lut(lambda l, r: l ^ r, p, c)
    got = eng.pbs_bivariate(left, right, lut, p)
    kernel = eng.last_blind_rotate_kernel()
    assert np.array_equal(got, eng.pbs_univariate(packed, lut)) and eng.last_blind_rotate_kernel() == kernel
    for i in (0, B // 2, B - 1):
        assert np.array_equal(got[i], O.pbs_univariate(packed[i], lut, ks.bsk_fft, ks.params)), i
    fns = [lambda l, r: l ^ r, lambda l, r: l & r, lambda l, r: l | r, lambda l, r: l & (1 - r)]
    tables = [spf_amd.generate_bivariate_lut(f, p, c) for f in fns]
    luts = np.stack([tables[i % 4] for i in range(B)])
    got = eng.pbs_bivariate(left, right, luts, p)
    assert luts.shape == (B, P.glwe_words)
    assert np.array_equal(got, eng.pbs_univariate(packed, luts))
    for i in (1, B - 2):
        assert np.array_equal(got[i], O.pbs_univariate(packed[i], luts[i], ks.bsk_fft, ks.params)), i


def test_bivariate_ragged_1031_one_device_launch(full):
    ks, eng = full
    B, p = 1031, 2
    left, right = random_lwe_batch(0xB103, B, 637), random_lwe_batch(0xB104, B, 637)
    packed = pack(left, right, p)
    lut = spf_amd.generate_bivariate_lut(lambda l, r: (l * r) % 4, p, 3)
    got = bivariate_dev(eng, left, right, lut, p)
    kernel = eng.last_blind_rotate_kernel()
    assert np.array_equal(got, dev_bootstrap(eng, packed, lut, extract=True))
    assert eng.last_blind_rotate_kernel() == kernel and kernel.startswith("blind_rotate2p_kernel<")
    for i in (0, 1027, 1030):
        assert np.array_equal(got[i], O.pbs_univariate(packed[i], lut, ks.bsk_fft, ks.params)), i


@pytest.mark.parametrize("p,fns", [
    (1, {"xor": lambda l, r: l ^ r, "and": lambda l, r: l & r, "or": lambda l, r: l | r, "l.!r": lambda l, r: l & (1 - r)}),
    (2, {"add": lambda l, r: (l + r) % 4, "mul": lambda l, r: (l * r) % 4}),
], ids=["p1c1", "p2c2"])
def test_bivariate_decrypts_at_default128(full, p, fns):
    """inputs at m << (64 - p - c - 1) (a padding bit and c carry bits, as the reference's test encodes them); every
    (l, r) decrypts to f(l, r) under the GLWE key.  A 5-bit slot has a half-width of 64 units of 1/4096; the modulus switch
    of a 637-bit key adds about 5 (an estimate)."""
    ks, eng = full
    c = p
    P = ks.params
    rng = O.Rng(0xB1DEC + p)
    pairs = [(l, r) for l in range(1 << p) for r in range(1 << p)]
    enc = lambda m: O.encrypt_lwe(rng, ks.lwe_sk, m << (64 - p - c - 1), P.lwe_std)  # noqa: E731
    left = np.stack([enc(l) for l, _ in pairs])
    right = np.stack([enc(r) for _, r in pairs])
    for name, f in fns.items():
        lut = spf_amd.generate_bivariate_lut(f, p, c)
        got = eng.pbs_bivariate(left, right, lut, p)
        dec = [decode_with_carry(O.decrypt_lwe_raw(got[i], ks.glwe_sk), p, c) for i in range(len(pairs))]
        assert dec == [f(l, r) for l, r in pairs], name


def test_reference_can_bootstrap_with_bivariate_map_replayed():
    """programmable_bootstrapping.rs:791-904 at TEST_LWE_DEF_1 / TEST_GLWE_DEF_1 / TEST_RADIX (the generic kernels):
    p = c = 1 with (l + r) % 2 decrypts for every pair; p = c = 2 is checked word for word only (at 2N = 256 the
    modulus-switch noise is too close to a 5-bit slot for a decryption to be reliable)."""
    P = TEST1
    ks = O.gen_keyset(0xB1CAFE, P, with_ksk=False)
    eng = spf_amd.Engine(to_engine_params(P))
    eng.load_bootstrap_key(ks.bsk_fft)
    rng = O.Rng(0xB1CAFF)
    for p, f in [(1, lambda l, r: (l + r) % 2), (2, lambda l, r: (l + 2 * r + 1) % 4)]:
        c = p
        pairs = [(l, r) for l in range(1 << p) for r in range(1 << p)]
        enc = lambda m: O.encrypt_lwe(rng, ks.lwe_sk, m << (64 - p - c - 1), P.lwe_std)  # noqa: E731
        left = np.stack([enc(l) for l, _ in pairs])
        right = np.stack([enc(r) for _, r in pairs])
        lut = spf_amd.generate_bivariate_lut(f, p, c, eng.params)
        m = 1 << p
        assert np.array_equal(lut, O.trivial_lut_glwe(O.generate_lut(P.N, [lambda x: f((x >> p) % m, x % m)], p + c), P))
        got = eng.pbs_bivariate(left, right, lut, p)
        assert eng.last_blind_rotate_kernel() == "generic_pbs_kernel"
        packed = pack(left, right, p)
        for i in range(len(pairs)):
            assert np.array_equal(got[i], O.pbs_univariate(packed[i], lut, ks.bsk_fft, P)), (p, i)
        if p == 1:
            dec = [decode_with_carry(O.decrypt_lwe_raw(got[i], ks.glwe_sk), p, c) for i in range(len(pairs))]
            assert dec == [f(l, r) for l, r in pairs]


def test_device_resident_keyswitch_then_bivariate(full):
    """two L1 batches: spf_keyswitch_lwe_l1_lwe_l0_dev on each, then spf_pbs_bivariate_dev, all enqueued on one stream
    (the default stream) with one wait at the end; and left is right (f(x, x))"""
    ks, eng = full
    P, OP = eng.params, ks.params
    B, p = 256, 2
    l1 = [random_lwe_batch(0xB5E0 + j, B, OP.k * OP.N) for j in range(2)]
    lut = spf_amd.generate_bivariate_lut(lambda l, r: (3 * l + r) % 4, p, p)
    h = None
    bufs = []

    def alloc(nbytes):
        ptr = eng.device_alloc(nbytes)
        bufs.append(ptr)
        return ptr

    try:
        d_l1 = [alloc(x.nbytes) for x in l1]
        for d, x in zip(d_l1, l1):
            eng.device_upload(d, x)
        d_l0 = [alloc(B * P.lwe0_words * 8) for _ in l1]
        d_lut = alloc(lut.nbytes)
        eng.device_upload(d_lut, lut)
        d_out = [alloc(B * P.lwe1_words * 8) for _ in range(2)]
        for d_in, d_o in zip(d_l1, d_l0):
            eng.keyswitch_dev(h, B, d_in, d_o)
        eng.pbs_bivariate_dev(h, B, d_l0[0], d_l0[1], d_lut, 0, p, d_out[0])
        eng.pbs_bivariate_dev(h, B, d_l0[0], d_l0[0], d_lut, 0, p, d_out[1])
        got = [np.empty((B, P.lwe1_words), dtype=np.uint64) for _ in range(2)]
        for g, d in zip(got, d_out):
            eng.device_download(h, g, d)
    finally:
        for ptr in bufs:
            eng.device_free(ptr)
    l0 = [np.stack([O.keyswitch_lwe(x[i], ks.ksk, OP.k * OP.N, OP.lwe_n, OP.ks_radix_log, OP.ks_count) for i in range(B)])
          for x in l1]
    assert np.array_equal(got[0], oracle_bivariate(pack(l0[0], l0[1], p), lut, ks))
    assert np.array_equal(got[1], oracle_bivariate(pack(l0[0], l0[0], p), lut, ks))


def test_bivariate_group_and_errors(full):
    ks, eng = full
    P = eng.params
    B, p = 300, 2
    left, right = random_lwe_batch(0xB600, B, 637), random_lwe_batch(0xB601, B, 637)
    lut = spf_amd.generate_bivariate_lut(lambda l, r: l ^ r, p, p)
    want = eng.pbs_bivariate(left, right, lut, p)
    grp = spf_amd.Group(P, devices=[0, 0])
    grp.load_bootstrap_key(ks.bsk_fft)
    assert np.array_equal(grp.pbs_bivariate(left, right, lut, p), want)
    ev = spf_amd.Evaluation(spf_amd.ComputeKey(ks.bsk_fft, None), P)   # the Python mirror, one ciphertext
    one = np.zeros(P.lwe1_words, dtype=np.uint64)
    ev.programmable_bootstrap_bivariate(one, left[7], right[7], lut, p)
    assert np.array_equal(one, want[7])
    ev.engine.close()
    with pytest.raises(spf_amd.SpfError) as e:
        grp.pbs_bivariate(left, right, lut, 64)
    assert e.value.status == 1
    grp.close()
    # a ragged split (2 + 1) with a table per ciphertext: both inputs and the table's stride follow the range
    Q = TEST1
    qs = O.gen_keyset(0xB1CAFE, Q, with_ksk=False)
    small, grp = spf_amd.Engine(to_engine_params(Q)), spf_amd.Group(to_engine_params(Q), devices=[0, 0])
    try:
        for member in (small, grp):
            member.load_bootstrap_key(qs.bsk_fft)
        left3, right3 = random_lwe_batch(0xB602, 3, Q.lwe_n), random_lwe_batch(0xB603, 3, Q.lwe_n)
        luts = np.stack([spf_amd.generate_bivariate_lut(f, 1, 1, small.params) for f in (lambda l, r: l ^ r, lambda l, r: l & r, lambda l, r: l | r)])
        assert np.array_equal(grp.pbs_bivariate(left3, right3, luts, 1), small.pbs_bivariate(left3, right3, luts, 1))
    finally:
        grp.close()
        small.close()

    # the device-pointer checks get one real buffer, large enough for every operand of B = 4 (nothing may launch)
    keyless = spf_amd.Engine(P)
    with pytest.raises(spf_amd.SpfError) as e:
        keyless.pbs_bivariate(left[:4], right[:4], lut, p)
    assert e.value.status == 3
    d = keyless.device_alloc(4 * P.lwe1_words * 8)
    assert keyless._lib.spf_pbs_bivariate_dev(keyless._h, None, 4, d, d, d, 0, p, d) == 3
    keyless.device_free(d)
    keyless.close()
    with pytest.raises(spf_amd.SpfError) as e:
        eng.pbs_bivariate(left[:4], right[:4], lut, 64)
    assert e.value.status == 1
    lib, h = eng._lib, eng._h
    d = eng.device_alloc(4 * P.lwe1_words * 8)
    x = np.zeros((4, P.lwe0_words), dtype=np.uint64)
    out = np.empty((4, P.lwe1_words), dtype=np.uint64)
    ptr = spf_amd._ffi._ptr
    assert lib.spf_pbs_bivariate_batch(h, 4, ptr(x), None, ptr(lut), 0, p, ptr(out)) == 1
    assert lib.spf_pbs_bivariate_batch(h, 4, None, ptr(x), ptr(lut), 0, p, ptr(out)) == 1
    assert lib.spf_pbs_bivariate_batch(h, 4, ptr(x), ptr(x), None, 0, p, ptr(out)) == 1
    assert lib.spf_pbs_bivariate_batch(h, 4, ptr(x), ptr(x), ptr(lut), 0, p, None) == 1
    assert lib.spf_pbs_bivariate_dev(h, None, 4, d, None, d, 0, p, d) == 1
    assert lib.spf_pbs_bivariate_dev(h, None, 4, d, d, d, 0, 64, d) == 1
    eng.device_free(d)
    assert lib.spf_pbs_bivariate_batch(h, 0, None, None, None, 0, p, None) == 0
    assert lib.spf_pbs_bivariate_dev(h, None, 0, None, None, None, 0, p, None) == 0


def test_cpp_evaluation_bivariate_matches_the_oracle(tmp_path):
    """tests/cpp/bivariate_parity.cpp, built and run as tests/test_gpu_cpp_host.py builds its program"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(spf_amd.lib_path())
    oracle_so = O.library_path()
    exe = tmp_path / "bivariate_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(root, "include"),
                    "-I", os.path.join(root, "oracle"), os.path.join(root, "tests", "cpp", "bivariate_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", oracle_so,
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.dirname(oracle_so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
