"""Packed integers on the GPU: `spf_glwe_pack_*`, `spf_glwe_unpack_l1_*`, `spf_unpack_circuit_bootstrap_*` and their group
forms (include/spf_hip.h), int-major (bit i of packed ciphertext b is row b * n + i).

Pack is held word for word to the closed form sum_i X^i * bit_i (tests/test_packed_plaintext.py pins that closed form to the
reference's MulXN + GlweAdd tree, dynamic_generic_int_graph_nodes.rs:139-200) and, on sampled ciphertexts, to the tree
itself; unpack to `O.sample_extract(ct_b, i)` for every row (packed_dynamic_generic_int_graph_node.rs:24-39); the unpack to
GGSW bit for bit to spf_keyswitch_circuit_bootstrap_batch of the unpacked LWEs, and on sampled rows to the oracle's
keyswitch + circuit bootstrap.  Decryptions replay the reference's `can_unpack_int` / `can_pack_int` (fluent/int.rs:170-243)
at DEFAULT_128.  Bit counts of 2048 run at B = 1 and 31 only: at B = 1031 the batch would be 69 GB of bit GLWEs.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests.test_gpu_generic import TEST1, TEST2
from tests.test_packed_plaintext import oracle_tree_pack
from tests.util import keyset, random_glwe, to_engine_params

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SIZES = [(B, n) for B in (1, 31, 1031) for n in (1, 2, 15, 16, 64)] + [(1, 2048), (31, 2048)]


def _eng_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count,
                                       ss_radix_log=P.ss_radix_log, ss_radix_count=P.ss_count)


@pytest.fixture(scope="module")
def engines():
    """keyless contexts: DEFAULT_128 (the tuned kernels' shape) and the generic TEST1 (N 128, k 2) / TEST2 (N 256, k 3)"""
    out = {name: (OP, spf_amd.Engine(to_engine_params(OP))) for name, OP in
           [("N2048k1", O.DEFAULT_128), ("N128k2", TEST1), ("N256k3", TEST2)]}
    yield out
    for _, e in out.values():
        e.close()


@pytest.fixture(scope="module")
def full():
    """DEFAULT_128 with all four keys"""
    ks = keyset(0x5EED0001, 637)
    r = O.Rng(0x9AC4)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, ks.params), O.gen_ssk_fft(r, ks.glwe_sk, ks.params)
    eng = spf_amd.Engine(to_engine_params(ks.params))
    for e in (eng,):
        e.load_bootstrap_key(ks.bsk_fft)
        e.load_keyswitch_key(ks.ksk)
        e.load_automorphism_key(ak)
        e.load_scheme_switch_key(ssk)
    yield ks, ak, ssk, eng
    eng.close()


def _words(seed: int, shape) -> np.ndarray:
    """random full-range words, with the extremes 0, 2^63 and 2^64 - 1 on whole rows and sprinkled"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    flat = x.reshape(-1, shape[-1])
    for r, v in zip(range(min(3, flat.shape[0])), (0, 1 << 63, M64)):
        flat[r] = np.uint64(v)
    idx = rng.integers(0, x.size, size=max(1, x.size // 64))
    x.reshape(-1)[idx] = rng.choice(np.array([0, 1 << 63, M64], dtype=np.uint64), size=idx.size)
    return x


def _on_device(eng, host_arrays, out_shape, out_dtype, call):
    """upload, run one _dev call on the default stream, download"""
    bufs = []
    try:
        ptrs = []
        for a in host_arrays:
            a = np.ascontiguousarray(a)
            p = eng.device_alloc(a.nbytes)
            bufs.append(p)
            eng.device_upload(p, a)
            ptrs.append(p)
        out = np.empty(out_shape, dtype=out_dtype)
        d_out = eng.device_alloc(out.nbytes)
        bufs.append(d_out)
        call(*ptrs, d_out)
        eng.device_download(None, out, d_out)
        return out
    finally:
        for p in bufs:
            eng.device_free(p)


def _closed_form_batch(bits, N, k):
    """closed_form_pack over a (B, n, (k+1)N) batch, vectorised over B"""
    B, n, _ = bits.shape
    x = bits.reshape(B, n, k + 1, N)
    out = np.zeros((B, k + 1, N), dtype=np.uint64)
    for i in range(n):
        r = np.roll(x[:, i], i, axis=-1)
        r[..., :i] = np.uint64(0) - r[..., :i]
        out += r
    return out.reshape(B, -1)


@pytest.mark.parametrize("B,n", SIZES, ids=[f"B{B}n{n}" for B, n in SIZES])
def test_pack_default128_batch_and_dev(engines, B, n):
    OP, eng = engines["N2048k1"]
    bits = _words(0x9A00 + 7 * B + n, (B, n, OP.glwe_len))
    got = eng.glwe_pack(bits)
    want = _closed_form_batch(bits, OP.N, OP.k)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} packed ciphertexts differ from the closed form, first {bad[:8]}"
    for b in sorted({0, B - 1}):
        if n <= 64:
            assert np.array_equal(got[b], oracle_tree_pack(bits[b], OP.N, OP.k)), b
    dev = _on_device(eng, [bits], got.shape, np.uint64, lambda d_in, d_out: eng.glwe_pack_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev, got)


def test_pack_4096x16_past_one_grid_slice(engines):
    """65 536 bit GLWEs in: more rows than one kMaxGridRows launch slice"""
    OP, eng = engines["N2048k1"]
    B, n = 4096, 16
    bits = _words(0x9A10, (B, n, OP.glwe_len))
    got = eng.glwe_pack(bits)
    assert np.array_equal(got, _closed_form_batch(bits, OP.N, OP.k))
    for b in (0, 2047, 4095):
        assert np.array_equal(got[b], oracle_tree_pack(bits[b], OP.N, OP.k)), b
    dev = _on_device(eng, [bits], got.shape, np.uint64, lambda d_in, d_out: eng.glwe_pack_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev, got)


@pytest.mark.parametrize("B,n", SIZES, ids=[f"B{B}n{n}" for B, n in SIZES])
def test_unpack_default128_batch_and_dev(engines, B, n):
    OP, eng = engines["N2048k1"]
    packed = _words(0x9A20 + 7 * B + n, (B, OP.glwe_len))
    got = eng.glwe_unpack_l1(packed, n)
    assert got.shape == (B, n, OP.k * OP.N + 1)
    for b in range(B):
        for i in range(n):
            assert np.array_equal(got[b, i], O.sample_extract(packed[b], i, OP.N, OP.k)), (b, i)
    dev = _on_device(eng, [packed], got.shape, np.uint64, lambda d_in, d_out: eng.glwe_unpack_l1_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev, got)


def test_unpack_4096x16(engines):
    OP, eng = engines["N2048k1"]
    B, n = 4096, 16
    packed = _words(0x9A30, (B, OP.glwe_len))
    got = eng.glwe_unpack_l1(packed, n)
    dev = _on_device(eng, [packed], got.shape, np.uint64, lambda d_in, d_out: eng.glwe_unpack_l1_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev, got)
    for b in range(0, B, 97):
        for i in range(n):
            assert np.array_equal(got[b, i], O.sample_extract(packed[b], i, OP.N, OP.k)), (b, i)
    assert np.array_equal(got[B - 1, n - 1], O.sample_extract(packed[B - 1], n - 1, OP.N, OP.k))


@pytest.mark.parametrize("name", ["N128k2", "N256k3"])
@pytest.mark.parametrize("B,n", [(1, 1), (31, 15), (1031, 16), (3, 64), (2, "N")])
def test_pack_and_unpack_in_generic_contexts(engines, name, B, n):
    OP, eng = engines[name]
    n = OP.N if n == "N" else n
    bits = _words(0x9A40 + OP.N + B + n, (B, n, OP.glwe_len))
    got = eng.glwe_pack(bits)
    assert np.array_equal(got, _closed_form_batch(bits, OP.N, OP.k))
    assert np.array_equal(got[B - 1], oracle_tree_pack(bits[B - 1], OP.N, OP.k))
    dev = _on_device(eng, [bits], got.shape, np.uint64, lambda d_in, d_out: eng.glwe_pack_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev, got)
    packed = _words(0x9A50 + OP.N + B + n, (B, OP.glwe_len))
    lwe = eng.glwe_unpack_l1(packed, n)
    for b in range(B):
        for i in range(n):
            assert np.array_equal(lwe[b, i], O.sample_extract(packed[b], i, OP.N, OP.k)), (b, i)
    dev = _on_device(eng, [packed], lwe.shape, np.uint64, lambda d_in, d_out: eng.glwe_unpack_l1_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev, lwe)


@pytest.mark.parametrize("B,n", [(1, 16), (64, 16), (256, 16)])
def test_unpack_circuit_bootstrap_equals_the_keyswitch_cbs_of_the_unpacked_lwes(full, B, n):
    ks, ak, ssk, eng = full
    P = eng.params
    packed = random_glwe(0x9A60 + B, B, P.glwe_words)
    got = eng.unpack_circuit_bootstrap(packed, n)
    assert got.shape == (B, n, P.cbs_ggsw_complex)
    lwe = eng.glwe_unpack_l1(packed, n)
    want = eng.keyswitch_circuit_bootstrap(lwe.reshape(B * n, -1))
    assert np.array_equal(got.reshape(B * n, -1).view(np.uint64), want.view(np.uint64))
    dev = _on_device(eng, [packed], got.shape, np.complex128,
                     lambda d_in, d_out: eng.unpack_circuit_bootstrap_dev(None, B, n, d_in, d_out))
    assert np.array_equal(dev.view(np.uint64), got.view(np.uint64))
    OP = ks.params
    for b, i in sorted({(0, 0), (B - 1, n - 1), (B // 2, 7), (B - 1, 3)})[:8 if B > 1 else 4]:
        l0 = O.keyswitch_lwe(O.sample_extract(packed[b], i, OP.N, OP.k), ks.ksk, OP.k * OP.N, OP.lwe_n, OP.ks_radix_log,
                             OP.ks_count)
        assert np.array_equal(got[b, i].view(np.uint64), O.circuit_bootstrap(l0, ks.bsk_fft, ak, ssk, OP).view(np.uint64)), (b, i)


def test_unpack_circuit_bootstrap_in_a_generic_context():
    P = TEST1.replace(lwe_n=6, tr_radix_log=7, tr_count=6, ss_radix_log=3, ss_count=15)
    ks = O.gen_keyset(0x5EED0009, P)
    r = O.Rng(0x9A70)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, P), O.gen_ssk_fft(r, ks.glwe_sk, P)
    eng = spf_amd.Engine(_eng_params(P))
    eng.load_bootstrap_key(ks.bsk_fft)
    eng.load_keyswitch_key(ks.ksk)
    eng.load_automorphism_key(ak)
    eng.load_scheme_switch_key(ssk)
    B, n = 3, 5
    packed = random_glwe(0x9A71, B, P.glwe_len)
    got = eng.unpack_circuit_bootstrap(packed, n)
    want = eng.keyswitch_circuit_bootstrap(eng.glwe_unpack_l1(packed, n).reshape(B * n, -1))
    assert np.array_equal(got.reshape(B * n, -1).view(np.uint64), want.view(np.uint64))
    for b in range(B):
        for i in range(n):
            l0 = O.keyswitch_lwe(O.sample_extract(packed[b], i, P.N, P.k), ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count)
            assert np.array_equal(got[b, i].view(np.uint64), O.circuit_bootstrap(l0, ks.bsk_fft, ak, ssk, P).view(np.uint64)), (b, i)
    eng.close()


def _decrypt_bits(glwe, ks, n):
    P = ks.params
    return np.array([O.decode(int(t), 1) for t in O.decrypt_glwe_raw(glwe, ks.glwe_sk, P.N, P.k)[:n]], dtype=np.uint64)


def test_reference_can_unpack_int_replayed(full):
    """fluent/int.rs:170-193: -42 packed in 16 bits, unpacked; every LWE decrypts (glwe_sk is the L1 LWE key) to its bit"""
    ks, _, _, eng = full
    P = ks.params
    rng = O.Rng(0x9A80)
    ct = O.encrypt_glwe(rng, ks.glwe_sk, spf_amd.packed_plaintext(-42, 16) << np.uint64(63), P.N, P.k, P.glwe_std)
    lwe = eng.glwe_unpack_l1(ct, 16)[0]
    bits = [O.decode(O.decrypt_lwe_raw(lwe[i], ks.glwe_sk), 1) for i in range(16)]
    assert bits == [((-42) >> i) & 1 for i in range(16)]
    assert spf_amd.packed_decode(bits, 16, True) == -42


def test_reference_can_pack_int_replayed(full):
    """fluent/int.rs:222-243: the 15 bits of -42, each a GLWE encryption of the constant polynomial bit, packed; the packed
    GLWE decrypts to -42"""
    ks, _, _, eng = full
    P = ks.params
    rng = O.Rng(0x9A81)
    cts = []
    for i in range(15):
        m = np.zeros(P.N, dtype=np.uint64)
        m[0] = O.encode(((-42) >> i) & 1, 1)
        cts.append(O.encrypt_glwe(rng, ks.glwe_sk, m, P.N, P.k, P.glwe_std))
    packed = eng.glwe_pack(np.stack(cts)[None])
    assert spf_amd.packed_decode(_decrypt_bits(packed[0], ks, P.N), 15, True) == -42


def test_round_trip_unpack_to_ggsw_not_and_pack(full):
    """packed x -> unpack_circuit_bootstrap -> multiply_glwe_ggsw with the trivial one (a GLWE of each bit) -> glwe_not ->
    pack: decrypts to ~x mod 2^n"""
    ks, _, _, eng = full
    P = ks.params
    n, values = 16, [0, 0xA5C3, 0xFFFF]
    rng = O.Rng(0x9A82)
    packed = np.stack([O.encrypt_glwe(rng, ks.glwe_sk, spf_amd.packed_plaintext(v, n) << np.uint64(63), P.N, P.k, P.glwe_std)
                       for v in values])
    ggsw = eng.unpack_circuit_bootstrap(packed, n)
    one = spf_amd.trivial_packed_glwe(1, 1)
    glwe = eng.multiply_glwe_ggsw(np.tile(one, (len(values) * n, 1)), ggsw.reshape(len(values) * n, -1))
    out = eng.glwe_pack(eng.glwe_not(glwe).reshape(len(values), n, -1))
    for v, ct in zip(values, out):
        assert spf_amd.packed_decode(_decrypt_bits(ct, ks, n), n, False) == ~v & ((1 << n) - 1), hex(v)


def test_group_equals_one_context(full):
    ks, ak, ssk, eng = full
    P = eng.params
    grp = spf_amd.Group(P, devices=[0, 0])
    try:
        grp.load_bootstrap_key(ks.bsk_fft)
        grp.load_keyswitch_key(ks.ksk)
        grp.load_automorphism_key(ak)
        grp.load_scheme_switch_key(ssk)
        B, n = 37, 16
        bits = _words(0x9A90, (B, n, P.glwe_words))
        packed = _words(0x9A91, (B, P.glwe_words))
        assert np.array_equal(grp.glwe_pack(bits), eng.glwe_pack(bits))
        assert np.array_equal(grp.glwe_unpack_l1(packed, n), eng.glwe_unpack_l1(packed, n))
        assert np.array_equal(grp.unpack_circuit_bootstrap(packed[:5], n).view(np.uint64),
                              eng.unpack_circuit_bootstrap(packed[:5], n).view(np.uint64))
        for bad in (0, P.polynomial_degree + 1):
            with pytest.raises(spf_amd.SpfError) as e:
                grp.glwe_unpack_l1(packed[:1], bad)
            assert e.value.status == 1 and "n_bits" in str(e.value)
        lib, h = grp._raw, grp._h
        ptr = spf_amd._ffi._ptr
        assert lib.spf_group_glwe_pack_batch(h, 1 << 40, 1 << 10, ptr(bits), ptr(packed)) == 1
        assert lib.spf_group_glwe_pack_batch(h, 1, 16, None, ptr(packed)) == 1
        assert lib.spf_group_unpack_circuit_bootstrap_batch(h, 0, 16, None, None) == 0
    finally:
        grp.close()


def test_errors(full):
    ks, _, _, eng = full
    P = eng.params
    lib, h = eng._lib, eng._h
    ptr = spf_amd._ffi._ptr
    gw = P.glwe_words
    x = np.zeros((4, gw), dtype=np.uint64)
    out = np.empty(4 * 2 * P.lwe1_words, dtype=np.uint64)
    cout = np.empty(2 * P.cbs_ggsw_complex, dtype=np.complex128)

    def err():
        return lib.spf_last_error(h).decode()

    batch = [lambda B, n, a, o: lib.spf_glwe_pack_batch(h, B, n, a, o),
             lambda B, n, a, o: lib.spf_glwe_unpack_l1_batch(h, B, n, a, o),
             lambda B, n, a, o: lib.spf_unpack_circuit_bootstrap_batch(h, B, n, a, o)]
    outs = [ptr(out), ptr(out), ptr(cout)]
    for f, o in zip(batch, outs):
        assert f(1, 2, None, o) == 1 and "null" in err()
        assert f(1, 2, ptr(x), None) == 1 and "null" in err()
        assert f(1, 0, ptr(x), o) == 1 and "n_bits" in err()
        assert f(1, P.polynomial_degree + 1, ptr(x), o) == 1 and "n_bits" in err()
        assert f(0x0fffffff // 16 + 1, 16, ptr(x), o) == 1 and "0x0fffffff" in err()
        assert f(1 << 62, 1 << 10, ptr(x), o) == 1 and "0x0fffffff" in err()
        assert f(0, 2, None, None) == 0
    assert lib.spf_glwe_pack_batch(None, 1, 2, ptr(x), ptr(out)) == 1

    # device pointers: one buffer of 4 GLWEs (nothing may launch on a refused call)
    d = eng.device_alloc(4 * gw * 8)
    try:
        dev = [lib.spf_glwe_pack_dev, lib.spf_glwe_unpack_l1_dev, lib.spf_unpack_circuit_bootstrap_dev]
        for f in dev:
            assert f(h, None, 1, 2, None, d) == 1 and "null" in err()
            assert f(h, None, 1, 0, d, d + 2 * gw * 8) == 1 and "n_bits" in err()
            assert f(h, None, 1, P.polynomial_degree + 1, d, d + 2 * gw * 8) == 1 and "n_bits" in err()
            assert f(h, None, 1 << 62, 1 << 10, d, d) == 1 and "0x0fffffff" in err()
            assert f(h, None, 0, 2, None, None) == 0
        # pack: bits [d, d + 2 GLWEs), output one GLWE: overlapping is refused, adjacent is not
        for o in (d, d + gw * 8, d + gw * 8 + 8):
            assert lib.spf_glwe_pack_dev(h, None, 1, 2, d, o) == 1 and "overlap" in err()
        assert lib.spf_glwe_pack_dev(h, None, 1, 2, d + gw * 8, d) == 0
        assert lib.spf_glwe_pack_dev(h, None, 1, 2, d, d + 2 * gw * 8) == 0
        eng.device_download(None, np.empty(gw, dtype=np.uint64), d + 2 * gw * 8)
    finally:
        eng.device_free(d)

    # without the circuit-bootstrap keys: the same failure as spf_keyswitch_circuit_bootstrap_batch
    for keys in ([], ["bsk"], ["bsk", "ksk"]):
        e = spf_amd.Engine(P)
        try:
            if "bsk" in keys:
                e.load_bootstrap_key(ks.bsk_fft)
            if "ksk" in keys:
                e.load_keyswitch_key(ks.ksk)
            with pytest.raises(spf_amd.SpfError) as a:
                e.unpack_circuit_bootstrap(x[:1], 4)
            with pytest.raises(spf_amd.SpfError) as b:
                e.keyswitch_circuit_bootstrap(e.glwe_unpack_l1(x[:1], 4).reshape(4, -1))
            assert (a.value.status, str(a.value)) == (b.value.status, str(b.value)), keys
            assert a.value.status == 3, keys
        finally:
            e.close()


def test_cpp_evaluation_packed_matches_the_oracle(tmp_path):
    """tests/cpp/packed_parity.cpp, built and run as tests/test_gpu_cpp_host.py builds its program"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(spf_amd.lib_path())
    oracle_so = O.library_path()
    exe = tmp_path / "packed_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(root, "include"),
                    "-I", os.path.join(root, "oracle"), os.path.join(root, "tests", "cpp", "packed_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", oracle_so,
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.dirname(oracle_so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
