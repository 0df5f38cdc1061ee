"""The oracle's FFT-based operations against tests/poly_ref.py, an exact integer statement of the same polynomial arithmetic that
shares nothing with the oracle (CPU only; the HIP kernels meet the same expectations in tests/test_gpu_polynomial_reference.py).

Tier A: single operations under uniform / shaped time-domain "keys", distance word by word.  Tier B: chains under honest
integer keys, distance between exact phases.  Bounds and their origin: tests/polyref_cases.py, profiles/r07_fft_error.md,
profiles/r14_exact_reference_new_ops.md.
Run with -s to see every figure."""
import ast
import json
import os
import time

import numpy as np
import pytest

import oracle as O
from tests import poly_ref as R
from tests import polyref_cases as C

M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------- poly_ref checks itself


def test_poly_ref_imports_neither_oracle_nor_library():
    """its independence is the whole point: parse its imports"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "poly_ref.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add(node.module or "")
            mods.update(f"{node.module}.{a.name}" for a in node.names)
    assert mods, "no imports parsed"
    for m in mods:
        parts = m.split(".")
        assert "oracle" not in parts and "spf_amd" not in parts and "polyref_cases" not in parts and "util" not in parts, m
    assert not any(name in open(path).read() for name in ("__import__", "importlib", "ctypes"))


def test_poly_ref_against_the_reference_vectors(golden_dir):
    with open(os.path.join(golden_dir, "reference_kats.json")) as f:
        kats = json.load(f)
    s = lambda vals: np.array([int(v) & M64 for v in vals], dtype=np.uint64)  # noqa: E731
    k = kats["negacyclic_conv"]
    x = s(k["x"])
    assert np.array_equal(R.negacyclic_mul(x, x), s(k["expect"]))
    assert np.array_equal(R.NUMPY.sum_products(R.signed(x)[None, None], x[None, None])[0, 0], s(k["expect"]))
    for name, sign in (("pos_monomial", 1), ("neg_monomial", -1)):
        for deg, exp in kats[name]["cases"].items():
            assert np.array_equal(R.mul_monomial(s(kats[name]["p"]), sign * int(deg)), s(exp)), (name, deg)
    k = kats["poly_pow_k"]
    p = np.zeros(k["N"], dtype=np.uint64)
    for i, v in k["in"].items():
        p[int(i)] = v
    want = np.zeros(k["N"], dtype=np.uint64)
    for i, v in k["out"].items():
        want[int(i)] = v & M64
    assert np.array_equal(R.automorphism(p, k["k"]), want)
    k = kats["poly_shr_round"]
    assert np.array_equal(R.shr_round(s(k["x"]), k["n"]), s(k["expect"]))
    k = kats["modulus_switch"]
    for c in k["cases"]:
        assert R.modulus_switch(int(k["x"], 16), c["log_chi"], c["log_v"], c["log_modulus"]) == int(c["expect"], 16)


@pytest.mark.parametrize("n", [16, 64])
def test_poly_ref_product_against_schoolbook_on_python_integers(n):
    rng = np.random.default_rng(n)
    for _ in range(4):
        a = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        b = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        want = R.schoolbook_mul(a, b)
        assert [int(v) for v in R.negacyclic_mul(a, b)] == want
        assert [int(v) for v in R.negacyclic_mul(b, a)] == want
    # the monomial, the automorphism and the stacked form agree with the product they are special cases of
    x = np.zeros(n, dtype=np.uint64)
    for e in (0, 1, n - 1, n, n + 5, 2 * n - 1):
        x[:] = 0
        x[e % n] = 1 if e < n else M64
        assert np.array_equal(R.mul_monomial(a, e), R.negacyclic_mul(a, x)), e
        assert np.array_equal(R.mul_monomial(R.mul_monomial(a, e), -e), a), e
    assert np.array_equal(R.automorphism(R.negacyclic_mul(a, b), n + 1), R.negacyclic_mul(R.automorphism(a, n + 1), R.automorphism(b, n + 1)))
    assert np.array_equal(R.negacyclic_mul(np.stack([a, b]), b), np.stack([R.negacyclic_mul(a, b), R.negacyclic_mul(b, b)]))


def test_poly_ref_sample_extract_phase_and_long_double_inverse():
    rng = np.random.default_rng(5)
    n, k = 64, 2
    sk = R.binary_key(rng, k * n)
    ct = R.glwe_encrypt(rng, sk, rng.integers(0, 1 << 64, (1, n), dtype=np.uint64), 0)[0]
    ph = R.glwe_phase(ct, sk)
    for h in (0, 1, n - 1):
        lwe = R.sample_extract(ct, h)
        assert (lwe[-1:] - (lwe[:-1] * sk).sum(dtype=np.uint64, keepdims=True))[0] == ph[h]
    # the inverse takes the oracle's bins of a 40-bit polynomial (the f64 transform's error is far below 1/2 there) back to the same words
    for n in (16, 2048):
        p = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64).view(np.uint64)
        assert np.array_equal(R.inverse_twisted_dft_longdouble(O.poly_fft(p)), p)


# ----------------------------------------------------------------------------------------------- tier A


@pytest.mark.parametrize("cls", C.CLASSES)
@pytest.mark.parametrize("shape", list(C.PBS_SHAPES))
def test_one_step_pbs_against_exact_arithmetic(shape, cls):
    for c in C.pbs_cases(shape, cls):
        bsk = C.key_fft(c.key)
        got = [C.pbs_oracle(c, it, bsk) for it in c.items]
        C.check_tier_a(c, got, [C.pbs_exact(c, it) for it in c.items], [C.pbs_exact(c, it, R.NUMPY) for it in c.items], "oracle")


def oracle_cmux(c, d0, d1, g):
    P = c.P
    return O.cmux(d0.reshape(-1), d1.reshape(-1), g, P.N, P.k, P.cbs_radix_log, P.cbs_count).reshape(d0.shape)


@pytest.mark.parametrize("cls", C.CLASSES)
@pytest.mark.parametrize("shape", list(C.CMUX_SHAPES))
def test_cmux_family_against_exact_arithmetic(shape, cls):
    for c in C.cmux_cases(shape, cls):
        g, lb, cnt = C.key_fft(c.key), c.P.cbs_radix_log, c.P.cbs_count
        got, ex, nf = [], [], []
        for d0, d1 in c.items:
            got.append(oracle_cmux(c, d0, d1, g))
            ex.append(R.cmux(d0, d1, c.key, lb, cnt))
            nf.append(R.cmux(d0, d1, c.key, lb, cnt, R.NUMPY))
            got.append(oracle_cmux(c, np.zeros_like(d0), d1 - d0, g))           # multiply_glwe_ggsw
            ex.append(R.multiply_glwe_ggsw(d1 - d0, c.key, lb, cnt))
            nf.append(R.multiply_glwe_ggsw(d1 - d0, c.key, lb, cnt, R.NUMPY))
        a, b = C.glev_of(c)
        got.append(np.stack([oracle_cmux(c, a[i], b[i], g) for i in range(cnt)]))  # glev_cmux: every level
        ex.append(R.glev_cmux(a, b, c.key, lb, cnt))
        nf.append(R.glev_cmux(a, b, c.key, lb, cnt, R.NUMPY))
        C.check_tier_a(c, got, ex, nf, "oracle")


@pytest.mark.parametrize("cls", C.CLASSES)
@pytest.mark.parametrize("shape", list(C.SS_SHAPES))
def test_scheme_switch_every_row_against_exact_arithmetic(shape, cls):
    for c in C.ss_cases(shape, cls):
        P = c.P
        ssk = C.key_fft(c.key)
        got = [C.ggsw_bins_to_words(O.scheme_switch_fft(glev.reshape(-1), ssk, P), P) for glev in c.items]
        ex = [R.scheme_switch(glev, c.key, P.ss_radix_log, P.ss_count) for glev in c.items]
        nf = [R.scheme_switch(glev, c.key, P.ss_radix_log, P.ss_count, R.NUMPY) for glev in c.items]
        C.check_scheme_switch(c, got, ex, nf, "oracle")


# ----------------------------------------------------------------------------------------------- tier B


@pytest.mark.parametrize("shape", list(C.TRACE_SHAPES))
def test_mod_switch_trace_and_rotate_phases_against_the_exact_chain(shape):
    P = C.TRACE_SHAPES[shape]
    hk = C.honest_keys(P, 1, ak=True)
    x = C.honest_glwes(P, hk, 1, 1)[0]
    args = (P.tr_radix_log, P.tr_count, P.cbs_radix_log, P.cbs_count)
    ex = R.glwe_phase(R.mod_switch_trace_and_rotate(x, hk.ak, *args), hk.glwe_sk)
    nf = R.glwe_phase(R.mod_switch_trace_and_rotate(x, hk.ak, *args, R.NUMPY), hk.glwe_sk)
    got = O.mod_switch_trace_and_rotate(x.reshape(-1), C.key_fft(hk.ak), P).reshape(P.cbs_count, P.k + 1, P.N)
    C.check_tier_b(f"trace-{shape}", R.glwe_phase(got, hk.glwe_sk), ex, nf, "oracle")


def rotation_case(P, tag, count=1):
    """`count` independent (LWE, LUT) pairs under one key, their phases pooled.  A phase is b - sum a_i s_i: the error of every mask
    coefficient enters every phase coefficient, so at N = 128 the phase polynomial of ONE ciphertext holds few independent values and
    the rms ratio of two pipelines scatters between 0.9 and 2.1 from input to input while their word distances stay at 1.19 .. 1.26
    (profiles/r07_fft_error.md); the small shape therefore pools eight inputs."""
    hk = C.honest_keys(P, 2, bsk=True)
    lwe, lut = C.rotation_inputs(P, 2, count)
    bsk = C.key_fft(hk.bsk)
    lb, cnt = P.pbs_radix_log, P.pbs_count
    t0 = time.time()
    steps = [[] for _ in range(count)]
    ex = [R.generalized_pbs(lwe[i], lut[i], hk.bsk, lb, cnt, steps=steps[i]) for i in range(count)]
    t1 = time.time()
    nf = [R.generalized_pbs(lwe[i], lut[i], hk.bsk, lb, cnt, be=R.NUMPY) for i in range(count)]
    got = [O.generalized_pbs(lwe[i], lut[i].reshape(-1), bsk, P).reshape(P.k + 1, P.N) for i in range(count)]
    print(f"rotation-{tag}: exact chain {t1 - t0:.1f} s")
    ph = lambda xs: R.glwe_phase(np.stack(xs), hk.glwe_sk)  # noqa: E731
    # no bias condition on the phases: the numpy chain itself misses it (8.4 at S = 64, up to 11 for single inputs at N = 128): every
    # mask error enters every phase coefficient through the same key, the coefficients are not independent samples ...
    C.check_tier_b(f"rotation-{tag}", ph(got), ph(ex), ph(nf), "oracle", mean_test=False)
    # ... so the bias of a chain is asserted on WORDS, step by step along the exact chain: every step restarted from the exact
    # accumulator, its signed word error pooled over all S steps.  The word errors of a step are independent roundings, and a bias of
    # b a step (truncation where the reference rounds), which would grow to S b over the chain, shows at 6 rms / sqrt(S (k+1) N).
    glen = bsk.size // P.lwe_n
    d_or, d_np = [], []
    for st, final in zip(steps, ex):
        for i, (acc, a_t) in enumerate(st):
            nxt = st[i + 1][0] if i + 1 < len(st) else final
            rot = R.mul_monomial(acc, a_t)
            o = O.cmux(acc.reshape(-1), rot.reshape(-1), bsk[i * glen:(i + 1) * glen], P.N, P.k, lb, cnt).reshape(acc.shape)
            d_or.append(R.signed_difference(o, nxt))
            d_np.append(R.signed_difference(R.cmux(acc, rot, hk.bsk[i], lb, cnt, R.NUMPY), nxt))
    d_or, d_np = np.concatenate(d_or, axis=None), np.concatenate(d_np, axis=None)
    z = lambda d: d.mean() / (d.std() / np.sqrt(d.size))  # noqa: E731
    print(f"rotation-{tag}: per-step word bias over {d_or.size} words: oracle mean/(rms/sqrt n) {z(d_or):.2f}, numpy {z(d_np):.2f}, "
          f"rms ratio {d_or.std() / d_np.std():.3f}")
    assert abs(z(d_or)) <= 6.0, (tag, z(d_or))


@pytest.mark.parametrize("shape", list(C.ROTATION_SHAPES))
def test_blind_rotation_phases_against_the_exact_chain(shape):
    """S = 64 and S = 637 (the whole rotation) at the DEFAULT_128 shape, S = 20 at N = 128, k = 2"""
    rotation_case(C.ROTATION_SHAPES[shape], shape, count=8 if C.ROTATION_SHAPES[shape].N < 2048 else 1)


def test_circuit_bootstrap_feeding_an_exact_cmux_against_the_exact_chain():
    P = C.CBS_SHAPE
    hk = C.honest_keys(P, 3, bsk=True, ak=True, ssk=True)
    bsk, ak, ssk = C.key_fft(hk.bsk), C.key_fft(hk.ak), C.key_fft(hk.ssk)
    d = C.honest_glwes(P, hk, 3, 2)
    rng = np.random.default_rng(33)
    # Eight inputs pooled: the trace keeps ONE coefficient of the bootstrap's output for each level, so the selector's error, and with
    # it the whole phase polynomial of the CMUX, hangs on cbs_count scalars; for a single input the rms ratio of two pipelines is a
    # ratio of a few Gaussian draws (measured 1.4 and 3.6 for two inputs), not a statistic
    phases, want = [], []
    for i in range(8):
        lwe = R.lwe_encrypt(rng, hk.lwe_sk, (i % 2) << 63, 1 << 50)
        phases.append(C.cbs_cmux_phases(hk, lwe, d, lambda x: C.ggsw_bins_to_words(O.circuit_bootstrap(x, bsk, ak, ssk, P), P)))
        want.append(R.glwe_phase(d[i % 2], hk.glwe_sk))
    ex, nf, got = (np.stack([p[j] for p in phases]) for j in range(3))
    # no bias condition: the numpy chain misses it (-30 and -17 for single inputs), as in the blind rotation
    C.check_tier_b("cbs-cmux", got, ex, nf, "oracle", mean_test=False)
    # and the chain means what it should: the phase of the selected ciphertext (uniform message words), up to the noise of a
    # circuit-bootstrapped selector at 4 x 4 bits (measured 2^-15.4; a wrong selection is a uniform distance, 1/4 on average)
    assert R.torus_distance(ex, np.stack(want)).max() < 2.0 ** -10


# ----------------------------------------------------------------------------------------------- rotation by an encrypted shift


@pytest.mark.parametrize("cls", C.CLASSES)
def test_rotate_cmux_step_against_exact_arithmetic(cls):
    for c in C.rot_cases(cls):
        g = C.key_fft(c.key)
        C.check_tier_a(c, [C.rot_oracle(c, it, g) for it in c.items], [C.rot_exact(c, it) for it in c.items],
                       [C.rot_exact(c, it, R.NUMPY) for it in c.items], "oracle")


@pytest.mark.parametrize("shape", list(C.ENC_SHIFT_SHAPES))
def test_encrypted_shift_rotation_phases_against_the_exact_chain(shape):
    c = C.enc_shift_case(shape)             # asserts that the exact chain rotates the input's phase
    # (the issue of the bias condition on these phases, and why the seed of a shape is chosen: profiles/r14_exact_reference_new_ops.md)
    got = np.stack([C.enc_shift_oracle(c, i, C.key_fft(c.sel[i]).reshape(c.n_bits, -1)) for i in range(len(c.shifts))])
    C.check_tier_b(c.name, R.glwe_phase(got, c.hk.glwe_sk), c.exact, c.numpy, "oracle")
    sel = [C.key_fft(g).reshape(c.n_bits, -1) for g in c.sel]
    P = c.P
    C.check_step_bias(c, lambda i, j, acc, r: O.cmux(acc.reshape(-1), O.glwe_mul_xn(acc.reshape(-1), 2 * P.N - r, P.N, P.k), sel[i][j],
                                                     P.N, P.k, P.cbs_radix_log, P.cbs_count).reshape(acc.shape), "oracle")


# ----------------------------------------------------------------------------------------------- the forward transform


@pytest.mark.parametrize("n", C.FFT_SIZES)
def test_forward_transform_against_the_long_double_dft(n):
    refs = C.fft_references(n)
    for name, polys in C.fft_cases(n):
        C.check_forward(name, np.stack([O.poly_fft(p) for p in polys]), *refs[name], "oracle")
    # the two long-double transforms are inverses of each other, word for word.  Their round trip's own rounding is about 2^-60
    # of the coefficients' magnitude (two N/2-term sums at a 64-bit mantissa; up to 16 words on full 64-bit coefficients at
    # N = 2048), so the polynomial is uniform below 2^55: 2^-5 of a word
    p = np.random.default_rng([0xA6, n]).integers(-(1 << 55), 1 << 55, n, dtype=np.int64)
    assert np.array_equal(R.inverse_twisted_dft_longdouble(R.forward_twisted_dft_longdouble(p)), p.view(np.uint64))
    # and a delta at coefficient 1 has the twiddle e^{i pi (1 - 4m) / N} in bin m
    d = np.zeros(n, dtype=np.int64)
    d[1] = 1 << 62
    m = np.arange(n // 2)
    want = 2.0 ** 62 * np.exp(1j * np.pi * ((1 - 4 * m) % (2 * n)) / n)
    assert np.abs(R.forward_twisted_dft_longdouble(d).astype(np.complex128) - want).max() <= 2.0 ** 62 * 2.0 ** -50


# ----------------------------------------------------------------------------------------------- packed integers


def test_pack_unpack_and_bivariate_pack_statements():
    """the oracle has no pack, unpack or bivariate packing of its own: the project states them with its glwe_mul_xn + glwe_xor
    tree (tests/test_packed_plaintext.py), its sample_extract, and a wrapping multiply-add (tests/test_gpu_bivariate.py)"""
    from tests.test_packed_plaintext import oracle_tree_pack
    for P in (C.D128, C.N128K2):
        n, k = P.N, P.k
        rng = np.random.default_rng([0xA7, n, k])
        for n_bits in (1, 16, n):
            bits = rng.integers(0, 1 << 64, (n_bits, k + 1, n), dtype=np.uint64)
            packed = R.pack(bits)
            if n_bits <= 16 or n <= 128:        # the tree costs a glwe_mul_xn for each bit
                assert np.array_equal(packed.reshape(-1), oracle_tree_pack(bits.reshape(n_bits, -1), n, k)), (n, n_bits)
            lwes = R.unpack(packed, n_bits)
            assert lwes.shape == (n_bits, k * n + 1)
            for i in sorted({0, n_bits // 2, n_bits - 1}):
                assert np.array_equal(lwes[i], O.sample_extract(packed.reshape(-1), i, n, k)), (n, n_bits, i)
        # honest encryptions of constant polynomials: the packed phase carries bit i in coefficient i, and unpacking returns it
        sk = R.binary_key(rng, k * n)
        value = [int(b) for b in rng.integers(0, 2, 16)]
        msgs = np.zeros((16, n), dtype=np.uint64)
        msgs[:, 0] = np.array(value, dtype=np.uint64) << np.uint64(63)
        packed = R.pack(R.glwe_encrypt(rng, sk, msgs, C.NOISE))
        ph = R.glwe_phase(packed, sk)
        want = np.zeros(n, dtype=np.uint64)
        want[:16] = msgs[:, 0]
        assert R.torus_distance(ph, want).max() <= 16 * C.NOISE / 2.0 ** 64
        for i, lwe in enumerate(R.unpack(packed, 16)):
            assert (lwe[-1:] - (lwe[:-1] * sk).sum(dtype=np.uint64, keepdims=True))[0] == ph[i]
    left, right = rng.integers(0, 1 << 64, (2, 5, 638), dtype=np.uint64)
    for p in (1, 2, 7, 63):
        want = [[(int(a) * (1 << p) + int(b)) & M64 for a, b in zip(ra, rb)] for ra, rb in zip(left, right)]
        assert R.bivariate_pack(left, right, p).tolist() == want, p


# ----------------------------------------------------------------------------------------------- the new conditions bite


def _must_fail(what: str, check) -> str:
    """the check raises an AssertionError for the wrong variant; its message is printed (profiles/r14_exact_reference_new_ops.md)"""
    with pytest.raises(AssertionError) as e:
        check()
    print(f"bites: {what}: {str(e.value).splitlines()[0][:160]}")
    return str(e.value)


def test_the_new_conditions_bite():
    """wrong variants built from poly_ref's own pieces in EXACT arithmetic (or numpy's transform), so that the structure alone is
    wrong: each must fail the condition that holds the oracle and the kernels"""
    c = C.rot_cases("uniform")[0]
    lb, cnt = c.P.cbs_radix_log, c.P.cbs_count

    def no_flip(acc, r):
        return np.roll(acc, -r, axis=-1)

    wrong_steps = {"r + 1 for r": lambda acc, r: R.mul_monomial(acc, -(r + 1)),
                   "no sign flip at the wrap": no_flip,
                   "X^+r for X^-r": lambda acc, r: R.mul_monomial(acc, r)}
    for what, high in wrong_steps.items():
        for it in c.items[::4]:             # every r on its own: r = 1 moves a single coefficient of each polynomial past the wrap
            one = C.Case(c.name, c.cls, c.P, c.key, [it], c.sigma)
            bad = R.cmux(it[0], high(*it), c.key, lb, cnt)
            _must_fail(f"{what}, r = {it[1]}",
                       lambda: C.check_tier_a(one, [bad], [C.rot_exact(one, it)], [C.rot_exact(one, it, R.NUMPY)], "wrong"))

    e = C.enc_shift_case("default128_4bit_stride8")
    P = e.P
    bad = R.glwe_phase(np.stack([R.blind_rotation_by_shift(e.glwe[i], e.sel[i][::-1], e.log_stride, P.cbs_radix_log, P.cbs_count)
                                 for i in range(len(e.shifts))]), e.hk.glwe_sk)
    # (shifts 0 and 15 read the same backwards and still rotate as they should; 5 and 10 are each other's reverse)
    _must_fail("bits consumed in descending order, against the exact chain", lambda: C.check_tier_b(e.name, bad, e.exact, e.numpy, "wrong"))
    _must_fail("bits consumed in descending order, against the rotated input", lambda: C.check_rotated_phase(e, bad, "wrong"))

    for n in C.FFT_SIZES:
        refs = C.fft_references(n)
        tw = np.exp(1j * np.pi * np.arange(n // 2) / n)
        tw[3] *= 1.0 + 2.0 ** -40
        h = n // 2
        rev = np.array([int(format(m, f"0{h.bit_length() - 1}b")[::-1], 2) for m in range(h)])
        for name, polys in C.fft_cases(n):
            exact, nb = refs[name]
            _must_fail(f"{name}: one twist entry off by 2^-40",       # entry 3: the delta at coefficient 3 reads it in every bin
                       lambda: C.check_forward(name, R.NUMPY.forward_bins(R.signed(polys), tw), exact, nb, "wrong"))
            _must_fail(f"{name}: bins in bit-reversed order", lambda: C.check_forward(name, nb[..., rev], exact, nb, "wrong"))
