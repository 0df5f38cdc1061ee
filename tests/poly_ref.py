"""An independent, exact statement of every polynomial operation the FFT-based kernels perform (test infrastructure).

Neither the oracle nor the library is imported here.  Everything in the exact path is wrapping uint64 numpy arithmetic or
Python integers, written from the definitions over R = Z_{2^64}[X] / (X^N + 1); digits come from tests/decomp_ref.py.  Both
the oracle and the HIP kernels are held to it up to the rounding of their f64 transform.

Two product engines share the structure of every operation below:

  EXACT   sum_t d_t * K_t in R by the signed Toeplitz (negacyclic convolution) matrix of each key polynomial, as one wrapping
          uint64 matrix product over all digit polynomials of a call.
  NUMPY   the same sum through numpy.fft in complex128 (twist by e^{i pi j / N}, np.fft.fft, pointwise multiply-add,
          inverse, exact reduction mod 2^64 on Python integers).  It stands in for the reference's library transform
          (rustfft): a library-grade f64 FFT that shares no butterfly, table or operation order with the project's own
          transform.  It is a YARDSTICK for how much rounding an f64 pipeline may show, never an expected value.

Citations are to the reference (sunscreen_tfhe/src/...), as in oracle/spf_oracle.h; the text is a restatement of the
mathematics those lines implement, not of their code.

Layouts (time domain, uint64): GLWE (k+1, N), mask polynomials then body; GGSW (k+1, L, k+1, N) = [row][level][poly];
GLWE keyswitch key (k, L, k+1, N); automorphism keys (log2 N, k, L, k+1, N); scheme-switch key (k(k+1)/2, L, k+1, N) with
the pairs (i <= j) in row-major upper-triangular order.  Level `lvl` of a GLEV carries its message times 2^(64 - logB*(lvl+1)).
"""
import functools

import numpy as np

from tests.decomp_ref import M64, digits_array

U = np.uint64

# the long-double inverse below needs the 64-bit mantissa of x87 extended precision
assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an 80-bit (or wider) type on this host"


def _u(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def signed(x) -> np.ndarray:
    """torus words as signed integers in [-2^63, 2^63)"""
    return _u(x).view(np.int64)


def torus_distance(a, b) -> np.ndarray:
    """|a - b| on the torus, as a fraction of 2^64 (float64; only used to report and bound distances)"""
    return np.abs((_u(a) - _u(b)).view(np.int64).astype(np.float64)) / 2.0 ** 64


def signed_difference(a, b) -> np.ndarray:
    """(a - b) mod 2^64 centred on 0, as a fraction of 2^64, with its sign"""
    return (_u(a) - _u(b)).view(np.int64).astype(np.float64) / 2.0 ** 64


# ----------------------------------------------------------------------------------------------- the ring


def toeplitz(key) -> np.ndarray:
    """T with T[i, j] = coefficient of X^i in key * X^j mod X^N + 1:  key[i - j] for i >= j, -key[N + i - j] below.
    A strided view of (-key, key), no copy: T @ d is the negacyclic product key * d."""
    key = _u(key)
    n = key.size
    ext = np.concatenate([U(0) - key, key])
    return np.lib.stride_tricks.as_strided(ext[n:], shape=(n, n), strides=(ext.itemsize, -ext.itemsize), writeable=False)


def negacyclic_mul(a, key) -> np.ndarray:
    """a * key mod (X^N + 1, 2^64) for one polynomial a (N,) or a stack (M, N) of them (math/fft/negacyclic/mod.rs:147-164
    states the product this way: X^N = -1)"""
    a = _u(a)
    out = toeplitz(key) @ a.reshape(-1, a.shape[-1]).T
    return np.ascontiguousarray(out.T).reshape(a.shape)


def schoolbook_mul(a, b) -> list:
    """the same product on Python integers, term by term (self-check of the Toeplitz form)"""
    n = len(a)
    c = [0] * n
    for i in range(n):
        for j in range(n):
            if i + j < n:
                c[i + j] += int(a[i]) * int(b[j])
            else:
                c[i + j - n] -= int(a[i]) * int(b[j])
    return [v & M64 for v in c]


def mul_monomial(p, e: int) -> np.ndarray:
    """p * X^e over the last axis, any integer e (X^(2N) = 1, X^N = -1; entities/polynomial.rs:171-236)"""
    p = _u(p)
    n = p.shape[-1]
    e %= 2 * n
    s = e % n
    out = np.roll(p, s, axis=-1)
    out[..., :s] = U(0) - out[..., :s]
    return U(0) - out if e >= n else out


def automorphism(p, t: int) -> np.ndarray:
    """p(X^t) over the last axis, t odd: the coefficient of X^i moves to X^(i t mod N) with the sign (-1)^floor(i t / N)
    (ops/polynomial/mod.rs:62-84)"""
    p = _u(p)
    n = p.shape[-1]
    it = np.arange(n) * t
    out = np.empty_like(p)
    out[..., it % n] = np.where((it // n) % 2 == 1, U(0) - p, p)
    return out


def shr_round(x, n: int) -> np.ndarray:
    """x / 2^n rounded half up, as an n-bits-shorter unsigned integer (ops/polynomial/mod.rs:86-96)"""
    x = _u(x)
    return (x >> U(n)) + ((x >> U(n - 1)) & U(1))


def sample_extract(glwe, h: int) -> np.ndarray:
    """the LWE ciphertext under the flattened GLWE secret whose phase is coefficient h of the GLWE's phase:
    (a * s)_h = sum_{j <= h} a[h - j] s[j] - sum_{j > h} a[N + h - j] s[j]   (ops/ciphertext/glwe_ciphertext_ops.rs:31-76)"""
    glwe = _u(glwe)
    k, n = glwe.shape[0] - 1, glwe.shape[1]
    j = np.arange(n)
    mask = np.where(j <= h, glwe[:k, (h - j) % n], U(0) - glwe[:k, (n + h - j) % n])
    return np.concatenate([mask.reshape(-1), glwe[k, h:h + 1]])


def pack(bits_glwe) -> np.ndarray:
    """sum_i bit_i * X^i over GLWEs (n_bits, k+1, N): bit i's message moves to coefficient i
    (parasol_runtime fluent/dynamic_generic_int_graph_nodes.rs:139-200)"""
    bits = _u(bits_glwe)
    out = np.zeros(bits.shape[1:], dtype=np.uint64)
    for i, b in enumerate(bits):
        out += mul_monomial(b, i)
    return out


def unpack(glwe, n_bits: int) -> np.ndarray:
    """sample_extract(glwe, i) for i < n_bits: (n_bits, k N + 1)   (fluent/packed_dynamic_generic_int_graph_node.rs:24-39)"""
    return np.stack([sample_extract(glwe, i) for i in range(n_bits)])


def bivariate_pack(left, right, plaintext_bits: int) -> np.ndarray:
    """left * 2^p + right on every LWE word, wrapping (ops/bootstrapping/programmable_bootstrapping.rs:603-610)"""
    return _u(left) * U((1 << plaintext_bits) & M64) + _u(right)


def modulus_switch(x: int, log_chi: int, log_v: int, log_modulus: int) -> int:
    """x * 2^log_chi (mod 2^64) rounded half up to its top (log_modulus - log_v) bits, times 2^log_v
    (ops/ciphertext/lwe_ciphertext_ops.rs:130-142)"""
    x = (int(x) << log_chi) & M64
    shift = 64 - (log_modulus - log_v)
    return ((((x >> shift) + ((x >> (shift - 1)) & 1)) & ((1 << log_modulus) - 1)) << log_v)


# ----------------------------------------------------------------------------------------------- product engines


class Exact:
    """sum_t D[:, t] * K[t, q] in R, wrapping uint64"""
    name = "exact"

    @staticmethod
    def through_transform(x) -> np.ndarray:
        """a polynomial that only passes through the transform and back: unchanged"""
        return _u(x)

    @staticmethod
    def sum_products(D, K) -> np.ndarray:
        D = np.ascontiguousarray(D, dtype=np.int64).view(np.uint64)       # (B, T, N) two's complement digits
        K = _u(K)                                                         # (T, Q, N)
        b, t_, n = D.shape
        out = np.zeros((b, K.shape[1], n), dtype=np.uint64)
        for t in range(t_):
            d = np.ascontiguousarray(D[:, t, :].T)                        # (N, B)
            for q in range(K.shape[1]):
                out[:, q, :] += (toeplitz(K[t, q]) @ d).T
        return out


def _twist(n):
    return np.exp(1j * np.pi * np.arange(n) / n)


def float_to_torus(x) -> np.ndarray:
    """round each float to the nearest integer and reduce it mod 2^64 on Python integers (exact for any finite float)"""
    flat = np.rint(np.asarray(x)).reshape(-1)
    return np.array([int(v) & M64 for v in flat], dtype=np.uint64).reshape(np.shape(x))


class NumpyFft:
    """the same sum through numpy's complex128 FFT; keys and digits enter as signed integers converted to f64 (as
    entities/polynomial.rs:257-274 does), the accumulation happens in the transform domain, one inverse per output"""
    name = "numpy"

    @staticmethod
    def forward(p_signed) -> np.ndarray:
        p = np.asarray(p_signed, dtype=np.float64)
        return np.fft.fft(p * _twist(p.shape[-1]), axis=-1)

    @staticmethod
    def inverse(spec) -> np.ndarray:
        n = spec.shape[-1]
        return float_to_torus((np.fft.ifft(spec, axis=-1) * np.conj(_twist(n))).real)

    @staticmethod
    def forward_bins(p_signed, twist=None) -> np.ndarray:
        """the N/2 bins of the folded transform (math/fft/negacyclic/mod.rs:96-107) in natural order, as the oracle and the
        kernels store a polynomial's spectrum: fold z_j = p_j + i p_{j+N/2}, twist by e^{i pi j / N}, one N/2-point np.fft.fft.
        The yardstick of forward_twisted_dft_longdouble's error measure; `twist` replaces the N/2 twist factors."""
        p = np.asarray(p_signed, dtype=np.float64)
        h = p.shape[-1] // 2
        tw = _twist(2 * h)[:h] if twist is None else twist
        return np.fft.fft((p[..., :h] + 1j * p[..., h:]) * tw, axis=-1)

    @classmethod
    def through_transform(cls, x) -> np.ndarray:
        return cls.inverse(cls.forward(signed(x)))

    @classmethod
    def sum_products(cls, D, K) -> np.ndarray:
        fd = cls.forward(np.asarray(D, dtype=np.int64))                   # (B, T, N)
        fk = cls.forward(signed(K))                                       # (T, Q, N)
        return cls.inverse(np.einsum("btn,tqn->bqn", fd, fk))


EXACT, NUMPY = Exact, NumpyFft


@functools.lru_cache(maxsize=4)
def _inverse_kernel(h: int):
    """cos and sin of pi (4 j m - j) / N for j, m < N/2 in long double; the angle is reduced mod 2N in integers first"""
    ld = np.longdouble
    n = 2 * h
    pi = ld("3.14159265358979323846264338327950288419716939937510")
    j = np.arange(h)
    ang = ((4 * np.outer(j, j) - j[:, None]) % (2 * n)).astype(ld) * (pi / ld(n))
    return np.cos(ang), np.sin(ang)


def inverse_twisted_dft_longdouble(bins) -> np.ndarray:
    """Torus words of the polynomial whose N/2 transform bins are `bins` (..., N/2), by a direct O(N^2) inverse in
    np.longdouble.  The forward transform (math/fft/negacyclic/mod.rs:96-107) folds p into z_j = (p_j + i p_{j+N/2}) and
    evaluates X_m = sum_j z_j e^{i pi j / N} e^{-2 pi i j m / (N/2)}; hence z_j = e^{-i pi j / N} (2/N) sum_m X_m e^{+4 pi i j m / N}."""
    bins = np.asarray(bins)
    if bins.dtype != np.clongdouble:               # long-double bins (forward_twisted_dft_longdouble's) are taken as they are
        bins = bins.astype(np.complex128)
    h = bins.shape[-1]
    ld = np.longdouble
    cr, ci = _inverse_kernel(h)
    xr, xi = bins.real.astype(ld), bins.imag.astype(ld)
    zr = (xr @ cr.T - xi @ ci.T) / ld(h)
    zi = (xr @ ci.T + xi @ cr.T) / ld(h)
    coeff = np.rint(np.concatenate([zr, zi], axis=-1))
    two64, two32 = ld(2) ** 64, ld(2) ** 32
    r = np.fmod(coeff, two64)                      # exact
    hi = np.floor(r / two32)                       # exact: |r| < 2^64 is an integer of at most 64 bits
    lo = r - hi * two32
    return (hi.astype(np.int64).view(np.uint64) << U(32)) + lo.astype(np.int64).view(np.uint64)


def forward_twisted_dft_longdouble(p_signed) -> np.ndarray:
    """The N/2 transform bins (natural order) of the polynomial with the exact signed integer coefficients `p_signed` (..., N),
    |p| <= 2^63, by a direct O(N^2) sum in np.longdouble (np.clongdouble out): the counterpart of the inverse above,
    X_m = sum_j (p_j + i p_{j+N/2}) e^{i pi (j - 4 j m) / N}.  The angles are those of _inverse_kernel negated (reduced mod 2N in
    integers there); a 64-bit mantissa holds every coefficient without loss."""
    p = np.asarray(p_signed)
    assert p.dtype == np.int64, p.dtype
    h = p.shape[-1] // 2
    ld = np.longdouble
    cr, ci = _inverse_kernel(h)                    # cos, sin of pi (4 j m - j) / N at [j, m]
    zr, zi = p[..., :h].astype(ld), p[..., h:].astype(ld)
    out = np.empty(zr.shape, dtype=np.clongdouble)
    out.real = zr @ cr + zi @ ci
    out.imag = zi @ cr - zr @ ci
    return out


# ----------------------------------------------------------------------------------------------- GGSW (x) GLWE


def _glev_digits(polys, radix_log: int, count: int) -> np.ndarray:
    """digit polynomials of `polys` (..., N) ordered BY KEY LEVEL: (..., count, N), entry lvl is digit count - 1 - lvl.
    Digit j (least significant first) weighs 2^(64 - logB*(count - j)), the factor level count - 1 - j of a GLEV carries
    (ops/fft_ops.rs:67-98; entities/glev_ciphertext.rs)."""
    d = digits_array(polys, radix_log, count)                 # (..., N, count), least significant first
    return np.moveaxis(d[..., ::-1], -1, -2)


def external_product(glwe, ggsw, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """GGSW (x) GLWE: out_q = sum_p sum_lvl digit_{count-1-lvl}(glwe_p) * GGSW[p][lvl][q]   (ops/fft_ops.rs:23-56).
    glwe (k+1, N) or (B, k+1, N)."""
    glwe, ggsw = _u(glwe), _u(ggsw)
    single = glwe.ndim == 2
    g = glwe.reshape((-1,) + glwe.shape[-2:])
    k1, n = g.shape[1], g.shape[2]
    assert ggsw.shape == (k1, count, k1, n)
    D = _glev_digits(g, radix_log, count).reshape(g.shape[0], k1 * count, n)
    out = be.sum_products(D, ggsw.reshape(k1 * count, k1, n))
    return out[0] if single else out


def cmux(d0, d1, ggsw, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """d0 + GGSW (x) (d1 - d0)   (ops/fft_ops.rs:149-181)"""
    d0, d1 = _u(d0), _u(d1)
    return d0 + external_product(d1 - d0, ggsw, radix_log, count, be)


def glev_cmux(a, b, ggsw, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """cmux of each constituent GLWE of two GLEVs (levels, k+1, N)   (ops/fft_ops.rs:203-220)"""
    return cmux(a, b, ggsw, radix_log, count, be)


def multiply_glwe_ggsw(glwe, ggsw, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    return external_product(glwe, ggsw, radix_log, count, be)


def blind_rotate_step(acc, a_tilde: int, ggsw, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """acc <- cmux(acc, acc * X^a~, GGSW(s_i))   (ops/bootstrapping/programmable_bootstrapping.rs:342-410)"""
    return cmux(acc, mul_monomial(acc, a_tilde), ggsw, radix_log, count, be)


def rotate_cmux_step(acc, r: int, ggsw, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """one step of the rotation by an encrypted shift: acc <- cmux(acc, acc * X^-r, GGSW(bit))   (blind_rotation.rs:216-221)"""
    return cmux(acc, mul_monomial(acc, -r), ggsw, radix_log, count, be)


def blind_rotation_by_shift(glwe, shift_ggsws, log_stride: int, radix_log: int, count: int, be=EXACT, steps=None) -> np.ndarray:
    """glwe * X^-(s << log_stride), s given as the GGSWs of its bits, least significant first (n_bits, k+1, L, k+1, N): step i
    rotates by r = 2^(i + log_stride), i ascending (ops/bootstrapping/blind_rotation.rs:202-223; the reference has log_stride 0).
    A list given as `steps` receives (accumulator before the step, r) for every step."""
    acc = _u(glwe)
    for i, g in enumerate(shift_ggsws):
        r = 1 << (i + log_stride)
        if steps is not None:
            steps.append((acc, r))
        acc = rotate_cmux_step(acc, r, g, radix_log, count, be)
    return acc


def generalized_pbs(lwe, lut_glwe, bsk, radix_log: int, count: int, log_chi=0, log_v=0, body_rotate=0, be=EXACT, steps=None):
    """lut * X^(-b~) blind-rotated by the mask: every LWE word modulus-switched to log2(2N) bits first; bsk (n, k+1, L, k+1, N);
    `body_rotate` is added to the body before the switch (ops/homomorphisms/lwe.rs:9-20).  A list given as `steps` receives
    (accumulator before the step, a~) for every step."""
    lwe, lut = _u(lwe), _u(lut_glwe)
    n_lwe, two_n = lwe.size - 1, (2 * lut.shape[-1]).bit_length() - 1
    words = [int(w) for w in lwe]
    words[n_lwe] = (words[n_lwe] + body_rotate) & M64
    ms = [modulus_switch(w, log_chi, log_v, two_n) for w in words]
    acc = mul_monomial(lut, -ms[n_lwe])
    for i in range(n_lwe):
        if steps is not None:
            steps.append((acc, ms[i]))
        acc = blind_rotate_step(acc, ms[i], bsk[i], radix_log, count, be)
    return acc


def cbs_lut(n: int, k: int, cbs_radix_log: int, cbs_count: int) -> np.ndarray:
    """the circuit bootstrap's LUT: body coefficient i holds -1/2 of level (i mod v)'s unit, 2^(64 - logB*(lvl+1) - 1), v the
    next power of two of cbs_count, zero for the padding functions (circuit_bootstrapping.rs:430-482)"""
    v = 1 << (cbs_count - 1).bit_length()
    lut = np.zeros((k + 1, n), dtype=np.uint64)
    for i in range(n):
        lvl = i % v
        if lvl < cbs_count:
            lut[k, i] = (-(1 << (64 - cbs_radix_log * (lvl + 1) - 1))) & M64
    return lut


def cbs_pbs(lwe, bsk, n: int, k: int, pbs_radix_log, pbs_count, cbs_radix_log, cbs_count, be=EXACT):
    """hi_noise_lwe_to_lo_noise_glwe (circuit_bootstrapping.rs:387-427): body + 1/4, the LUT above, log_v = log2 v"""
    log_v = (cbs_count - 1).bit_length()
    return generalized_pbs(lwe, cbs_lut(n, k, cbs_radix_log, cbs_count), bsk, pbs_radix_log, pbs_count, 0, log_v, 1 << 62, be)


# ----------------------------------------------------------------------------------------------- keyswitch, trace, scheme switch


def keyswitch_glwe(glwe, ksk, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """(0, ..., 0, b) - sum_{i<k} sum_lvl digit_{count-1-lvl}(a_i) * KSK[i][lvl]   (ops/fft_ops.rs:457-495); glwe (k+1, N) or
    (B, k+1, N)"""
    glwe, ksk = _u(glwe), _u(ksk)
    single = glwe.ndim == 2
    g = glwe.reshape((-1,) + glwe.shape[-2:])
    k, n = g.shape[1] - 1, g.shape[2]
    D = _glev_digits(g[:, :k], radix_log, count).reshape(g.shape[0], k * count, n)
    out = U(0) - be.sum_products(D, ksk.reshape(k * count, k + 1, n))
    out[:, k] += g[:, k]
    return out[0] if single else out


def trace_exponents(n: int) -> list:
    """N/2^(i-1) + 1 for i = 1 .. log2 N   (ops/automorphisms/mod.rs:35-36, 72-73)"""
    return [n // (1 << (i - 1)) + 1 for i in range(1, n.bit_length())]


def trace(glwe, ak, radix_log: int, count: int, be=EXACT) -> np.ndarray:
    """x <- x + KS_i(x(X^t_i)) for every exponent in turn: N times the constant coefficient survives
    (ops/automorphisms/mod.rs:53-85)"""
    out = _u(glwe).copy()
    for i, t in enumerate(trace_exponents(out.shape[-1])):
        out = out + keyswitch_glwe(automorphism(out, t), ak[i], radix_log, count, be)
    return out


def mod_switch_trace_and_rotate(glwe, ak, tr_radix_log, tr_count, cbs_radix_log, cbs_count, be=EXACT) -> np.ndarray:
    """level i of the output GLEV = trace(shr_round(X^(-i) * (glwe + sum_{l <= i} 2^(64 - logB(l+1) - 1) X^l), log2 N))
    (circuit_bootstrapping.rs:260-298): the half units added back accumulate from level to level.  (cbs_count, k+1, N)."""
    rotated = _u(glwe).copy()
    k, n = rotated.shape[0] - 1, rotated.shape[1]
    staged = []
    for i in range(cbs_count):
        rotated[k, i] += U(1 << (64 - cbs_radix_log * (i + 1) - 1))
        staged.append(shr_round(mul_monomial(rotated, -i), n.bit_length() - 1))
    return trace(np.stack(staged), ak, tr_radix_log, tr_count, be)          # the levels run through the rounds side by side


def pair_index(i: int, j: int, k: int) -> int:
    """position of the pair {i, j} among the upper-triangular pairs in row-major order (entities/scheme_switch_key.rs)"""
    r, c = min(i, j), max(i, j)
    return r * k - r * (r - 1) // 2 + c - r


def scheme_switch(glev, ssk, ss_radix_log: int, ss_count: int, be=EXACT) -> np.ndarray:
    """GLEV (levels, k+1, N) -> GGSW (k+1, levels, k+1, N) in the time domain (ops/fft_ops.rs:225-279, 403-442).  Row k is the
    GLEV itself; row j < k encrypts -m s_j = -b s_j + sum_r a_r (s_r s_j): the trivial ciphertext with b in mask position j
    plus sum_r sum_lvl digit(a_r) * SSK[{j, r}][lvl]."""
    glev, ssk = _u(glev), _u(ssk)
    levels, k1, n = glev.shape
    k = k1 - 1
    out = np.zeros((k1, levels, k1, n), dtype=np.uint64)
    out[k] = be.through_transform(glev)
    D = _glev_digits(glev[:, :k], ss_radix_log, ss_count).reshape(levels, k * ss_count, n)
    for j in range(k):
        key = np.stack([ssk[pair_index(j, r, k)] for r in range(k)]).reshape(k * ss_count, k1, n)
        out[j] = be.sum_products(D, key)
        out[j, :, j] += be.through_transform(glev[:, k])
    return out


def circuit_bootstrap(lwe, bsk, ak, ssk, P, be=EXACT) -> np.ndarray:
    """circuit_bootstrap_via_trace_and_scheme_switch (circuit_bootstrapping.rs:342-385), result as time-domain GGSW rows"""
    glwe = cbs_pbs(lwe, bsk, P.N, P.k, P.pbs_radix_log, P.pbs_count, P.cbs_radix_log, P.cbs_count, be)
    glev = mod_switch_trace_and_rotate(glwe, ak, P.tr_radix_log, P.tr_count, P.cbs_radix_log, P.cbs_count, be)
    return scheme_switch(glev, ssk, P.ss_radix_log, P.ss_count, be)


# ----------------------------------------------------------------------------------------------- honest keys, phases


def binary_key(rng, size: int) -> np.ndarray:
    return rng.integers(0, 2, size, dtype=np.uint64)


def small_noise(rng, shape, bound: int) -> np.ndarray:
    """integers uniform in [-bound, bound] as torus words"""
    return rng.integers(-bound, bound + 1, shape, dtype=np.int64).view(np.uint64)


def glwe_encrypt(rng, sk, msgs, noise_bound: int) -> np.ndarray:
    """msgs (M, N) -> (M, k+1, N): uniform masks, b = sum_i a_i s_i + m + e exactly (ops/encryption/glwe_encryption.rs:22-61)"""
    msgs = _u(msgs)
    sk = _u(sk).reshape(-1, msgs.shape[-1])
    k, (m, n) = sk.shape[0], msgs.shape
    ct = np.empty((m, k + 1, n), dtype=np.uint64)
    ct[:, :k] = rng.integers(0, 1 << 64, (m, k, n), dtype=np.uint64)
    ct[:, k] = msgs + small_noise(rng, (m, n), noise_bound)
    for i in range(k):
        ct[:, k] += negacyclic_mul(ct[:, i], sk[i])
    return ct


def glwe_phase(ct, sk) -> np.ndarray:
    """b - sum_i a_i s_i over the last two axes (k+1, N)"""
    ct = _u(ct)
    n = ct.shape[-1]
    sk = _u(sk).reshape(-1, n)
    flat = ct.reshape(-1, ct.shape[-2], n)
    ph = flat[:, -1].copy()
    for i in range(sk.shape[0]):
        ph -= negacyclic_mul(flat[:, i], sk[i])
    return ph.reshape(ct.shape[:-2] + (n,))


def lwe_encrypt(rng, sk, msg: int, noise_bound: int) -> np.ndarray:
    sk = _u(sk)
    a = rng.integers(0, 1 << 64, sk.size, dtype=np.uint64)
    b = (a * sk).sum(dtype=np.uint64, keepdims=True) + U(msg) + small_noise(rng, (1,), noise_bound)
    return np.concatenate([a, b])


def _glev_messages(m, radix_log: int, count: int) -> np.ndarray:
    """m * 2^(64 - logB*(lvl+1)) for every level: (..., count, N)"""
    m = _u(m)
    return np.stack([m << U(64 - radix_log * (lvl + 1)) for lvl in range(count)], axis=-2)


def ggsw_encrypt(rng, sk, msg_poly, n: int, k: int, radix_log: int, count: int, noise_bound: int) -> np.ndarray:
    """rows p < k encrypt -m s_p, row k encrypts m, each as a GLEV (ops/encryption/ggsw_encryption.rs:16-72): (k+1, L, k+1, N)"""
    skp = _u(sk).reshape(k, n)
    rows = [U(0) - negacyclic_mul(msg_poly, skp[p]) for p in range(k)] + [_u(msg_poly)]
    msgs = _glev_messages(np.stack(rows), radix_log, count).reshape((k + 1) * count, n)
    return glwe_encrypt(rng, sk, msgs, noise_bound).reshape(k + 1, count, k + 1, n)


def bootstrap_key(rng, lwe_sk, glwe_sk, n: int, k: int, radix_log: int, count: int, noise_bound: int) -> np.ndarray:
    """GGSW(s_i) for every LWE key bit (programmable_bootstrapping.rs:34-58): (n_lwe, k+1, L, k+1, N)"""
    const = np.zeros(n, dtype=np.uint64)
    out = []
    for bit in _u(lwe_sk):
        const[0] = bit
        out.append(ggsw_encrypt(rng, glwe_sk, const, n, k, radix_log, count, noise_bound))
    return np.stack(out)


def glwe_keyswitch_key(rng, sk_from, sk_to, n: int, k: int, radix_log: int, count: int, noise_bound: int) -> np.ndarray:
    """row i = GLEV of sk_from_i under sk_to (ops/keyswitch/glwe_keyswitch_key.rs): (k, L, k+1, N)"""
    msgs = _glev_messages(_u(sk_from).reshape(k, n), radix_log, count).reshape(k * count, n)
    return glwe_encrypt(rng, sk_to, msgs, noise_bound).reshape(k, count, k + 1, n)


def automorphism_keys(rng, sk, n: int, k: int, radix_log: int, count: int, noise_bound: int) -> np.ndarray:
    """for every trace exponent t: the keyswitch key from s(X^t) back to s (ops/automorphisms/mod.rs:18-46)"""
    skp = _u(sk).reshape(k, n)
    return np.stack([glwe_keyswitch_key(rng, automorphism(skp, t), sk, n, k, radix_log, count, noise_bound)
                     for t in trace_exponents(n)])


def scheme_switch_key(rng, sk, n: int, k: int, radix_log: int, count: int, noise_bound: int) -> np.ndarray:
    """GLEV(s_i s_j) for the pairs i <= j (ops/bootstrapping/scheme_switch.rs:22-70): (k(k+1)/2, L, k+1, N)"""
    skp = _u(sk).reshape(k, n)
    prods = np.stack([negacyclic_mul(skp[i], skp[j]) for i in range(k) for j in range(i, k)])
    msgs = _glev_messages(prods, radix_log, count).reshape(-1, n)
    return glwe_encrypt(rng, sk, msgs, noise_bound).reshape(prods.shape[0], count, k + 1, n)
