"""Every loop of spf_amd/csrc/spf_hip.hip that cuts one call into several launches, run past its first launch (the table and the
arithmetic of each case: tests/launch_slice_cases.py, held to the sources by tests/test_launch_slice_cases.py on the CPU).  A wrong
stride or a dropped offset gives the right words for every batch that fits one launch, so each batch here is one ragged launch
longer.  It repeats seven distinct items, and 7 divides no launch size: row i of the output must equal the reference of item i % 7,
computed for the seven only.  Every operation is integer arithmetic or held bit-equal to the oracle elsewhere: there is no
tolerance in this file.  The calls go through the device-pointer forms, the output between sentinel rows that must survive."""
import time

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import launch_slice_cases as LS
from tests import lwe_linear_cases as LC
from tests import pbs_graph_cases as K
from tests import pfks_cases as PC
from tests import pufks_cases as PU
from tests.polyref_cases import key_fft
from tests.test_gpu_private_functional_keyswitch import components_ref
from tests.util import random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
GUARD = 2                       # sentinel rows before and behind the output
D = LS.DISTINCT
C = LS.constants()
P16 = K.SMALL16
LWE0, LWE1 = 0, 1


def test_the_tables_contexts_are_the_suites():
    for name, P in (("small16", P16), ("default128", O.DEFAULT_128)):
        assert LS.CONTEXTS[name] == dict(N=P.N, k=P.k, lwe_n=P.lwe_n, cbs_count=P.cbs_count), name


@pytest.fixture(scope="module")
def small16():
    """the N = 16, k = 1, n = 5 context with the oracle's bootstrap and keyswitch keys"""
    e = K.make_engine("n16k1")
    yield e
    e.close()


@pytest.fixture(scope="module")
def default128():
    e = spf_amd.Engine(to_engine_params(O.DEFAULT_128))     # no keys: the linear maps need none
    yield e
    e.close()


def repeat(items, B):
    return np.ascontiguousarray(items[np.arange(B) % D])


def on_device(eng, inputs, rows, row_words, call):
    """`call(device pointers of the inputs, device pointer of the output)` with the output's `rows` rows of `row_words` words
    between GUARD sentinel rows on each side -> the output rows; the sentinels are checked here"""
    bufs = []
    try:
        d_in = []
        for a in inputs:
            a = np.ascontiguousarray(a)
            d_in.append(eng.device_alloc(a.nbytes))
            bufs.append(d_in[-1])
            eng.device_upload(d_in[-1], a)
        whole = np.full((rows + 2 * GUARD, row_words), SENTINEL, dtype=np.uint64)
        d_out = eng.device_alloc(whole.nbytes)
        bufs.append(d_out)
        eng.device_upload(d_out, whole)
        t0 = time.perf_counter()
        call(d_in, d_out + GUARD * row_words * 8)
        eng.device_download(None, whole, d_out)
        print(f"call and download: {time.perf_counter() - t0:.3f} s")
    finally:
        for p in bufs:
            eng.device_free(p)
    assert (whole[:GUARD] == SENTINEL).all(), "words before the output were written"
    assert (whole[GUARD + rows:] == SENTINEL).all(), "words behind the output were written"
    return whole[GUARD:GUARD + rows]


def assert_rows(got, want, in_first, what):
    """every row equal; a failure says on which side of the first launch's last row the wrong rows lie"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    first = int(np.count_nonzero(in_first[bad]))
    assert bad.size == 0, (f"{what}: {first} wrong rows in the first launch, {bad.size - first} beyond it; "
                           f"first wrong rows {bad[:4].tolist()}, last {bad[-2:].tolist()}")


def plan(case_id):
    p = LS.BY_ID[case_id].plan(C)
    print(f"{case_id}: {p.total} units, {p.step} per launch, {p.launches} launches, the last of {p.last}; "
          f"host {p.host_bytes / 1e6:.1f} MB, HBM {p.hbm_bytes / 1e6:.1f} MB")
    assert p.launches >= 2 and 0 < p.last < p.step
    return p


# ---- the keyless operations of the generic family ---------------------------------------------------------------------------

def np_sample_extract(g, h, N, k):
    """sample_extract (glwe_ciphertext_ops.rs:31-76) over a batch: mask word p N + j is coefficient h - j of polynomial p for
    j <= h and minus coefficient h + N - j beyond; the body is coefficient h of the last polynomial"""
    x = g.reshape(len(g), k + 1, N)
    j = np.arange(N)
    vals = x[:, :k, np.where(j <= h, h - j, h + N - j)]
    out = np.empty((len(g), k * N + 1), dtype=np.uint64)
    out[:, :k * N] = np.where(j <= h, vals, np.uint64(0) - vals).reshape(len(g), k * N)
    out[:, k * N] = x[:, k, h]
    return out


def np_mul_xn(g, n, N):
    """every polynomial times X^n in Z[X] / (X^N + 1)"""
    x = g.reshape(len(g), -1, N)
    r = n % N
    out = np.empty_like(x)
    out[..., r:] = x[..., :N - r]
    out[..., :r] = np.uint64(0) - x[..., N - r:]
    if (n // N) % 2:
        out = np.uint64(0) - out
    return out.reshape(g.shape)


def test_generic_sample_extract(small16):
    P, case = P16, LS.BY_ID["generic_sample_extract"]
    p, h = plan(case.id), case.shape["idx"]
    items = random_glwe(0xF0, D, P.glwe_len)
    want = np_sample_extract(items, h, P.N, P.k)
    assert np.array_equal(want, np.stack([O.sample_extract(x, h, P.N, P.k) for x in items]))
    B = p.total
    got = on_device(small16, [repeat(items, B)], B, P.k * P.N + 1,
                    lambda i, o: small16.sample_extract_l1_dev(None, B, i[0], h, o))
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


@pytest.mark.parametrize("op", ["not", "xor", "mul_xn"])
def test_generic_linear_kernel(small16, op):
    P, case = P16, LS.BY_ID["generic_" + op]
    p = plan(case.id)
    a, b = random_glwe(0xF1, D, P.glwe_len), random_glwe(0xF2, D, P.glwe_len)
    B = p.total
    if op == "not":
        want = a.copy()
        want[:, P.k * P.N] += np.uint64(1 << 63)
        assert np.array_equal(want, np.stack([O.glwe_not(x, P.N, P.k) for x in a]))
        got = on_device(small16, [repeat(a, B)], B, P.glwe_len, lambda i, o: small16.glwe_not_dev(None, B, i[0], o))
    elif op == "xor":
        want = a + b
        assert np.array_equal(want, np.stack([O.glwe_xor(x, y, P.N, P.k) for x, y in zip(a, b)]))
        got = on_device(small16, [repeat(a, B), repeat(b, B)], B, P.glwe_len, lambda i, o: small16.glwe_xor_dev(None, B, i[0], i[1], o))
    else:
        n = case.shape["n"]
        want = np_mul_xn(a, n, P.N)
        assert np.array_equal(want, np.stack([O.glwe_mul_xn(x, n, P.N, P.k) for x in a]))
        got = on_device(small16, [repeat(a, B)], B, P.glwe_len, lambda i, o: small16.glwe_mul_xn_dev(None, B, i[0], n, o))
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


def test_gather_rows_through_a_shuffled_pointer_table(small16):
    case = LS.BY_ID["gather_rows"]
    p, w = plan(case.id), case.shape["words"]
    rows = p.total
    src = (np.arange(rows * w, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(rows, w)
    perm = np.random.default_rng(0xF3).permutation(rows)
    assert (perm != np.arange(rows)).sum() > rows - 50
    d_src = small16.device_alloc(src.nbytes)
    try:
        small16.device_upload(d_src, src)
        table = (np.uint64(d_src) + perm.astype(np.uint64) * np.uint64(8 * w)).astype(np.uint64)
        got = on_device(small16, [table], rows, w,
                        lambda i, o: small16._ck(small16._lib.spf_gather_rows_dev(small16._h, None, rows, w, i[0], o)))
    finally:
        small16.device_free(d_src)
    assert_rows(got, src[perm], np.arange(rows) < p.step, case.id)


# ---- the functional keyswitches ---------------------------------------------------------------------------------------------

def test_generic_public_functional_keyswitch(small16):
    P, case = P16, LS.BY_ID["generic_pufks"]
    p, s = plan(case.id), case.shape
    key = np.random.default_rng([0xF4]).integers(0, 1 << 64, (s["n"], s["count"], P.k + 1, P.N), dtype=np.uint64)
    small16.load_public_functional_keyswitch_key_std(key, s["log"], s["count"])
    keyf = key_fft(key)
    items = np.random.default_rng([0xF5]).integers(0, 1 << 64, (D, s["p"], s["n"] + 1), dtype=np.uint64)
    want = np.stack([PU.pufks_oracle(x, keyf, P.N, P.k, s["log"], s["count"]).reshape(-1) for x in items])
    B = p.total
    got = on_device(small16, [repeat(items, B)], B, P.glwe_len,
                    lambda i, o: small16.public_functional_keyswitch_enqueue(None, B, s["p"], i[0], o))
    assert small16.last_public_functional_keyswitch_kernel() == "generic_pufks_kernel"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


def pfks_case(eng, s, n_keys, seed):
    keys, items = PC.uniform_case(seed, P16.N, P16.k, s["n"], s["p"], s["log"], s["count"], D, n_keys)
    eng.load_private_functional_keyswitch_keys_std(keys, s["log"], s["count"])
    return keys, items


def test_private_functional_keyswitch_valu_kernel(small16):
    case = LS.BY_ID["pfks_valu_single"]
    p, s = plan(case.id), case.shape
    keys, items = pfks_case(small16, s, 1, 0xF6)
    want = PC.pfks_ref(items, keys[0], s["log"], s["count"])
    B = p.total
    got = on_device(small16, [repeat(items, B)], B, P16.glwe_len,
                    lambda i, o: small16.private_functional_keyswitch_enqueue(None, 0, B, i[0], o))
    assert small16.last_private_functional_keyswitch_kernel() == "pfks_valu_kernel"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


def test_ggsw_components_valu_kernel(small16):
    """launches of whole items: kMaxGridRows / L * L rows"""
    P, case = P16, LS.BY_ID["pfks_valu_components"]
    p, s, L = plan(case.id), case.shape, P16.cbs_count
    keys = np.random.default_rng([0xF7]).integers(0, 1 << 64, (P.k + 1, 1, s["n"] + 1, s["count"], P.k + 1, P.N), dtype=np.uint64)
    small16.load_private_functional_keyswitch_keys_std(keys, s["log"], s["count"])
    items = np.random.default_rng([0xF8]).integers(0, 1 << 64, (D, L, s["n"] + 1), dtype=np.uint64)
    want = components_ref(items, keys, s["log"], s["count"]).reshape(D, -1)
    assert p.total % L == 0 and p.step % L == 0
    B = p.total // L
    got = on_device(small16, [repeat(items, B)], B, want.shape[1],
                    lambda i, o: small16.apply_pfks_on_ggsw_components_enqueue(None, B, i[0], o))
    assert small16.last_private_functional_keyswitch_kernel() == "pfks_valu_kernel"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step // L, case.id)


def test_private_functional_keyswitch_gemm_past_the_digit_cap(small16):
    """one-bit digits x 63 of 130 words: 8190 limb bytes a row, padded to 8192, so kPfksDigitCap holds 131 072 rows; the second
    launch is one full row tile and one row"""
    case = LS.BY_ID["pfks_gemm_cap"]
    p, s = plan(case.id), case.shape
    assert p.last == C["PFKS_TILE"] + 1
    keys, items = pfks_case(small16, s, 1, 0xF9)
    want = PC.pfks_ref(items, keys[0], s["log"], s["count"])
    assert want[0].tolist() == PC.pfks_literal(items[0], keys[0], s["log"], s["count"])
    B = p.total
    try:
        got = on_device(small16, [repeat(items, B)], B, P16.glwe_len,
                        lambda i, o: small16.private_functional_keyswitch_enqueue(None, 0, B, i[0], o))
        assert small16.last_private_functional_keyswitch_kernel() == "pfks_gemm_kernel<1>"
    finally:
        small = np.zeros((1, 1, 2, 2, P16.k + 1, P16.N), dtype=np.uint64)
        small16.load_private_functional_keyswitch_keys_std(small, 4, 2)
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


def test_circuit_bootstrap_via_pfks_extract_loop(small16):
    """keys on the matrix cores, where launch_pfks takes these rows in one launch: of the chain's loops only the one around
    pfks_extract_rotate_kernel slices.  The reference per distinct item: the oracle's bootstrap, numpy's extract-and-rotate,
    pfks_ref, the oracle's forward transform"""
    P, case = P16, LS.BY_ID["cbs_via_pfks_extract"]
    p, s, L = plan(case.id), case.shape, P16.cbs_count
    _, ks, _, _ = K.keys_of("n16k1")
    keys = np.random.default_rng([0xFA]).integers(0, 1 << 64, (P.k + 1, 1, s["n"] + 1, s["count"], P.k + 1, P.N), dtype=np.uint64)
    small16.load_private_functional_keyswitch_keys_std(keys, s["log"], s["count"])
    items = random_lwe_batch(0xFB, D, P.lwe_n)
    glwe = np.stack([O.cbs_pbs(x, ks.bsk_fft, P) for x in items])
    assert np.array_equal(glwe, small16.circuit_bootstrap_pbs(items)), "the bootstrap stage differs from the oracle at B = 7"
    ggsw = components_ref(PC.extract_and_rotate(glwe.reshape(D, P.k + 1, P.N), L, P.cbs_radix_log), keys, s["log"], s["count"])
    want = np.stack([O.poly_fft(poly) for poly in ggsw.reshape(-1, P.N)]).view(np.uint64).reshape(D, -1)
    B = p.total // L
    got = on_device(small16, [repeat(items, B)], B, want.shape[1],
                    lambda i, o: small16.circuit_bootstrap_via_pfks_enqueue(None, B, i[0], o))
    assert small16.last_private_functional_keyswitch_kernel() == "pfks_gemm_kernel<1>"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step // L, case.id)


# ---- plaintext linear maps --------------------------------------------------------------------------------------------------

def lin_case(eng, ctx, s, cls, slot, seed, with_bias):
    W = LS.words(ctx, s["kind"])
    w = LC.class_weights(seed, s["M"], s["K"], cls)
    bias = np.random.default_rng([0xFC, seed]).integers(0, 1 << 64, s["M"], dtype=np.uint64) if with_bias else None
    eng.load_lwe_linear_weights(slot, w, bias)
    items = LC.uniform_inputs(seed, D, s["K"], W)
    return W, w, items, LC.linear_ref(items, w, bias).reshape(D, s["M"] * W)


def test_linear_map_valu_kernel_items(small16, monkeypatch):
    case = LS.BY_ID["lin_valu_items"]
    p, s = plan(case.id), case.shape
    W, w, items, want = lin_case(small16, "small16", s, "int64", 11, 0x51, False)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", "valu")
    B = p.total
    got = on_device(small16, [repeat(items, B)], B, s["M"] * W, lambda i, o: small16.lwe_linear_enqueue(None, 11, LWE0, B, i[0], o))
    assert small16.last_lwe_linear_kernel() == LC.VALU
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


def test_linear_map_valu_kernel_rows_with_a_bias(small16, monkeypatch):
    """the `m0` loop over groups of output rows: it offsets the weights, the bias and the output.  The M rows repeat seven
    distinct weight rows and bias words; the two items differ."""
    case = LS.BY_ID["lin_valu_rows"]
    p, s = plan(case.id), case.shape
    M, B, W = p.total, s["B"], LS.words("small16", s["kind"])
    w7 = LC.class_weights(0x52, D, s["K"], "int64")
    b7 = np.random.default_rng([0xFC, 0x52]).integers(0, 1 << 64, D, dtype=np.uint64)
    x = LC.uniform_inputs(0x52, B, s["K"], W)
    want7 = LC.linear_ref(x, w7, b7)                                       # (B, 7, W)
    small16.load_lwe_linear_weights(12, repeat(w7, M), repeat(b7, M))
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", "valu")
    try:
        got = on_device(small16, [x], B * M, W, lambda i, o: small16.lwe_linear_enqueue(None, 12, LWE0, B, i[0], o))
        assert small16.last_lwe_linear_kernel() == LC.VALU
    finally:
        small16.load_lwe_linear_weights(12, np.zeros((1, 1), dtype=np.int64))
    want = np.ascontiguousarray(want7[:, np.arange(M) % D]).reshape(B * M, W)
    assert_rows(got, want, np.arange(B * M) % M < p.step, case.id)


def test_linear_map_matrix_cores_past_the_plane_cap_with_a_bias(default128, monkeypatch):
    """level-0 ciphertexts of DEFAULT_128: 8 * 638 * 128 bytes of planes per item, 1643 items per launch"""
    case = LS.BY_ID["lin_mfma_cap"]
    p, s = plan(case.id), case.shape
    assert p.step == C["kLweLinearImageCap"] // (8 * LS.words("default128", s["kind"]) * 128)
    W, w, items, want = lin_case(default128, "default128", s, 2, 13, 0x53, True)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", "mfma")
    B = p.total
    got = on_device(default128, [repeat(items, B)], B, s["M"] * W, lambda i, o: default128.lwe_linear_enqueue(None, 13, LWE0, B, i[0], o))
    assert default128.last_lwe_linear_kernel() == LC.kernel_name(w) == "pfks_gemm_kernel<2>"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


def test_linear_map_matrix_cores_past_the_grid_limit(small16, monkeypatch):
    case = LS.BY_ID["lin_mfma_grid"]
    p, s = plan(case.id), case.shape
    assert p.step == C["lin_per"]
    W, w, items, want = lin_case(small16, "small16", s, 2, 14, 0x54, False)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", "mfma")
    B = p.total
    got = on_device(small16, [repeat(items, B)], B, s["M"] * W, lambda i, o: small16.lwe_linear_enqueue(None, 14, LWE0, B, i[0], o))
    assert small16.last_lwe_linear_kernel() == LC.kernel_name(w) == "pfks_gemm_kernel<2>"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)


# ---- the keyswitch ----------------------------------------------------------------------------------------------------------

def test_keyswitch_past_the_grid_limit(small16):
    """one ciphertext more than 65535 groups of KS_CT: what launch_keyswitch's batch check accepts, it has to compute"""
    P, case = P16, LS.BY_ID["keyswitch_grid_y"]
    p = plan(case.id)
    _, ks, _, _ = K.keys_of("n16k1")
    items = random_lwe_batch(0xFD, D, P.k * P.N)
    want = np.stack([O.keyswitch_lwe(x, ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count) for x in items])
    B = p.total
    got = on_device(small16, [repeat(items, B)], B, P.lwe_n + 1, lambda i, o: small16.keyswitch_dev(None, B, i[0], o))
    assert small16.last_keyswitch_kernel() == "keyswitch_kernel"
    assert_rows(got, repeat(want, B), np.arange(B) < p.step, case.id)
