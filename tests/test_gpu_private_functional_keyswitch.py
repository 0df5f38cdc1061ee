"""The private functional keyswitch (`private_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/private_functional_keyswitch.rs:
107-142), `apply_pfks_on_ggsw_components` and `circuit_bootstrap_via_pfks` (ops/bootstrapping/circuit_bootstrapping.rs:162-252,
:485-514) on the GPU.  The operation is wrapping 64-bit integer arithmetic: every output word equals tests/pfks_cases.py's
`pfks_ref`.  There is no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import hip_runtime as HR
from tests import pfks_cases as PC
from tests.polyref_cases import N128K2
from tests.util import keyset, to_engine_params

pytestmark = pytest.mark.gpu
TUNED = O.DEFAULT_128.replace(lwe_n=2)
GENERIC = N128K2
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
NO_KEY, INVALID = 3, 1
TILE = 128            # spf_pfks.hpp: the row tile of the GEMM
VALU = "pfks_valu_kernel"


def kernel_name(log):
    """include/spf_hip.h: one limb up to 8 bits, ceil((log + 1) / 8) up to 23 (two balanced int8 limbs reach +-32 896 only from
    -32 896 to 32 639, so 16 bits already take three), the VALU kernel from 24"""
    if log >= 24:
        return VALU
    return f"pfks_gemm_kernel<{1 if log <= 8 else -(-(log + 1) // 8)}>"


@pytest.fixture(scope="module")
def tuned():
    e = spf_amd.Engine(to_engine_params(TUNED))
    yield e
    e.close()


@pytest.fixture(scope="module")
def generic():
    e = spf_amd.Engine(to_engine_params(GENERIC))
    yield e
    e.close()


def pick(tuned, generic, which):
    return (tuned, TUNED) if which == "tuned" else (generic, GENERIC)


def ref_batch(lwes, key, log, count):
    return PC.pfks_ref(lwes, key, log, count)


# ---- words equal pfks_ref ---------------------------------------------------------------------------------------------------

GPU_RADICES = [(4, 3), (8, 2), (9, 2), (11, 3), (16, 2), (17, 2), (23, 2), (24, 2), (31, 2), (63, 1)]


@pytest.mark.parametrize("which", ["generic", "tuned"])
@pytest.mark.parametrize("log,count", GPU_RADICES)
def test_words_equal_the_reference(tuned, generic, which, log, count):
    eng, P = pick(tuned, generic, which)
    for n in (1, 2, 5, 64):
        for p in (1, 3):
            for n_keys in (1, 3):
                if which == "tuned" and n == 64 and (p, n_keys) not in ((1, 1), (3, 3)):
                    continue                                     # (the largest tuned keys once each: 6 and 57 MB)
                keys, lwes = PC.uniform_case(7, P.N, P.k, n, p, log, count, 3, n_keys)
                before = lwes.copy()
                eng.load_private_functional_keyswitch_keys_std(keys, log, count)
                for q in range(n_keys):
                    got = eng.private_functional_keyswitch(lwes, q)
                    assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
                    want = ref_batch(lwes, keys[q], log, count)
                    assert np.array_equal(got, want), (which, log, count, n, p, n_keys, q, np.flatnonzero((got != want).any(axis=1)))
                assert np.array_equal(lwes, before)
                one = eng.private_functional_keyswitch(lwes[2:], n_keys - 1)
                assert np.array_equal(one, want[2:]), (which, log, count, n, p, n_keys, "B=1")


def test_the_reported_kernel_on_each_side_of_each_boundary(generic):
    """8 | 9 bits (one limb | two), 15 | 16 (two | three), 23 | 24 (matrix cores | VALU)"""
    P = GENERIC
    for log, name in [(8, "pfks_gemm_kernel<1>"), (9, "pfks_gemm_kernel<2>"), (15, "pfks_gemm_kernel<2>"),
                      (16, "pfks_gemm_kernel<3>"), (17, "pfks_gemm_kernel<3>"), (23, "pfks_gemm_kernel<3>"), (24, VALU)]:
        assert kernel_name(log) == name
        keys, lwes = PC.uniform_case(8, P.N, P.k, 3, 2, log, 2, 2)
        generic.load_private_functional_keyswitch_keys_std(keys, log, 2)
        got = generic.private_functional_keyswitch(lwes)
        assert generic.last_private_functional_keyswitch_kernel() == name, log
        assert np.array_equal(got, ref_batch(lwes, keys[0], log, 2)), log


@pytest.mark.parametrize("which", ["generic", "tuned"])
@pytest.mark.parametrize("log,count", [(8, 2), (17, 2), (31, 2)])
def test_tile_seams(tuned, generic, which, log, count):
    """B one below, at and one above the GEMM's row tile.  The generic context's GLWE has 384 words, the tuned one's 4096; with
    eight plane columns per word both are whole column tiles, as (k+1) N always is for N >= 16: the seam in the columns is the
    one between two keys of a set, so the middle key of three is used."""
    eng, P = pick(tuned, generic, which)
    n, p = 2, 1
    keys, items = PC.uniform_case(9, P.N, P.k, n, p, log, count, 7, 3)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    want = ref_batch(items, keys[1], log, count)
    for B in (TILE - 1, TILE, TILE + 1):
        which_item = np.arange(B) % 7
        got = eng.private_functional_keyswitch(items[which_item], 1)
        assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
        bad = np.flatnonzero((got != want[which_item]).any(axis=1))
        assert bad.size == 0, (which, log, B, bad[:8])


@pytest.mark.parametrize("which", ["generic", "tuned"])
@pytest.mark.parametrize("log,count", GPU_RADICES + [(7, 9)])
def test_extreme_operands(tuned, generic, which, log, count):
    """inputs from decomp_ref.extreme_words against key words 0, 2^64 - 1, 2^63 and 0x8080...80: every limb and every byte plane
    at an end of its range"""
    eng, P = pick(tuned, generic, which)
    key, lwes = PC.extreme_case(10, P.N, P.k, 5, 3, log, count, 4)
    eng.load_private_functional_keyswitch_keys_std(key[None], log, count)
    got = eng.private_functional_keyswitch(lwes)
    assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
    assert np.array_equal(got, ref_batch(lwes, key, log, count)), (which, log, count)


@pytest.mark.parametrize("lwe_count", [292, 294])
def test_the_int32_bound_of_the_accumulators(generic, lwe_count):
    """8 bits x 7, from_dimension 63, every input word 0x7f7f7f7f7f7f8000 (all seven digits -128), an all-zero key (every stored
    plane -128): every product is +2^14.  lwe_count = 292 gives 130 816 limb columns and the sum 2 143 289 344 < 2^31; 294 gives
    131 712 columns and a sum above 2^31 unless K is split.  The output is all zeros either way."""
    P, log, count, n = GENERIC, 8, 7, 63
    assert PC.radix_digits(0x7f7f7f7f7f7f8000, log, count) == [-128] * count
    cols = lwe_count * (n + 1) * count
    assert (cols * (1 << 14) < (1 << 31)) == (lwe_count == 292)
    keys = np.zeros((1, lwe_count, n + 1, count, P.k + 1, P.N), dtype=np.uint64)
    generic.load_private_functional_keyswitch_keys_std(keys, log, count)
    lwes = np.full((2, lwe_count, n + 1), 0x7f7f7f7f7f7f8000, dtype=np.uint64)
    lwes[1, 5:] = 0                                                 # a second row with other sums beside it
    got = generic.private_functional_keyswitch(lwes)
    assert generic.last_private_functional_keyswitch_kernel() == "pfks_gemm_kernel<1>"
    assert not got.any(), (lwe_count, np.flatnonzero(got.reshape(-1))[:8])
    small = np.zeros((1, 1, 2, 2, P.k + 1, P.N), dtype=np.uint64)   # (the 405 MB of the large key go back)
    generic.load_private_functional_keyswitch_keys_std(small, 4, 2)


# ---- isolation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["generic", "tuned"])
@pytest.mark.parametrize("log,count", [(17, 2), (31, 2)])
def test_an_output_depends_on_its_own_inputs_only_and_nothing_else_is_written(tuned, generic, which, log, count):
    eng, P = pick(tuned, generic, which)
    n, p, B, guard = 5, 3, 5, 2
    keys, item = PC.uniform_case(11, P.N, P.k, n, p, log, count, 1)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    want = ref_batch(item, keys[0], log, count)[0]
    gw = P.glwe_len
    d_in, d_out = eng.device_alloc(B * p * (n + 1) * 8), eng.device_alloc((B + 2 * guard) * gw * 8)
    try:
        for pos in (0, 1, B - 1):
            _, lwes = PC.uniform_case(12 + pos, P.N, P.k, n, p, log, count, B)    # other neighbours every time
            lwes[pos] = item[0]
            eng.device_upload(d_in, lwes)
            eng.device_upload(d_out, np.full((B + 2 * guard) * gw, SENTINEL, dtype=np.uint64))
            eng.private_functional_keyswitch_enqueue(None, 0, B, d_in, d_out + guard * gw * 8)
            got = np.empty((B + 2 * guard, gw), dtype=np.uint64)
            eng.device_download(None, got, d_out)
            assert np.array_equal(got[guard + pos], want), (which, pos)
            assert (got[:guard] == SENTINEL).all() and (got[guard + B:] == SENTINEL).all(), (which, pos, "words around the outputs")
            assert not (got[guard:guard + B] == SENTINEL).all(axis=1).any()
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)


# ---- the GGSW components ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cbs_uniform_keys(which, log, count):
    P = TUNED if which == "tuned" else GENERIC
    n = P.k * P.N
    return np.random.default_rng([0xD4, P.N, P.k, log, count]).integers(0, 1 << 64, (P.k + 1, 1, n + 1, count, P.k + 1, P.N),
                                                                        dtype=np.uint64)


def components_ref(rows, keys, log, count):
    """rows (B, L, k N + 1) -> (B, k+1, L, k+1, N): GGSW row (r, level) = pfks_ref of row `level` under key r"""
    B, L = rows.shape[:2]
    k1, N = keys.shape[-2:]
    flat = rows.reshape(B * L, 1, -1)
    return np.stack([ref_batch(flat, keys[r], log, count).reshape(B, L, k1, N) for r in range(k1)], axis=1)


@pytest.mark.parametrize("which,log,count", [("generic", 17, 2), ("generic", 31, 2), ("tuned", 17, 2)])
def test_components_equal_the_single_calls_placed_by_hand(tuned, generic, which, log, count):
    eng, P = pick(tuned, generic, which)
    L, n, B, guard = P.cbs_count, P.k * P.N, 3, 1
    keys = cbs_uniform_keys(which, log, count)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    rows = np.random.default_rng([0xD5, P.N, log]).integers(0, 1 << 64, (B, L, n + 1), dtype=np.uint64)
    got = eng.apply_pfks_on_ggsw_components(rows)
    assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
    by_hand = np.empty_like(got)
    for r in range(P.k + 1):
        by_hand[:, r] = eng.private_functional_keyswitch(rows.reshape(B * L, 1, n + 1), r).reshape(B, L, P.k + 1, P.N)
    assert np.array_equal(got, by_hand)
    assert np.array_equal(got, components_ref(rows, keys, log, count))
    # the device-pointer form between sentinels
    words = got[0].size
    d_in, d_out = eng.device_alloc(rows.nbytes), eng.device_alloc((B + 2 * guard) * words * 8)
    try:
        eng.device_upload(d_in, rows)
        eng.device_upload(d_out, np.full((B + 2 * guard) * words, SENTINEL, dtype=np.uint64))
        eng.apply_pfks_on_ggsw_components_enqueue(None, B, d_in, d_out + guard * words * 8)
        back = np.empty((B + 2 * guard, words), dtype=np.uint64)
        eng.device_download(None, back, d_out)
        assert np.array_equal(back[guard:guard + B], got.reshape(B, words))
        assert (back[:guard] == SENTINEL).all() and (back[guard + B:] == SENTINEL).all()
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)


# ---- circuit bootstrap via PFKS ---------------------------------------------------------------------------------------------

def load_some_bootstrap_key(eng, which):
    if which == "tuned":
        eng.load_bootstrap_key(keyset(0x5EED0007, TUNED.lwe_n, with_ksk=False).bsk_fft)
    else:   # words equal a composition that uses the same key: any key serves
        words = np.random.default_rng([0xD6]).integers(-(1 << 30), 1 << 30, 2 * eng.params.bsk_complex, dtype=np.int64)
        eng.load_bootstrap_key_std(words.view(np.uint64))


@pytest.mark.parametrize("which,log,count", [("generic", 17, 2), ("generic", 24, 2), ("tuned", 17, 2)])
def test_circuit_bootstrap_via_pfks_words_equal_the_composition(tuned, generic, which, log, count):
    """the library's circuit_bootstrap_pbs, numpy's extract-and-rotate, pfks_ref, the library's poly_fft"""
    eng, P = pick(tuned, generic, which)
    L = P.cbs_count
    keys = cbs_uniform_keys(which, log, count)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    load_some_bootstrap_key(eng, which)
    lwe0 = np.random.default_rng([0xD7, P.N]).integers(0, 1 << 64, (5, P.lwe_n + 1), dtype=np.uint64)
    glwe = eng.circuit_bootstrap_pbs(lwe0).reshape(5, P.k + 1, P.N)
    rows = PC.extract_and_rotate(glwe, L, P.cbs_radix_log)
    ggsw = components_ref(rows, keys, log, count)
    want = eng.poly_fft(ggsw.reshape(-1, P.N)).reshape(5, -1)
    for B in (1, 2, 5):
        got = eng.circuit_bootstrap_via_pfks(lwe0[:B])
        assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
        assert got.shape == (B, P.cbs_ggsw_fft_len)
        assert np.array_equal(got.view(np.uint64), want[:B].view(np.uint64)), (which, B)


def test_circuit_bootstrap_via_pfks_selects_in_the_cmux(tuned):
    """an oracle key set and honest PFKS keys at the reference benchmark's radix 17 bits x 2 (constant-polynomial masks: valid
    GLWE samples, built in seconds); the result selects the right operand for an encrypted 0 and an encrypted 1"""
    P, log, count = TUNED, 17, 2
    ks = keyset(0x5EED0007, P.lwe_n, with_ksk=False)
    rng = np.random.default_rng([0xD8])
    keys = PC.cbs_pfks_keys(rng, ks.glwe_sk, ks.glwe_sk, P.N, log, count, constant_mask=True)
    tuned.load_private_functional_keyswitch_keys_std(keys, log, count)
    tuned.load_bootstrap_key(ks.bsk_fft)
    bits = [0, 1, 1, 0]
    lwe0 = O.encrypt_bits_l0(77, ks, bits)
    sel = tuned.circuit_bootstrap_via_pfks(lwe0)
    assert tuned.last_private_functional_keyswitch_kernel() == "pfks_gemm_kernel<3>"
    r = O.Rng(18)
    msgs = [np.array([O.encode(int(v), 3) for v in np.random.default_rng(s).integers(0, 8, P.N)], dtype=np.uint64) for s in (1, 2)]
    d = [O.encrypt_glwe(r, ks.glwe_sk, m, P.N, P.k, P.glwe_std) for m in msgs]
    out = tuned.cmux(sel, np.stack([d[0]] * len(bits)), np.stack([d[1]] * len(bits)))
    for i, bit in enumerate(bits):
        dec = [O.decode(int(v), 3) for v in O.decrypt_glwe_raw(out[i], ks.glwe_sk, P.N, P.k)]
        assert dec == [O.decode(int(v), 3) for v in msgs[bit]], i


# ---- the stream contract of the `_enqueue` forms ----------------------------------------------------------------------------
# In the manner of tests/test_gpu_public_functional_keyswitch.py: the call runs behind a closed gate on each of four non-blocking
# streams that are alive together; until the gate opens the operands hold decoys and the output a sentinel; the words are those
# of the null-stream call.

SWEEP = 4


class StagedCall:
    def __init__(self, eng, B, p, n, seed):
        self.eng, self.B = eng, B
        self.gw = eng.params.glwe_words
        rng = np.random.default_rng([0xD9, seed, B, p, n])
        self.real, self.decoy = (rng.integers(0, 1 << 64, (B, p, n + 1), dtype=np.uint64) for _ in range(2))
        self.in_bytes, self.out_bytes = self.real.nbytes, B * self.gw * 8
        self.bufs = [eng.device_alloc(b) for b in (self.in_bytes, self.in_bytes, self.in_bytes, max(self.out_bytes, HR.MIN_READ), self.out_bytes)]
        self.src_real, self.src_decoy, self.work_in, self.work_out, self.kept = self.bufs
        eng.device_upload(self.src_real, self.real)
        eng.device_upload(self.src_decoy, self.decoy)
        HR.reserve_pinned(self.out_bytes)
        self.want = self._null_stream(self.src_real)

    def free(self):
        while self.bufs:
            self.eng.device_free(self.bufs.pop())

    def _fetch(self, ptr, shape):
        host = np.empty(shape, dtype=np.uint64)
        self.eng.device_download(None, host, ptr)
        return host

    def _null_stream(self, src):
        HR.check(HR.runtime().hipMemcpyAsync(self.work_in, src, self.in_bytes, HR.MEMCPY_DEVICE_TO_DEVICE, None), "hipMemcpyAsync")
        self.eng.private_functional_keyswitch_enqueue(None, 0, self.B, self.work_in, self.work_out)
        return self._fetch(self.work_out, (self.B, self.gw))

    def reset(self):
        """a warm call at this batch size with the decoys (nothing left to grow; the decoys give other words), then decoys in the
        input and a sentinel in the output"""
        assert not np.array_equal(self._null_stream(self.src_decoy), self.want)
        sentinel = np.full(self.B * self.gw, SENTINEL, dtype=np.uint64)
        self.eng.device_upload(self.work_out, sentinel)
        self.eng.device_upload(self.kept, sentinel)
        assert (self._fetch(self.work_out, (self.B, self.gw)) == SENTINEL).all()

    def enqueue(self, S):
        S.copy(self.work_in, self.src_real, self.in_bytes)
        self.eng.private_functional_keyswitch_enqueue(S.handle, 0, self.B, self.work_in, self.work_out)
        S.copy(self.kept, self.work_out, self.out_bytes)
        S.copy(self.work_in, self.src_decoy, self.in_bytes)

    def assert_not_started(self, reader):
        got = reader.read(self.work_out, np.empty((self.B, self.gw), dtype=np.uint64))
        assert (got == SENTINEL).all(), "the output was written while the caller's stream was held"

    def check_done(self):
        kept = self._fetch(self.kept, (self.B, self.gw))
        assert np.array_equal(kept, self.want), np.flatnonzero((kept != self.want).any(axis=1))
        assert np.array_equal(self._fetch(self.work_in, self.decoy.shape), self.decoy)


def _held(S):
    assert not any(g.capped for g in S.gates), "the call returned only after the gate's cap: it waited for the device"
    assert S.busy(), "the caller's stream is idle although its gate is closed: the case proves nothing"


def _stream_engine(tuned, generic, which, log):
    eng, P = pick(tuned, generic, which)
    n, p, count = 5, 3, 2
    keys, _ = PC.uniform_case(13, P.N, P.k, n, p, log, count, 1)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    return eng, keys, n, p, count


@pytest.mark.parametrize("which", ["tuned", "generic"])
@pytest.mark.parametrize("log", [17, 31])
def test_enqueue_only_enqueues_on_the_callers_stream(tuned, generic, which, log):
    eng, keys, n, p, count = _stream_engine(tuned, generic, which, log)
    st = StagedCall(eng, 3, p, n, 500)
    try:
        assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
        assert np.array_equal(st.want, ref_batch(st.real, keys[0], log, count))
        with HR.streams(SWEEP + 1) as (reader, *callers):
            for S in callers:
                st.reset()
                S.gate()
                st.enqueue(S)
                _held(S)
                st.assert_not_started(reader)
                _held(S)
                S.release()
                st.check_done()
    finally:
        st.free()


@pytest.mark.parametrize("which", ["tuned", "generic"])
def test_two_enqueues_back_to_back_share_the_contexts_scratch_in_stream_order(tuned, generic, which):
    """both read the context's limb scratch; the second call is the larger batch (two row tiles against one), the one the scratch
    had to grow for"""
    eng, keys, n, p, count = _stream_engine(tuned, generic, which, 17)
    calls = []
    try:
        calls = [StagedCall(eng, 2, p, n, 600), StagedCall(eng, TILE + 2, p, n, 700)]
        for st in calls:
            assert np.array_equal(st.want, ref_batch(st.real, keys[0], 17, count))
        with HR.streams(SWEEP + 1) as (reader, *callers):
            for S in callers:
                for st in reversed(calls):
                    st.reset()
                S.gate()
                for st in calls:
                    st.enqueue(S)
                _held(S)
                for st in calls:
                    st.assert_not_started(reader)
                _held(S)
                S.release()
                for st in calls:
                    st.check_done()
    finally:
        for st in calls:
            st.free()


# ---- statuses, reload, group ------------------------------------------------------------------------------------------------

def test_statuses_with_a_device_and_reload():
    P = GENERIC
    eng = spf_amd.Engine(to_engine_params(P))
    try:
        lib, h = eng._lib, eng._h
        x = np.zeros((4, 1, 4), dtype=np.uint64)
        out = np.zeros(P.cbs_ggsw_fft_len * 2, dtype=np.uint64)
        xp, op = x.ctypes.data, out.ctypes.data
        assert lib.spf_private_functional_keyswitch_batch(h, 0, 1, xp, op) == NO_KEY          # before a load
        assert lib.spf_private_functional_keyswitch_enqueue(h, None, 0, 1, xp, op) == NO_KEY
        assert lib.spf_apply_pfks_on_ggsw_components_batch(h, 1, xp, op) == NO_KEY
        assert lib.spf_circuit_bootstrap_via_pfks_batch(h, 1, xp, op) == NO_KEY
        assert lib.spf_private_functional_keyswitch_batch(h, 0, 1, None, op) == INVALID
        with pytest.raises(spf_amd.SpfError) as no_shape:                                     # no shape yet
            eng.key_blob(5)
        assert no_shape.value.status == NO_KEY
        keys, lwes = PC.uniform_case(14, P.N, P.k, 3, 1, 17, 2, 2, 2)
        eng.load_private_functional_keyswitch_keys_std(keys, 17, 2)
        assert np.array_equal(eng.private_functional_keyswitch(lwes, 1), ref_batch(lwes, keys[1], 17, 2))
        assert lib.spf_private_functional_keyswitch_batch(h, 2, 1, xp, op) == INVALID         # key_index = n_keys
        assert lib.spf_private_functional_keyswitch_enqueue(h, None, 2, 1, xp, op) == INVALID
        assert lib.spf_private_functional_keyswitch_batch(h, 0, 0, xp, op) == 0               # B = 0
        assert lib.spf_private_functional_keyswitch_batch(h, 0, 1 << 40, xp, op) == INVALID
        assert lib.spf_apply_pfks_on_ggsw_components_batch(h, 1, xp, op) == INVALID           # a key set of the wrong shape
        assert lib.spf_apply_pfks_on_ggsw_components_enqueue(h, None, 1, xp, op) == INVALID
        assert lib.spf_circuit_bootstrap_via_pfks_batch(h, 1, xp, op) == INVALID
        d = eng.device_alloc(1 << 16)
        try:                                                                                  # overlapping ranges
            assert lib.spf_private_functional_keyswitch_enqueue(h, None, 0, 2, d, d + 8) == INVALID
        finally:
            eng.device_free(d)
        flat = keys.reshape(-1)
        for n_words, n_keys, n, p, log, count in [(flat.size - 1, 2, 3, 1, 17, 2), (flat.size, 2, 3, 1, 32, 2), (flat.size, 2, 3, 1, 0, 2),
                                                  (flat.size, 0, 3, 1, 17, 2), (flat.size, 2, 0, 1, 17, 2), (flat.size, 2, 3, 0, 17, 2),
                                                  (flat.size, 2, 3, 1, 64, 1), (flat.size, 2, 3, 1, 17, 0)]:
            assert lib.spf_load_private_functional_keyswitch_keys_std(h, flat.ctypes.data, n_words, n_keys, n, p, log, count) == INVALID
            assert lib.spf_private_functional_keyswitch_batch(h, 0, 1, xp, op) == NO_KEY      # after a failed load
        # a reload at another radix and shape is honoured by the next call, on each side of the dispatcher
        for log, count, n, p in [(31, 2, 2, 3), (8, 3, 4, 1)]:
            keys2, lwes2 = PC.uniform_case(15, P.N, P.k, n, p, log, count, 2)
            eng.load_private_functional_keyswitch_keys_std(keys2, log, count)
            assert np.array_equal(eng.private_functional_keyswitch(lwes2), ref_batch(lwes2, keys2[0], log, count))
            assert eng.last_private_functional_keyswitch_kernel() == kernel_name(log)
            blob, nbytes = eng.key_blob(5)
            assert blob and nbytes == keys2.nbytes
    finally:
        eng.close()


@pytest.mark.parametrize("which", ["tuned", "generic"])
def test_group_over_one_device_twice_is_word_equal_to_one_context(tuned, generic, which):
    eng, P = pick(tuned, generic, which)
    log, count, n, p, B = 17, 2, 5, 3, 5
    keys, lwes = PC.uniform_case(16, P.N, P.k, n, p, log, count, B, 2)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    want = eng.private_functional_keyswitch(lwes, 1)
    assert np.array_equal(want, ref_batch(lwes, keys[1], log, count))
    grp = spf_amd.Group(to_engine_params(P), devices=[0, 0])
    try:
        with pytest.raises(spf_amd.SpfError):
            grp.private_functional_keyswitch(lwes, 1)                                          # no key yet
        grp.load_private_functional_keyswitch_keys_std(keys, log, count)
        got = grp.private_functional_keyswitch(lwes, 1)                                        # ragged: 3 + 2
        assert np.array_equal(got, want)
        with pytest.raises(spf_amd.SpfError):
            grp.private_functional_keyswitch(lwes, 2)                                          # key_index = n_keys
    finally:
        grp.close()


def test_group_circuit_bootstrap_via_pfks_is_word_equal_to_one_context(generic):
    P, log, count, B = GENERIC, 17, 2, 5
    keys = cbs_uniform_keys("generic", log, count)
    generic.load_private_functional_keyswitch_keys_std(keys, log, count)
    load_some_bootstrap_key(generic, "generic")
    lwe0 = np.random.default_rng([0xDB]).integers(0, 1 << 64, (B, P.lwe_n + 1), dtype=np.uint64)
    want = generic.circuit_bootstrap_via_pfks(lwe0)
    grp = spf_amd.Group(to_engine_params(P), devices=[0, 0])
    try:
        grp.load_private_functional_keyswitch_keys_std(keys, log, count)
        load_some_bootstrap_key(grp, "generic")
        got = grp.circuit_bootstrap_via_pfks(lwe0)                                             # ragged: 3 + 2
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    finally:
        grp.close()
