"""The public functional keyswitch (`public_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/public_functional_keyswitch.rs:
74-148, message j to coefficient j) on the GPU.  Every output word equals tests/pufks_cases.py's `pufks_oracle`, the composition
of the oracle's glwe_ggsw_mad and poly_ifft: no tolerance.  The exact-arithmetic conditions are asserted on the GPU's own words as
well, so the test still means something on the day the oracle and the kernel are wrong together."""
import functools

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import hip_runtime as HR
from tests import poly_ref as R
from tests import pufks_cases as PC
from tests.polyref_cases import N128K2, NOISE, check_tier_a, key_fft
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu
TUNED = O.DEFAULT_128.replace(lwe_n=1)
GENERIC = N128K2
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
NO_KEY = 3


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


@functools.lru_cache(maxsize=None)
def uniform_key(N, k, n, count, seed=0):
    """(time-domain words (n, count, k+1, N), the oracle's spectra of them)"""
    key = np.random.default_rng([0xC0, N, k, n, count, seed]).integers(0, 1 << 64, (n, count, k + 1, N), dtype=np.uint64)
    return key, key_fft(key)


def uniform_lwes(seed, B, p, n):
    return np.random.default_rng([0xC1, seed, B, p, n]).integers(0, 1 << 64, (B, p, n + 1), dtype=np.uint64)


def oracle_batch(lwes, keyf, P, log, count):
    return np.stack([PC.pufks_oracle(x, keyf, P.N, P.k, log, count).reshape(-1) for x in lwes])


def tuned_name(count, G):
    """G outputs per workgroup; G = 1: the four-waves-per-output latency shape"""
    return f"pufks4_kernel<4,{count}>" if G == 1 else f"pufks_kernel<4,{count},{G}>"


# ---- bit equality -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 64])
@pytest.mark.parametrize("count", [8, 4])
def test_tuned_kernel_words_are_the_oracles(tuned, shape_boundaries, count, n):
    key, keyf = uniform_key(TUNED.N, TUNED.k, n, count)
    tuned.load_public_functional_keyswitch_key_std(key, 4, count)
    for p in (1, 3, 65, 2048):
        lwes = uniform_lwes(count, 3, p, n)
        before = lwes.copy()
        want = oracle_batch(lwes, keyf, TUNED, 4, count)
        got = tuned.public_functional_keyswitch(lwes)
        assert tuned.last_public_functional_keyswitch_kernel() == tuned_name(count, 1)
        assert np.array_equal(lwes, before)
        assert np.array_equal(got, want), (count, n, p, "B=3", np.flatnonzero((got != want).any(axis=1)))
        one = tuned.public_functional_keyswitch(lwes[:1])
        assert np.array_equal(one, want[:1]), (count, n, p, "B=1")
        if n <= 5 or p == 65:   # the same items through the two-outputs-per-workgroup shape (inputs of at most 35 MB)
            which = np.arange(shape_boundaries[2]) % 3
            got = tuned.public_functional_keyswitch(lwes[which])
            assert tuned.last_public_functional_keyswitch_kernel() == tuned_name(count, 2)
            assert np.array_equal(got, want[which]), (count, n, p, "two outputs per workgroup")


@pytest.fixture(scope="module")
def shape_boundaries(tuned):
    """the smallest batch that reaches each shape, found from the kernel name the library REPORTS"""
    key, _ = uniform_key(TUNED.N, TUNED.k, 1, 4)
    tuned.load_public_functional_keyswitch_key_std(key, 4, 4)
    cap = 4096
    d_in, d_out = tuned.device_alloc(cap * 2 * 8), tuned.device_alloc(cap * TUNED.glwe_len * 8)
    names = [tuned_name(4, 1), tuned_name(4, 2), tuned_name(4, 4)]
    try:
        tuned.device_upload(d_in, np.zeros(cap * 2, dtype=np.uint64))

        def shape(B):
            tuned.public_functional_keyswitch_enqueue(None, B, 1, d_in, d_out)
            return names.index(tuned.last_public_functional_keyswitch_kernel())

        def first(at_least, lo, hi):   # smallest B in (lo, hi] with shape(B) >= at_least; false at lo, true at hi
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if shape(mid) >= at_least else (mid, hi)
            return hi

        assert shape(1) == 0 and shape(cap) == 2
        found = {2: first(1, 1, cap), 4: first(2, 1, cap)}
        tuned.device_download(None, np.empty(1, dtype=np.uint64), d_out)   # (waits for the probes)
    finally:
        tuned.device_free(d_in)
        tuned.device_free(d_out)
    assert 1 < found[2] < found[4] < cap
    print(f"smallest batch per outputs-per-workgroup shape: {found}")
    return found


PER_LAUNCH = 4096   # include/spf_hip.h: a launch holds at most 4096 outputs
SIDES = ["last_of_latency", "first_of_two", "last_of_two", "first_of_four", "one_launch", "two_launches"]


@pytest.mark.parametrize("count", [8, 4])
@pytest.mark.parametrize("side", SIDES)
def test_both_sides_of_every_dispatcher_boundary(tuned, shape_boundaries, count, side):
    """outputs per workgroup (four waves per output -> 2 -> 4) and grid shape (one launch -> two); the batch repeats seven
    distinct items, so a ragged last workgroup and a second launch both hold real work"""
    b2, b4 = shape_boundaries[2], shape_boundaries[4]
    B, G = {"last_of_latency": (b2 - 1, 1), "first_of_two": (b2, 2), "last_of_two": (b4 - 1, 2), "first_of_four": (b4, 4),
            "one_launch": (PER_LAUNCH, 4), "two_launches": (PER_LAUNCH + 1, 4)}[side]
    n, p = 5, 65
    key, keyf = uniform_key(TUNED.N, TUNED.k, n, count)
    tuned.load_public_functional_keyswitch_key_std(key, 4, count)
    items = uniform_lwes(70 + count, 7, p, n)
    want = oracle_batch(items, keyf, TUNED, 4, count)
    which = np.arange(B) % 7
    got = tuned.public_functional_keyswitch(items[which])
    assert tuned.last_public_functional_keyswitch_kernel() == tuned_name(count, G)
    bad = np.flatnonzero((got != want[which]).any(axis=1))
    assert bad.size == 0, (side, B, bad[:8])


@pytest.mark.parametrize("n", [1, 7, 16])
def test_generic_kernel_words_are_the_oracles(generic, n):
    P, log, count = GENERIC, 4, 3
    key, keyf = uniform_key(P.N, P.k, n, count)
    generic.load_public_functional_keyswitch_key_std(key, log, count)
    for p in (1, 5, 128):
        lwes = uniform_lwes(3, 5, p, n)
        want = oracle_batch(lwes, keyf, P, log, count)
        got = generic.public_functional_keyswitch(lwes)
        assert generic.last_public_functional_keyswitch_kernel() == "generic_pufks_kernel"
        assert np.array_equal(got, want), (n, p, "B=5")
        assert np.array_equal(generic.public_functional_keyswitch(lwes[:1]), want[:1]), (n, p, "B=1")


def test_tuned_context_at_another_radix_runs_the_generic_kernel(tuned):
    log, count, n, p = 7, 6, 3, 5
    key, keyf = uniform_key(TUNED.N, TUNED.k, n, count)
    tuned.load_public_functional_keyswitch_key_std(key, log, count)
    lwes = uniform_lwes(67, 2, p, n)
    got = tuned.public_functional_keyswitch(lwes)
    assert tuned.last_public_functional_keyswitch_kernel() == "generic_pufks_kernel"
    assert np.array_equal(got, oracle_batch(lwes, keyf, TUNED, log, count))


def test_full_size_call(tuned):
    """n = 2048, 4 x 4 bits, p = 1024, B = 2 with distinct inputs: a uniform key of 268 MB"""
    n, count, p = 2048, 4, 1024
    key, keyf = uniform_key(TUNED.N, TUNED.k, n, count)
    tuned.load_public_functional_keyswitch_key_std(key, 4, count)
    lwes = uniform_lwes(2048, 2, p, n)
    got = tuned.public_functional_keyswitch(lwes)
    assert tuned.last_public_functional_keyswitch_kernel() == tuned_name(count, 1)
    assert np.array_equal(got, oracle_batch(lwes, keyf, TUNED, 4, count))
    uniform_key.cache_clear()


# ---- exact arithmetic from the GPU's own output -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", PC.TIER_A, ids=PC.tier_a_name)
def test_gpu_words_against_exact_arithmetic(tuned, generic, shape):
    N, k, n, count, log, p, _ = shape
    eng = tuned if N == 2048 else generic
    assert (eng.params.polynomial_degree, eng.params.glwe_size) == (N, k)
    c, lwes, exact, nump = PC.tier_a_case(shape)
    eng.load_public_functional_keyswitch_key_std(c.key, log, count)
    got = eng.public_functional_keyswitch(lwes[None]).reshape(k + 1, N)
    check_tier_a(c, [got], [exact], [nump], "gpu")
    assert np.array_equal(got, PC.pufks_oracle(lwes, key_fft(c.key), N, k, log, count))


# ---- placement and independence ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["tuned", "generic"])
def test_an_output_depends_on_its_own_inputs_only_and_nothing_else_is_written(tuned, generic, which):
    eng, P, log, count = (tuned, TUNED, 4, 8) if which == "tuned" else (generic, GENERIC, 4, 3)
    n, p, B = 5, 65, 5
    key, keyf = uniform_key(P.N, P.k, n, count)
    eng.load_public_functional_keyswitch_key_std(key, log, count)
    item = uniform_lwes(900, 1, p, n)[0]
    want = PC.pufks_oracle(item, keyf, P.N, P.k, log, count).reshape(-1)
    gw, guard = P.glwe_len, 2
    d_in, d_out = eng.device_alloc(B * p * (n + 1) * 8), eng.device_alloc((B + guard) * gw * 8)
    try:
        for pos in (0, 1, B - 1):
            lwes = uniform_lwes(901 + pos, B, p, n)          # other neighbours every time
            lwes[pos] = item
            eng.device_upload(d_in, lwes)
            eng.device_upload(d_out, np.full((B + guard) * gw, SENTINEL, dtype=np.uint64))
            eng.public_functional_keyswitch_enqueue(None, B, p, d_in, d_out)
            got = np.empty((B + guard, gw), dtype=np.uint64)
            eng.device_download(None, got, d_out)
            assert np.array_equal(got[pos], want), (which, pos)
            assert (got[B:] == SENTINEL).all(), (which, pos, "words beyond the B outputs were written")
            assert not (got[:B] == SENTINEL).all(axis=1).any()
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)


# ---- meaning ----------------------------------------------------------------------------------------------------------------

def test_honest_key_on_the_gpu_meets_the_derived_bound(tuned):
    shape = PC.MEANING[1]
    N, k, n, count, log = shape
    assert (N, k) == (TUNED.N, TUNED.k)
    lwe_sk, glwe_sk, key = PC.meaning_keys(shape)
    tuned.load_public_functional_keyswitch_key_std(key, log, count)
    for p in (1, 33, N):
        lwes = PC.meaning_lwes(shape, p)
        got = tuned.public_functional_keyswitch(lwes[None]).reshape(k + 1, N)
        assert tuned.last_public_functional_keyswitch_kernel() == tuned_name(count, 1)
        PC.check_meaning(got, lwes, lwe_sk, glwe_sk, count, log, "gpu")


def test_round_trip_unpack_then_public_functional_keyswitch(generic):
    """glwe_unpack_l1 of a packed GLWE, then this call with an honest key from the GLWE key (as the LWE key of the sample
    extracts, n = k N = 256) back to itself: the packed bits again"""
    P, log, count, n_bits = GENERIC, 4, 3, 37
    n = P.k * P.N
    rng = np.random.default_rng([0xC2, P.N, P.k])
    glwe_sk = R.binary_key(rng, n)
    key = PC.honest_key(rng, glwe_sk, glwe_sk, P.N, log, count)
    generic.load_public_functional_keyswitch_key_std(key, log, count)
    bits = rng.integers(0, 2, (2, n_bits), dtype=np.uint64)
    msgs = np.zeros((2, P.N), dtype=np.uint64)
    msgs[:, :n_bits] = bits << np.uint64(63)
    packed = R.glwe_encrypt(rng, glwe_sk, msgs, NOISE).reshape(2, -1)
    lwes = generic.glwe_unpack_l1(packed, n_bits).reshape(2, n_bits, n + 1)
    out = generic.public_functional_keyswitch(lwes).reshape(2, P.k + 1, P.N)
    assert generic.last_public_functional_keyswitch_kernel() == "generic_pufks_kernel"
    ph = R.glwe_phase(out, glwe_sk)
    decoded = ((ph + np.uint64(1 << 62)) >> np.uint64(63)).astype(np.uint64)
    assert np.array_equal(decoded[:, :n_bits], bits)
    assert not decoded[:, n_bits:].any()
    assert float(R.torus_distance(ph, msgs).max()) <= PC.meaning_bounds(n, count, log, n_bits)[0] + 2.0 ** -40


# ---- the stream contract of the `_enqueue` form -----------------------------------------------------------------------------
# In the manner of test (a) of tests/test_gpu_stream_contract.py: the call runs behind a closed gate on each of four non-blocking
# streams that are alive together; until the gate opens the operands hold decoys and the output a sentinel; the words are those
# of the null-stream call.

SWEEP = 4


class StagedCall:
    def __init__(self, eng, B, p, n, seed):
        self.eng, self.B, self.p = eng, B, p
        self.gw = eng.params.glwe_words
        self.real, self.decoy = uniform_lwes(seed, B, p, n), uniform_lwes(seed + 1, B, p, n)
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
        self.eng.public_functional_keyswitch_enqueue(None, self.B, self.p, self.work_in, self.work_out)
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
        self.eng.public_functional_keyswitch_enqueue(S.handle, self.B, self.p, self.work_in, self.work_out)
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


def _stream_engine(tuned, generic, which):
    eng, P, log, count = (tuned, TUNED, 4, 4) if which == "tuned" else (generic, GENERIC, 4, 3)
    n = 5
    key, _ = uniform_key(P.N, P.k, n, count)
    eng.load_public_functional_keyswitch_key_std(key, log, count)
    return eng, n, (tuned_name(count, 1) if which == "tuned" else "generic_pufks_kernel")


@pytest.mark.parametrize("which", ["tuned", "generic"])
def test_enqueue_only_enqueues_on_the_callers_stream(tuned, generic, which):
    eng, n, kernel = _stream_engine(tuned, generic, which)
    st = StagedCall(eng, 3, 33, n, 500)
    try:
        assert eng.last_public_functional_keyswitch_kernel() == kernel
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
    """B grows from the first call to the second; both read the context's digit scratch (the tuned kernel's pre-pass)"""
    eng, n, _ = _stream_engine(tuned, generic, which)
    calls = []
    try:
        calls = [StagedCall(eng, 2, 33, n, 600), StagedCall(eng, 6, 65, n, 700)]
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
    eng = spf_amd.Engine(to_engine_params(TUNED))
    try:
        lib, h = eng._lib, eng._h
        x = np.zeros((1, 1, 4), dtype=np.uint64)
        out = np.zeros(TUNED.glwe_len, dtype=np.uint64)
        xp, op = x.ctypes.data, out.ctypes.data
        assert lib.spf_public_functional_keyswitch_batch(h, 1, 1, xp, op) == NO_KEY       # before a load
        assert lib.spf_public_functional_keyswitch_enqueue(h, None, 1, 1, xp, op) == NO_KEY
        assert lib.spf_public_functional_keyswitch_batch(h, 1, 0, xp, op) == 1
        assert lib.spf_public_functional_keyswitch_batch(h, 1, TUNED.N + 1, xp, op) == 1
        assert lib.spf_public_functional_keyswitch_batch(h, 1 << 40, 2, xp, op) == 1
        assert lib.spf_public_functional_keyswitch_batch(h, 1, 1, None, op) == 1
        with pytest.raises(spf_amd.SpfError) as no_shape:                                 # no shape yet
            eng.key_blob(4)
        assert no_shape.value.status == NO_KEY
        key, keyf = uniform_key(TUNED.N, TUNED.k, 3, 4)
        eng.load_public_functional_keyswitch_key_std(key, 4, 4)
        lwes = uniform_lwes(800, 2, 3, 3)
        assert np.array_equal(eng.public_functional_keyswitch(lwes), oracle_batch(lwes, keyf, TUNED, 4, 4))
        assert lib.spf_public_functional_keyswitch_batch(h, 0, 1, xp, op) == 0            # B = 0
        flat = key.reshape(-1)
        for n_words, n, log, count in [(flat.size - 1, 3, 4, 4), (flat.size, 3, 16, 4), (flat.size, 0, 4, 4), (flat.size, 3, 0, 4)]:
            assert lib.spf_load_public_functional_keyswitch_key_std(h, flat.ctypes.data, n_words, n, log, count) == 1
            assert lib.spf_public_functional_keyswitch_batch(h, 1, 1, xp, op) == NO_KEY   # after a failed load
        # a reload with another from_dimension and radix is honoured by the next call
        key2, keyf2 = uniform_key(TUNED.N, TUNED.k, 2, 8)
        eng.load_public_functional_keyswitch_key_std(key2, 4, 8)
        lwes2 = uniform_lwes(801, 2, 3, 2)
        assert np.array_equal(eng.public_functional_keyswitch(lwes2), oracle_batch(lwes2, keyf2, TUNED, 4, 8))
        assert eng.last_public_functional_keyswitch_kernel() == tuned_name(8, 1)
        blob, nbytes = eng.key_blob(4)
        assert blob and nbytes == key2.nbytes
    finally:
        eng.close()


@pytest.mark.parametrize("which", ["tuned", "generic"])
def test_group_over_one_device_twice_is_word_equal_to_one_context(tuned, generic, which):
    eng, P, log, count = (tuned, TUNED, 4, 4) if which == "tuned" else (generic, GENERIC, 4, 3)
    n, p, B = 5, 33, 5
    key, _ = uniform_key(P.N, P.k, n, count)
    eng.load_public_functional_keyswitch_key_std(key, log, count)
    lwes = uniform_lwes(950, B, p, n)
    want = eng.public_functional_keyswitch(lwes)
    grp = spf_amd.Group(to_engine_params(P), devices=[0, 0])
    try:
        with pytest.raises(spf_amd.SpfError):
            grp.public_functional_keyswitch(lwes)                                          # no key yet
        grp.load_public_functional_keyswitch_key_std(key, log, count)
        got = grp.public_functional_keyswitch(lwes)                                        # ragged: 3 + 2
        assert np.array_equal(got, want)
    finally:
        grp.close()
