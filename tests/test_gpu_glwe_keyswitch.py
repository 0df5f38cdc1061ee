"""GLWE keyswitch, one automorphism round and the homomorphic trace on the GPU (`keyswitch_glwe_to_glwe`, sunscreen_tfhe
ops/fft_ops.rs:457-495; `polynomial_pow_k`, ops/polynomial/mod.rs:62-84; `trace`, ops/automorphisms/mod.rs:53-85): every output
word of every item equals the oracle's (tests/glwe_keyswitch_cases.py).  There is no tolerance in this file; the two decryption
checks use the reference's decode at 12 plaintext bits."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import glwe_keyswitch_cases as KC
from tests import hip_runtime as HR
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu
U = np.uint64
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
INVALID, NO_KEY = 1, 3
SHAPES = list(KC.SHAPES)
TUNED = "default128_6x7"
HAND_WRITTEN, GENERIC = "glwe_ks_kernel", "generic_glwe_ks_kernel"
BATCHES = (1, 4, 5)      # one unit of a workgroup of four, a full workgroup, a ragged workgroup past the first
A2B_SLOT, AK_SLOT = 3, 15


def kernel_of(shape):
    return HAND_WRITTEN if shape == TUNED else GENERIC


def engine_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count, ss_radix_log=P.ss_radix_log,
                                       ss_radix_count=P.ss_count)


@pytest.fixture(scope="module")
def engines():
    """one context per shape, made when a test first asks for it: the automorphism key loaded in integer form, the a -> b key in
    slot A2B_SLOT, round 2's slice of the automorphism key in slot AK_SLOT"""
    made = {}

    def get(shape):
        if shape not in made:
            c = KC.case(shape)
            eng = spf_amd.Engine(engine_params(c.P))
            eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
            eng.load_glwe_keyswitch_key_std(A2B_SLOT, c.ksk, c.P.tr_radix_log, c.P.tr_count)
            eng.load_glwe_keyswitch_key_std(AK_SLOT, np.ascontiguousarray(c.hk.ak[1]), c.P.tr_radix_log, c.P.tr_count)
            made[shape] = eng
        return made[shape]
    yield get
    for e in made.values():
        e.close()


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:8])


# ---- trace ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_trace_equals_the_oracle(engines, shape, B):
    c, eng = KC.case(shape), engines(shape)
    got = eng.glwe_trace(c.x[:B])
    assert eng.last_glwe_keyswitch_kernel() == kernel_of(shape)
    assert_words(got, KC.oracle_traces(shape)[:B], (shape, B))


def test_the_fused_circuit_bootstrap_trace_equals_the_trace_of_its_host_made_levels(engines):
    """spf_mod_switch_trace_and_rotate_batch = un-rotate, X^-level, shr_round (here in exact integers on the host), then the trace:
    the new kernel against the shipped one"""
    c, eng = KC.case(TUNED), engines(TUNED)
    P = c.P
    fused = eng.mod_switch_trace_and_rotate(c.x.reshape(KC.ITEMS, -1)).reshape(KC.ITEMS * P.cbs_count, P.k + 1, P.N)
    levels = np.concatenate([KC.cbs_levels(P, g) for g in c.x])
    got = eng.glwe_trace(levels)
    assert eng.last_glwe_keyswitch_kernel() == HAND_WRITTEN
    assert_words(got, fused, "fused")


@pytest.mark.parametrize("shape", SHAPES)
def test_can_trace_on_the_gpu(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    KC.check_can_trace(c, eng.glwe_trace(KC.all_ones_glwe(c)[None])[0], "gpu")


# ---- one automorphism round ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_every_round_equals_pow_k_then_the_keyswitch_of_the_oracle(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    last = KC.log2n(c.P)
    for rnd in range(1, last + 1):
        got = eng.glwe_automorphism(rnd, c.x[2:3])
        assert eng.last_glwe_keyswitch_kernel() == kernel_of(shape)
        assert_words(got[0], KC.oracle_round(c, c.x[2], rnd), (shape, rnd))
    for rnd in (1, last):
        assert_words(eng.glwe_automorphism(rnd, c.x), KC.oracle_round(c, c.x, rnd), (shape, rnd, "B=5"))


@pytest.mark.parametrize("shape", SHAPES)
def test_folding_the_gpus_rounds_with_a_host_add_is_the_gpus_trace(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    x = c.x.copy()
    for rnd in range(1, KC.log2n(c.P) + 1):
        x = x + eng.glwe_automorphism(rnd, x)
    assert_words(x, eng.glwe_trace(c.x), shape)


# ---- keyswitch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_keyswitch_equals_the_oracle_in_two_slots(engines, shape, B):
    c, eng = KC.case(shape), engines(shape)
    got = eng.glwe_keyswitch(A2B_SLOT, c.x[:B])
    assert eng.last_glwe_keyswitch_kernel() == kernel_of(shape)
    want = KC.oracle_keyswitch(c.P, c.x[:B], c.ksk_fft)
    assert_words(got, want, (shape, B, "a->b"))
    KC.check_switched_phase(c, c.x[:B], got, "gpu")
    other = eng.glwe_keyswitch(AK_SLOT, c.x[:B])
    assert_words(other, KC.oracle_keyswitch(c.P, c.x[:B], c.ak_fft[1]), (shape, B, "ak[1]"))
    assert not np.array_equal(other, got), "two slots share storage"
    assert_words(eng.glwe_keyswitch(A2B_SLOT, c.x[:B]), want, (shape, B, "a->b again"))
    assert eng.glwe_keyswitch_slot_shape(A2B_SLOT) == (c.P.tr_radix_log, c.P.tr_count)


@pytest.mark.parametrize("shape", [TUNED, "N16"])
def test_a_reload_replaces_the_key_of_the_slot(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    words, fft = KC.second_key(c)
    eng.load_glwe_keyswitch_key_std(7, c.ksk, c.P.tr_radix_log, c.P.tr_count)
    first = eng.glwe_keyswitch(7, c.x)
    assert_words(first, KC.oracle_keyswitch(c.P, c.x, c.ksk_fft), (shape, "first"))
    eng.load_glwe_keyswitch_key_std(7, words, c.P.tr_radix_log, c.P.tr_count)
    second = eng.glwe_keyswitch(7, c.x)
    assert_words(second, KC.oracle_keyswitch(c.P, c.x, fft), (shape, "reloaded"))
    assert not np.array_equal(first, second)
    assert_words(eng.glwe_keyswitch(A2B_SLOT, c.x), first, (shape, "the other slot is untouched"))


def test_another_radix_on_a_tuned_context_runs_the_generic_kernel(engines):
    c, eng = KC.case(TUNED), engines(TUNED)
    words, fft = KC.other_radix_key(c)
    lg, cnt = KC.OTHER_RADIX
    eng.load_glwe_keyswitch_key_std(9, words, lg, cnt)
    assert eng.glwe_keyswitch_slot_shape(9) == (lg, cnt)
    for B in BATCHES:
        got = eng.glwe_keyswitch(9, c.x[:B])
        assert eng.last_glwe_keyswitch_kernel() == GENERIC
        assert_words(got, KC.oracle_keyswitch(c.P, c.x[:B], fft, KC.OTHER_RADIX), ("4x8", B))
    KC.check_switched_phase(c, c.x, eng.glwe_keyswitch(9, c.x), "gpu4x8")
    assert_words(eng.glwe_keyswitch(A2B_SLOT, c.x[:1]), KC.oracle_keyswitch(c.P, c.x[:1], c.ksk_fft), "6x7 after 4x8")
    assert eng.last_glwe_keyswitch_kernel() == HAND_WRITTEN


# ---- the device-pointer forms -------------------------------------------------------------------------------------------------

class DeviceRows:
    """B GLWEs in a device buffer with `guard` sentinel rows before and after"""

    def __init__(self, eng, W, B, guard=2):
        self.eng, self.W, self.B, self.guard = eng, W, B, guard
        self.base = eng.device_alloc((B + 2 * guard) * W * 8)
        self.ptr = self.base + guard * W * 8
        self.fill()

    def fill(self, rows=None):
        host = np.full((self.B + 2 * self.guard, self.W), SENTINEL, dtype=U)
        if rows is not None:
            host[self.guard:self.guard + self.B] = np.asarray(rows).reshape(self.B, self.W)
        self.eng.device_upload(self.base, host)

    def fetch(self, stream=None):
        host = np.empty((self.B + 2 * self.guard, self.W), dtype=U)
        self.eng.device_download(stream, host, self.base)
        assert (host[:self.guard] == SENTINEL).all() and (host[self.guard + self.B:] == SENTINEL).all(), "words around the rows were written"
        return host[self.guard:self.guard + self.B]

    def free(self):
        self.eng.device_free(self.base)


def _calls(c, eng):
    """(name, enqueue(stream, B, d_in, d_out), expected words of the five items)"""
    return [("trace", lambda s, B, i, o: eng.glwe_trace_enqueue(s, B, i, o), KC.oracle_traces(c.name)),
            ("automorphism", lambda s, B, i, o: eng.glwe_automorphism_enqueue(s, 2, B, i, o), KC.oracle_round(c, c.x, 2)),
            ("keyswitch", lambda s, B, i, o: eng.glwe_keyswitch_enqueue(s, A2B_SLOT, B, i, o), KC.oracle_keyswitch(c.P, c.x, c.ksk_fft))]


@pytest.mark.parametrize("shape", SHAPES)
def test_enqueue_writes_its_rows_only_and_runs_in_place(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    W, B = (c.P.k + 1) * c.P.N, KC.ITEMS
    src, dst = DeviceRows(eng, W, B), DeviceRows(eng, W, B)
    try:
        for name, call, want in _calls(c, eng):
            src.fill(c.x)
            dst.fill()
            call(None, 0, src.ptr, dst.ptr)                      # B = 0 is legal and writes nothing
            assert (dst.fetch() == SENTINEL).all(), name
            call(None, B, src.ptr, dst.ptr)
            assert eng.last_glwe_keyswitch_kernel() == kernel_of(shape)
            assert_words(dst.fetch().reshape(want.shape), want, (shape, name))
            assert_words(src.fetch().reshape(c.x.shape), c.x, (shape, name, "the input was written"))
            call(None, B, src.ptr, src.ptr)                      # out == in exactly
            assert_words(src.fetch().reshape(want.shape), want, (shape, name, "in place"))
            # any other overlap is refused before anything is queued
            dst.fill()
            with pytest.raises(spf_amd.SpfError) as e:
                call(None, B, src.ptr, src.ptr + 8)
            assert e.value.status == INVALID and "overlap" in str(e.value)
            with pytest.raises(spf_amd.SpfError):
                call(None, B, dst.ptr + W * 8, dst.ptr)
            assert (dst.fetch() == SENTINEL).all(), name
    finally:
        src.free()
        dst.free()


@pytest.mark.parametrize("shape", [TUNED, "N256k3_7x5"])
def test_two_enqueues_back_to_back_on_one_stream_are_both_right(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    W = (c.P.k + 1) * c.P.N
    a_in, a_out, b_in, b_out = DeviceRows(eng, W, 5), DeviceRows(eng, W, 5), DeviceRows(eng, W, 3), DeviceRows(eng, W, 3)
    try:
        a_in.fill(c.x)
        b_in.fill(c.x[::-1][:3])
        with HR.streams(1) as (S,):
            eng.glwe_trace_enqueue(S.handle, 5, a_in.ptr, a_out.ptr)
            eng.glwe_keyswitch_enqueue(S.handle, A2B_SLOT, 3, b_in.ptr, b_out.ptr)
            eng.glwe_automorphism_enqueue(S.handle, 1, 3, b_out.ptr, b_out.ptr)     # reads what the call before it wrote
            S.synchronize()
        assert_words(a_out.fetch().reshape(c.x.shape), KC.oracle_traces(shape), (shape, "first"))
        switched = KC.oracle_keyswitch(c.P, c.x[::-1][:3], c.ksk_fft)
        assert_words(b_out.fetch().reshape(switched.shape), KC.oracle_round(c, switched, 1), (shape, "second and third"))
    finally:
        for r in (a_in, a_out, b_in, b_out):
            r.free()


@pytest.mark.parametrize("shape", [TUNED, "N16"])
def test_enqueue_only_enqueues_on_the_callers_stream(engines, shape):
    """in the manner of tests/test_gpu_glwe_poly_linear.py: behind a closed gate on the caller's stream the three calls return at
    once, the stream stays busy and the output keeps its sentinel; once the gate opens the words are the oracle's"""
    c, eng = KC.case(shape), engines(shape)
    W, B = (c.P.k + 1) * c.P.N, KC.ITEMS
    nbytes = max(B * W * 8, HR.MIN_READ)            # read while the gate is closed: at least MIN_READ bytes
    rows = nbytes // 8
    src, outs = eng.device_alloc(B * W * 8), [eng.device_alloc(nbytes) for _ in range(3)]
    HR.reserve_pinned(nbytes)
    try:
        eng.device_upload(src, c.x)
        for o in outs:
            eng.device_upload(o, np.full(rows, SENTINEL, dtype=U))
        with HR.streams(2) as (reader, S):
            S.gate()
            for (name, call, want), o in zip(_calls(c, eng), outs):
                call(S.handle, B, src, o)
            assert not any(g.capped for g in S.gates), "a call returned only after the gate's cap: it waited for the device"
            assert S.busy(), "the caller's stream is idle although its gate is closed: the case proves nothing"
            for o in outs:
                assert (reader.read(o, np.empty(rows, dtype=U)) == SENTINEL).all(), "written while the caller's stream was held"
            assert S.busy()
            S.release()
            for (name, call, want), o in zip(_calls(c, eng), outs):
                got = np.empty(rows, dtype=U)
                eng.device_download(None, got, o)
                assert_words(got[:B * W].reshape(want.shape), want, (shape, name))
                assert (got[B * W:] == SENTINEL).all(), (shape, name)
    finally:
        for p in [src] + outs:
            eng.device_free(p)


# ---- statuses -----------------------------------------------------------------------------------------------------------------

def test_statuses_and_the_context_stays_usable():
    c = KC.case("N16")
    P = c.P
    eng = spf_amd.Engine(engine_params(P))
    try:
        lib, h = eng._lib, eng._h
        W = (P.k + 1) * P.N
        x = np.ascontiguousarray(c.x)
        out = np.zeros_like(x)
        xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        key = np.ascontiguousarray(c.ksk)
        kp = key.ctypes.data_as(C.c_void_p)
        lg, cnt = P.tr_radix_log, P.tr_count
        want = KC.oracle_keyswitch(P, x, c.ksk_fft)

        def err():
            return lib.spf_last_error(h).decode()

        # nothing loaded: no automorphism key, an empty slot
        assert lib.spf_glwe_trace_batch(h, 5, xp, op) == NO_KEY and "automorphism key" in err()
        assert lib.spf_glwe_automorphism_batch(h, 1, 5, xp, op) == NO_KEY
        assert lib.spf_glwe_keyswitch_batch(h, 0, 5, xp, op) == NO_KEY and "slot 0" in err()
        assert lib.spf_glwe_keyswitch_enqueue(h, None, 15, 5, xp, op) == NO_KEY
        shape = (C.c_uint32(), C.c_uint32())
        assert lib.spf_glwe_keyswitch_slot_shape(h, 0, C.byref(shape[0]), C.byref(shape[1])) == NO_KEY
        assert lib.spf_glwe_keyswitch_slot_shape(h, 16, C.byref(shape[0]), C.byref(shape[1])) == INVALID
        # a slot >= SPF_GLWE_KSK_SLOTS, whatever else
        for slot in (16, 17, 0xFFFFFFFF):
            assert lib.spf_glwe_keyswitch_batch(h, slot, 5, xp, op) == INVALID and "SPF_GLWE_KSK_SLOTS" in err()
            assert lib.spf_glwe_keyswitch_enqueue(h, None, slot, 5, xp, op) == INVALID
            assert lib.spf_load_glwe_keyswitch_key_std(h, slot, kp, key.size, lg, cnt) == INVALID
        # the loader's shape check, each rejection with its numbers
        eng.load_glwe_keyswitch_key_std(4, key, lg, cnt)
        for bad_lg, bad_cnt, words, text in ((0, cnt, key.size, "radix_log 0"), (lg, 0, 0, "radix_count 0"), (8, 8, key.size, "= 64"),
                                             (9, 8, key.size, "72 > 64"), (lg, cnt, key.size - 1, str(key.size - 1)),
                                             (lg, cnt + 1, key.size, str(key.size // cnt * (cnt + 1)))):
            assert lib.spf_load_glwe_keyswitch_key_std(h, 4, kp, words, bad_lg, bad_cnt) == INVALID, (bad_lg, bad_cnt, words)
            assert text in err(), (text, err())
            assert eng.glwe_keyswitch_slot_shape(4) == (lg, cnt), "a refused load touched the slot"
        assert_words(eng.glwe_keyswitch(4, x), want, "after the refused loads")
        # the automorphism key: rounds outside 1 .. log2 N
        eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
        for rnd in (0, KC.log2n(P) + 1, 0xFFFFFFFF):
            assert lib.spf_glwe_automorphism_batch(h, rnd, 5, xp, op) == INVALID and "log2 N" in err()
            assert lib.spf_glwe_automorphism_enqueue(h, None, rnd, 5, xp, op) == INVALID
        # B = 0 is SPF_OK and touches nothing, null pointers included
        out[...] = SENTINEL
        assert lib.spf_glwe_trace_batch(h, 0, xp, op) == 0 and lib.spf_glwe_trace_batch(h, 0, None, None) == 0
        assert lib.spf_glwe_automorphism_batch(h, 1, 0, xp, op) == 0 and lib.spf_glwe_keyswitch_batch(h, 4, 0, xp, op) == 0
        assert lib.spf_glwe_keyswitch_enqueue(h, None, 4, 0, None, None) == 0
        assert (out == SENTINEL).all()
        # null pointers with B > 0; a batch above the limit
        assert lib.spf_glwe_trace_batch(h, 5, None, op) == INVALID and lib.spf_glwe_keyswitch_batch(h, 4, 5, xp, None) == INVALID
        assert lib.spf_glwe_trace_batch(h, 1 << 31, xp, op) == INVALID and "batch too large" in err()
        # the context is as usable as before
        assert_words(eng.glwe_trace(x), KC.oracle_traces("N16"), "trace after the failures")
        assert_words(eng.glwe_automorphism(KC.log2n(P), x), KC.oracle_round(c, x, KC.log2n(P)), "round after the failures")
        assert_words(eng.glwe_keyswitch(4, x), want, "keyswitch after the failures")
        # the timer of all three
        eng.set_timing(True)
        eng.glwe_trace(x); eng.glwe_automorphism(1, x); eng.glwe_keyswitch(4, x)   # noqa: E702
        ms, n = eng.last_kernel_ms("glwe_keyswitch")
        assert n == 3 and ms > 0.0
        eng.set_timing(False)
    finally:
        eng.close()


# ---- group --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, "N256k3_7x5"])
def test_group_over_one_device_twice_is_word_equal_to_one_context(engines, shape):
    c, eng = KC.case(shape), engines(shape)
    grp = spf_amd.Group(engine_params(c.P), devices=[0, 0])
    try:
        with pytest.raises(spf_amd.SpfError) as e:
            grp.glwe_trace(c.x)
        assert e.value.status == NO_KEY
        grp.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
        grp.load_glwe_keyswitch_key_std(A2B_SLOT, c.ksk, c.P.tr_radix_log, c.P.tr_count)
        assert grp.glwe_keyswitch_slot_shape(A2B_SLOT) == (c.P.tr_radix_log, c.P.tr_count)
        assert_words(grp.glwe_trace(c.x), eng.glwe_trace(c.x), (shape, "trace"))      # B = 5 over two members: shards of 3 and 2
        assert grp.last_glwe_keyswitch_kernel() == kernel_of(shape)
        assert_words(grp.glwe_automorphism(3, c.x), eng.glwe_automorphism(3, c.x), (shape, "automorphism"))
        assert_words(grp.glwe_keyswitch(A2B_SLOT, c.x), eng.glwe_keyswitch(A2B_SLOT, c.x), (shape, "keyswitch"))
        assert_words(grp.glwe_keyswitch(A2B_SLOT, c.x), KC.oracle_keyswitch(c.P, c.x, c.ksk_fft), (shape, "oracle"))
    finally:
        grp.close()


def test_evaluation_wrappers(engines):
    c, eng = KC.case("N16"), engines("N16")
    ev = spf_amd.Evaluation.__new__(spf_amd.Evaluation)
    ev.engine = eng
    out = np.zeros_like(c.x)
    ev.keyswitch_glwe_to_glwe(out, c.x, A2B_SLOT)
    assert_words(out, KC.oracle_keyswitch(c.P, c.x, c.ksk_fft), "keyswitch_glwe_to_glwe")
    ev.trace(out, c.x)
    assert_words(out, KC.oracle_traces("N16"), "trace")
