"""Ring packing on the GPU (spf_lwe_ring_pack_*; include/spf_hip.h, "ring packing"): every output word equals the composition of
oracle functions in tests/lwe_ring_pack_cases.py.  There is no tolerance in this file; the decryption check uses the reference's
decode at 12 plaintext bits.  The device forms run between sentinel rows, around the output and around the scratch."""
import ctypes as C
import os

import numpy as np
import pytest

import spf_amd
from tests import glwe_keyswitch_cases as KC
from tests import hip_runtime as HR
from tests import lwe_ring_pack_cases as RC
from tests.test_gpu_glwe_keyswitch import DeviceRows, assert_words, engine_params

pytestmark = pytest.mark.gpu
U = np.uint64
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
INVALID, NO_KEY = 1, 3
TUNED = "default128_6x7"
HAND_WRITTEN, GENERIC = "ring_pack_kernel", "generic_ring_pack_kernel"
LWE1, GLWE1 = RC.LWE1, RC.GLWE1
CAP = "SPF_LWE_RING_PACK_SCRATCH_BYTES"


def kernel_of(shape):
    return HAND_WRITTEN if shape == TUNED else GENERIC


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(shape):
        if shape not in made:
            c = KC.case(shape)
            eng = spf_amd.Engine(engine_params(c.P))
            eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
            made[shape] = eng
        return made[shape]
    yield get
    for e in made.values():
        e.close()


def pack_between_sentinels(eng, c, lv, p, kind, B):
    """the host-pointer form into rows 2 .. 2 + B of a larger array: (B, k+1, N)"""
    W = (c.P.k + 1) * c.P.N
    big = np.full((B + 4, W), SENTINEL, dtype=U)
    eng.lwe_ring_pack(lv, p, kind, out=big[2:2 + B])
    assert (big[:2] == SENTINEL).all() and (big[2 + B:] == SENTINEL).all(), "words around the output were written"
    return big[2:2 + B].reshape(B, c.P.k + 1, c.P.N)


def run_case(engines, shape, B, p, kind):
    c, eng = KC.case(shape), engines(shape)
    lv = RC.leaves(shape, kind)[:B * p]
    eng.set_timing(True)
    eng.last_kernel_ms("lwe_ring_pack")
    got = pack_between_sentinels(eng, c, lv, p, kind, B)
    ms, n = eng.last_kernel_ms("lwe_ring_pack")
    eng.set_timing(False)
    assert eng.last_lwe_ring_pack_kernel() == kernel_of(shape)
    assert n == RC.launches(c.P, p), (shape, B, p, n)
    assert_words(got, RC.oracle_outputs(shape, B, p, kind), (shape, B, p, kind))
    return got


# (3, 8): levels of 12, 6 and 3 units — a ragged workgroup of four on two levels; (1, 32): a level of one unit; (5, 1): no tree
@pytest.mark.parametrize("B,p,kind", [(3, 8, LWE1), (1, 32, LWE1), (2, 2, LWE1), (5, 1, LWE1), (3, 4, GLWE1)])
def test_the_hand_written_kernel_equals_the_composition(engines, B, p, kind):
    got = run_case(engines, TUNED, B, p, kind)
    for b in range(B):
        RC.check_decrypts(KC.case(TUNED), got[b], b * p, p, "gpu")


# the generic kernel with its k = 3 row loop; p = N: the last tree level writes the output, no tail
@pytest.mark.parametrize("B,p", [(3, 8), (1, 256)])
def test_the_generic_kernel_equals_the_composition(engines, B, p):
    got = run_case(engines, "N256k3_7x5", B, p, LWE1)
    RC.check_decrypts(KC.case("N256k3_7x5"), got[0], 0, p, "gpu")


@pytest.mark.parametrize("kind", [LWE1, GLWE1])
@pytest.mark.parametrize("p", [1, 2, 4, 8, 16])
def test_every_p_at_degree_16(engines, p, kind):
    run_case(engines, "N16", 5, p, kind)


# ---- the device-pointer form ------------------------------------------------------------------------------------------------

class DeviceWords(DeviceRows):
    """`words` words in a device buffer between sentinel rows (the scratch: its contents are undefined, its surroundings are not)"""

    def __init__(self, eng, words):
        super().__init__(eng, max(words, 1), 1)


@pytest.mark.parametrize("shape,B,p,kind", [(TUNED, 3, 8, LWE1), ("N256k3_7x5", 3, 8, LWE1), ("N16", 5, 4, GLWE1), ("N16", 5, 16, LWE1),
                                            ("N16", 5, 1, LWE1)])
def test_enqueue_on_another_stream_gives_the_words_of_batch(engines, shape, B, p, kind):
    c, eng = KC.case(shape), engines(shape)
    W = (c.P.k + 1) * c.P.N
    lv = RC.leaves(shape, kind)[:B * p]
    words = eng.lwe_ring_pack_scratch_words(p, B)
    rows = 1 if p == 1 else (p // 2 if (p > 2 or c.P.N > 2) else 0) + (p // 4 if p >= 4 and (p > 4 or c.P.N > 4) else 0)
    assert words == B * rows * W
    d_leaves = eng.device_alloc(lv.nbytes)
    out, scratch = DeviceRows(eng, W, B), DeviceWords(eng, words)
    try:
        eng.device_upload(d_leaves, lv)
        with HR.streams(1) as (S,):
            eng.lwe_ring_pack_enqueue(S.handle, kind, p, 0, d_leaves, scratch.ptr, words, out.ptr)     # B = 0 writes nothing
            S.synchronize()
            assert (out.fetch() == SENTINEL).all() and (scratch.fetch() == SENTINEL).all()
            eng.lwe_ring_pack_enqueue(S.handle, kind, p, B, d_leaves, scratch.ptr, words, out.ptr)
            S.synchronize()
        assert eng.last_lwe_ring_pack_kernel() == kernel_of(shape)
        got = out.fetch().reshape(B, c.P.k + 1, c.P.N)
        scratch.fetch()                                                                                    # the sentinels around it
        assert_words(got, RC.oracle_outputs(shape, B, p, kind), (shape, B, p, "enqueue"))
        assert_words(got, eng.lwe_ring_pack(lv, p, kind).reshape(got.shape), (shape, B, p, "batch"))
        back = np.empty_like(lv)
        eng.device_download(None, back, d_leaves)
        assert_words(back, lv, "the leaves were written")
    finally:
        eng.device_free(d_leaves)
        out.free()
        scratch.free()


# ---- slices -----------------------------------------------------------------------------------------------------------------

def test_three_slices_are_word_equal_to_one(engines, monkeypatch):
    """N16, (B, p) = (7, 8) under a cap of three outputs' worth of scratch: slices of 3, 3 and 1 outputs"""
    c, eng = KC.case("N16"), engines("N16")
    B, p = 7, 8
    lv = RC.leaves("N16", LWE1)[:B * p]
    monkeypatch.delenv(CAP, raising=False)
    one = run_case(engines, "N16", B, p, LWE1)
    monkeypatch.setenv(CAP, str(eng.lwe_ring_pack_scratch_words(p, 3) * 8))
    eng.set_timing(True)
    eng.last_kernel_ms("lwe_ring_pack")
    sliced = pack_between_sentinels(eng, c, lv, p, LWE1, B)
    _, n = eng.last_kernel_ms("lwe_ring_pack")
    eng.set_timing(False)
    assert n == 3 * RC.launches(c.P, p), n
    assert_words(sliced, one, "three slices")
    monkeypatch.setenv(CAP, "1")                  # below one output's worth: slices of one output
    assert_words(pack_between_sentinels(eng, c, lv, p, LWE1, B), one, "seven slices")


# ---- statuses ---------------------------------------------------------------------------------------------------------------

def test_statuses_leave_output_and_scratch_untouched():
    c = KC.case("N16")
    P = c.P
    W, B, p = (P.k + 1) * P.N, 3, 4
    eng = spf_amd.Engine(engine_params(P))
    lv = np.ascontiguousarray(RC.leaves("N16", LWE1)[:B * p])
    out = np.full((B, W), SENTINEL, dtype=U)
    lp, op = lv.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    try:
        lib, h = eng._lib, eng._h
        words = eng.lwe_ring_pack_scratch_words(p, B)
        d_leaves, d_out, d_scr = eng.device_alloc(lv.nbytes), DeviceRows(eng, W, B), DeviceWords(eng, words)
        eng.device_upload(d_leaves, lv)

        def err():
            return lib.spf_last_error(h).decode()

        def enqueue(kind=LWE1, pp=p, BB=B, leaves=d_leaves, scr=None, w=words, o=None):
            return lib.spf_lwe_ring_pack_enqueue(h, None, kind, pp, BB, leaves, d_scr.ptr if scr is None else scr, w,
                                                 d_out.ptr if o is None else o)

        def untouched():
            return (out == SENTINEL).all() and (d_out.fetch() == SENTINEL).all() and (d_scr.fetch() == SENTINEL).all()

        # no automorphism key
        assert lib.spf_lwe_ring_pack_batch(h, LWE1, p, B, lp, op) == NO_KEY and "automorphism key" in err()
        assert enqueue() == NO_KEY
        assert untouched()
        eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
        # p = 0, not a power of two, above N; another leaf kind: the numbers are in the message
        for bad in (0, 3, 12, 32, 1 << 40):
            assert lib.spf_lwe_ring_pack_batch(h, LWE1, bad, B, lp, op) == INVALID and f"p = {bad}" in err() and "N = 16" in err()
            assert enqueue(pp=bad) == INVALID and f"p = {bad}" in err()
            w = C.c_size_t(77)
            assert lib.spf_lwe_ring_pack_scratch_words(h, bad, B, C.byref(w)) == INVALID and w.value == 77
        for kind in (0, 3, 4, 17):
            assert lib.spf_lwe_ring_pack_batch(h, kind, p, B, lp, op) == INVALID and f"leaf kind {kind}" in err()
            assert enqueue(kind=kind) == INVALID
        # a scratch that is too small names the words needed; a null scratch where one is needed
        assert enqueue(w=words - 1) == INVALID and str(words) in err() and str(words - 1) in err()
        assert enqueue(w=0) == INVALID and str(words) in err()
        assert lib.spf_lwe_ring_pack_enqueue(h, None, LWE1, p, B, d_leaves, None, words, d_out.ptr) == INVALID
        # any overlap of the output with the leaves or the scratch
        assert enqueue(o=d_leaves) == INVALID and "overlap" in err()
        assert enqueue(o=d_leaves + lv.nbytes - 8) == INVALID and "overlap" in err()
        assert enqueue(o=d_scr.ptr) == INVALID and "overlap" in err()
        assert enqueue(o=d_scr.ptr + words * 8 - 8) == INVALID and "overlap" in err()
        assert enqueue(scr=d_leaves) == INVALID and "overlap" in err()
        assert lib.spf_lwe_ring_pack_batch(h, LWE1, p, B, lp, lp) == INVALID and "overlap" in err()
        # null pointers with B > 0
        assert lib.spf_lwe_ring_pack_batch(h, LWE1, p, B, None, op) == INVALID and lib.spf_lwe_ring_pack_batch(h, LWE1, p, B, lp, None) == INVALID
        assert untouched()
        # B = 0 is SPF_OK and touches nothing, null pointers included
        assert lib.spf_lwe_ring_pack_batch(h, LWE1, p, 0, lp, op) == 0 and lib.spf_lwe_ring_pack_batch(h, LWE1, p, 0, None, None) == 0
        assert lib.spf_lwe_ring_pack_enqueue(h, None, LWE1, p, 0, None, None, 0, None) == 0
        assert untouched()
        # the context is as usable as before
        assert enqueue() == 0
        want = RC.oracle_outputs("N16", B, p, LWE1)
        assert_words(d_out.fetch().reshape(want.shape), want, "after the failures")
        d_scr.fetch()
        eng.device_free(d_leaves)
        d_out.free()
        d_scr.free()
    finally:
        eng.close()


# ---- group, another radix, wrappers ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, "N16"])
def test_group_over_one_device_twice_is_word_equal_to_one_context(engines, shape):
    c = KC.case(shape)
    B, p = (3, 8) if shape == TUNED else (5, 4)
    lv = RC.leaves(shape, LWE1)[:B * p]
    grp = spf_amd.Group(engine_params(c.P), devices=[0, 0])
    try:
        with pytest.raises(spf_amd.SpfError) as e:
            grp.lwe_ring_pack(lv, p)
        assert e.value.status == NO_KEY
        grp.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
        got = grp.lwe_ring_pack(lv, p)                      # shards of 2 and 1 (3 and 2) outputs, their leaves with them
        assert grp.last_lwe_ring_pack_kernel() == kernel_of(shape)
        assert_words(got.reshape(B, c.P.k + 1, c.P.N), RC.oracle_outputs(shape, B, p, LWE1), (shape, "group"))
        with pytest.raises(spf_amd.SpfError) as e:
            grp.lwe_ring_pack(lv, 3 if shape == TUNED else 5)     # (divides the leaves: the library is asked, and refuses)
        assert e.value.status == INVALID and "power of two" in str(e.value)
    finally:
        grp.close()


def test_a_tuned_context_with_another_automorphism_radix_runs_the_generic_kernel():
    """N = 2048, k = 1 with tr_radix 4 levels x 8 bits: the generic kernel, against the same composition under that radix"""
    c = KC.case(TUNED)
    lg, cnt = KC.OTHER_RADIX
    P = c.P.replace(tr_radix_log=lg, tr_count=cnt)
    rng = np.random.default_rng([0xD2, P.N])
    ak = RC.R.automorphism_keys(rng, c.hk.glwe_sk, P.N, P.k, lg, cnt, RC.C.NOISE)
    other = KC.KsCase("default128_4x8", P, c.hk, RC.C.key_fft(ak).reshape(KC.log2n(P), -1), c.sk_b, c.ksk, c.ksk_fft, c.x)
    eng = spf_amd.Engine(engine_params(P))
    try:
        eng.load_automorphism_key_std(np.ascontiguousarray(ak))
        B, p = 2, 4
        lv = RC.leaves(TUNED, LWE1)[:B * p]
        got = eng.lwe_ring_pack(lv, p).reshape(B, P.k + 1, P.N)
        assert eng.last_lwe_ring_pack_kernel() == GENERIC
        want = np.stack([RC.oracle_ring_pack(other, lv[b * p:(b + 1) * p], p, LWE1) for b in range(B)])
        assert_words(got, want, "4x8")
    finally:
        eng.close()


def test_evaluation_wrapper_and_the_strided_helpers(engines):
    from spf_amd import packed
    c, eng = KC.case("N16"), engines("N16")
    ev = spf_amd.Evaluation.__new__(spf_amd.Evaluation)
    ev.engine = eng
    B, p = 2, 8
    out = np.zeros((B, c.P.k + 1, c.P.N), dtype=U)
    ev.lwe_ring_pack(out, RC.leaves("N16", LWE1)[:B * p], p)
    assert_words(out, RC.oracle_outputs("N16", B, p, LWE1), "lwe_ring_pack")
    params = eng.params
    phase = KC.decode(RC.R.glwe_phase(out[1], c.hk.glwe_sk))
    assert list(packed.strided_positions(p, params)) == [2 * j for j in range(p)]
    assert list(packed.strided_decode(phase, p, params)) == [RC.message(p + j) for j in range(p)]
    assert np.array_equal(packed.strided_plaintext([RC.message(p + j) for j in range(p)], params), phase)
