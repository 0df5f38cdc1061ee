"""Blind rotation by an encrypted shift by handle (`spf_pool_submit_blind_rotation_v`, include/spf_hip.h): one rotate-CMUX step per
bit pushed on the pending result of the step before, step i of many callers one launch over a pointer table.  Words only
(tests/blind_rotation_graph_cases.py `same_words`), against `Engine.blind_rotation` and against the blocking sequence."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import ValueKind
from tests import blind_rotation_graph_cases as K
from tests.util import keyset, random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu


def _load(e, ks, ak, ssk):
    e.load_bootstrap_key(ks.bsk_fft)
    e.load_keyswitch_key(ks.ksk)
    e.load_automorphism_key(ak)
    e.load_scheme_switch_key(ssk)


@pytest.fixture(scope="module")
def rigs():
    """the tuned kernels (DEFAULT_128 with a short LWE side, test_gpu_values.py's keys) and the generic ones (SMALL16), all keys in"""
    ks = keyset(0x5EED0001, 12)
    r = O.Rng(0x7A11)
    tuned = spf_amd.Engine(to_engine_params(ks.params))
    _load(tuned, ks, O.gen_auto_key_fft(r, ks.glwe_sk, ks.params), O.gen_ssk_fft(r, ks.glwe_sk, ks.params))
    Q = K.SMALL16
    kq = O.gen_keyset(0x5EED0009, Q)
    r = O.Rng(0x7A12)
    small = spf_amd.Engine(K.engine_params(Q))
    _load(small, kq, O.gen_auto_key_fft(r, kq.glwe_sk, Q), O.gen_ssk_fft(r, kq.glwe_sk, Q))
    out = {"tuned": (ks.params, tuned, K.FOUR_WAVE_SCATTERED), "small16": (Q, small, K.GENERIC_ROT)}
    yield out
    tuned.close()
    small.close()


def _push_gate_cbs(pool, lwe1):
    """spf_pool_submit_keyswitch_circuit_bootstrap_v without a ticket: the result stays pending until somebody waits"""
    h = C.c_void_p()
    pool._ck(pool._lib.spf_pool_submit_keyswitch_circuit_bootstrap_v(pool._h, lwe1._h, C.byref(h), None),
             "spf_pool_submit_keyswitch_circuit_bootstrap_v")
    return spf_amd.Value(pool, h)


@pytest.mark.parametrize("which,n_bits,log_stride", [("tuned", 3, 8), ("tuned", 1, 0), ("small16", 2, 2), ("small16", 4, 0)])
def test_uploaded_selectors_give_the_engines_words(rigs, which, n_bits, log_stride):
    P, eng, kernel = rigs[which]
    glwe, sels = random_glwe(0xB70 + n_bits, 1, P.glwe_len), K.random_selectors(0xB71 + n_bits, n_bits, P)
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    try:
        start = pool.value_stats()["live_values"]
        vx = pool.upload(ValueKind.GLWE1, glwe[0])
        vs = [pool.upload(ValueKind.GGSW1, s) for s in sels]
        out = pool.blind_rotation_v(vx, vs, log_stride)
        assert eng.last_cmux_kernel() == kernel
        got = out.download()
        assert K.same_words(vx.download(), glwe[0]) and all(K.same_words(v.download(), s) for v, s in zip(vs, sels))
        for v in [vx, out] + vs:
            v.release()
        assert pool.value_stats()["live_values"] == start
    finally:
        pool.close()
    assert K.same_words(got, eng.blind_rotation(sels[None], glwe, log_stride)[0])
    assert K.same_words(got, K.oracle_loop(glwe[0], sels, log_stride, P))


@pytest.mark.parametrize("which", ["tuned", "small16"])
def test_pending_selectors_and_nothing_waited_for_but_the_result(rigs, which):
    P, eng, _ = rigs[which]
    n_bits, log_stride = 3, 1
    glwe, lwe1 = random_glwe(0xB80, 1, P.glwe_len), random_lwe_batch(0xB81, n_bits, P.k * P.N)
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=100000)     # (a long quiet time: only the wait below launches anything)
    try:
        start = pool.value_stats()["live_values"]
        vx = pool.upload(ValueKind.GLWE1, glwe[0])
        vl = [pool.upload(ValueKind.LWE1, x) for x in lwe1]
        sels = [_push_gate_cbs(pool, v) for v in vl]
        out = pool.push_blind_rotation_v(vx, sels, log_stride)
        assert not out.info()["valid"] and not any(s.info()["valid"] for s in sels)
        pushed = out.wait().download()
        # the blocking sequence: every selector waited for, then the rotation waited for
        bsels = [pool.keyswitch_circuit_bootstrap_v(v) for v in vl]
        bout = pool.blind_rotation_v(vx, bsels, log_stride)
        blocking = bout.download()
        for v in [vx, out, bout] + vl + sels + bsels:
            v.release()
        gc.collect()
        assert pool.value_stats()["live_values"] == start
    finally:
        pool.close()
    assert K.same_words(pushed, blocking)
    assert K.same_words(pushed, eng.blind_rotation(eng.keyswitch_circuit_bootstrap(lwe1)[None], glwe, log_stride)[0])


def test_sixteen_callers_chains_are_coalesced_step_by_step(rigs):
    P, eng, _ = rigs["tuned"]
    callers, n_bits, log_stride = 16, 4, 3
    glwe, sels = random_glwe(0xB90, callers, P.glwe_len), K.random_selectors(0xB91, 2 * n_bits, P)
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=100000)
    try:
        start = pool.value_stats()["live_values"]
        vs = [pool.upload(ValueKind.GGSW1, s) for s in sels]
        vx = [pool.upload(ValueKind.GLWE1, x) for x in glwe]
        mine = [[vs[(c % 2) * n_bits + i] for i in range(n_bits)] for c in range(callers)]   # two sets of selectors, interleaved
        c0 = pool.counters()
        outs = [pool.push_blind_rotation_v(vx[c], mine[c], log_stride) for c in range(callers)]
        got = [o.wait().download() for o in outs]
        c1 = pool.counters()
        ops, launches = c1["handle_ops"] - c0["handle_ops"], c1["handle_launches"] - c0["handle_launches"]
        print(f"{callers} chains of {n_bits} steps: {ops} operations in {launches} launches")
        assert ops == callers * n_bits and launches < ops, (c0, c1)
        for v in vs + vx + outs:
            v.release()
        assert pool.value_stats()["live_values"] == start
    finally:
        pool.close()
    for c in range(callers):
        want = eng.blind_rotation(sels[None, (c % 2) * n_bits:(c % 2 + 1) * n_bits], glwe[c:c + 1], log_stride)[0]
        assert K.same_words(got[c], want), c


def test_bad_arguments_leave_no_pending_work(rigs):
    P, eng, _ = rigs["tuned"]
    glwe, sels = random_glwe(0xBA0, 1, P.glwe_len), K.random_selectors(0xBA1, 2, P)
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    grp = spf_amd.Group(to_engine_params(P), devices=[0, 0])
    gpool = spf_amd.Pool(grp, max_batch=64, max_wait_us=200)
    try:
        vx = pool.upload(ValueKind.GLWE1, glwe[0])
        vs = [pool.upload(ValueKind.GGSW1, s) for s in sels]
        before = (pool.value_stats()["live_values"], pool.counters()["handle_ops"])
        submit = pool._lib.spf_pool_submit_blind_rotation_v
        arr = (C.c_void_p * 12)(*([vs[0]._h] * 12))
        h, t = C.c_void_p(), C.c_uint64()

        def refused(call, word):
            with pytest.raises(spf_amd.SpfError) as e:
                call()
            assert e.value.status == 1 and word in str(e.value), str(e.value)
            assert (pool.value_stats()["live_values"], pool.counters()["handle_ops"]) == before

        refused(lambda: pool.blind_rotation_v(vx, []), "n_bits")
        refused(lambda: pool.blind_rotation_v(vx, [vs[0]] * 12), "n_bits + log_stride")
        refused(lambda: pool.blind_rotation_v(vx, vs, 10), "n_bits + log_stride")                # 2 + 10 = log2 N + 1
        refused(lambda: pool.blind_rotation_v(vx, [vs[0], vx]), "selector is not an L1 GGSW")
        refused(lambda: pool.blind_rotation_v(vs[0], vs), "operand is not an L1 GLWE")
        refused(lambda: pool._ck(submit(pool._h, None, arr, 2, 0, C.byref(h), C.byref(t)), "x"), "null")
        refused(lambda: pool._ck(submit(pool._h, vx._h, None, 2, 0, C.byref(h), C.byref(t)), "x"), "null")
        refused(lambda: pool._ck(submit(pool._h, vx._h, arr, 2, 0, None, C.byref(t)), "x"), "null")
        refused(lambda: pool._ck(submit(pool._h, vx._h, (C.c_void_p * 2)(vs[0]._h, None), 2, 0, C.byref(h), C.byref(t)), "x"), "null")
        assert submit(None, vx._h, arr, 2, 0, C.byref(h), C.byref(t)) == 1
        out = pool.blind_rotation_v(vx, vs, 9)                                                    # 2 + 9 = log2 N: accepted
        assert K.same_words(out.download(), K.oracle_loop(glwe[0], sels, 9, P))
        # operands on different members of a group pool
        gx = gpool.upload(ValueKind.GLWE1, glwe[0], member=0)
        gs = [gpool.upload(ValueKind.GGSW1, sels[0], member=0), gpool.upload(ValueKind.GGSW1, sels[1], member=1)]
        with pytest.raises(spf_amd.SpfError, match="different members") as e:
            gpool.blind_rotation_v(gx, gs)
        assert e.value.status == 1
        moved = gpool.copy_to_member(gs[1], 0)
        assert K.same_words(gpool.blind_rotation_v(gx, [gs[0], moved]).download(), K.oracle_loop(glwe[0], sels, 0, P))
    finally:
        gc.collect()
        gpool.close()
        grp.close()
        pool.close()
