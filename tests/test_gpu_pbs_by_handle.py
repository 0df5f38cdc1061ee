"""The bootstraps by a caller's table by handle: `spf_pool_submit_op_v` with `SPF_OP_PBS_UNIVARIATE` / `SPF_OP_PBS_BIVARIATE`
(include/spf_hip.h) — the table an L1 GLWE value like any other, batched and paced like the circuit bootstraps.  Words only
(tests/pbs_graph_cases.py `same_words`), against `Engine.pbs_univariate` / `pbs_bivariate` on the same rows and against the oracle."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import pbs_graph_cases as K
from tests.util import random_glwe, random_lwe_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs():
    made = {w: K.make_engine(w) for w in ("tuned", "n16k1")}
    yield {w: (K.keys_of(w)[0], e, K.keys_of(w)[1]) for w, e in made.items()}
    for e in made.values():
        e.close()


@pytest.mark.parametrize("which", ["tuned", "n16k1"])
def test_valid_operands_give_the_engines_and_the_oracles_words(rigs, which):
    P, eng, ks = rigs[which]
    x, lut = random_lwe_batch(0xF00, 2, P.lwe_n), random_glwe(0xF01, 1, P.glwe_len)[0]
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    try:
        start = pool.value_stats()["live_values"]
        va, vb, vt = pool.upload(ValueKind.LWE0, x[0]), pool.upload(ValueKind.LWE0, x[1]), pool.upload(ValueKind.GLWE1, lut)
        outs = {"uni": pool.run_v(FheOp.PBS_UNIVARIATE, [va, vt], 99),                # (its parameter is forced to 0)
                "biv0": pool.run_v(FheOp.PBS_BIVARIATE, [va, vb, vt], 0),
                "biv2": pool.run_v(FheOp.PBS_BIVARIATE, [vb, va, vt], 2),
                "biv63": pool.run_v(FheOp.PBS_BIVARIATE, [va, vb, vt], 63),
                "same": pool.run_v(FheOp.PBS_BIVARIATE, [va, va, vt], 2)}                # f(x, x): one value twice
        got = {k: v.download() for k, v in outs.items()}
        assert K.same_words(va.download(), x[0]) and K.same_words(vt.download(), lut)     # operands unchanged
        for v in [va, vb, vt] + list(outs.values()):
            v.release()
        assert pool.value_stats()["live_values"] == start
    finally:
        pool.close()
    assert K.same_words(got["uni"], eng.pbs_univariate(x[:1], lut)[0])
    assert K.same_words(got["uni"], O.pbs_univariate(x[0], lut, ks.bsk_fft, P))
    for name, (l, r, p) in {"biv0": (0, 1, 0), "biv2": (1, 0, 2), "biv63": (0, 1, 63), "same": (0, 0, 2)}.items():
        assert K.same_words(got[name], eng.pbs_bivariate(x[l:l + 1], x[r:r + 1], lut, p)[0]), name
        assert K.same_words(got[name], O.pbs_univariate(K.pack(x[l], x[r], p), lut, ks.bsk_fft, P)), name


@pytest.mark.parametrize("which", ["tuned", "n16k1"])
def test_pending_operands_a_keyswitch_result_as_the_lwe_and_a_mul_xn_result_as_the_table(rigs, which):
    P, eng, ks = rigs[which]
    l1, x, lut = random_lwe_batch(0xF10, 1, P.k * P.N)[0], random_lwe_batch(0xF11, 1, P.lwe_n)[0], random_glwe(0xF12, 1, P.glwe_len)[0]
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=100000)     # (a long quiet time: only the waits below launch anything)
    try:
        start = pool.value_stats()["live_values"]
        v1, vx, vt = pool.upload(ValueKind.LWE1, l1), pool.upload(ValueKind.LWE0, x), pool.upload(ValueKind.GLWE1, lut)
        l0 = pool.push_v(FheOp.KeyswitchL1toL0, [v1])
        t5 = pool.push_v(FheOp.MulXN, [vt], 5)
        uni = pool.push_v(FheOp.PBS_UNIVARIATE, [l0, t5])
        biv = pool.push_v(FheOp.PBS_BIVARIATE, [l0, vx, t5], 1)
        assert not uni.info()["valid"] and not biv.info()["valid"] and not l0.info()["valid"] and not t5.info()["valid"]
        got_uni, got_biv = uni.wait().download(), biv.wait().download()
        for v in (v1, vx, vt, l0, t5, uni, biv):
            v.release()
        gc.collect()
        assert pool.value_stats()["live_values"] == start
    finally:
        pool.close()
    l0_want = O.keyswitch_lwe(l1, ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count)
    t_want = O.glwe_mul_xn(lut, 5, P.N, P.k)
    assert K.same_words(got_uni, O.pbs_univariate(l0_want, t_want, ks.bsk_fft, P))
    assert K.same_words(got_biv, O.pbs_univariate(K.pack(l0_want, x, 1), t_want, ks.bsk_fft, P))
    assert K.same_words(got_biv, eng.pbs_bivariate(l0_want[None], x[None], t_want, 1)[0])


@pytest.mark.parametrize("op", [FheOp.PBS_UNIVARIATE, FheOp.PBS_BIVARIATE], ids=["univariate", "bivariate"])
def test_sixteen_callers_land_in_fewer_launches_than_operations(rigs, op):
    P, eng, ks = rigs["tuned"]
    callers = 16
    x, luts = random_lwe_batch(0xF20, callers + 1, P.lwe_n), random_glwe(0xF21, 2, P.glwe_len)
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=100000)
    try:
        start = pool.value_stats()["live_values"]
        vx = [pool.upload(ValueKind.LWE0, v) for v in x]
        vt = [pool.upload(ValueKind.GLWE1, v) for v in luts]
        c0 = pool.counters()
        if op == FheOp.PBS_UNIVARIATE:
            outs = [pool.push_v(op, [vx[c], vt[c % 2]]) for c in range(callers)]
        else:
            outs = [pool.push_v(op, [vx[c], vx[c + 1], vt[c % 2]], 2) for c in range(callers)]
        got = [o.wait().download() for o in outs]
        c1 = pool.counters()
        ops, launches = c1["handle_ops"] - c0["handle_ops"], c1["handle_launches"] - c0["handle_launches"]
        print(f"{callers} callers, one {op.name} each: {ops} operations in {launches} launches")
        assert ops == callers and launches < ops, (c0, c1)
        for v in vx + vt + outs:
            v.release()
        assert pool.value_stats()["live_values"] == start
    finally:
        pool.close()
    tables = luts[np.arange(callers) % 2]
    want = eng.pbs_univariate(x[:callers], tables) if op == FheOp.PBS_UNIVARIATE else eng.pbs_bivariate(x[:callers], x[1:], tables, 2)
    assert K.same_words(np.stack(got), want)


def test_bad_arguments_are_refused_before_anything_is_queued(rigs):
    P, eng, ks = rigs["tuned"]
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    grp = spf_amd.Group(K.engine_params(P), devices=[0, 0])
    gpool = None
    try:
        K.load_keys(grp, "tuned")
        gpool = spf_amd.Pool(grp, max_batch=64, max_wait_us=200)
        x, lut = random_lwe_batch(0xF30, 2, P.lwe_n), random_glwe(0xF31, 1, P.glwe_len)[0]
        va, vt = pool.upload(ValueKind.LWE0, x[0]), pool.upload(ValueKind.GLWE1, lut)
        v1 = pool.upload(ValueKind.LWE1, random_lwe_batch(0xF32, 1, P.k * P.N)[0])
        before = (pool.value_stats()["live_values"], pool.counters()["handle_ops"])

        def refused(call, word):
            with pytest.raises(spf_amd.SpfError) as e:
                call()
            assert e.value.status == 1 and word in str(e.value), str(e.value)
            assert (pool.value_stats()["live_values"], pool.counters()["handle_ops"]) == before

        refused(lambda: pool.run_v(FheOp.PBS_UNIVARIATE, [va]), "wrong number of operands")
        refused(lambda: pool.run_v(FheOp.PBS_UNIVARIATE, [va, va, vt]), "wrong number of operands")
        refused(lambda: pool.run_v(FheOp.PBS_BIVARIATE, [va, vt], 2), "wrong number of operands")
        refused(lambda: pool.run_v(FheOp.PBS_BIVARIATE, [va, va, vt], 64), "plaintext_bits")
        refused(lambda: pool.run_v(FheOp.PBS_UNIVARIATE, [v1, vt]), "wrong ciphertext type")
        refused(lambda: pool.run_v(FheOp.PBS_UNIVARIATE, [vt, va]), "wrong ciphertext type")
        refused(lambda: pool.run_v(FheOp.PBS_BIVARIATE, [va, va, va], 2), "wrong ciphertext type")
        h, t = C.c_void_p(), C.c_uint64()
        arr = (C.c_void_p * 2)(va._h, None)
        refused(lambda: pool._ck(pool._lib.spf_pool_submit_op_v(pool._h, int(FheOp.PBS_UNIVARIATE), arr, 2, 0, C.byref(h), C.byref(t)), "x"),
                "null operand")
        assert K.same_words(pool.run_v(FheOp.PBS_BIVARIATE, [va, va, vt], 63).download(),
                            O.pbs_univariate(K.pack(x[0], x[0], 63), lut, ks.bsk_fft, P))
        # the member rule of a group pool: operands on different members are refused, moved they are taken
        ga, gb = gpool.upload(ValueKind.LWE0, x[0], member=0), gpool.upload(ValueKind.LWE0, x[1], member=0)
        gt = gpool.upload(ValueKind.GLWE1, lut, member=1)
        with pytest.raises(spf_amd.SpfError, match="different members") as e:
            gpool.run_v(FheOp.PBS_BIVARIATE, [ga, gb, gt], 2)
        assert e.value.status == 1
        moved = gpool.copy_to_member(gt, 0)
        assert K.same_words(gpool.run_v(FheOp.PBS_BIVARIATE, [ga, gb, moved], 2).download(),
                            O.pbs_univariate(K.pack(x[0], x[1], 2), lut, ks.bsk_fft, P))
    finally:
        gc.collect()
        if gpool is not None:
            gpool.close()
        grp.close()
        pool.close()
