"""A pool with mixed parameters (`spf_pool_set_mixed_parameters`): SampleExtract, MulXN, GLWE keyswitch and automorphism calls
whose parameters differ share a batch, which runs as ONE launch of the per-item kernels.

The submission pattern is that of tests/test_gpu_glwe_keyswitch_pool.py::test_rounds_and_slots_submitted_interleaved_never_
share_a_launch — item i under (round 1, slot A, round log2 N, slot B) in turn, all before any wait, A and B of one radix shape —
which pins 4 B launches for a pool without mixing; with it the same pushes are exactly 2 launches, one per kind.  The rigs, keys and
oracle rows are those of tests/test_gpu_each_parameters.py.  Every comparison is word for word: against the oracle and against a
pool without mixing.  No test waits out a quiet time: batches by handle are closed by the wait for a value, batches by host
pointer by filling up (max_batch = the operations submitted)."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, SpfError, ValueKind
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as G
from tests import test_gpu_each_parameters as E

pytestmark = pytest.mark.gpu
GLWE = ValueKind.GLWE1
U = np.uint64
TUNED, SMALL = E.TUNED, E.SMALL
KS, AU, SE, MX = FheOp.GLWE_KEYSWITCH, FheOp.GLWE_AUTOMORPHISM, FheOp.SampleExtract, FheOp.MulXN
NAME = {KS: "ks", AU: "au", SE: "se", MX: "mx"}
B = KC.ITEMS
OPERANDS = [0, 1, 2, 3, 0]          # item 0's operand stands twice in the pointer table


def plan_of(c):
    return [(AU, 1), (KS, E.A), (AU, KC.log2n(c.P)), (KS, E.B2)]


def oracle(shape, op, param, item):
    return E.oracle_row(shape, NAME[op], int(param), item)


@pytest.fixture(scope="module")
def rigs():
    """shape -> (case, engine with every key, pool by handle with mixing ON, the same with mixing off), 100 ms quiet time"""
    made = {}

    def get(shape):
        if shape not in made:
            c = KC.case(shape)
            eng = spf_amd.Engine(G.engine_params(c.P))
            E.load_keys(eng, c)
            on = spf_amd.Pool(eng, max_batch=64, max_wait_us=100_000)
            on.set_mixed_parameters(True)
            made[shape] = (c, eng, on, spf_amd.Pool(eng, max_batch=64, max_wait_us=100_000))
        return made[shape]

    yield get
    gc.collect()
    for _, eng, on, off in made.values():
        on.close()
        off.close()
        eng.close()


def push_all(pool, vals, todo):
    """every (operand index, op, param) of `todo` pushed without a ticket; the last value of every kind is waited for"""
    outs = [pool.push_v(op, [vals[i]], param) for i, op, param in todo]
    for op in {op for _, op, _ in todo}:
        [v for v, (_, o, _) in zip(outs, todo) if o == op][-1].wait()
    return outs


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_interleaved_rounds_and_slots_are_two_launches(rigs, shape):
    c, eng, on, off = rigs(shape)
    start = on.value_stats()["live_values"], off.value_stats()["live_values"]
    todo = [(i, op, param) for i in OPERANDS for op, param in plan_of(c)]
    results = {}
    for pool in (on, off):
        vals = pool.upload_batch(GLWE, np.ascontiguousarray(c.x).reshape(B, -1))
        before = pool.counters()
        outs = push_all(pool, vals, todo)
        after = pool.counters()
        assert after["handle_ops"] - before["handle_ops"] == 4 * B
        # one launch per kind with mixing; without it every switch of the parameter opens another batch
        assert after["handle_launches"] - before["handle_launches"] == (2 if pool is on else 4 * B), shape
        if pool is on:
            assert eng.last_glwe_keyswitch_kernel() == E.EACH_KERNEL[shape == TUNED]
        results[pool] = pool.download_batch(outs)
        assert G.same_words(pool.download_batch(vals), c.x)                      # the operands are unchanged
        for v in outs + vals:
            v.release()
    assert G.same_words(results[on], results[off]), shape
    for row, (i, op, param) in zip(results[on], todo):
        assert G.same_words(row, oracle(shape, op, param, i)), (shape, i, op, param)
    assert (on.value_stats()["live_values"], off.value_stats()["live_values"]) == start


@pytest.mark.parametrize("shape", [TUNED, SMALL])
@pytest.mark.parametrize("op", [SE, MX], ids=["sample-extract", "mul-xn"])
def test_distinct_indices_and_amounts_are_one_launch(rigs, shape, op):
    c, eng, on, off = rigs(shape)
    N = c.P.N
    params = [0, 1, N - 1, 5, N // 2] if op == SE else [0, N + 77, 2 * N - 1, 1, 4 * N + 3]
    todo = [(i, op, p) for i, p in zip(OPERANDS, params)]
    start = on.value_stats()["live_values"]
    results = {}
    for pool in (on, off):
        vals = pool.upload_batch(GLWE, np.ascontiguousarray(c.x).reshape(B, -1))
        before = pool.counters()
        outs = push_all(pool, vals, todo)
        after = pool.counters()
        assert (after["handle_ops"] - before["handle_ops"], after["handle_launches"] - before["handle_launches"]) == (B, 1 if pool is on else B)
        results[pool] = pool.download_batch(outs)
        for v in outs + vals:
            v.release()
    assert G.same_words(results[on], results[off])
    for row, (i, _, p) in zip(results[on], todo):
        assert G.same_words(row, oracle(shape, op, p % (2 * N), i)), (shape, op, i, p)
    assert on.value_stats()["live_values"] == start


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_by_host_pointer_the_same_launch_counts(rigs, shape):
    c, eng, _, _ = rigs(shape)
    lib, N = eng._lib, c.P.N
    x = np.ascontiguousarray(c.x)
    plan = plan_of(c)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # the interleaved pattern: 2 B operations of each kind fill one batch of each kind
    hp = spf_amd.Pool(eng, max_batch=2 * B, max_wait_us=100_000)
    hp.set_mixed_parameters(True)
    try:
        res = np.zeros((B, len(plan)) + x.shape[1:], dtype=U)
        tickets = []
        for n, i in enumerate(OPERANDS):
            for j, (op, param) in enumerate(plan):
                t = C.c_uint64()
                fn = lib.spf_pool_submit_glwe_keyswitch if op == KS else lib.spf_pool_submit_glwe_automorphism
                assert fn(hp._h, param, ptr(x[i]), ptr(res[n, j]), C.byref(t)) == 0
                tickets.append(t.value)
        for t in tickets:
            hp.wait(t)
        assert hp.stats() == (4 * B, 2), shape
        for n, i in enumerate(OPERANDS):
            for j, (op, param) in enumerate(plan):
                assert G.same_words(res[n, j], oracle(shape, op, param, i)), (shape, i, op, param)
    finally:
        hp.close()
    # B distinct indices, then B distinct amounts: one launch each
    hp = spf_amd.Pool(eng, max_batch=B, max_wait_us=100_000)
    hp.set_mixed_parameters(True)
    try:
        idx, amounts = [0, 1, N - 1, 5, N // 2], [0, N + 77, 2 * N - 1, 1, 4 * N + 3]
        lwes = np.zeros((B, c.P.k * N + 1), dtype=U)
        rot = np.zeros((B,) + x.shape[1:], dtype=U)
        tickets = []
        for n, i in enumerate(OPERANDS):
            t = C.c_uint64()
            assert lib.spf_pool_submit_sample_extract(hp._h, ptr(x[i]), idx[n], ptr(lwes[n]), C.byref(t)) == 0
            tickets.append(t.value)
        for n, i in enumerate(OPERANDS):
            t = C.c_uint64()
            assert lib.spf_pool_submit_mul_xn(hp._h, ptr(x[i]), amounts[n], ptr(rot[n]), C.byref(t)) == 0
            tickets.append(t.value)
        for t in tickets:
            hp.wait(t)
        assert hp.stats() == (2 * B, 2), shape
        for n, i in enumerate(OPERANDS):
            assert G.same_words(lwes[n], oracle(shape, SE, idx[n], i)) and G.same_words(rot[n], oracle(shape, MX, amounts[n] % (2 * N), i)), (shape, n)
    finally:
        hp.close()


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_a_chain_on_pending_operands_with_a_parameter_per_caller_runs_behind_one_wait(rigs, shape):
    """MulXN(x_j, n_j) -> automorphism(round_j) -> SampleExtract(idx_j) for three callers' worth of parameters, pushed level by level"""
    c, eng, on, _ = rigs(shape)
    P, log_n = c.P, KC.log2n(c.P)
    start = on.value_stats()["live_values"]
    amounts, rounds, idx = [3, P.N + 1, 2 * P.N - 2], [1, log_n, 2], [P.N - 1, 0, 7]
    vals = [on.upload(GLWE, c.x[j]) for j in range(3)]
    before = on.counters()
    m = [on.push_v(MX, [vals[j]], amounts[j]) for j in range(3)]
    a = [on.push_v(AU, [m[j]], rounds[j]) for j in range(3)]
    s = [on.push_v(SE, [a[j]], idx[j]) for j in range(3)]
    assert not any(v.info()["valid"] for v in a + s)                              # nothing of the pending levels is valid before the single wait
    s[-1].wait()
    assert all(v.info()["valid"] for v in a + s)
    after = on.counters()
    # the first level has valid operands and sits in its lane; the two pending levels are one deferred batch each
    assert after["handle_ops"] - before["handle_ops"] == 9 and after["handle_launches"] - before["handle_launches"] == 3
    for j in range(3):
        w_m = O.glwe_mul_xn(c.x[j].reshape(-1), amounts[j], P.N, P.k)
        w_a = KC.oracle_round(c, np.asarray(w_m, dtype=U).reshape(P.k + 1, P.N), rounds[j])
        assert G.same_words(m[j].wait().download(), w_m), (shape, j)
        assert G.same_words(a[j].download(), w_a), (shape, j)
        assert G.same_words(s[j].download(), O.sample_extract(np.asarray(w_a, dtype=U).reshape(-1), idx[j], P.N, P.k)), (shape, j)
    for v in m + a + s + vals:
        v.release()
    assert on.value_stats()["live_values"] == start


def test_the_setter_is_refused_after_a_submit(rigs):
    c, eng, on, off = rigs(SMALL)
    v = off.upload(GLWE, c.x[0])
    r = off.push_v(MX, [v], 1).wait()
    w = on.upload(GLWE, c.x[0])
    on.push_v(MX, [w], 1).wait().release()
    w.release()
    for pool in (on, off):
        with pytest.raises(SpfError) as e:
            pool.set_mixed_parameters(pool is off)
        assert e.value.status == 1
    # `off` is still off: two amounts are two launches
    before = off.counters()
    outs = push_all(off, [v], [(0, MX, 1), (0, MX, 2)])
    assert off.counters()["handle_launches"] - before["handle_launches"] == 2
    for x in outs + [r, v]:
        x.release()
    fresh = spf_amd.Pool(eng, max_batch=8, max_wait_us=100_000)                  # before any submit: on, off and on again are all legal
    try:
        fresh.set_mixed_parameters(True)
        fresh.set_mixed_parameters(False)
        fresh.set_mixed_parameters(True)
    finally:
        fresh.close()


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_a_group_pool_applies_it_to_every_member(shape):
    c = KC.case(shape)
    grp = spf_amd.Group(G.engine_params(c.P), devices=[0, 0])
    gpool = None
    try:
        E.load_keys(grp, c)
        gpool = spf_amd.Pool(grp, max_batch=64, max_wait_us=100_000)
        gpool.set_mixed_parameters(True)
        start = gpool.value_stats()["live_values"]
        vals = [gpool.upload(GLWE, c.x[i], member=i % 2) for i in range(B)]
        todo = [(i, op, param) for i in range(B) for op, param in plan_of(c)]
        before = gpool.counters()
        outs = [gpool.push_v(op, [vals[i]], param) for i, op, param in todo]
        for member in (0, 1):                                                     # one wait per member and kind closes that member's batch
            for kind in (KS, AU):
                [v for v, (i, op, _) in zip(outs, todo) if op == kind and i % 2 == member][-1].wait()
        after = gpool.counters()
        assert after["handle_ops"] - before["handle_ops"] == 4 * B
        assert after["handle_launches"] - before["handle_launches"] == 4              # two kinds on each of the two members
        for v, (i, op, param) in zip(outs, todo):
            assert G.same_words(v.download(), oracle(shape, op, param, i)), (shape, i, op, param)
        for v in outs + vals:
            v.release()
        assert gpool.value_stats()["live_values"] == start
        with pytest.raises(SpfError):
            gpool.set_mixed_parameters(False)
    finally:
        if gpool is not None:
            gpool.close()
        grp.close()
