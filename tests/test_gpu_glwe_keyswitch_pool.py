"""The GLWE keyswitch, one automorphism round and the homomorphic trace in the pool — by host pointer
(`spf_pool_submit_glwe_keyswitch` / `_automorphism` / `_trace`), by handle (`..._v`, `spf_pool_submit_op_v` with
`SPF_OP_GLWE_*`), on a group pool — and behind the generic door of the gate graphs (`spf_graph_add_op`).

Three rigs: DEFAULT_128 under a 6 x 7 key (the hand-written kernels), the same context under the `OTHER_RADIX` key (the generic
kernels on a tuned context), and `N16`, a generic context.  Every comparison is word for word: against the oracle
(tests/glwe_keyswitch_cases.py) and against the engine's `_batch` call on the same rows.  There is no tolerance in this file; the
one decryption check is the reference's `can_trace` at 12 plaintext bits.

The batch is `glwe_keyswitch_cases.ITEMS` = 5: one full workgroup of four GLWEs of the tuned kernels plus a ragged one with padding
units, the smallest size at which their unit indexing can go wrong; and B = 1.  The pools by handle have a quiet time of 100 ms
that no test waits out: what one thread pushes is closed by the wait for a value, as ONE batch."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as G
from tests.util import random_lwe_batch

pytestmark = pytest.mark.gpu
GLWE = ValueKind.GLWE1
U = np.uint64
INVALID, NO_KEY = 1, 3
TUNED, SMALL = G.TUNED, "N16"
KEY_SLOT, SECOND_SLOT, OTHER_SLOT, RELOAD_SLOT, EMPTY_SLOT = 0, 1, 2, 5, 12
KS, AU, TR = FheOp.GLWE_KEYSWITCH, FheOp.GLWE_AUTOMORPHISM, FheOp.GLWE_TRACE
B = KC.ITEMS


def load_keys(eng, c):
    """the automorphism key; slot 0: sk_a -> sk_b at the trace radix, slot 1: `second_key`, slot 2 (tuned): the OTHER_RADIX key"""
    P = c.P
    eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
    eng.load_glwe_keyswitch_key_std(KEY_SLOT, c.ksk, P.tr_radix_log, P.tr_count)
    eng.load_glwe_keyswitch_key_std(SECOND_SLOT, KC.second_key(c)[0], P.tr_radix_log, P.tr_count)
    if c.name == TUNED:
        eng.load_glwe_keyswitch_key_std(OTHER_SLOT, KC.other_radix_key(c)[0], *KC.OTHER_RADIX)


def slot_fft(c, slot):
    """(spectra, radix) of the key load_keys puts in `slot`"""
    radix = (c.P.tr_radix_log, c.P.tr_count)
    return {KEY_SLOT: (c.ksk_fft, radix), SECOND_SLOT: (KC.second_key(c)[1], radix), RELOAD_SLOT: (c.ksk_fft, radix),
            OTHER_SLOT: (KC.other_radix_key(c)[1], KC.OTHER_RADIX)}[slot]


def oracle_op(c, op, param, x):
    """the oracle's words of one operation on GLWEs (k+1, N) or (n, k+1, N)"""
    x = np.asarray(x, dtype=U)
    if x.ndim == 3:
        return np.stack([oracle_op(c, op, param, g) for g in x])
    x = x.reshape(c.P.k + 1, c.P.N)
    if op == KS:
        return KC.oracle_keyswitch(c.P, x, *slot_fft(c, param))
    if op == AU:
        return KC.oracle_round(c, x, param)
    return G.oracle_trace(c, x)


@functools.lru_cache(maxsize=None)
def want(shape, op, param):
    """the oracle on the case's five GLWEs, computed once in a process and shared by the tests: (ITEMS, k+1, N)"""
    c = KC.case(shape)
    out = KC.oracle_traces(shape) if op == TR else oracle_op(c, op, param, c.x)
    out = np.array(out)
    out.setflags(write=False)
    return out


def modes(shape):
    """(id, shape, op, param, served by the hand-written kernels): the three operations on both contexts, and the other radix"""
    out = [("keyswitch", shape, KS, KEY_SLOT, shape == TUNED), ("automorphism", shape, AU, 2, shape == TUNED), ("trace", shape, TR, 0, shape == TUNED)]
    if shape == TUNED:
        out.append(("keyswitch-other-radix", shape, KS, OTHER_SLOT, False))
    return out


DRAWN = [pytest.param(s, op, param, tuned, id=f"{s}-{name}") for shape in (TUNED, SMALL) for name, s, op, param, tuned in modes(shape)]


def engine_batch(eng, op, param, x):
    x = np.ascontiguousarray(x, dtype=U)
    return eng.glwe_keyswitch(param, x) if op == KS else eng.glwe_automorphism(param, x) if op == AU else eng.glwe_trace(x)


@pytest.fixture(scope="module")
def rigs():
    """shape -> (case, engine with load_keys, pool by handle with a 100 ms quiet time), made when a test first asks"""
    made = {}

    def get(shape):
        if shape not in made:
            c = KC.case(shape)
            eng = spf_amd.Engine(G.engine_params(c.P))
            load_keys(eng, c)
            made[shape] = (c, eng, spf_amd.Pool(eng, max_batch=64, max_wait_us=100_000))
        return made[shape]

    yield get
    gc.collect()
    for _, eng, pool in made.values():
        pool.close()
        eng.close()


def same(got, want_words):
    return G.same_words(got, want_words)


def named_push(pool, op, param, v):
    """the named `_v` submit without a ticket"""
    return pool.glwe_keyswitch_v(param, v, wait=False) if op == KS else pool.glwe_automorphism_v(param, v, wait=False) if op == AU else pool.glwe_trace_v(v, wait=False)


def scattered_uploads(pool, c):
    """the case's GLWEs uploaded one at a time with other uploads in between, then taken by DESCENDING address — wherever the
    allocator put them, no operand row then lies behind the one before: (values in that order, their item numbers, the values in
    between, kept alive)"""
    P = c.P
    lwe = random_lwe_batch(0x5CA, 1, P.k * P.N)[0]
    vals, between = [], []
    for i, row in enumerate(c.x):
        vals.append(pool.upload(GLWE, row))
        between.append(pool.upload(ValueKind.LWE1, lwe) if i % 2 else pool.upload(GLWE, c.x[(i + 1) % B]))
    order = sorted(range(B), key=lambda i: -vals[i].device_ptr())
    vals = [vals[i] for i in order]
    ptrs = [v.device_ptr() for v in vals]
    gb = 8 * (P.k + 1) * P.N
    assert all(ptrs[i + 1] != ptrs[i] + gb for i in range(B - 1)) and len(set(ptrs)) == B, ptrs     # no two operand rows are consecutive
    return vals, order, between


# ---- 1. by host pointer -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,op,param,tuned", DRAWN)
def test_by_host_pointer_five_submits_then_the_waits(rigs, shape, op, param, tuned):
    c, eng, _ = rigs(shape)
    lib = eng._lib
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    try:
        for n in (B, 1):
            x = np.ascontiguousarray(c.x[:n])
            out = np.zeros_like(x)
            tickets = []
            for i in range(n):
                t = C.c_uint64()
                xi, oi = x[i].ctypes.data_as(C.c_void_p), out[i].ctypes.data_as(C.c_void_p)
                if op == KS:
                    st = lib.spf_pool_submit_glwe_keyswitch(pool._h, param, xi, oi, C.byref(t))
                elif op == AU:
                    st = lib.spf_pool_submit_glwe_automorphism(pool._h, param, xi, oi, C.byref(t))
                else:
                    st = lib.spf_pool_submit_glwe_trace(pool._h, xi, oi, C.byref(t))
                assert st == 0, lib.spf_last_error(eng._h)
                tickets.append(t.value)
            for t in tickets:
                pool.wait(t)
            assert same(out, want(shape, op, param)[:n]), (shape, op, n)
            assert same(out, engine_batch(eng, op, param, x)), (shape, op, n)
            assert same(x, c.x[:n])                                               # the inputs are the caller's: untouched
        one = np.zeros_like(c.x[3])                                               # the synchronous wrappers of the binding
        if op == KS:
            pool.glwe_keyswitch(one, c.x[3], param)
        elif op == AU:
            pool.glwe_automorphism(one, c.x[3], param)
        else:
            pool.glwe_trace(one, c.x[3])
        assert same(one, want(shape, op, param)[3])
    finally:
        pool.close()


# ---- 2. / 3. / 4. by handle: scattered, consecutive, one value five times --------------------------------------------------------------

@pytest.mark.parametrize("shape,op,param,tuned", DRAWN)
def test_by_handle_scattered_operands_are_one_launch_of_a_rows_kernel(rigs, shape, op, param, tuned):
    c, eng, pool = rigs(shape)
    start = pool.value_stats()["live_values"]
    vals, order, between = scattered_uploads(pool, c)
    before = pool.counters()
    outs = [pool.push_v(op, [v], param) for v in vals]                            # the generic door, no ticket
    assert not any(o.info()["valid"] for o in outs)
    outs[-1].wait()
    assert eng.last_glwe_keyswitch_kernel() == G.ROWS[tuned], shape
    after = pool.counters()
    assert (after["handle_ops"] - before["handle_ops"], after["handle_launches"] - before["handle_launches"]) == (B, 1)
    got = pool.download_batch(outs)
    assert same(got, want(shape, op, param)[order]) and same(got, engine_batch(eng, op, param, c.x[order])), shape
    out_ptrs = [o.device_ptr() for o in outs]
    gb = 8 * (c.P.k + 1) * c.P.N
    assert all(out_ptrs[i] == out_ptrs[0] + i * gb for i in range(B))             # one fresh block ...
    for p in [v.device_ptr() for v in vals]:                                      # ... that overlaps no operand
        assert p + gb <= out_ptrs[0] or out_ptrs[0] + B * gb <= p
    assert same(pool.download_batch(vals), c.x[order])                            # the operands are unchanged
    # the named submits, with tickets, give the same words
    named = [named_push(pool, op, param, v) for v in vals]
    named[0].wait()
    assert same(pool.download_batch(named), got)
    for v in outs + named + vals + between:
        v.release()
    assert pool.value_stats()["live_values"] == start


@pytest.mark.parametrize("shape,op,param,tuned", DRAWN)
def test_by_handle_consecutive_operands_go_to_the_in_place_kernel(rigs, shape, op, param, tuned):
    c, eng, pool = rigs(shape)
    start = pool.value_stats()["live_values"]
    for n in (B, 1):
        vals = pool.upload_batch(GLWE, np.ascontiguousarray(c.x[:n]).reshape(n, -1))
        gb = 8 * (c.P.k + 1) * c.P.N
        ptrs = [v.device_ptr() for v in vals]
        assert all(ptrs[i] == ptrs[0] + i * gb for i in range(n))
        before = pool.counters()
        outs = [pool.push_v(op, [v], param) for v in vals]
        outs[0].wait()
        assert eng.last_glwe_keyswitch_kernel() == G.IN_PLACE[tuned], (shape, n)
        after = pool.counters()
        assert (after["handle_ops"] - before["handle_ops"], after["handle_launches"] - before["handle_launches"]) == (n, 1)
        got = pool.download_batch(outs)
        assert same(got, want(shape, op, param)[:n]), (shape, n)                  # (the words of the scattered case: both equal the oracle's)
        assert same(pool.download_batch(vals), c.x[:n])
        for v in outs + vals:
            v.release()
    # B = 1 through the blocking door: one operand alone lies consecutively
    v = pool.upload(GLWE, c.x[2])
    r = pool.run_v(op, [v], param)
    assert eng.last_glwe_keyswitch_kernel() == G.IN_PLACE[tuned]
    assert same(r.download(), want(shape, op, param)[2])
    r.release()
    v.release()
    assert pool.value_stats()["live_values"] == start


@pytest.mark.parametrize("shape,op,param,tuned", DRAWN)
def test_one_value_five_times_in_one_batch(rigs, shape, op, param, tuned):
    c, eng, pool = rigs(shape)
    start = pool.value_stats()["live_values"]
    v = pool.upload(GLWE, c.x[4])
    before = pool.counters()
    outs = [pool.push_v(op, [v], param) for _ in range(B)]                        # the same pointer five times in the table
    outs[2].wait()
    after = pool.counters()
    assert (after["handle_ops"] - before["handle_ops"], after["handle_launches"] - before["handle_launches"]) == (B, 1)
    assert eng.last_glwe_keyswitch_kernel() == G.ROWS[tuned]
    got = pool.download_batch(outs)
    for j in range(B):
        assert same(got[j], want(shape, op, param)[4]), (shape, j)
    assert same(v.download(), c.x[4])
    for o in outs + [v]:
        o.release()
    assert pool.value_stats()["live_values"] == start


# ---- 5. pending operands ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_a_chain_on_pending_operands_runs_behind_one_wait(rigs, shape):
    """MulXN(x, 2N - 3) -> trace -> SampleExtract(0); on the trace's pending result a keyswitch under slot 0, then one under slot 1"""
    c, eng, pool = rigs(shape)
    P = c.P
    start = pool.value_stats()["live_values"]
    ones = KC.all_ones_glwe(c)                                                    # every coefficient 1: X^-3 * ones traces to N at coefficient 0
    vx = pool.upload(GLWE, ones)
    m = pool.push_v(FheOp.MulXN, [vx], 2 * P.N - 3)
    t = pool.push_v(TR, [m])
    se = pool.push_v(FheOp.SampleExtract, [t], 0)
    k0 = pool.glwe_keyswitch_v(KEY_SLOT, t, wait=False)
    k1 = pool.push_v(KS, [k0], SECOND_SLOT)
    chain = [m, t, se, k0, k1]
    assert not any(v.info()["valid"] for v in chain)                             # nothing is valid before the single wait
    k1.wait()
    assert all(v.info()["valid"] for v in (t, se, k0, k1))
    w_m = O.glwe_mul_xn(ones.reshape(-1), 2 * P.N - 3, P.N, P.k)
    w_t = G.oracle_trace(c, w_m)
    w_k0 = oracle_op(c, KS, KEY_SLOT, w_t)
    assert same(t.download(), w_t) and same(t.download(), eng.glwe_trace(np.asarray(w_m, dtype=U).reshape(1, P.k + 1, P.N)))
    assert same(se.download(), O.sample_extract(w_t.reshape(-1), 0, P.N, P.k))
    assert same(k0.download(), w_k0)
    assert same(k1.download(), oracle_op(c, KS, SECOND_SLOT, w_k0))
    assert same(m.wait().download(), w_m)
    KC.check_can_trace(c, t.download(), "pool, pending chain")
    for v in chain + [vx]:
        v.release()
    assert pool.value_stats()["live_values"] == start


# ---- 6. parameters kept apart -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_rounds_and_slots_submitted_interleaved_never_share_a_launch(rigs, shape):
    c, eng, pool = rigs(shape)
    log_n = KC.log2n(c.P)
    start = pool.value_stats()["live_values"]
    vals = pool.upload_batch(GLWE, np.ascontiguousarray(c.x).reshape(B, -1))
    plan = [(AU, 1), (KS, KEY_SLOT), (AU, log_n), (KS, SECOND_SLOT)]
    before = pool.counters()
    outs, tickets = [], []
    for i in range(B):                                                           # item i under every parameter in turn, before any wait
        for op, param in plan:
            v, t = pool.submit_v(op, [vals[i]], param)
            outs.append((i, op, param, v))
            tickets.append(t)
    for t in tickets:
        pool.wait(t)
    after = pool.counters()
    assert after["handle_ops"] - before["handle_ops"] == 4 * B
    assert after["handle_launches"] - before["handle_launches"] == 4 * B            # a batch holds ONE parameter: every switch opens another
    for i, op, param, v in outs:
        assert same(v.download(), want(shape, op, param)[i]), (shape, i, op, param)
        v.release()
    # by host pointer the same way, from one thread, all tickets before any wait (three items: every submit is a batch of its own
    # and holds a staging set until it is collected, and there are sixteen)
    hp = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    try:
        x = np.ascontiguousarray(c.x[:3])
        res = np.zeros((len(plan),) + x.shape, dtype=U)
        tickets = []
        for i in range(3):
            for j, (op, param) in enumerate(plan):
                t = C.c_uint64()
                fn = eng._lib.spf_pool_submit_glwe_keyswitch if op == KS else eng._lib.spf_pool_submit_glwe_automorphism
                assert fn(hp._h, param, x[i].ctypes.data_as(C.c_void_p), res[j, i].ctypes.data_as(C.c_void_p), C.byref(t)) == 0
                tickets.append(t.value)
        for t in tickets:
            hp.wait(t)
        for j, (op, param) in enumerate(plan):
            assert same(res[j], want(shape, op, param)[:3]), (shape, op, param)
    finally:
        hp.close()
    for v in vals:
        v.release()
    assert pool.value_stats()["live_values"] == start


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_refusals_create_no_value_and_take_no_ticket(rigs, shape):
    c, eng, pool = rigs(shape)
    lib = eng._lib
    log_n = KC.log2n(c.P)
    other = spf_amd.Pool(eng, max_batch=64, max_wait_us=200)
    bare = spf_amd.Engine(G.engine_params(KC.case(SMALL).P))                      # no key at all
    bare_pool = spf_amd.Pool(bare, max_batch=64, max_wait_us=200)
    try:
        v = pool.upload(GLWE, c.x[0])
        l1 = pool.upload(ValueKind.LWE1, random_lwe_batch(0x7E, 1, c.P.k * c.P.N)[0])
        foreign = other.upload(GLWE, c.x[0])
        before = (pool.value_stats()["live_values"], pool.counters()["handle_ops"], pool.counters()["ops"])
        x = np.ascontiguousarray(c.x[0])
        out = np.zeros_like(x)
        xp, op_ = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

        def by_handle(fn, *args):
            h, t = C.c_void_p(), C.c_uint64(77)
            st = fn(pool._h, *args, C.byref(h), C.byref(t))
            assert not h.value and t.value == 77, (st, h.value, t.value)          # the handle stays null, no ticket is taken
            return st

        def generic(op, operand, param):
            arr = (C.c_void_p * 1)(operand._h)
            return by_handle(lambda p, *a: lib.spf_pool_submit_op_v(p, int(op), arr, 1, param, *a))

        def by_pointer(fn, *args):
            t = C.c_uint64(77)
            st = fn(pool._h, *args, xp, op_, C.byref(t))
            assert t.value == 77 and not out.any()
            return st

        def message():
            return lib.spf_last_error(eng._h).decode()

        # the slot and the round: through the named door, the generic door and by host pointer
        assert by_handle(lib.spf_pool_submit_glwe_keyswitch_v, 16, v._h) == INVALID and "slot 16 >= SPF_GLWE_KSK_SLOTS = 16" in message()
        assert generic(KS, v, 16) == INVALID and "slot 16" in message()
        assert generic(KS, v, 1 << 32) == INVALID and "4294967296" in message()   # (not truncated to slot 0)
        assert by_pointer(lib.spf_pool_submit_glwe_keyswitch, 16) == INVALID
        for rnd in (0, log_n + 1):
            assert by_handle(lib.spf_pool_submit_glwe_automorphism_v, rnd, v._h) == INVALID and f"round {rnd} outside 1 .. log2 N = {log_n}" in message()
            assert generic(AU, v, rnd) == INVALID and f"round {rnd} outside" in message()
            assert by_pointer(lib.spf_pool_submit_glwe_automorphism, rnd) == INVALID
        # an empty slot
        assert by_handle(lib.spf_pool_submit_glwe_keyswitch_v, EMPTY_SLOT, v._h) == NO_KEY and f"slot {EMPTY_SLOT}" in message()
        assert generic(KS, v, EMPTY_SLOT) == NO_KEY
        assert by_pointer(lib.spf_pool_submit_glwe_keyswitch, EMPTY_SLOT) == NO_KEY
        # an operand of the wrong kind, a null operand, an operand homed in another pool
        for fn, lead in ((lib.spf_pool_submit_glwe_keyswitch_v, (KEY_SLOT,)), (lib.spf_pool_submit_glwe_automorphism_v, (1,)), (lib.spf_pool_submit_glwe_trace_v, ())):
            assert by_handle(fn, *lead, l1._h) == INVALID and "wrong ciphertext type" in message()
            assert by_handle(fn, *lead, None) == INVALID and "null operand" in message()
            assert by_handle(fn, *lead, foreign._h) == INVALID and "another pool" in message()
        for op, param in ((KS, KEY_SLOT), (AU, 1), (TR, 0)):
            assert generic(op, l1, param) == INVALID and generic(op, foreign, param) == INVALID
        assert (pool.value_stats()["live_values"], pool.counters()["handle_ops"], pool.counters()["ops"]) == before
        # the binding raises with the status
        for call, status in ((lambda: pool.glwe_keyswitch_v(16, v), INVALID), (lambda: pool.run_v(AU, [v], 0), INVALID),
                             (lambda: pool.glwe_keyswitch_v(EMPTY_SLOT, v), NO_KEY), (lambda: pool.glwe_keyswitch(out, x, EMPTY_SLOT), NO_KEY)):
            with pytest.raises(spf_amd.SpfError) as e:
                call()
            assert e.value.status == status, (status, e.value.status)
        # no automorphism key: the trace and a round are SPF_ERR_NO_KEY, a keyswitch on an empty slot too
        bv = bare_pool.upload(GLWE, KC.case(SMALL).x[0])
        for call in (lambda: bare_pool.glwe_trace_v(bv), lambda: bare_pool.run_v(AU, [bv], 1), lambda: bare_pool.run_v(KS, [bv], 0)):
            with pytest.raises(spf_amd.SpfError) as e:
                call()
            assert e.value.status == NO_KEY
        assert bare_pool.value_stats()["live_values"] == 1
        bv.release()
        # ... and the pool still serves
        r = pool.glwe_keyswitch_v(KEY_SLOT, v)
        assert same(r.download(), want(shape, KS, KEY_SLOT)[0])
        for w in (r, v, l1, foreign):
            w.release()
    finally:
        gc.collect()
        bare_pool.close()
        bare.close()
        other.close()


# ---- 8. reload in the legal order --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_a_slot_reloaded_between_waits_serves_the_new_key(rigs, shape):
    c, eng, pool = rigs(shape)
    radix = (c.P.tr_radix_log, c.P.tr_count)
    eng.load_glwe_keyswitch_key_std(RELOAD_SLOT, c.ksk, *radix)
    vals, order, between = scattered_uploads(pool, c)
    first = [pool.push_v(KS, [v], RELOAD_SLOT) for v in vals]
    first[-1].wait()                                                              # submit, WAIT, then load: the legal order
    got_first = pool.download_batch(first)
    eng.load_glwe_keyswitch_key_std(RELOAD_SLOT, KC.second_key(c)[0], *radix)
    second = [pool.push_v(KS, [v], RELOAD_SLOT) for v in vals]
    second[-1].wait()
    assert same(got_first, want(shape, KS, KEY_SLOT)[order])                      # (slot 0 holds the first key, slot 1 the second)
    assert same(pool.download_batch(second), want(shape, KS, SECOND_SLOT)[order])
    assert not same(got_first, want(shape, KS, SECOND_SLOT)[order]), "the two keys give the same words: the case proves nothing"
    for v in first + second + vals + between:
        v.release()


# ---- 9. graphs -----------------------------------------------------------------------------------------------------------------------------

def door_graph(g, c, door, picks):
    """keyswitches over scattered inputs, a round over consecutive ones, traces over the keyswitches' rows, a keyswitch of a trace:
    through spf_graph_add_op (`door`) or through the named constructors"""
    ins = [g.add_input(GLWE, row) for row in c.x]

    def node(op, param, n):
        if door:
            return g.add_op(op, [n], param)
        return g.add_glwe_keyswitch(param, n) if op == KS else g.add_glwe_automorphism(param, n) if op == AU else g.add_glwe_trace(n)

    ks = [node(KS, KEY_SLOT, ins[i]) for i in picks]
    au = [node(AU, 2, n) for n in ins]
    tr = [node(TR, 0, n) for n in ks]
    last = node(KS, SECOND_SLOT, tr[0])
    return [g.add_output(n, GLWE) for n in ks + au + tr + [last]]


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_the_generic_door_of_a_graph_gives_the_named_constructors_words(rigs, shape):
    c, eng, _ = rigs(shape)
    picks = [4, 0, 4, 2, 1]
    results = {}
    for door in (False, True):
        g = spf_amd.FheCircuit(eng)
        outs = door_graph(g, c, door, picks)
        g.run()
        results[door] = (np.stack(outs).copy(), g.stats())
        g.close()
    assert results[True][1] == results[False][1], results
    assert results[True][1]["levels"] == 3 and results[True][1]["nodes"] == B + 3 * B + 1
    assert same(results[True][0], results[False][0])
    got = results[True][0]
    assert same(got[:B], want(shape, KS, KEY_SLOT)[picks]) and same(got[B:2 * B], want(shape, AU, 2))
    assert same(got[2 * B], G.oracle_trace(c, got[0]))
    # refusals of the door: the table's texts, nothing recorded
    g = spf_amd.FheCircuit(eng)
    a = g.add_input(GLWE, c.x[0])
    l1 = g.add_input(ValueKind.LWE1, random_lwe_batch(0x9A, 1, c.P.k * c.P.N)[0])
    log_n = KC.log2n(c.P)
    for call, word in ((lambda: g.add_op(KS, [a], 16), "slot 16 >= SPF_GLWE_KSK_SLOTS = 16"), (lambda: g.add_op(AU, [a], 0), f"round 0 outside 1 .. log2 N = {log_n}"),
                       (lambda: g.add_op(AU, [a], log_n + 1), f"round {log_n + 1} outside"), (lambda: g.add_op(TR, [a, a]), "unknown operation: value 14 over 2 operands (the GLWE keyswitch, automorphism round and trace take one GLWE1)"),
                       (lambda: g.add_op(KS, [], 0), "unknown operation: value 12 over 0 operands"),
                       (lambda: g.add_op(TR, [l1]), "not an L1 GLWE"), (lambda: g.add_op(KS, [7], 0), "not a node")):
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == INVALID and word in str(e.value), (word, str(e.value))
        assert g.stats()["nodes"] == 2
    g.close()


def test_two_jobs_of_a_group_through_the_generic_door(rigs):
    c, eng, _ = rigs(SMALL)
    all_picks = ([4, 0, 4, 2, 1], [1, 3, 2, 2, 0])
    alone = []
    for picks in all_picks:
        g = spf_amd.FheCircuit(eng)
        outs = door_graph(g, c, False, picks)
        g.run()
        alone.append(np.stack(outs).copy())
        g.close()
    grp = spf_amd.Group(G.engine_params(c.P), devices=[0, 0])
    jobs = []
    try:
        load_keys(grp, c)
        for picks in all_picks:
            g = spf_amd.FheCircuit(grp)
            jobs.append((g, door_graph(g, c, True, picks)))
        grp.run_graphs([g for g, _ in jobs])
        for j, (_, outs) in enumerate(jobs):
            assert same(np.stack(outs), alone[j]), j
    finally:
        for g, _ in jobs:
            g.close()
        grp.close()


# ---- 10. group pool --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_a_group_pool_deals_the_three_operations_over_both_members(shape):
    c = KC.case(shape)
    grp = spf_amd.Group(G.engine_params(c.P), devices=[0, 0])
    gpool = None
    try:
        load_keys(grp, c)
        gpool = spf_amd.Pool(grp, max_batch=64, max_wait_us=2000)   # (its host-pointer calls below close on the quiet time)
        start = gpool.value_stats()["live_values"]
        for op, param in ((KS, KEY_SLOT), (AU, 2), (TR, 0)):
            vals = [gpool.upload(GLWE, c.x[i], member=i % 2) for i in range(B)]
            assert [v.info()["member"] for v in vals] == [i % 2 for i in range(B)]
            outs = [gpool.push_v(op, [v], param) for v in vals]
            for o in outs[-2:]:                                                  # one wait per member closes that member's batch
                o.wait()
            assert [o.info()["member"] for o in outs] == [i % 2 for i in range(B)]
            for i, o in enumerate(outs):
                assert same(o.wait().download(), want(shape, op, param)[i]), (shape, op, i)
            named = [named_push(gpool, op, param, v) for v in vals]
            for i, o in enumerate(named):
                assert same(o.wait().download(), want(shape, op, param)[i]), (shape, op, i)
            for v in outs + named + vals:
                v.release()
        # by host pointer the calling thread is dealt to one member
        out = np.zeros_like(c.x[1])
        gpool.glwe_keyswitch(out, c.x[1], SECOND_SLOT)
        assert same(out, want(shape, KS, SECOND_SLOT)[1])
        gpool.glwe_trace(out, c.x[1])
        assert same(out, want(shape, TR, 0)[1])
        # a refused submit on a group pool: no value, on either member
        v = gpool.upload(GLWE, c.x[0], member=1)
        for call, status in ((lambda: gpool.glwe_keyswitch_v(EMPTY_SLOT, v), NO_KEY), (lambda: gpool.glwe_automorphism_v(0, v), INVALID)):
            with pytest.raises(spf_amd.SpfError) as e:
                call()
            assert e.value.status == status
        v.release()
        assert gpool.value_stats()["live_values"] == start
    finally:
        gc.collect()
        if gpool is not None:
            gpool.close()
        grp.close()
