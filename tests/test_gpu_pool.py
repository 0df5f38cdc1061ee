"""The call-coalescing pool: many threads call single-ciphertext operations the way
the reference's rayon tasks call `Evaluation` (circuit_processor/mod.rs:192-253); the pool must
return exactly what the batch entry points return, and must actually coalesce."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests.util import keyset, random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu

SMALL_N = 12


@pytest.fixture(scope="module")
def rig():
    ks = keyset(0x5EED0001, SMALL_N)
    P = ks.params
    r = O.Rng(0x7A11)
    eng = spf_amd.Engine(to_engine_params(P))
    eng.load_bootstrap_key(ks.bsk_fft)
    eng.load_keyswitch_key(ks.ksk)
    eng.load_automorphism_key(O.gen_auto_key_fft(r, ks.glwe_sk, P))
    eng.load_scheme_switch_key(O.gen_ssk_fft(r, ks.glwe_sk, P))
    return ks, eng


def test_pool_matches_batch_entry_points_and_coalesces(rig):
    ks, eng = rig
    P = ks.params
    n_ops = 96
    lwe1 = random_lwe_batch(1, n_ops, P.N * P.k)
    a = random_glwe(2, n_ops, P.glwe_len)
    b = random_glwe(3, n_ops, P.glwe_len)
    # expected, through the ordinary batch entry points
    exp_ggsw = eng.circuit_bootstrap(eng.keyswitch_lwe_l1_lwe_l0(lwe1))
    exp_mux = eng.cmux(exp_ggsw, a, b)

    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=20000)
    ggsw = np.zeros((n_ops, eng.params.cbs_ggsw_complex), dtype=np.complex128)
    mux = np.zeros((n_ops, P.glwe_len), dtype=np.uint64)

    def gate(i):  # what one rayon task of the reference does: convert its bit, then use it
        pool.keyswitch_circuit_bootstrap(ggsw[i], lwe1[i])
        pool.cmux(mux[i], ggsw[i], a[i], b[i])
        return i

    with ThreadPoolExecutor(max_workers=48) as ex:
        assert sorted(ex.map(gate, range(n_ops))) == list(range(n_ops))
    ops, launches = pool.stats()
    pool.close()
    assert np.array_equal(ggsw.view(np.float64), exp_ggsw.view(np.float64))
    assert np.array_equal(mux, exp_mux)
    assert ops == 2 * n_ops
    assert launches < ops / 4, (ops, launches)   # it really batched


def test_pool_big_batches_leave_in_chunks_and_every_caller_gets_its_own_bytes(rig, monkeypatch):
    """A batch of more than 64 members copies its outputs out in several chunks, each with its own event and wake-up word
    (the callers of the first chunk copy out while the last is still crossing PCIe).  200 callers at once, twice in a row (the
    second round re-uses staging sets and words), every output against the batch entry point.  (One caller group, so that the
    200 meet in one batch: by default the pool deals callers to several groups that run side by side.)"""
    monkeypatch.setenv("SPF_POOL_GROUPS", "1")
    ks, eng = rig
    P = ks.params
    n_ops = 200
    ggsw = eng.circuit_bootstrap(eng.keyswitch_lwe_l1_lwe_l0(random_lwe_batch(21, 4, P.N * P.k)))
    sel = ggsw[np.arange(n_ops) % 4]
    pool = spf_amd.Pool(eng, max_batch=4096, max_wait_us=20000)
    avg = []
    try:
        for rnd in range(2):
            a = random_glwe(30 + rnd, n_ops, P.glwe_len)
            b = random_glwe(40 + rnd, n_ops, P.glwe_len)
            exp = eng.cmux(sel, a, b)
            got = np.zeros((n_ops, P.glwe_len), dtype=np.uint64)

            def one(i):
                pool.cmux(got[i], sel[i], a[i], b[i])
                return i

            ops0, launches0 = pool.stats()
            with ThreadPoolExecutor(max_workers=n_ops) as ex:
                assert sorted(ex.map(one, range(n_ops))) == list(range(n_ops))
            ops1, launches1 = pool.stats()
            assert np.array_equal(got, exp)
            assert ops1 - ops0 == n_ops
            avg.append((ops1 - ops0) / (launches1 - launches0))
        assert max(avg) > 64, avg   # some batch had several chunks (fresh executor threads per round: the second round may split)
    finally:
        pool.close()


def test_pool_one_thread_many_tickets_beyond_4096_slots(rig):
    """One thread may hold many tickets (asynchronous submit, wait later).  5 000 keyswitches in a row: the batches grow up to —
    and, with the usual timing, past — the 4 096 slots that have wake-up words of their own (the slots beyond share the last
    word, which only the last copy wakes); collected last ticket first."""
    ks, eng = rig
    P = ks.params
    n_ops = 5000
    lwe1 = random_lwe_batch(77, n_ops, P.N * P.k)
    exp = eng.keyswitch_lwe_l1_lwe_l0(lwe1)
    pool = spf_amd.Pool(eng, max_batch=8192, max_wait_us=20000)
    try:
        got = np.zeros((n_ops, P.lwe_n + 1), dtype=np.uint64)
        for rnd in range(3):   # the first rounds grow the staging sets (the slot count doubles whenever a batch fills up)
            got[:] = 0
            ops0, launches0 = pool.stats()
            tickets = [pool.submit_keyswitch(got[i], lwe1[i]) for i in range(n_ops)]
            for t in reversed(tickets):   # the last slots first
                pool.wait(t)
            ops1, launches1 = pool.stats()
            assert np.array_equal(got, exp)
            assert ops1 - ops0 == n_ops
        assert launches1 - launches0 <= 3, launches1 - launches0   # (typically two: ~400 at once, then everything else)
    finally:
        pool.close()


def test_pool_single_caller_and_keyswitch(rig):
    ks, eng = rig
    P = ks.params
    pool = spf_amd.Pool(eng, max_batch=8, max_wait_us=100)
    lwe1 = random_lwe_batch(9, 3, P.N * P.k)
    for i in range(3):
        out = np.zeros(P.lwe_n + 1, dtype=np.uint64)
        pool.keyswitch_lwe_l1_lwe_l0(out, lwe1[i])
        assert np.array_equal(out, O.keyswitch_lwe(lwe1[i], ks.ksk, P.N, P.lwe_n, P.ks_radix_log, P.ks_count))
    pool.close()


def test_pool_reports_errors_to_the_waiter():
    ks = keyset(0x5EED0001, SMALL_N)
    eng = spf_amd.Engine(to_engine_params(ks.params))      # no keys loaded
    pool = spf_amd.Pool(eng, max_batch=4, max_wait_us=100)
    out = np.zeros(eng.params.cbs_ggsw_complex, dtype=np.complex128)
    with pytest.raises(spf_amd.SpfError):
        pool.circuit_bootstrap(out, random_lwe_batch(1, 1, SMALL_N)[0])
    pool.close()


def test_concurrent_batch_callers_on_one_context(rig):
    """The host-pointer entry points share the context's staging buffers; calls from many threads
    (ctypes drops the GIL) must serialise as whole calls — stage, launch, copy back — not interleave."""
    ks, eng = rig
    P = ks.params
    jobs = []
    for t in range(24):
        B = 1 + (t * 5) % 9
        jobs.append((t % 3, random_lwe_batch(700 + t, B, P.N * P.k), random_glwe(800 + t, B, P.glwe_len),
                     random_glwe(900 + t, B, P.glwe_len)))
    ggsw = eng.circuit_bootstrap(eng.keyswitch_lwe_l1_lwe_l0(random_lwe_batch(5, 1, P.N * P.k)))

    def run(job):
        kind, lwe1, a, b = job
        if kind == 0:
            return eng.keyswitch_lwe_l1_lwe_l0(lwe1)
        if kind == 1:
            return eng.cmux(np.repeat(ggsw, a.shape[0], axis=0), a, b)
        return eng.sample_extract_l1(eng.glwe_xor(a, b), 3)

    expected = [run(j) for j in jobs]                      # one at a time
    with ThreadPoolExecutor(max_workers=12) as ex:
        got = list(ex.map(run, jobs * 3))
    for i, g in enumerate(got):
        assert np.array_equal(g, expected[i % len(jobs)]), i


def test_pool_ticket_is_collected_once_and_backpressure_blocks(rig):
    """ADVICE r1 / VERDICT weak #12: a second wait on a ticket is an error, not a hang; with max_inflight
    tickets open a further submit blocks until one is collected (the reference's bounded token channel,
    circuit_processor/mod.rs:139)."""
    import threading
    import time
    ks, eng = rig
    P = ks.params
    pool = spf_amd.Pool(eng, max_batch=4, max_wait_us=100)
    pool.set_max_inflight(2)
    lwe1 = random_lwe_batch(11, 3, P.N * P.k)
    outs = [np.zeros(P.lwe_n + 1, dtype=np.uint64) for _ in range(3)]
    t0 = pool.submit_keyswitch(outs[0], lwe1[0])
    t1 = pool.submit_keyswitch(outs[1], lwe1[1])
    third = {}

    def late():
        third["t"] = pool.submit_keyswitch(outs[2], lwe1[2])

    th = threading.Thread(target=late)
    th.start()
    time.sleep(0.3)
    assert "t" not in third, "submit must block while max_inflight tickets are open"
    pool.wait(t0)
    th.join(timeout=10)
    assert "t" in third
    with pytest.raises(spf_amd.SpfError):
        pool.wait(t0)                       # already collected
    with pytest.raises(spf_amd.SpfError):
        pool.wait(123456)                   # never issued
    pool.wait(t1)
    pool.wait(third["t"])
    for i in range(3):
        assert np.array_equal(outs[i], O.keyswitch_lwe(lwe1[i], ks.ksk, P.N, P.lwe_n, P.ks_radix_log, P.ks_count))
    pool.close()


def test_keyswitch_circuit_bootstrap_keeps_l0_on_device(rig):
    ks, eng = rig
    lwe1 = random_lwe_batch(21, 5, ks.params.N * ks.params.k)
    got = eng.keyswitch_circuit_bootstrap(lwe1)
    exp = eng.circuit_bootstrap(eng.keyswitch_lwe_l1_lwe_l0(lwe1))
    assert np.array_equal(got.view(np.float64), exp.view(np.float64))


def test_mismatched_batches_raise(rig):
    ks, eng = rig
    P = ks.params
    g = np.zeros((2, eng.params.cbs_ggsw_complex), dtype=np.complex128)
    a = random_glwe(1, 3, P.glwe_len)
    with pytest.raises(spf_amd.SpfError):
        eng.cmux(g, a, a)
    with pytest.raises(spf_amd.SpfError):
        eng.multiply_glwe_ggsw(a, g)


def test_pool_survives_tickets_nobody_collects_in_time(rig, monkeypatch):
    """r04 pipeline: a batch's pinned staging set returns to the pool when all its tickets are collected.  Tickets nobody
    waits for must not wedge it: with every set held by uncollected batches a further submit delivers the oldest batch's
    outputs itself after the grace period and goes on; the late waits still return the right status, the outputs are in the
    callers' buffers, and a pool destroyed with uncollected tickets cleans up."""
    ks, eng = rig
    P = ks.params
    monkeypatch.setenv("SPF_POOL_SETS", "3")                 # (sixteen by default: the test would never run out of sets)
    pool = spf_amd.Pool(eng, max_batch=2, max_wait_us=100)   # batches of two: three staging sets hold six tickets
    assert pool.counters()["staging_sets"] == 3
    pool.set_max_inflight(64)
    n = 10
    lwe1 = random_lwe_batch(31, n, P.N * P.k)
    outs = [np.zeros(P.lwe_n + 1, dtype=np.uint64) for _ in range(n)]
    tickets = [pool.submit_keyswitch(outs[i], lwe1[i]) for i in range(n)]   # nobody waits in between
    exp = [O.keyswitch_lwe(lwe1[i], ks.ksk, P.N, P.lwe_n, P.ks_radix_log, P.ks_count) for i in range(n)]
    for i in (0, 1, 2, 3):                                   # delivered on the submitters' behalf, or by these waits
        pool.wait(tickets[i])
    for i in range(n - 2):
        if i >= 4:
            pool.wait(tickets[i])
        assert np.array_equal(outs[i], exp[i]), i
    ops, launches = pool.stats()
    assert ops >= n - 2 and launches >= (n - 2) // 2
    assert pool.counters()["reclaimed"] >= 2                 # reclaim() really ran: outputs were delivered on their owners' behalf
    pool.close()                                             # tickets n-2, n-1 never collected


def test_pool_wait_during_a_delivery_on_the_callers_behalf(rig, monkeypatch):
    """reclaim() copies an uncollected output to the caller's buffer with the pool's lock dropped; a wait() for
    that ticket arriving DURING the copy must not return before the copy has ended (the caller may read or free `out` the
    moment wait returns).  Circuit bootstraps (256 KiB outputs, the longest copies); every set held by uncollected batches;
    one thread's submit triggers the delivery while other threads wait for exactly those tickets and compare at once."""
    import threading
    import time
    ks, eng = rig
    P = ks.params
    lwe0 = random_lwe_batch(41, 8, SMALL_N)
    exp = eng.circuit_bootstrap(lwe0)
    monkeypatch.setenv("SPF_POOL_SETS", "3")
    reclaimed = 0
    for rnd in range(6):
        pool = spf_amd.Pool(eng, max_batch=2, max_wait_us=100)
        pool.set_max_inflight(64)
        outs = [np.zeros(eng.params.cbs_ggsw_complex, dtype=np.complex128) for _ in range(8)]
        tk = []
        for i in range(6):                                   # three batches of two: every staging set held
            t = spf_amd._ffi.C.c_uint64()
            x = np.ascontiguousarray(lwe0[i])
            st = pool._lib.spf_pool_submit_circuit_bootstrap(pool._h, x.ctypes.data_as(spf_amd._ffi.C.c_void_p),
                                                             outs[i].ctypes.data_as(spf_amd._ffi.C.c_void_p), spf_amd._ffi.C.byref(t))
            assert st == 0
            tk.append(t.value)
        time.sleep(0.3 + 0.01 * rnd)                         # past the grace period: the next submit delivers the leftovers
        bad = []

        def waiter(i):
            pool._wait(tk[i])
            if not np.array_equal(outs[i].view(np.float64), exp[i].view(np.float64)):
                bad.append(i)

        def submitter():
            pool.circuit_bootstrap(outs[6], lwe0[6])         # no set free: reclaim() runs inside this submit

        # the submitter first: no set is free, its 20 ms look-out passes, reclaim() starts delivering — the waiters arrive around
        # that moment, spread over the copies
        th = [threading.Thread(target=submitter)] + [threading.Thread(target=waiter, args=(i,)) for i in range(6)]
        th[0].start()
        time.sleep(0.018 + 0.001 * rnd)
        for t in th[1:]:
            t.start()
            time.sleep(0.0005)
        for t in th:
            t.join()
        assert not bad, (rnd, bad)
        assert np.array_equal(outs[6].view(np.float64), exp[6].view(np.float64))
        reclaimed += pool.counters()["reclaimed"]
        pool.close()
    assert reclaimed > 0                                     # the delivered 0 / 1 / 2 hand-over was exercised


def test_pool_under_native_load_every_caller_gets_its_own_output(rig):
    """The drop-in scenario with the load generator of the bench leg (tools/pool_driver.cpp: native threads, each looping
    KeyswitchL1toL0 -> CircuitBootstrap on its own ciphertext through the pool for a second): 300 callers, so the batches leave
    in several chunks and close by the rules of a running pipeline; afterwards every caller's last output must be the circuit
    bootstrap of ITS input (against the batch entry points on the same inputs)."""
    import ctypes as C
    import os
    import subprocess
    ks, eng = rig
    P = ks.params
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    drv_path = os.path.join(root, "tools", "bin", "libpool_driver.so")
    src = os.path.join(root, "tools", "pool_driver.cpp")
    if not os.path.exists(drv_path) or os.path.getmtime(drv_path) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(drv_path), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", os.path.join(root, "include"),
                        "-o", drv_path, src], check=True)
    drv = C.CDLL(drv_path)
    drv.spf_pool_drive_collect.restype = C.c_long
    drv.spf_pool_drive_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_size_t,
                                           C.c_size_t, C.POINTER(C.c_double), C.c_void_p]
    T = int(os.environ.get("SPF_POOL_SOAK_THREADS", "300"))          # (a soak: 1024 threads for 20 s, profiles/r04_fuzz.md)
    seconds = float(os.environ.get("SPF_POOL_SOAK_SECONDS", "1.0"))
    lwe1 = random_lwe_batch(0xD21, 1, P.N * P.k)[0]
    inputs = np.tile(lwe1, (T, 1))
    inputs[:, 0] += np.arange(T, dtype=np.uint64)
    exp = eng.circuit_bootstrap(eng.keyswitch_lwe_l1_lwe_l0(inputs))
    n_doubles = eng.params.cbs_ggsw_complex * 2
    got = np.zeros((T, n_doubles), dtype=np.float64)
    pool = spf_amd.Pool(eng, max_batch=4096, max_wait_us=200)
    try:
        el = C.c_double()
        lib = eng._lib
        n = drv.spf_pool_drive_collect(pool._h, C.cast(lib.spf_pool_submit_keyswitch_circuit_bootstrap, C.c_void_p),
                                       C.cast(lib.spf_pool_wait, C.c_void_p), T, seconds, lwe1.ctypes.data, lwe1.size, n_doubles,
                                       C.byref(el), got.ctypes.data)
        ops, launches = pool.stats()
    finally:
        pool.close()
    assert n >= T, n                       # every caller completed at least one operation
    assert ops == n and launches < n / 16, (n, ops, launches)
    assert np.array_equal(got, exp.reshape(T, -1).view(np.float64))
    print(f"pool soak: {T} callers, {el.value:.1f} s, {n} operations in {launches} launches")


def test_pool_every_exec_op_kind_against_the_oracle(rig):
    """The remaining `FheOp` kinds of `CircuitProcessor::exec_op` (circuit_processor/mod.rs:341-540) through the pool, one
    ciphertext per call from many threads: SampleExtract (two different indices: two batches), Not, GlweAdd, MulXN,
    MultiplyGgswGlwe, GlevCMux, SchemeSwitch — each output against the oracle."""
    ks, eng = rig
    P = ks.params
    EP = eng.params
    n = 12
    r = np.random.default_rng(91)
    ggsw = ((r.standard_normal((n, EP.cbs_ggsw_complex)) + 1j * r.standard_normal((n, EP.cbs_ggsw_complex))) * 2.0 ** 58)
    a = random_glwe(92, n, P.glwe_len)
    b = random_glwe(93, n, P.glwe_len)
    ga = random_glwe(94, n * P.cbs_count, P.glwe_len).reshape(n, P.cbs_count, P.glwe_len)
    gb = random_glwe(95, n * P.cbs_count, P.glwe_len).reshape(n, P.cbs_count, P.glwe_len)
    ssk = O.gen_ssk_fft(O.Rng(0x7A11 + 1), ks.glwe_sk, P)   # any key: parity needs the SAME key on both sides
    eng.load_scheme_switch_key(ssk)
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=2000)
    out_se = np.zeros((n, P.N * P.k + 1), dtype=np.uint64)
    out_not = np.zeros((n, P.glwe_len), dtype=np.uint64)
    out_add = np.zeros_like(out_not)
    out_xn = np.zeros_like(out_not)
    out_mul = np.zeros_like(out_not)
    out_gc = np.zeros((n, P.cbs_count * P.glwe_len), dtype=np.uint64)
    out_ss = np.zeros((n, EP.cbs_ggsw_complex), dtype=np.complex128)

    def task(i):
        pool.sample_extract_l1(out_se[i], a[i], 0 if i % 2 else 1234)
        pool.glwe_not(out_not[i], a[i])
        pool.glwe_add(out_add[i], a[i], b[i])
        pool.mul_xn(out_xn[i], a[i], 4096 + 77)          # taken mod 2N
        pool.multiply_glwe_ggsw(out_mul[i], a[i], ggsw[i])
        pool.glev_cmux(out_gc[i], ggsw[i], ga[i], gb[i])
        pool.scheme_switch(out_ss[i], ga[i])
        return i

    try:
        with ThreadPoolExecutor(max_workers=n) as ex:
            assert sorted(ex.map(task, range(n))) == list(range(n))
        ops, launches = pool.stats()
        assert ops == 7 * n and launches < ops            # coalesced
        with pytest.raises(spf_amd.SpfError):
            pool.sample_extract_l1(out_se[0], a[0], P.N)  # index out of range: refused at submit
    finally:
        pool.close()
    for i in range(n):
        assert np.array_equal(out_se[i], O.sample_extract(a[i], 0 if i % 2 else 1234, P.N, P.k)), i
        assert np.array_equal(out_not[i], O.glwe_not(a[i], P.N, P.k)), i
        assert np.array_equal(out_add[i], O.glwe_xor(a[i], b[i], P.N, P.k)), i
        assert np.array_equal(out_xn[i], O.glwe_mul_xn(a[i], 77, P.N, P.k)), i
        fft = O.glwe_ggsw_mad(np.zeros(P.glwe_len // 2, dtype=np.complex128), a[i], ggsw[i], P.N, P.k, P.cbs_radix_log, P.cbs_count)
        assert np.array_equal(out_mul[i], np.concatenate([O.poly_ifft(fft[:P.N // 2]), O.poly_ifft(fft[P.N // 2:])])), i
        for j in range(P.cbs_count):
            exp = O.cmux(ga[i, j], gb[i, j], ggsw[i], P.N, P.k, P.cbs_radix_log, P.cbs_count)
            assert np.array_equal(out_gc[i].reshape(P.cbs_count, P.glwe_len)[j], exp), (i, j)
        assert np.array_equal(out_ss[i].view(np.float64), O.scheme_switch_fft(ga[i], ssk, P).view(np.float64)), i


def test_pool_reports_how_many_streams_run_side_by_side(rig):
    """spf_pool_create measures whether its streams really run concurrently (a host that touched HIP
    before the library was loaded keeps 4 hardware queues and the resident batches take turns) and says so: the counter is
    filled, and with the library's own GPU_MAX_HW_QUEUES=24 in effect most of the sixteen streams overlap."""
    ks, eng = rig
    pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=100)
    try:
        c = pool.counters()
        assert c["staging_sets"] == 16
        assert 1 <= c["stream_concurrency"] <= 16, c     # filled; in THIS process, after dozens of pools came and went, the
    finally:                                             # runtime's hardware queues are shared as it happened to hand them out
        pool.close()
    # the claim itself in a fresh process: the library loaded first, one context, one pool.  GPU_MAX_HW_QUEUES is left unset
    # there, so the library's own request is the one in effect (a value the caller's environment exports would win over it)
    import json
    import subprocess
    import sys
    code = ("import json, spf_amd\n"
            "eng = spf_amd.Engine(spf_amd.DEFAULT_128.replace(lwe_dimension=8))\n"
            "pool = spf_amd.Pool(eng, max_batch=64, max_wait_us=100)\n"
            "print('COUNTERS ' + json.dumps(pool.counters()))\n"
            "pool.close()\n")
    env = {k: v for k, v in __import__("os").environ.items() if k != "GPU_MAX_HW_QUEUES"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env,
                       cwd=__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
    line = [l for l in r.stdout.splitlines() if l.startswith("COUNTERS ")]
    assert r.returncode == 0 and line, r.stdout + r.stderr
    fresh = json.loads(line[0][len("COUNTERS "):])
    assert 8 <= fresh["stream_concurrency"] <= 16, fresh
    v = eng._lib.spf_version().decode()
    assert v.startswith("spf_hip 0.6 gfx950 (blind rotation: BR_OPT=") and "ABLATION" not in v
