"""The by-handle wake-up tree of the pool (spf_amd/csrc/spf_wake.hpp) in the shapes where it has children, on the GPU.

Batches of n = 9, 72, 73 and 585 ticketed `GlweAdd` submits from one thread (2, 9, 10 and 74 groups of eight; 585 has three
levels), ONE batch each, with the waiting threads arriving in three adverse orders; every output must be word-equal to numpy's
wrapping a + b and every thread must come back.  This test cannot see a lost wake-up whose window is a few stores wide and does
not try to: tests/cpp/wake_protocol.cpp (tests/test_wake_protocol.py) forces those interleavings on the CPU.  What runs here is
the library's own copy of that protocol behind real completions.

Everything runs once, in a child process under a time limit; waiting threads are joined with a time limit.  A thread that has to
be given up fails the test and ends the child at once: nothing more is started on the GPU."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (9, 72, 73, 585)
ORDERS = ("leaf groups first, group 0 50 ms later", "group 0 first", "one ticket per group abandoned, three Value.wait() on one value")
QUIET_US = 250_000   # the batch under test closes this long after its last member: by then every waiter of the order is asleep
JOIN_S = 20.0


def _give_up(what):
    print(f"GAVE UP: {what}", flush=True)
    os._exit(3)   # (threads may still sit in the library: no clean-up, nothing more on the GPU)


def _join(threads, what):
    deadline = time.monotonic() + JOIN_S
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
        if t.is_alive():
            _give_up(what)


def _child():
    import oracle as O
    import spf_amd
    from spf_amd import FheOp, ValueKind
    from tests.util import random_glwe, to_engine_params

    P = O.DEFAULT_128.replace(lwe_n=12)
    eng = spf_amd.Engine(to_engine_params(P))   # (GlweAdd needs no key)
    pool = spf_amd.Pool(eng, max_batch=4096, max_wait_us=QUIET_US)
    n_max = max(SIZES)
    a, b = random_glwe(1501, n_max, P.glwe_len), random_glwe(1502, n_max, P.glwe_len)
    want = a + b                                # uint64: wraps
    va, vb = pool.upload_batch(ValueKind.GLWE1, a), pool.upload_batch(ValueKind.GLWE1, b)
    errors = []

    def submit(n):
        return [pool.submit_v(FheOp.GlweAdd, [va[i], vb[i]]) for i in range(n)]

    def waiter(ticket):
        def run():
            try:
                pool.wait(ticket)
            except Exception as e:   # noqa: BLE001 (reported by the main thread)
                errors.append(repr(e))
        return threading.Thread(target=run, daemon=True)

    def value_waiter(value):
        def run():
            try:
                value.wait()
            except Exception as e:   # noqa: BLE001
                errors.append(repr(e))
        return threading.Thread(target=run, daemon=True)

    # a pool's batches start at 64 slots and double whenever one fills up: four full batches, and the next one holds 1024
    for size in (64, 128, 256, 512):
        ops0, launches0 = pool.stats()
        subs = submit(size)
        for _, t in subs:
            pool.wait(t)
        assert tuple(np.subtract(pool.stats(), (ops0, launches0))) == (size, 1), (size, pool.stats())
        assert np.array_equal(pool.download_batch([v for v, _ in subs]), want[:size])

    for order in ORDERS:
        for n in SIZES:
            what = f"n = {n}, {order}"
            ops0, launches0 = pool.stats()
            subs = submit(n)
            tickets = [t for _, t in subs]
            later = []
            if order == ORDERS[0]:
                threads = [waiter(t) for t in tickets[8:]]
                for t in threads:
                    t.start()
                time.sleep(0.05)
                root = [waiter(t) for t in tickets[:8]]
                for t in root:
                    t.start()
                threads += root
            elif order == ORDERS[1]:
                threads = [waiter(t) for t in tickets]   # (slot order: group 0 arrives first)
                for t in threads:
                    t.start()
            else:
                # nobody waits for the first ticket of each group — the parent of groups 1, 9, 17, ...: the completing thread's
                # walk has to wake those; the batch is closed by the first Value.wait() (no quiet time to sit out)
                later = tickets[0::8]
                threads = [waiter(t) for i, t in enumerate(tickets) if i % 8 != 0]
                for t in threads:
                    t.start()
                values = [value_waiter(subs[n - 1][0]) for _ in range(3)]
                for t in values:
                    t.start()
                threads += values
            _join(threads, what)
            assert not errors, (what, errors)
            got_ops, got_launches = np.subtract(pool.stats(), (ops0, launches0))
            assert (got_ops, got_launches) == (n, 1), (what, got_ops, got_launches)
            got = pool.download_batch([v for v, _ in subs])
            assert np.array_equal(got, want[:n]), what
            for t in later:   # (the abandoned tickets, collected once it is all over: they return at once)
                pool.wait(t)
            print(f"ok: {what}", flush=True)
    del subs, va, vb
    pool.close()
    print("wakeups ok", flush=True)


def test_every_waiter_returns_in_three_adverse_orders():
    code = "import tests.test_gpu_pool_wakeups as t\nt._child()\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=240)
    assert "GAVE UP" not in r.stdout, r.stdout[-3000:]
    assert r.returncode == 0 and r.stdout.rstrip().endswith("wakeups ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok: n = ") == len(SIZES) * len(ORDERS), r.stdout
