"""Every destroy order of the ABI's handles on the GPU, on real objects after real work (include/spf_hip.h, "Lifetimes": a
child keeps its parent alive, the destroy functions may be called in any order).

tests/cpp/lifetimes_gpu.cpp is a native driver against libspf_hip.so, one scenario per child process: a graph and a pool
outliving their context, all 24 orders of {context, graph, pool, value}, a group's jobs and a group pool outliving the
group, a pool and a graph on a borrowed member context, and the value of a destroyed pool offered to the next pool.  What
runs through the survivor is a CMUX chain compared word for word with spf_cmux_batch on a context nobody touches;
`spf_live_objects` must be all zero at the end.  The Python layer's own orders (Engine.close() before its circuits, a
group closed while a traceback holds its jobs, interpreter exit with everything alive) run in child interpreters.  The same
orders on hand-made parents under the sanitizers: tests/test_lifetimes_host.py.

A child that ends by a signal or at its time limit makes every later test of this module fail at once: nothing more is
started on a device that may be in trouble."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spf_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT = 300   # per child, as the other native drivers of the suite
_dead = []         # the child that ended by signal or time limit, if any

SCENARIOS = ["ctx-graph", "ctx-pool-value", "permutations", "group-jobs", "group-pool", "borrowed-member", "stale-value"]


def _run_child(argv, what, **kw):
    assert not _dead, f"not started: {_dead[0]} ended by a signal or at its time limit"
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=TIME_LIMIT, **kw)
    except subprocess.TimeoutExpired:
        _dead.append(what)
        raise
    if r.returncode < 0:
        _dead.append(what)
    return r


def _quiet(stderr):
    """nothing from the allocator ("free(): invalid pointer", "double free or corruption", ...), the runtime or a signal"""
    low = stderr.lower()
    for word in ("free()", "double free", "corrupt", "invalid pointer", "munmap_chunk", "malloc", "segmentation", "abort", "core dumped",
                 "memory access fault", "hsa_status", "traceback", "hipfree"):
        assert word not in low, stderr[-4000:]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.dirname(spf_amd.lib_path())
    exe = tmp_path_factory.mktemp("lifetimes") / "lifetimes_gpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lifetimes_gpu.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
    return str(exe)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_native_destroy_orders(driver, scenario):
    r = _run_child([driver, scenario], scenario)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout and r.stdout.rstrip().endswith("all equal"), r.stdout[-4000:]
    assert "every live count is zero" in r.stdout
    if scenario == "permutations":
        assert r.stdout.count("nothing is left") == 24, r.stdout
    _quiet(r.stderr)


# ---- the Python layer, in child interpreters

def _operands(seed, P, depth=2):
    rng = np.random.default_rng(seed)
    sel = [(rng.standard_normal(2 * P.cbs_ggsw_complex) * 2.0 ** 50).view(np.complex128) for _ in range(depth)]
    a = rng.integers(0, 1 << 64, P.glwe_words, dtype=np.uint64)
    b = [rng.integers(0, 1 << 64, P.glwe_words, dtype=np.uint64) for _ in range(depth)]
    return sel, a, b


def _chain(engine, seed, P):
    """a CMUX chain as a circuit of `engine` (an Engine or a Group), and what an untouched engine must make of it"""
    from spf_amd import FheCircuit, FheOp, ValueKind
    sel, a, b = _operands(seed, P)
    g = FheCircuit(engine)
    x = g.add_input(ValueKind.GLWE1, a)
    for s, hi in zip(sel, b):
        x = g.add_op(FheOp.CMux, [g.add_input(ValueKind.GGSW1, s), x, g.add_input(ValueKind.GLWE1, hi)])
    return g, g.add_output(x, ValueKind.GLWE1), (sel, a, b)


def _expected(ref, operands):
    sel, x, b = operands
    for s, hi in zip(sel, b):
        x = ref.cmux(s, x, hi)[0]
    return x


def _params():
    return spf_amd.DEFAULT_128.replace(lwe_dimension=12)


def _all_zero():
    live = spf_amd.live_objects()
    assert not any(live.values()), live


def _child_engine_close():
    """Engine.close(), then FheCircuit.run() and .close()"""
    P = _params()
    ref, eng = spf_amd.Engine(P), spf_amd.Engine(P)
    g, out, ops = _chain(eng, 1, P)
    g.run()
    assert np.array_equal(out, _expected(ref, ops))
    eng.close()
    ops[1][:] = np.random.default_rng(2).integers(0, 1 << 64, P.glwe_words, dtype=np.uint64)   # new input contents
    g.run()
    assert np.array_equal(out, _expected(ref, ops))
    assert spf_amd.live_objects() == dict(contexts=2, groups=0, graphs=1, pools=0, values=0)
    g.close()
    ref.close()
    _all_zero()
    print("engine-close ok")


def _child_group_close_under_traceback():
    """Group.close() while an exception's traceback holds the group's jobs, then del and gc.collect()"""
    import gc
    P = _params()
    ref = spf_amd.Engine(P)
    grp = spf_amd.Group(P, devices=[0, 0])

    def work():
        made = [_chain(grp, 10 + k, P) for k in range(4)]
        grp.run_graphs([m[0] for m in made])
        for _, out, ops in made:
            assert np.array_equal(out, _expected(ref, ops))
        assert {m[0].member() for m in made} == {0, 1}
        assert False, "a failed assertion leaves the jobs open"

    held = None
    try:
        work()
    except AssertionError as e:
        held = e   # its traceback holds work()'s frame, and that the jobs
    assert held is not None and "leaves the jobs open" in str(held)
    grp.close()   # (what a fixture's teardown does)
    live = spf_amd.live_objects()
    assert live["groups"] == 1 and live["graphs"] >= 4, live   # the jobs keep the group
    del held
    gc.collect()
    ref.close()
    _all_zero()
    print("group-close ok")


class _Holder:
    pass


def _child_exit_with_everything_alive():
    """interpreter exit with an engine, a group, circuits, a pool and values alive in module globals and in a reference cycle"""
    from spf_amd import ValueKind
    P = _params()
    mod = sys.modules[__name__]
    mod.KEEP_ENGINE = spf_amd.Engine(P)
    mod.KEEP_GROUP = spf_amd.Group(P, devices=[0, 0])
    mod.KEEP_CIRCUITS = [_chain(mod.KEEP_ENGINE, 20, P), _chain(mod.KEEP_GROUP, 21, P), _chain(mod.KEEP_GROUP.member(1), 22, P)]
    for g, out, ops in mod.KEEP_CIRCUITS:
        g.run()
        assert np.array_equal(out, _expected(mod.KEEP_ENGINE, ops))
    mod.KEEP_POOLS = [spf_amd.Pool(mod.KEEP_ENGINE, max_batch=64), spf_amd.Pool(mod.KEEP_GROUP, max_batch=64)]
    sel, a, b = _operands(23, P, 1)
    got = np.zeros_like(a)
    mod.KEEP_POOLS[0].cmux(got, sel[0], a, b[0])
    assert np.array_equal(got, mod.KEEP_ENGINE.cmux(sel[0], a, b[0])[0])
    mod.KEEP_VALUES = [mod.KEEP_POOLS[0].upload(ValueKind.GLWE1, a), mod.KEEP_POOLS[1].upload(ValueKind.GLWE1, a, member=1)]
    # the same kinds of object again, reachable only through a cycle
    x, y = _Holder(), _Holder()
    x.other, y.other = y, x
    x.engine = spf_amd.Engine(P)
    x.group = spf_amd.Group(P, devices=[0, 0])
    y.circuits = [_chain(x.engine, 24, P), _chain(x.group, 25, P)]
    for g, out, ops in y.circuits:
        g.run()
        assert np.array_equal(out, _expected(mod.KEEP_ENGINE, ops))
    y.pool = spf_amd.Pool(x.engine, max_batch=64)
    x.value = y.pool.upload(ValueKind.GLWE1, a)
    assert np.array_equal(x.value.download(), a)
    print("exit ok", flush=True)


def _python_child(fn, marker):
    code = f"import tests.test_gpu_lifetimes as t\nt.{fn}()\n"
    r = _run_child([sys.executable, "-c", code], fn, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith(marker), r.stdout[-2000:] + r.stderr[-4000:]
    _quiet(r.stderr)


def test_engine_close_before_its_circuit():
    _python_child("_child_engine_close", "engine-close ok")


def test_group_close_while_a_traceback_holds_its_jobs():
    _python_child("_child_group_close_under_traceback", "group-close ok")


def test_interpreter_exit_with_everything_alive():
    _python_child("_child_exit_with_everything_alive", "exit ok")
