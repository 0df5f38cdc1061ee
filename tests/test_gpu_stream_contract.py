"""The stream contract of the device-pointer entry points (include/spf_hip.h: "the call only ENQUEUES on `stream`", intermediates
in buffers of the context, one stream per context or streams ordered by events), on a caller's own non-blocking stream.

Everywhere else in the suite a `_dev` call sees the null stream or the context's own, with the device idle before and after.
Here every case of tests/stream_cases.py runs behind a closed gate (tests/hip_runtime.py) on a fresh `hipStreamNonBlocking`
stream whose earlier work writes the operands and whose later work overwrites them: a launch, memset or copy that the library
puts on any other stream reads decoys or finds the output consumed, and a word differs.  The reference is the same library on
the null stream — the path the rest of the suite holds to the oracle — so there is no tolerance: `same_words`."""
import re
import time

import numpy as np
import pytest

import spf_amd
from tests import hip_runtime as HR
from tests import stream_cases as SC
from tests.blind_rotation_graph_cases import same_words

pytestmark = pytest.mark.gpu
GROWTH_SCALE = 16   # test (c): batches large enough that the first call is still running when the second one grows the buffers


def make_engine(name: str, salt: int = 0) -> spf_amd.Engine:
    e = spf_amd.Engine(SC.CONTEXTS[name])
    bsk, ksk, ak, ssk = SC.context_keys(name, salt)
    e.load_bootstrap_key(bsk)
    e.load_keyswitch_key(ksk)
    e.load_automorphism_key(ak)
    e.load_scheme_switch_key(ssk)
    return e


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name, salt=0):
        if (name, salt) not in made:
            made[name, salt] = make_engine(name, salt)
        return made[name, salt]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def pbs_batches(ctx):
    """the smallest batch that reaches each blind-rotation shape, found from the kernel name the library REPORTS"""
    eng, cap = ctx("T"), 2048
    P = eng.params
    bufs = [eng.device_alloc(8 * n) for n in (cap * P.lwe0_words, P.glwe_words, cap * P.lwe1_words)]
    try:
        eng.device_upload(bufs[0], np.zeros(cap * P.lwe0_words, dtype=np.uint64))
        eng.device_upload(bufs[1], np.zeros(P.glwe_words, dtype=np.uint64))

        def reported(B):
            eng.pbs_univariate_dev(None, B, bufs[0], bufs[1], 0, bufs[2])
            return eng.last_blind_rotate_kernel()

        def first(pred, lo, hi):   # smallest B in (lo, hi] with pred(reported(B)); pred is false at lo, true at hi
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if pred(reported(mid)) else (mid, hi)
            return hi

        assert reported(2).startswith("blind_rotate8_kernel<") and reported(cap).startswith("blind_rotate2p_kernel<")
        found = {"blind_rotate8": 2,
                 "blind_rotate2p2": first(lambda n: not n.startswith("blind_rotate8_"), 2, cap),
                 "blind_rotate2p": first(lambda n: n.startswith("blind_rotate2p_"), 2, cap)}
        eng.device_download(None, np.empty(1, dtype=np.uint64), bufs[2])   # (waits for the probes)
        for shape, B in found.items():
            assert reported(B).startswith(shape + "_kernel<"), (shape, B)
        eng.device_download(None, np.empty(1, dtype=np.uint64), bufs[2])
    finally:
        for p in bufs:
            eng.device_free(p)
    print(f"smallest batch per blind-rotation shape: {found}")
    return found


def _copy_on_null_stream(dst, src, nbytes):
    HR.check(HR.runtime().hipMemcpyAsync(dst, src, nbytes, HR.MEMCPY_DEVICE_TO_DEVICE, None), "hipMemcpyAsync (D2D, null stream)")


class Staged:
    """One call of a case at one batch size: working buffers (what the call is given), device copies of the real and of the decoy
    operands, `kept` (where the caller's next work puts the result), and the null-stream result `want`.  `alias` gives an input
    the buffer of another call's output (test (d)): it has no contents of its own."""

    def __init__(self, eng, case, B=None, tag="", alias=None):
        self.eng, self.r, self.key, self.alias = eng, case.resolve(B), case.id + tag, dict(alias or {})
        self._owned, self.work, self.src, self.decoy_host = [], dict(self.alias), {"real": {}, "decoy": {}}, {}
        self.want = self.want_decoy = self.decoy_out = None
        out = self.r.output
        self.data_inputs = [o for o in self.r.inputs if o.role != "table" and o.name not in self.alias]
        self.tables = [o for o in self.r.inputs if o.role == "table"]
        try:
            for op in self.r.operands:
                if op.name not in self.alias:   # (what is read while a gate is closed has room for the smallest such read)
                    self.work[op.name] = self._alloc(max(op.nbytes, HR.MIN_READ) if op is out else op.nbytes)
            self.kept = self._alloc(out.nbytes)
            HR.reserve_pinned(out.nbytes)
            for op in self.data_inputs:
                for which in ("real", "decoy"):
                    host = SC.operand_data(self.key, op, which)
                    self.src[which][op.name] = self._alloc(op.nbytes)
                    eng.device_upload(self.src[which][op.name], host)
                    if which == "decoy":
                        self.decoy_host[op.name] = host
            if self.tables:   # the decoy tables point at the decoy operands and at an output of their own
                decoys = dict(self.src["decoy"])
                if out.role == "out":
                    decoys[out.name] = self._alloc(out.nbytes)
                    if any(e is not None and e[0] == out.name for op in self.tables for e in op.entries):
                        self.decoy_out = decoys[out.name]   # where a call given the decoy table writes
                for op in self.tables:
                    for which, base in (("real", self.work), ("decoy", decoys)):
                        host = SC.table_pointers(self.r, op, base)
                        self.src[which][op.name] = self._alloc(op.nbytes)
                        eng.device_upload(self.src[which][op.name], host)
                        if which == "decoy":
                            self.decoy_host[op.name] = host
            self.copied = self.data_inputs + self.tables
        except BaseException:
            self.free()
            raise

    def _alloc(self, nbytes):
        p = self.eng.device_alloc(nbytes)
        self._owned.append(p)
        return p

    def free(self):
        while self._owned:
            self.eng.device_free(self._owned.pop())

    def call(self, stream, eng=None) -> int:
        eng = eng or self.eng
        return getattr(eng._lib, self.r.case.entry)(eng._h, stream, *self.r.args(self.work))

    def _fetch(self, ptr, op):
        host = np.empty((op.rows, op.row_words) if op.role != "table" else (op.words,), dtype=np.uint64)
        self.eng.device_download(None, host, ptr)
        return host

    def _run_on_null_stream(self, which):
        for op in self.copied:
            _copy_on_null_stream(self.work[op.name], self.src[which][op.name], op.nbytes)
        st = self.call(None)
        assert st == 0, (self.key, st, self.eng._lib.spf_last_error(self.eng._h))
        at = self.decoy_out if which == "decoy" and self.decoy_out else self.work[self.r.output.name]
        return self._fetch(at, self.r.output)

    def compute_want(self):
        """1. the real operands on the null stream, behind a host synchronization"""
        self.want = self._run_on_null_stream("real")
        self.check_kernels()
        return self

    def reset(self, warm=True):
        """2. decoys in the inputs, a sentinel in the output; `warm`: the call once at this batch size, so that the context has
        nothing left to grow — and the decoys are shown to give other words than the real operands"""
        out = self.r.output
        if warm:
            self.want_decoy = self._run_on_null_stream("decoy")
            assert not same_words(self.want_decoy, self.want), f"{self.key}: the decoys give the words of the real operands"
        for op in self.copied:   # (again after the warm call: an operand transformed in place holds its decoy)
            _copy_on_null_stream(self.work[op.name], self.src["decoy"][op.name], op.nbytes)
        if out.role == "out":
            assert not (self.want == SC.SENTINEL).all()
            self.eng.device_upload(self.work[out.name], np.full(out.words, SC.SENTINEL, dtype=np.uint64))
            self.eng.device_upload(self.kept, np.full(out.words, SC.SENTINEL, dtype=np.uint64))
            assert (self._fetch(self.work[out.name], out) == SC.SENTINEL).all()   # (and the null stream is idle)
        else:
            assert same_words(self._fetch(self.work[out.name], out), self.decoy_host[out.name])
        return self

    def enqueue(self, S, eng=None) -> int:
        """3. on the caller's stream: the real operands arrive, the call, the result is taken, the operands are overwritten"""
        for op in self.copied:
            S.copy(self.work[op.name], self.src["real"][op.name], op.nbytes)
        st = self.call(S.handle, eng)
        S.copy(self.kept, self.work[self.r.output.name], self.r.output.nbytes)
        for op in self.copied:
            S.copy(self.work[op.name], self.src["decoy"][op.name], op.nbytes)
        return st

    def assert_not_started(self, reader):
        """4. the output as it was before the enqueue, read through another stream of the test"""
        out = self.r.output
        got = reader.read(self.work[out.name], np.empty((out.rows, out.row_words), dtype=np.uint64))
        if out.role == "out":
            assert (got == SC.SENTINEL).all(), \
                f"{self.key}: the output was written while the caller's stream was held ({self._rows(got)})"
        else:
            assert same_words(got, self.decoy_host[out.name]), f"{self.key}: the operand was transformed while the stream was held"

    def _rows(self, got) -> str:
        """what the rows of an output hold, for a failure message"""
        n = {"the sentinel": (got == SC.SENTINEL).all(axis=1), "the null-stream result": (got == self.want).all(axis=1)}
        if self.want_decoy is not None:
            n["the result of the decoys"] = (got == self.want_decoy).all(axis=1)
        return f"of {got.shape[0]} rows: " + ", ".join(f"{int(v.sum())} hold {k}" for k, v in n.items())

    def check_kernels(self, eng=None):
        eng = eng or self.eng
        names = {"pbs": eng.last_blind_rotate_kernel, "cmux": eng.last_cmux_kernel, "keyswitch": eng.last_keyswitch_kernel}
        for which, pattern in self.r.case.kernels:
            assert re.fullmatch(pattern, names[which]()), (self.key, self.r.B, which, names[which](), pattern)

    def check_done(self, eng=None):
        """5. the result the caller took is the null-stream result, the inputs hold what the caller wrote over them"""
        out = self.r.output
        kept = self._fetch(self.kept, out)
        bad = np.flatnonzero((kept != self.want).any(axis=1))
        assert same_words(kept, self.want), \
            f"{self.key}: {bad.size} of {out.rows} output rows differ from the null-stream run (first: {bad[:4]}; {self._rows(kept)})"
        for op in self.copied:
            got = self._fetch(self.work[op.name], op)
            assert same_words(got.reshape(-1), self.decoy_host[op.name].reshape(-1)), f"{self.key}: input {op.name} does not hold the decoy"
        self.check_kernels(eng)


def _status(staged, st, eng=None):
    eng = eng or staged.eng
    assert st == 0, (staged.key, st, eng._lib.spf_last_error(eng._h))


def _assert_held(*streams_):
    """the call returned while the gate was still closed, and not because the cap opened it; a stream that is already idle
    would prove nothing: that case FAILS"""
    for S in streams_:
        assert not any(g.capped for g in S.gates), "the call returned only after the gate's cap: it waited for the device"
        assert S.busy(), "the caller's stream is idle although its gate is closed: the case proves nothing"


def _batch(case, pbs_batches):
    return pbs_batches[case.B] if isinstance(case.B, str) else case.B


# ---- (a) every case, gated on a caller's stream ---------------------------------------------------------------------------
# A closed gate holds the HARDWARE queue its stream is dealt, and the runtime deals its few hardware queues (GPU_MAX_HW_QUEUES,
# 4 by default) to the streams of the process in turn: a launch misplaced on a stream that shares the gated stream's queue
# waits behind the gate as well, in submission order, and goes unseen (measured: profiles/r17_stream_contract.md).  So every
# case runs once on each of SWEEP streams that are alive together, hence spread over the queues: the stream a misplaced launch
# went to shares its queue with at most some of them.
SWEEP = 4


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_a_call_only_enqueues_on_the_callers_stream(case, ctx, pbs_batches):
    st = Staged(ctx(case.ctx), case, _batch(case, pbs_batches))
    try:
        st.compute_want()
        with HR.streams(SWEEP + 1) as (reader, *callers):
            for S in callers:
                st.reset()
                S.gate()
                _status(st, st.enqueue(S))
                _assert_held(S)
                st.assert_not_started(reader)
                _assert_held(S)
                S.release()
                st.check_done()
    finally:
        st.free()


# ---- (b) two calls of a multi-step entry point back to back: one context, one stream, no host synchronization between -----
@pytest.mark.parametrize("case_id,B1,B2", SC.MULTI_STEP, ids=[m[0] for m in SC.MULTI_STEP])
def test_b_two_calls_back_to_back_share_the_contexts_buffers_in_stream_order(case_id, B1, B2, ctx):
    case = SC.BY_ID[case_id]
    eng = ctx(case.ctx)
    calls = []
    try:
        calls = [Staged(eng, case, B1, "/b/first"), Staged(eng, case, B2, "/b/second")]
        for st in calls:
            st.compute_want()
        with HR.streams(SWEEP + 1) as (reader, *callers):   # (every hardware queue in turn, as in (a))
            for S in callers:
                for st in reversed(calls):
                    st.reset()
                S.gate()
                for st in calls:
                    _status(st, st.enqueue(S))
                _assert_held(S)
                for st in calls:
                    st.assert_not_started(reader)
                _assert_held(S)
                S.release()
                for st in calls:
                    st.check_done()
    finally:
        for st in calls:
            st.free()


# ---- (c) growth: the second call is larger than anything the context has seen, the first may still be running --------------
@pytest.mark.parametrize("case_id,B1,B2", SC.MULTI_STEP, ids=[m[0] for m in SC.MULTI_STEP])
def test_c_a_call_that_grows_the_contexts_buffers_keeps_both_results(case_id, B1, B2, ctx):
    """Not gated: a call that has to grow a buffer of the context may wait for the device (hipFree does), as the header says."""
    case = SC.BY_ID[case_id]
    shared = ctx(case.ctx)          # the null-stream results come from a context with the same keys
    fresh = make_engine(case.ctx)   # has never run anything
    calls = []
    try:
        calls = [Staged(shared, case, GROWTH_SCALE * B1, "/c/first"), Staged(shared, case, GROWTH_SCALE * B2, "/c/second")]
        for st in calls:
            st.compute_want().reset(warm=False)
        with HR.streams(1) as (S,):
            _status(calls[0], calls[0].enqueue(S, fresh), fresh)
            running = S.busy()
            t0 = time.perf_counter()
            st2 = calls[1].enqueue(S, fresh)
            dt = time.perf_counter() - t0
            _status(calls[1], st2, fresh)
            S.synchronize()
            print(f"growth {case_id}: B {calls[0].r.B} then {calls[1].r.B}; first call still in flight at the second: {running}; "
                  f"the growing call took {dt * 1e3:.2f} ms on the host")
            for st in calls:
                st.check_done(fresh)
    finally:
        for st in calls:
            st.free()
        fresh.close()


# ---- (d) two streams of one context ordered by an event -------------------------------------------------------------------
def test_d_two_streams_of_one_context_ordered_by_an_event(ctx):
    eng, B, n_bits = ctx("T"), 2, 3
    calls, done = [], HR.Event()
    try:
        cbs = Staged(eng, SC.BY_ID["circuit_bootstrap-T-B5"], B * n_bits, "/d")
        calls.append(cbs)
        rot = Staged(eng, SC.BY_ID["blind_rotation-T-B1-bits3"], B, "/d", alias={"shift": cbs.work["ggsw"]})
        calls.append(rot)
        cbs.compute_want()          # leaves the selectors where the rotation reads them
        rot.compute_want()
        cbs.reset()
        rot.reset()
        with HR.streams(3) as (S1, S2, reader):
            S1.gate()
            _status(cbs, cbs.enqueue(S1))
            done.record(S1)
            gate2 = S2.gate()
            S2.wait_event(done)
            _status(rot, rot.enqueue(S2))
            _assert_held(S1, S2)
            cbs.assert_not_started(reader)
            rot.assert_not_started(reader)
            gate2.open()            # S2 is now held by the event alone
            rot.assert_not_started(reader)
            assert S2.busy() and S1.busy()
            S1.release()
            S2.release()
            cbs.check_done()
            rot.check_done()
    finally:
        for st in calls:
            st.free()
        done.destroy()


# ---- (e) two contexts on two streams share nothing ------------------------------------------------------------------------
def test_e_two_contexts_on_two_streams_share_nothing(ctx):
    engines = (ctx("T"), ctx("T", salt=1))
    plan = (("circuit_bootstrap-T-B5", (3, 4)), ("keyswitch-T-B3", (5, 2)), ("blind_rotation-T-B1-bits2", (2, 3)))
    calls = []
    try:
        for case_id, batches in plan:
            for i, eng in enumerate(engines):
                calls.append(Staged(eng, SC.BY_ID[case_id], batches[i], f"/e/{i}").compute_want())
        for st in calls:
            st.reset()
        assert not same_words(calls[0].want[:3], calls[1].want[:3])   # different keys, different operands
        with HR.streams(3) as (SA, SB, reader):
            SA.gate()
            SB.gate()
            for i, st in enumerate(calls):     # context A, context B, A, B, ...: interleaved call by call
                _status(st, st.enqueue((SA, SB)[i % 2]))
            _assert_held(SA, SB)
            for st in calls:
                st.assert_not_started(reader)
            for S in (SA, SB):                 # opened together
                for g in S.gates:
                    g.open()
            SA.release()
            SB.release()
            for st in calls:
                st.check_done()
    finally:
        for st in calls:
            st.free()


# ---- (f) the timing bracket is recorded on the caller's stream ------------------------------------------------------------
def test_f_timing_brackets_are_recorded_on_the_callers_stream(ctx):
    eng = ctx("T")
    calls = []
    try:
        calls = [Staged(eng, SC.BY_ID["keyswitch-T-B3"], 3, "/f"), Staged(eng, SC.BY_ID["cmux-T-B1"], 1, "/f")]
        for st in calls:
            st.compute_want().reset()
        eng.set_timing(True)
        for family in ("keyswitch", "cmux"):
            eng.last_kernel_ms(family)         # (clears the record)
        with HR.streams(2) as (S, reader):
            S.gate()
            for st in calls:
                _status(st, st.enqueue(S))
            _assert_held(S)
            for st in calls:
                st.assert_not_started(reader)
            S.release()
            for family in ("keyswitch", "cmux"):
                ms, launches = eng.last_kernel_ms(family)
                print(f"timing on a caller's stream: {family} {ms:.4f} ms over {launches} launch(es)")
                assert launches == 1 and np.isfinite(ms) and ms > 0, (family, ms, launches)
            for st in calls:
                st.check_done()
    finally:
        eng.set_timing(False)
        for family in ("keyswitch", "cmux"):
            eng.last_kernel_ms(family)
        for st in calls:
            st.free()


# ---- (g) spf_device_download waits for the stream it is given -------------------------------------------------------------
def test_g_device_download_waits_for_the_callers_stream(ctx):
    eng = ctx("T")
    st = Staged(eng, SC.BY_ID["circuit_bootstrap-T-B5"], 5, "/g")
    try:
        st.compute_want().reset()
        with HR.streams(1) as (S,):
            _status(st, st.enqueue(S))         # not gated: the download is what waits
            got = np.empty_like(st.want)
            eng.device_download(S.handle, got, st.kept)
            assert same_words(got, st.want)
            S.synchronize()
            st.check_done()
    finally:
        st.free()
