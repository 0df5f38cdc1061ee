"""The plaintext polynomial linear maps over GLWE ciphertexts (`glwe_polynomial_mad`, `glwe_scalar_mad`, `sub_glwe_ciphertexts`,
`glwe_negate_inplace`, `glwe_rotate`: sunscreen_tfhe ops/ciphertext/glwe_ciphertext_ops.rs:164-183, :189-202, :121-141, :147-156,
:285-305) on the GPU.  The operation is wrapping 64-bit integer arithmetic in Z_2^64[X]/(X^N + 1): every output word equals
tests/glwe_poly_cases.py's `poly_linear_ref`.  There is no tolerance in this file but the noise bound of the decrypt-level case."""
import functools

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import glwe_poly_cases as GC
from tests import hip_runtime as HR
from tests import pbs_graph_cases as K
from tests import poly_ref
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu
U = np.uint64
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
NO_KEY, INVALID = 3, 1
PARAMS = {"tuned": O.DEFAULT_128, "n128k2": K.TEST1, "n16k1": K.SMALL16}     # (N, k) = (2048, 1), (128, 2), (16, 1)
VT = GC.row_tile()
PATHS = ["lds", "stream"]


def dims(which):
    P = PARAMS[which]
    return P.k + 1, P.N


def engine_params(which):
    return to_engine_params(PARAMS[which]) if which == "tuned" else K.engine_params(PARAMS[which])


@pytest.fixture(scope="module")
def engines():
    """the three contexts, each made when a test first asks for it; no keys: the operation needs none"""
    made = {}

    def get(which):
        if which not in made:
            made[which] = spf_amd.Engine(engine_params(which))
        return made[which]
    yield get
    for e in made.values():
        e.close()


def load(eng, slot, triple, M, Kk, bias=None):
    eng.load_glwe_poly_weights(slot, triple, bias, shape=(M, Kk))


def run(eng, monkeypatch, path, slot, x, triple):
    """one host-pointer call under SPF_GLWE_POLY_PATH = path (None: unset), and the kernel it must report"""
    if path is None:
        monkeypatch.delenv("SPF_GLWE_POLY_PATH", raising=False)
    else:
        monkeypatch.setenv("SPF_GLWE_POLY_PATH", path)
    got = eng.glwe_poly_linear(slot, x)
    assert eng.last_glwe_poly_kernel() == GC.kernel_name(triple, path), path
    return got


def assert_words(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (what, bad[:8])


# ---- shapes across the row tile ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (VT - 1, 2, 3), (VT, 5, 1), (VT + 1, 1, 3), (2 * VT + 1, 2, 1), (VT, 2, 3), (2 * VT + 1, 5, 3)]
assert {s[0] for s in SHAPES} == {1, VT - 1, VT, VT + 1, 2 * VT + 1} and {s[1] for s in SHAPES} == {1, 2, 5} and {s[2] for s in SHAPES} == {1, 3}


@functools.lru_cache(maxsize=4)
def shape_case(M, Kk, B, k1, N):
    general = GC.csr(GC.random_polys(10, M, Kk, N, terms=3, cls="mixed", empty_every=4), M, Kk)
    constants = GC.csr(GC.random_polys(11, M, Kk, N, terms=2, cls="constants", empty_every=5), M, Kk)
    bias, x = GC.random_bias(12, M, N), GC.uniform_inputs(13, B, Kk, k1, N)
    wants = GC.poly_linear_ref(x, general, M, Kk, bias), GC.poly_linear_ref(x, constants, M, Kk, bias)
    for a in (bias, x) + wants:
        a.setflags(write=False)
    return general, constants, bias, x, wants


@pytest.mark.parametrize("M,Kk,B", SHAPES)
@pytest.mark.parametrize("which", list(PARAMS))
def test_words_equal_the_reference_across_the_row_tile(engines, monkeypatch, which, M, Kk, B):
    eng, (k1, N) = engines(which), dims(which)
    general, constants, bias, x, (want_g, want_c) = shape_case(M, Kk, B, k1, N)
    load(eng, 3, general, M, Kk, bias)
    for path in (None, "lds", "stream"):                                     # a general slot: the LDS kernel whatever the variable says
        assert_words(run(eng, monkeypatch, path, 3, x, general), want_g, (which, M, Kk, B, path))
    load(eng, 3, constants, M, Kk, bias)
    for path in (None, "lds", "stream"):                                     # a constants-only slot: either kernel
        assert_words(run(eng, monkeypatch, path, 3, x, constants), want_c, (which, M, Kk, B, path))


# ---- exponents at every seam ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(PARAMS))
def test_exponents_at_every_seam_alone_and_mixed(engines, monkeypatch, which):
    eng, (k1, N) = engines(which), dims(which)
    seams = GC.seam_exponents(N)
    assert {0, 1, N - 1, N // 2} <= set(seams) and (N != 2048 or {255, 256, 257} <= set(seams))
    # row m < len(seams): the monomial -3 X^seam on operand 0; the last row: every seam in ONE polynomial, and on operand 1
    M, Kk, B = len(seams) + 1, 2, 2
    polys = [[[(e, -3)], []] for e in seams] + [[[(e, 5 + i) for i, e in enumerate(seams)], [(e, -1 - i) for i, e in enumerate(reversed(seams))]]]
    triple = GC.csr(polys, M, Kk)
    x = GC.uniform_inputs(20, B, Kk, k1, N)
    load(eng, 0, triple, M, Kk)
    got = run(eng, monkeypatch, None, 0, x, triple)
    assert_words(got, GC.poly_linear_ref(x, triple, M, Kk), which)
    for m, e in enumerate(seams):                                            # ... and each monomial row by its own definition
        assert np.array_equal(got[:, m], U(-3 & GC.M64) * poly_ref.mul_monomial(x[:, 0], e)), (which, e)


# ---- dense and empty weights ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(PARAMS))
def test_a_dense_polynomial_equals_the_toeplitz_product(engines, monkeypatch, which):
    eng, (k1, N) = engines(which), dims(which)
    d = np.random.default_rng([0xF5, N]).integers(GC.INT64_MIN, GC.INT64_MAX, (1, 1, N), dtype=np.int64, endpoint=True)
    d[d == 0] = 1
    x = GC.uniform_inputs(21, 2, 1, k1, N)
    eng.load_glwe_poly_weights(1, d)                                         # the dense form of the binding
    assert eng.glwe_poly_slot_shape(1) == (1, 1, N, False)
    got = eng.glwe_poly_linear(1, x)
    assert eng.last_glwe_poly_kernel() == GC.LDS
    want = poly_ref.negacyclic_mul(x.reshape(-1, N), d[0, 0].view(np.uint64)).reshape(x.shape)
    assert_words(got, want, which)


@pytest.mark.parametrize("which", list(PARAMS))
def test_empty_polynomials_rows_columns_and_matrices(engines, monkeypatch, which):
    eng, (k1, N) = engines(which), dims(which)
    M, Kk, B = VT + 2, 3, 2
    polys = GC.random_polys(22, M, Kk, N, terms=2, cls="seams")
    polys[1] = [[] for _ in range(Kk)]                                       # a whole empty row inside the first tile
    for m in range(M):
        polys[m][1] = []                                                     # a whole empty column: its operand is never staged
    polys[VT][0] = polys[VT + 1][0] = []                                     # the second tile has terms at k = 2 only
    triple = GC.csr(polys, M, Kk)
    x, bias = GC.uniform_inputs(23, B, Kk, k1, N), GC.random_bias(24, M, N)
    load(eng, 2, triple, M, Kk, bias)
    got = run(eng, monkeypatch, None, 2, x, triple)
    assert_words(got, GC.poly_linear_ref(x, triple, M, Kk, bias), which)
    poisoned = x.copy()
    poisoned[:, 1] = ~poisoned[:, 1]                                         # the empty column's operand decides nothing
    assert np.array_equal(run(eng, monkeypatch, None, 2, poisoned, triple), got)
    assert not got[:, 1, :k1 - 1].any() and np.array_equal(got[:, 1, k1 - 1], np.broadcast_to(bias[1], (B, N)))
    # an empty matrix: T = 0, the bias alone, on each kernel; and with no bias either, zero
    empty = GC.csr([[[] for _ in range(Kk)] for _ in range(M)], M, Kk)
    for b in (bias, None):
        load(eng, 2, empty, M, Kk, b)
        assert eng.glwe_poly_slot_shape(2) == (M, Kk, 0, b is not None)
        for path in (None, "lds"):
            got = run(eng, monkeypatch, path, 2, x, empty)
            assert_words(got, GC.poly_linear_ref(x, empty, M, Kk, b), (which, path))
            assert not got[:, :, :k1 - 1].any()


# ---- coefficients, duplicates, bias -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("inputs", ["uniform", "ones", "extreme"])
@pytest.mark.parametrize("which", ["tuned", "n16k1"])
def test_extreme_coefficients_on_each_kernel(engines, monkeypatch, which, inputs):
    eng, (k1, N) = engines(which), dims(which)
    cs = GC.EXTREME_COEFFICIENTS
    M, Kk, B = len(cs) + 1, 2, 2
    x = {"uniform": GC.uniform_inputs(30, B, Kk, k1, N), "ones": GC.ones_inputs(B, Kk, k1, N), "extreme": GC.extreme_inputs(B, Kk, k1, N)}[inputs]
    if inputs != "uniform":
        assert set(np.unique(x).tolist()) <= {0, GC.M64}
    for e in (0, N - 1):                                                     # e = 0: a constants-only slot, on both kernels
        polys = [[[(e, c)], [(e, cs[-1 - i])]] for i, c in enumerate(cs)] + [[[(e, c) for c in cs], [(0, GC.INT64_MIN), (e, GC.INT64_MIN)]]]
        triple = GC.csr(polys, M, Kk)
        load(eng, 4, triple, M, Kk)
        want = GC.poly_linear_ref(x, triple, M, Kk)
        for path in PATHS:
            assert_words(run(eng, monkeypatch, path, 4, x, triple), want, (which, inputs, e, path))


@pytest.mark.parametrize("which", list(PARAMS))
def test_duplicate_exponents_add(engines, monkeypatch, which):
    eng, (k1, N) = engines(which), dims(which)
    x = GC.uniform_inputs(31, 2, 1, k1, N)
    for e in (0, N // 2):
        dup = GC.csr([[[(e, GC.INT64_MAX), (e, GC.INT64_MAX), (e, 9), (e, -4)]]], 1, 1)   # 2 (2^63 - 1) + 5 = 3 mod 2^64
        load(eng, 5, dup, 1, 1)
        assert eng.glwe_poly_slot_shape(5) == (1, 1, 4, False)
        for path in PATHS:
            got = run(eng, monkeypatch, path, 5, x, dup)
            assert np.array_equal(got[:, 0], U(3) * poly_ref.mul_monomial(x[:, 0], e)), (which, e, path)
            assert_words(got, GC.poly_linear_ref(x, dup, 1, 1), (which, e, path))


@pytest.mark.parametrize("cls", ["constants", "seams"])
@pytest.mark.parametrize("which", list(PARAMS))
def test_the_bias_lands_on_the_body_only(engines, monkeypatch, which, cls):
    eng, (k1, N) = engines(which), dims(which)
    M, Kk, B = VT + 1, 2, 3
    triple = GC.csr(GC.random_polys(32, M, Kk, N, terms=2, cls=cls), M, Kk)
    x = GC.uniform_inputs(33, B, Kk, k1, N)
    plain = GC.poly_linear_ref(x, triple, M, Kk)
    constant = np.zeros((M, N), dtype=np.uint64)
    constant[:, 0] = U(1) << U(62)                                           # `glwe_rotate`: a constant on the body
    for path in (PATHS if cls == "constants" else [None]):
        outs = {}
        for name, bias in [("null", None), ("zero", np.zeros((M, N), dtype=np.uint64)), ("random", GC.random_bias(34, M, N)), ("constant", constant)]:
            load(eng, 6, triple, M, Kk, bias)
            outs[name] = run(eng, monkeypatch, path, 6, x, triple)
            assert_words(outs[name], GC.poly_linear_ref(x, triple, M, Kk, bias), (which, cls, path, name))
        assert np.array_equal(outs["null"], plain) and np.array_equal(outs["zero"], plain)
        for name in ("random", "constant"):
            assert np.array_equal(outs[name][:, :, :k1 - 1], plain[:, :, :k1 - 1])          # the mask polynomials: un-biased
        assert np.array_equal(outs["constant"][:, :, k1 - 1, 1:], plain[:, :, k1 - 1, 1:])
        assert np.array_equal(outs["constant"][:, :, k1 - 1, 0], plain[:, :, k1 - 1, 0] + (U(1) << U(62)))


# ---- agreement with the existing operations on the same device rows ---------------------------------------------------------

@pytest.mark.parametrize("which", list(PARAMS))
def test_agreement_with_mul_xn_and_xor_on_the_same_rows(engines, monkeypatch, which):
    eng, (k1, N) = engines(which), dims(which)
    B = 3
    x = GC.uniform_inputs(40, B, 2, k1, N)
    for e in GC.seam_exponents(N):
        mono = GC.csr([[[(e, 1)]]], 1, 1)
        load(eng, 7, mono, 1, 1)
        got = run(eng, monkeypatch, None, 7, np.ascontiguousarray(x[:, :1]), mono)
        assert np.array_equal(got.reshape(B, -1), eng.glwe_mul_xn(x[:, 0], e)), (which, e)
    add = GC.csr([[[(0, 1)], [(0, 1)]]], 1, 2)
    load(eng, 7, add, 1, 2)
    want = eng.glwe_xor(x[:, 0], x[:, 1])
    for path in PATHS:
        assert np.array_equal(run(eng, monkeypatch, path, 7, x, add).reshape(B, -1), want), (which, path)


# ---- the device-pointer form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which,cls", [("tuned", "constants"), ("tuned", "mixed"), ("n128k2", "constants"), ("n16k1", "mixed")])
def test_nothing_but_the_output_is_written(engines, monkeypatch, which, cls, path):
    eng, (k1, N) = engines(which), dims(which)
    M, Kk, B, guard = VT + 1, 2, 3, 2
    W = k1 * N
    triple = GC.csr(GC.random_polys(41, M, Kk, N, terms=2, cls=cls), M, Kk)
    bias = GC.random_bias(42, M, N)
    load(eng, 8, triple, M, Kk, bias)
    monkeypatch.setenv("SPF_GLWE_POLY_PATH", path)
    x = GC.uniform_inputs(43, B, Kk, k1, N)
    row = M * W
    d_in, d_out = eng.device_alloc(x.nbytes), eng.device_alloc((B + 2 * guard) * row * 8)
    try:
        eng.device_upload(d_in, x)
        eng.device_upload(d_out, np.full((B + 2 * guard) * row, SENTINEL, dtype=np.uint64))
        eng.glwe_poly_linear_enqueue(None, 8, 0, d_in, d_out + guard * row * 8)               # B = 0 is legal and writes nothing
        eng.glwe_poly_linear_enqueue(None, 8, B, d_in, d_out + guard * row * 8)
        assert eng.last_glwe_poly_kernel() == GC.kernel_name(triple, path)
        got = np.empty((B + 2 * guard, M, k1, N), dtype=np.uint64)
        eng.device_download(None, got, d_out)
        assert (got[:guard] == SENTINEL).all() and (got[guard + B:] == SENTINEL).all(), "words around the outputs"
        assert_words(got[guard:guard + B], GC.poly_linear_ref(x, triple, M, Kk, bias), (which, cls, path))
        back = np.empty_like(x)
        eng.device_download(None, back, d_in)
        assert np.array_equal(back, x), "the input was written"
        # an input that is 8-byte but not 16-byte aligned (the staging falls back to 8-byte loads): the same words
        d_odd = eng.device_alloc(x.nbytes + 8)
        try:
            eng.device_upload(d_odd + 8, x)
            eng.glwe_poly_linear_enqueue(None, 8, B, d_odd + 8, d_out + guard * row * 8)
            eng.device_download(None, got, d_out)
            assert_words(got[guard:guard + B], GC.poly_linear_ref(x, triple, M, Kk, bias), (which, cls, path, "odd"))
        finally:
            eng.device_free(d_odd)
        lib, h = eng._lib, eng._h
        assert lib.spf_glwe_poly_linear_enqueue(h, None, 8, B, d_in, d_in + 8) == INVALID        # overlapping ranges
        assert b"overlaps" in lib.spf_last_error(h)
        assert lib.spf_glwe_poly_linear_enqueue(h, None, 8, 1, d_out + Kk * W * 8 - 8, d_out) == INVALID
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)


# ---- the stream contract of `_enqueue` --------------------------------------------------------------------------------------
# In the manner of tests/test_gpu_lwe_linear.py: the call runs behind a closed gate on each of four non-blocking streams that are
# alive together; until the gate opens the operands hold decoys and the output a sentinel; the words are those of the null-stream
# call.

SWEEP = 4


class StagedCall:
    def __init__(self, eng, slot, B, M, Kk, k1, N, seed):
        self.eng, self.slot, self.B, self.shape = eng, slot, B, (B, M, k1, N)
        self.real, self.decoy = GC.uniform_inputs(seed, B, Kk, k1, N), GC.uniform_inputs(seed + 1, B, Kk, k1, N)
        self.in_bytes, self.out_bytes = self.real.nbytes, B * M * k1 * N * 8
        self.bufs = [eng.device_alloc(b) for b in (self.in_bytes, self.in_bytes, self.in_bytes, max(self.out_bytes, HR.MIN_READ), self.out_bytes)]
        self.src_real, self.src_decoy, self.work_in, self.work_out, self.kept = self.bufs
        eng.device_upload(self.src_real, self.real)
        eng.device_upload(self.src_decoy, self.decoy)
        HR.reserve_pinned(self.out_bytes)
        self.want = self._null_stream(self.src_real)

    def free(self):
        while self.bufs:
            self.eng.device_free(self.bufs.pop())

    def _fetch(self, ptr, shape):
        host = np.empty(shape, dtype=np.uint64)
        self.eng.device_download(None, host, ptr)
        return host

    def _null_stream(self, src):
        HR.check(HR.runtime().hipMemcpyAsync(self.work_in, src, self.in_bytes, HR.MEMCPY_DEVICE_TO_DEVICE, None), "hipMemcpyAsync")
        self.eng.glwe_poly_linear_enqueue(None, self.slot, self.B, self.work_in, self.work_out)
        return self._fetch(self.work_out, self.shape)

    def reset(self):
        assert not np.array_equal(self._null_stream(self.src_decoy), self.want)
        sentinel = np.full(int(np.prod(self.shape)), SENTINEL, dtype=np.uint64)
        self.eng.device_upload(self.work_out, sentinel)
        self.eng.device_upload(self.kept, sentinel)
        assert (self._fetch(self.work_out, self.shape) == SENTINEL).all()

    def enqueue(self, S):
        S.copy(self.work_in, self.src_real, self.in_bytes)
        self.eng.glwe_poly_linear_enqueue(S.handle, self.slot, self.B, self.work_in, self.work_out)
        S.copy(self.kept, self.work_out, self.out_bytes)
        S.copy(self.work_in, self.src_decoy, self.in_bytes)

    def assert_not_started(self, reader):
        got = reader.read(self.work_out, np.empty(self.shape, dtype=np.uint64))
        assert (got == SENTINEL).all(), "the output was written while the caller's stream was held"

    def check_done(self):
        kept = self._fetch(self.kept, self.shape)
        assert np.array_equal(kept, self.want), np.argwhere(kept != self.want)[:8]
        assert np.array_equal(self._fetch(self.work_in, self.decoy.shape), self.decoy)


def _held(S):
    assert not any(g.capped for g in S.gates), "the call returned only after the gate's cap: it waited for the device"
    assert S.busy(), "the caller's stream is idle although its gate is closed: the case proves nothing"


def _stream_weights(eng, which, cls, M, Kk):
    k1, N = dims(which)
    triple = GC.csr(GC.random_polys(50, M, Kk, N, terms=2, cls=cls), M, Kk)
    bias = GC.random_bias(51, M, N)
    load(eng, 9, triple, M, Kk, bias)
    return triple, bias


@pytest.mark.parametrize("which,cls,path", [("tuned", "mixed", "lds"), ("tuned", "constants", "stream"), ("n128k2", "constants", "lds"),
                                            ("n128k2", "seams", "stream")])
def test_enqueue_only_enqueues_on_the_callers_stream(engines, monkeypatch, which, cls, path):
    eng, (k1, N) = engines(which), dims(which)
    M, Kk = VT + 1, 2
    triple, bias = _stream_weights(eng, which, cls, M, Kk)
    monkeypatch.setenv("SPF_GLWE_POLY_PATH", path)
    st = StagedCall(eng, 9, 3, M, Kk, k1, N, 500)
    try:
        assert eng.last_glwe_poly_kernel() == GC.kernel_name(triple, path)
        assert np.array_equal(st.want, GC.poly_linear_ref(st.real, triple, M, Kk, bias))
        with HR.streams(SWEEP + 1) as (reader, *callers):
            for S in callers:
                st.reset()
                S.gate()
                st.enqueue(S)
                _held(S)
                st.assert_not_started(reader)
                _held(S)
                S.release()
                st.check_done()
    finally:
        st.free()


@pytest.mark.parametrize("which,cls", [("tuned", "mixed"), ("n128k2", "constants")])
def test_two_enqueues_back_to_back_stay_in_stream_order(engines, monkeypatch, which, cls):
    eng, (k1, N) = engines(which), dims(which)
    M, Kk = VT + 1, 2
    triple, bias = _stream_weights(eng, which, cls, M, Kk)
    monkeypatch.delenv("SPF_GLWE_POLY_PATH", raising=False)
    calls = []
    try:
        calls = [StagedCall(eng, 9, 2, M, Kk, k1, N, 600), StagedCall(eng, 9, 5, M, Kk, k1, N, 700)]
        for st in calls:
            assert np.array_equal(st.want, GC.poly_linear_ref(st.real, triple, M, Kk, bias))
        with HR.streams(SWEEP + 1) as (reader, *callers):
            for S in callers:
                for st in reversed(calls):
                    st.reset()
                S.gate()
                for st in calls:
                    st.enqueue(S)
                _held(S)
                for st in calls:
                    st.assert_not_started(reader)
                _held(S)
                S.release()
                for st in calls:
                    st.check_done()
    finally:
        for st in calls:
            st.free()


# ---- statuses, reload, group ------------------------------------------------------------------------------------------------

def test_statuses_with_a_device_and_reload(monkeypatch):
    P = K.TEST1
    eng = spf_amd.Engine(K.engine_params(P))
    monkeypatch.delenv("SPF_GLWE_POLY_PATH", raising=False)
    try:
        lib, h = eng._lib, eng._h
        k1, N = P.k + 1, P.N
        W = k1 * N
        x, out = np.zeros((4, 2, W), dtype=np.uint64), np.zeros((4, 2, W), dtype=np.uint64)
        off, exp, coef = np.array([0, 1, 2], dtype=np.uint32), np.array([0, 5], dtype=np.uint32), np.array([3, -4], dtype=np.int64)
        xp, op, o, e, c = (a.ctypes.data for a in (x, out, off, exp, coef))

        def message():
            return lib.spf_last_error(h).decode()
        assert lib.spf_glwe_poly_linear_batch(h, 0, 1, xp, op) == NO_KEY                       # an empty slot
        assert lib.spf_glwe_poly_linear_enqueue(h, None, 63, 1, xp, op) == NO_KEY
        with pytest.raises(spf_amd.SpfError) as err:
            eng.glwe_poly_slot_shape(0)
        assert err.value.status == NO_KEY
        assert lib.spf_glwe_poly_linear_batch(h, 64, 1, xp, op) == INVALID                     # slot 64
        assert lib.spf_glwe_poly_linear_enqueue(h, None, 64, 1, xp, op) == INVALID
        assert lib.spf_load_glwe_poly_weights(h, 64, 1, 2, o, e, c, None) == INVALID and "64" in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 0, 2, o, e, c, None) == INVALID and "M = 0" in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 2, 0, o, e, c, None) == INVALID and "K = 0" in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 4097, 1, o, e, c, None) == INVALID and "4097" in message() and "4096" in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 4096, 1025, o, e, c, None) == INVALID and "1025" in message() and str(1 << 22) in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, None, e, c, None) == INVALID and "null" in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, o, None, c, None) == INVALID and "null" in message()
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, o, e, None, None) == INVALID and "null" in message()
        bad = np.array([1, 1, 2], dtype=np.uint32)
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, bad.ctypes.data, e, c, None) == INVALID and "offsets[0] = 1" in message()
        bad = np.array([0, 2, 1], dtype=np.uint32)
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, bad.ctypes.data, e, c, None) == INVALID and "offsets[1] = 2" in message()
        bad = np.array([0, 1, (1 << 24) + 1], dtype=np.uint32)                                 # the cap, from the last offset alone
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, bad.ctypes.data, e, c, None) == INVALID and str((1 << 24) + 1) in message()
        bad = np.array([0, N], dtype=np.uint32)
        assert lib.spf_load_glwe_poly_weights(h, 0, 1, 2, o, bad.ctypes.data, c, None) == INVALID and f"exponents[1] = {N}" in message()
        assert lib.spf_glwe_poly_linear_batch(h, 0, 1, xp, op) == NO_KEY                       # nothing of that loaded anything
        for args in [(64, (off, exp, coef)), (0, (off, np.array([0, N], dtype=np.uint32), coef))]:   # ... and through Python
            with pytest.raises(spf_amd.SpfError) as err:
                eng.load_glwe_poly_weights(args[0], args[1], shape=(1, 2))
            assert err.value.status == INVALID
        with pytest.raises(spf_amd.SpfError) as err:
            eng.glwe_poly_linear(0, x[:1])
        assert err.value.status == NO_KEY
        # a load, then the argument checks of the calls
        ta = (off, exp, coef)
        ba = GC.random_bias(60, 1, N)
        eng.load_glwe_poly_weights(0, ta, ba, shape=(1, 2))
        assert eng.glwe_poly_slot_shape(0) == (1, 2, 2, True)
        xa = GC.uniform_inputs(61, 3, 2, k1, N)
        assert np.array_equal(eng.glwe_poly_linear(0, xa), GC.poly_linear_ref(xa, ta, 1, 2, ba))
        assert np.array_equal(eng.glwe_poly_linear(0, xa.reshape(3, 2, W)), GC.poly_linear_ref(xa, ta, 1, 2, ba))
        assert lib.spf_glwe_poly_linear_batch(h, 0, 1, None, op) == INVALID                    # null pointers
        assert lib.spf_glwe_poly_linear_batch(h, 0, 1, xp, None) == INVALID
        assert lib.spf_glwe_poly_linear_batch(h, 0, 0, xp, op) == 0                            # B = 0
        assert lib.spf_glwe_poly_linear_batch(h, 0, 1 << 40, xp, op) == INVALID
        assert lib.spf_glwe_poly_linear_batch(h, 0, 2, xp, xp + 8) == INVALID and "overlaps" in message()
        with pytest.raises(spf_amd.SpfError):                                                  # the binding checks the operand's shape
            eng.glwe_poly_linear(0, xa[:, :1])
        sz, flag = spf_amd._ffi._SZ(), spf_amd._ffi.C.c_int()
        assert lib.spf_glwe_poly_slot_shape(h, 0, None, None, None, None) == INVALID
        assert lib.spf_glwe_poly_slot_shape(h, 64, spf_amd._ffi.C.byref(sz), spf_amd._ffi.C.byref(sz), spf_amd._ffi.C.byref(sz),
                                            spf_amd._ffi.C.byref(flag)) == INVALID
        # two slots alive at once; a reload with another shape replaces the slot and slot_shape follows
        tb = GC.csr(GC.random_polys(62, VT + 2, 3, N, terms=2, cls="constants"), VT + 2, 3)
        eng.load_glwe_poly_weights(63, tb, shape=(VT + 2, 3))
        xb = GC.uniform_inputs(63, 2, 3, k1, N)
        assert np.array_equal(eng.glwe_poly_linear(63, xb), GC.poly_linear_ref(xb, tb, VT + 2, 3))
        assert eng.last_glwe_poly_kernel() == GC.STREAM
        assert np.array_equal(eng.glwe_poly_linear(0, xa), GC.poly_linear_ref(xa, ta, 1, 2, ba))
        assert eng.last_glwe_poly_kernel() == GC.LDS
        eng.load_glwe_poly_weights(0, tb, shape=(VT + 2, 3))
        assert eng.glwe_poly_slot_shape(0) == (VT + 2, 3, len(tb[1]), False)
        assert np.array_equal(eng.glwe_poly_linear(0, xb), GC.poly_linear_ref(xb, tb, VT + 2, 3))
        with pytest.raises(spf_amd.SpfError):
            eng.glwe_poly_linear(0, xa)                                                        # the old shape is gone
        # a load refused by its checks leaves the slot as it was
        assert lib.spf_load_glwe_poly_weights(h, 0, 0, 2, o, e, c, None) == INVALID
        assert eng.glwe_poly_slot_shape(0)[:2] == (VT + 2, 3)
        ms_before = eng.last_kernel_ms("glwe_poly_linear")
        assert ms_before == (0.0, 0)
        eng.set_timing(True)
        eng.glwe_poly_linear(0, xb)
        ms, launches = eng.last_kernel_ms("glwe_poly_linear")
        eng.set_timing(False)
        assert launches == 1 and ms > 0.0                                                      # one launch whatever the shape
    finally:
        eng.close()


@pytest.mark.parametrize("which,cls", [("tuned", "mixed"), ("n128k2", "constants")])
def test_group_over_one_device_twice_is_word_equal_to_one_context(engines, monkeypatch, which, cls):
    eng, (k1, N) = engines(which), dims(which)
    monkeypatch.delenv("SPF_GLWE_POLY_PATH", raising=False)
    M, Kk, B = VT + 1, 2, 3
    triple = GC.csr(GC.random_polys(70, M, Kk, N, terms=2, cls=cls), M, Kk)
    bias = GC.random_bias(71, M, N)
    x = GC.uniform_inputs(72, B, Kk, k1, N)
    load(eng, 10, triple, M, Kk, bias)
    want = eng.glwe_poly_linear(10, x)
    assert np.array_equal(want, GC.poly_linear_ref(x, triple, M, Kk, bias))
    grp = spf_amd.Group(engine_params(which), devices=[0, 0])
    try:
        with pytest.raises(spf_amd.SpfError) as e:
            grp.glwe_poly_linear(10, x)                                                        # no weights yet
        assert e.value.status == NO_KEY
        grp.load_glwe_poly_weights(10, triple, bias, shape=(M, Kk))
        assert grp.glwe_poly_slot_shape(10) == (M, Kk, len(triple[1]), True)
        assert np.array_equal(grp.glwe_poly_linear(10, x), want)                               # ragged: 2 + 1
        for i in range(2):                                                                     # every member ran its shard
            assert grp.member(i).last_glwe_poly_kernel() == GC.kernel_name(triple), i
        with pytest.raises(spf_amd.SpfError):
            grp.glwe_poly_linear(11, x)
    finally:
        grp.close()


# ---- decryption -------------------------------------------------------------------------------------------------------------

def test_decryption_of_the_map_is_the_plaintext_product(engines, monkeypatch):
    """tests/test_glwe_poly_reference.py's decrypt-level case through the GPU: the phase of out_m is within E * ||w[m]||_1 of the
    plaintext product of the packed messages, and the words are the reference's"""
    eng, (k1, N) = engines("n128k2"), dims("n128k2")
    k, Kk, M, E = k1 - 1, 3, 2, 1 << 20
    rng = np.random.default_rng(0xF4)
    sk = poly_ref.binary_key(rng, k * N)
    msgs = rng.integers(0, 16, (Kk, N), dtype=np.uint64) << U(60)
    x = poly_ref.glwe_encrypt(rng, sk, msgs, E)[None]
    polys = GC.random_polys(7, M, Kk, N, terms=4, cls="small")
    triple = GC.csr(polys, M, Kk)
    bias = rng.integers(0, 16, (M, N), dtype=np.uint64) << U(60)
    load(eng, 12, triple, M, Kk, bias)
    out = run(eng, monkeypatch, None, 12, x, triple)
    assert np.array_equal(out, GC.poly_linear_ref(x, triple, M, Kk, bias))
    phase = poly_ref.glwe_phase(out[0], sk)
    plain = GC.poly_linear_ref(msgs[None, :, None, :], triple, M, Kk, bias)[0, :, 0]
    for m in range(M):
        norm1 = sum(abs(c) for kk in range(Kk) for _, c in polys[m][kk])
        err = np.abs((phase[m] - plain[m]).view(np.int64))
        assert int(err.max()) <= E * norm1 and err.any(), (m, int(err.max()), E * norm1)
