"""The plaintext linear maps over LWE ciphertexts (`scalar_mul_ciphertext_mad` + `add_lwe_inplace`, sunscreen_tfhe
ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18) on the GPU.  The operation is wrapping 64-bit integer arithmetic: every output
word equals tests/lwe_linear_cases.py's `linear_ref`.  There is no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import hip_runtime as HR
from tests import lwe_linear_cases as LC
from tests import pbs_graph_cases as K
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
NO_KEY, INVALID = 3, 1
LWE0, LWE1 = 0, 1
PARAMS = {"tuned": O.DEFAULT_128, "n128k2": K.TEST1, "n16k1": K.SMALL16}     # tuned: lwe0 has 638 words, lwe1 2049
PATHS = ["valu", "mfma"]


def words(which, kind):
    P = PARAMS[which]
    return (P.lwe_n if kind == LWE0 else P.k * P.N) + 1


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


def run(eng, monkeypatch, path, slot, x, kind, weights):
    """one host-pointer call on the forced path; the name of the product kernel it must report"""
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", path)
    got = eng.lwe_linear(slot, x, kind)
    assert eng.last_lwe_linear_kernel() == (LC.VALU if path == "valu" else LC.kernel_name(weights)), path
    return got


# ---- shapes that straddle every seam ----------------------------------------------------------------------------------------
# M and K below, at and above the 128-row and 128-column tiles, K across two rounds and a ragged third, B 1 and 3; every value
# of every axis, and the all-ragged corner.  8 B W is no multiple of the 128-column tile for any of the six (context, kind) pairs.
SHAPES = [(1, 1, 1), (127, 127, 3), (128, 128, 1), (129, 129, 3), (1, 257, 1), (128, 1, 3), (127, 257, 1), (129, 257, 3)]
assert {s[0] for s in SHAPES} == {1, 127, 128, 129} and {s[1] for s in SHAPES} == {1, 127, 128, 129, 257} and {s[2] for s in SHAPES} == {1, 3}


@functools.lru_cache(maxsize=4)
def shape_case(M, Kk, B, W):
    w = LC.class_weights(20, M, Kk, 2)
    bias = np.random.default_rng([0xE4, M]).integers(0, 1 << 64, M, dtype=np.uint64)
    x = LC.uniform_inputs(21, B, Kk, W)
    want = LC.linear_ref(x, w, bias)
    for a in (w, bias, x, want):
        a.setflags(write=False)
    return w, bias, x, want


@pytest.mark.parametrize("M,Kk,B", SHAPES)
@pytest.mark.parametrize("kind", [LWE0, LWE1])
@pytest.mark.parametrize("which", list(PARAMS))
def test_words_equal_the_reference_across_the_seams(engines, monkeypatch, which, kind, M, Kk, B):
    eng, W = engines(which), words(which, kind)
    w, bias, x, want = shape_case(M, Kk, B, W)
    eng.load_lwe_linear_weights(3, w, bias)
    for path in PATHS:
        got = run(eng, monkeypatch, path, 3, x, kind, w)
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.size == 0, (which, kind, M, Kk, B, path, bad[:8])
    monkeypatch.delenv("SPF_LWE_LINEAR_PATH")
    assert np.array_equal(eng.lwe_linear(3, x, kind), want)                  # the dispatcher's own choice
    assert eng.last_lwe_linear_kernel() in (LC.VALU, LC.kernel_name(w))


def test_the_dispatchers_own_choice_on_each_side_of_its_boundary(engines, monkeypatch):
    """profiles/r24_lwe_linear.md: at K = 256 the VALU kernel won at every M measured; at K = 1024 one limb won from a full row
    tile on, three limbs only from two full tiles; a ragged second tile (M = 129) loses what a full one wins"""
    eng, W = engines("n16k1"), words("n16k1", LWE0)
    monkeypatch.delenv("SPF_LWE_LINEAR_PATH", raising=False)
    for M, Kk, cls, matrix_cores in [(128, 256, 1, False), (1024, 256, 1, False), (128, 1024, 1, True), (64, 1024, 1, False),
                                     (128, 1024, 3, False), (256, 1024, 3, True), (129, 2048, 3, False), (129, 2048, 1, True),
                                     (128, 1024, "int64", False)]:
        w, x = LC.class_weights(40, M, Kk, cls), LC.uniform_inputs(41, 1, Kk, W)
        eng.load_lwe_linear_weights(9, w)
        got = eng.lwe_linear(9, x, LWE0)
        assert eng.last_lwe_linear_kernel() == (LC.kernel_name(w) if matrix_cores else LC.VALU), (M, Kk, cls)
        assert np.array_equal(got, LC.linear_ref(x, w)), (M, Kk, cls)


# ---- weight classes, extreme operands, bias ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [1, 2, 3, "ends", "beyond", "int64"])
@pytest.mark.parametrize("which,kind", [("tuned", LWE0), ("n128k2", LWE1)])
def test_weight_classes_on_each_path(engines, monkeypatch, which, kind, cls):
    """uniform in each class with its two end values planted; every weight at an end of a class; the first value beyond three
    limbs; INT64_MIN, -1, 0, INT64_MAX.  The last two classes have no limb image: forcing the matrix cores changes nothing."""
    eng, W = engines(which), words(which, kind)
    M, Kk, B = 5, 131, 2
    w = LC.class_weights(22, M, Kk, cls)
    if cls == "int64":
        assert {LC.INT64_MIN, -1, 0, LC.INT64_MAX} <= set(w.reshape(-1).tolist())
    elif cls == "beyond":
        assert int(w.max()) == LC.FIRST_BEYOND[1]
    elif cls != "ends":
        assert (int(w.min()), int(w.max())) == LC.CLASS_RANGES[cls]
    x = LC.uniform_inputs(23, B, Kk, W)
    want = LC.linear_ref(x, w)
    eng.load_lwe_linear_weights(0, w)
    for path in PATHS:
        assert np.array_equal(run(eng, monkeypatch, path, 0, x, kind, w), want), (which, cls, path)
    if cls == "beyond":                                                       # ... and the first value beyond the other end
        w2 = w.copy()
        w2[w2 == LC.FIRST_BEYOND[1]] = LC.FIRST_BEYOND[0]
        eng.load_lwe_linear_weights(0, w2)
        assert np.array_equal(run(eng, monkeypatch, "mfma", 0, x, kind, w2), LC.linear_ref(x, w2))
        assert eng.last_lwe_linear_kernel() == LC.VALU


@pytest.mark.parametrize("cls", [1, "ends", "int64"])
@pytest.mark.parametrize("which,kind", [("tuned", LWE0), ("n16k1", LWE1)])
def test_extreme_operands(engines, monkeypatch, which, kind, cls):
    """input words 0, 2^64 - 1, 2^63 and 0x8080...80 (every byte plane at an end of its range) against weights at the limb ends"""
    eng, W = engines(which), words(which, kind)
    M, Kk, B = 7, 130, 2
    w = LC.class_weights(24, M, Kk, cls)
    if cls == 1:
        w = np.where(np.arange(M * Kk).reshape(M, Kk) % 2 == 0, np.int64(-127), np.int64(128))    # both ends of the one-limb class only
    x = LC.planted_inputs(25, B, Kk, W)
    assert set(np.unique(x).tolist()) == set(LC.PLANTED)
    eng.load_lwe_linear_weights(1, w)
    want = LC.linear_ref(x, w)
    for path in PATHS:
        assert np.array_equal(run(eng, monkeypatch, path, 1, x, kind, w), want), (which, cls, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which,kind", [("tuned", LWE1), ("n16k1", LWE0)])
def test_bias_null_zero_and_all_ones(engines, monkeypatch, which, kind, path):
    eng, W = engines(which), words(which, kind)
    M, Kk, B = 130, 9, 3
    w, x = LC.class_weights(26, M, Kk, 1), LC.uniform_inputs(27, B, Kk, W)
    plain = LC.linear_ref(x, w)
    outs = {}
    for name, bias in [("null", None), ("zero", np.zeros(M, dtype=np.uint64)), ("ones", np.full(M, LC.M64, dtype=np.uint64))]:
        eng.load_lwe_linear_weights(2, w, bias)
        outs[name] = run(eng, monkeypatch, path, 2, x, kind, w)
        assert np.array_equal(outs[name], LC.linear_ref(x, w, bias)), (which, path, name)
    assert np.array_equal(outs["null"], plain) and np.array_equal(outs["zero"], plain)
    assert np.array_equal(outs["ones"][..., :-1], plain[..., :-1])            # only word W - 1 differs
    assert np.array_equal(outs["ones"][..., -1], plain[..., -1] - np.uint64(1))


def test_the_int32_bound_of_the_accumulators(engines, monkeypatch):
    """K = 130 944 + 129 columns: one full segment, then a ragged round.  Every weight -128 is fed as the limbs (-128, +1) of
    +128; against input bytes 0x00 (stored plane -128) every product of the low limb is +2^14 and a full segment sums to
    130 944 * 2^14 = 2 145 386 496 < 2^31; against 0xff (plane +127) it is -128 * 127 each.  129 columns more in the same
    accumulators would pass 2^31."""
    eng, W = engines("n16k1"), words("n16k1", LWE1)
    M, Kk = 2, LC.SEG_COLUMNS + 129
    assert LC.SEG_COLUMNS * (1 << 14) < (1 << 31) < Kk * (1 << 14)
    w = np.full((M, Kk), -128, dtype=np.int64)
    assert LC.balanced_limbs(128, 2) == [-128, 1] and LC.kernel_name(w) == "pfks_gemm_kernel<2>"
    x = np.zeros((1, Kk, W), dtype=np.uint64)
    x[:, :, 1::3] = LC.M64                                                    # whole columns of 0xff bytes beside whole columns of 0x00
    x[:, 5::7, 2::3] = LC.M64                                                 # ... and columns that mix them
    assert x.nbytes < 20 << 20
    eng.load_lwe_linear_weights(5, w)
    try:
        want = LC.linear_ref(x, w)
        got = run(eng, monkeypatch, "mfma", 5, x, LWE1, w)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert not got[..., 0::3].any()
    finally:
        eng.load_lwe_linear_weights(5, np.zeros((1, 1), dtype=np.int64))      # (the images of the large matrix go back)


# ---- isolation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which,kind", [("tuned", LWE0), ("n128k2", LWE1)])
def test_an_output_depends_on_its_own_inputs_only_and_nothing_else_is_written(engines, monkeypatch, which, kind, path):
    eng, W = engines(which), words(which, kind)
    M, Kk, B, guard = 3, 5, 4, 2
    w = LC.class_weights(28, M, Kk, 3)
    bias = np.arange(1, M + 1, dtype=np.uint64)
    eng.load_lwe_linear_weights(4, w, bias)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", path)
    base = LC.uniform_inputs(29, B, Kk, W)
    row = M * W
    d_in, d_out = eng.device_alloc(base.nbytes), eng.device_alloc((B + 2 * guard) * row * 8)
    try:
        def call(x):
            eng.device_upload(d_in, x)
            eng.device_upload(d_out, np.full((B + 2 * guard) * row, SENTINEL, dtype=np.uint64))
            eng.lwe_linear_enqueue(None, 4, kind, B, d_in, d_out + guard * row * 8)
            got = np.empty((B + 2 * guard, M, W), dtype=np.uint64)
            eng.device_download(None, got, d_out)
            assert (got[:guard] == SENTINEL).all() and (got[guard + B:] == SENTINEL).all(), "words around the outputs"
            return got[guard:guard + B]
        first = call(base)
        assert np.array_equal(first, LC.linear_ref(base, w, bias))
        for b in (0, 1, B - 1):
            x = base.copy()
            x[b] = LC.uniform_inputs(30 + b, 1, Kk, W)[0]
            got = call(x)
            others = [i for i in range(B) if i != b]
            assert np.array_equal(got[others], first[others]), (which, path, b)
            assert np.array_equal(got[b], LC.linear_ref(x[b], w, bias))
            assert not np.array_equal(got[b], first[b])
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)


# ---- the stream contract of `_enqueue` --------------------------------------------------------------------------------------
# In the manner of tests/test_gpu_private_functional_keyswitch.py: the call runs behind a closed gate on each of four
# non-blocking streams that are alive together; until the gate opens the operands hold decoys and the output a sentinel; the
# words are those of the null-stream call.

SWEEP = 4


class StagedCall:
    def __init__(self, eng, slot, kind, B, M, Kk, W, seed):
        self.eng, self.slot, self.kind, self.B, self.shape = eng, slot, kind, B, (B, M, W)
        self.real, self.decoy = LC.uniform_inputs(seed, B, Kk, W), LC.uniform_inputs(seed + 1, B, Kk, W)
        self.in_bytes, self.out_bytes = self.real.nbytes, B * M * W * 8
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
        self.eng.lwe_linear_enqueue(None, self.slot, self.kind, self.B, self.work_in, self.work_out)
        return self._fetch(self.work_out, self.shape)

    def reset(self):
        """a warm call at this batch size with the decoys (nothing left to grow; the decoys give other words), then decoys in the
        input and a sentinel in the output"""
        assert not np.array_equal(self._null_stream(self.src_decoy), self.want)
        sentinel = np.full(int(np.prod(self.shape)), SENTINEL, dtype=np.uint64)
        self.eng.device_upload(self.work_out, sentinel)
        self.eng.device_upload(self.kept, sentinel)
        assert (self._fetch(self.work_out, self.shape) == SENTINEL).all()

    def enqueue(self, S):
        S.copy(self.work_in, self.src_real, self.in_bytes)
        self.eng.lwe_linear_enqueue(S.handle, self.slot, self.kind, self.B, self.work_in, self.work_out)
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


def _stream_weights(eng, M, Kk):
    w = LC.class_weights(31, M, Kk, 2)
    bias = np.arange(M, dtype=np.uint64)
    eng.load_lwe_linear_weights(6, w, bias)
    return w, bias


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which,kind", [("tuned", LWE0), ("n128k2", LWE1)])
def test_enqueue_only_enqueues_on_the_callers_stream(engines, monkeypatch, which, kind, path):
    eng, W = engines(which), words(which, kind)
    M, Kk = 3, 5
    w, bias = _stream_weights(eng, M, Kk)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", path)
    st = StagedCall(eng, 6, kind, 3, M, Kk, W, 500)
    try:
        assert eng.last_lwe_linear_kernel() == (LC.VALU if path == "valu" else LC.kernel_name(w))
        assert np.array_equal(st.want, LC.linear_ref(st.real, w, bias))
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


@pytest.mark.parametrize("which,kind", [("tuned", LWE0), ("n128k2", LWE1)])
def test_two_enqueues_back_to_back_share_the_contexts_scratch_in_stream_order(engines, monkeypatch, which, kind):
    """both write and read the context's byte planes; the second call is the larger batch, the one the planes had to grow for"""
    eng, W = engines(which), words(which, kind)
    M, Kk = 3, 5
    w, bias = _stream_weights(eng, M, Kk)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", "mfma")
    calls = []
    try:
        calls = [StagedCall(eng, 6, kind, 2, M, Kk, W, 600), StagedCall(eng, 6, kind, 7, M, Kk, W, 700)]
        assert eng.last_lwe_linear_kernel() == LC.kernel_name(w)
        for st in calls:
            assert np.array_equal(st.want, LC.linear_ref(st.real, w, bias))
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
    try:
        lib, h = eng._lib, eng._h
        W = P.lwe_n + 1
        x = np.zeros((4, 4, 2 * W), dtype=np.uint64)
        out = np.zeros((4, 4, 2 * W), dtype=np.uint64)
        w = np.ones((2, 2), dtype=np.int64)
        xp, op, wp = x.ctypes.data, out.ctypes.data, w.ctypes.data
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 1, xp, op) == NO_KEY                      # an empty slot
        assert lib.spf_lwe_linear_enqueue(h, None, 63, LWE0, 1, xp, op) == NO_KEY
        assert lib.spf_lwe_linear_batch(h, 64, LWE0, 1, xp, op) == INVALID                    # slot 64
        assert lib.spf_lwe_linear_enqueue(h, None, 64, LWE0, 1, xp, op) == INVALID
        assert lib.spf_load_lwe_linear_weights(h, 64, 2, 2, wp, None) == INVALID
        assert lib.spf_load_lwe_linear_weights(h, 0, 0, 2, wp, None) == INVALID               # M = 0, K = 0, null weights
        assert lib.spf_load_lwe_linear_weights(h, 0, 2, 0, wp, None) == INVALID
        assert lib.spf_load_lwe_linear_weights(h, 0, 2, 2, None, None) == INVALID
        assert lib.spf_load_lwe_linear_weights(h, 0, 1 << 14, (1 << 13) + 1, wp, None) == INVALID   # above the cap of 2^27 weights
        msg = eng._lib.spf_last_error(h).decode()
        assert str(1 << 14) in msg and str((1 << 13) + 1) in msg and str(1 << 27) in msg, msg
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 1, xp, op) == NO_KEY
        with pytest.raises(spf_amd.SpfError) as e:
            eng.lwe_linear(0, x[:1, :2, :W])
        assert e.value.status == NO_KEY
        with pytest.raises(spf_amd.SpfError) as e:
            eng.lwe_linear(64, x[:1, :2, :W])
        assert e.value.status == INVALID
        wa, ba = LC.class_weights(32, 2, 2, 1), np.array([5, 6], dtype=np.uint64)
        eng.load_lwe_linear_weights(0, wa, ba)
        xa = LC.uniform_inputs(33, 3, 2, W)
        assert np.array_equal(eng.lwe_linear(0, xa), LC.linear_ref(xa, wa, ba))
        for kind in (2, 3, 4, 5, -1):                                                         # not an LWE kind
            assert lib.spf_lwe_linear_batch(h, 0, kind, 1, xp, op) == INVALID
            assert lib.spf_lwe_linear_enqueue(h, None, 0, kind, 1, xp, op) == INVALID
        with pytest.raises(spf_amd.SpfError) as e:
            eng.lwe_linear(0, xa, 2)
        assert e.value.status == INVALID
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 1, None, op) == INVALID                   # null pointers
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 1, xp, None) == INVALID
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 0, xp, op) == 0                           # B = 0
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 1 << 40, xp, op) == INVALID
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 2, xp, xp + 8) == INVALID                 # overlapping ranges
        d = eng.device_alloc(1 << 16)
        try:
            assert lib.spf_lwe_linear_enqueue(h, None, 0, LWE0, 2, d, d + 8) == INVALID
            assert lib.spf_lwe_linear_enqueue(h, None, 0, LWE0, 2, d + 2 * 2 * W * 8 - 8, d) == INVALID
            assert lib.spf_lwe_linear_enqueue(h, None, 0, LWE0, 2, d, d + 2 * 2 * W * 8) == 0  # adjacent is not overlapping
            eng.device_download(None, np.empty(1, dtype=np.uint64), d)
        finally:
            eng.device_free(d)
        with pytest.raises(spf_amd.SpfError):                                                 # the binding checks the operand's shape
            eng.lwe_linear(0, xa[:, :1])
        # two slots alive at once, of different classes and kinds
        wb = LC.class_weights(34, 130, 3, "int64")
        eng.load_lwe_linear_weights(63, wb)
        xb = LC.uniform_inputs(35, 2, 3, P.k * P.N + 1)
        assert np.array_equal(eng.lwe_linear(63, xb, LWE1), LC.linear_ref(xb, wb))
        assert np.array_equal(eng.lwe_linear(0, xa), LC.linear_ref(xa, wa, ba))
        # a reload of a slot with another shape (and no bias), on each path
        for path in PATHS:
            monkeypatch.setenv("SPF_LWE_LINEAR_PATH", path)
            wc = LC.class_weights(36 + len(path), 129, 4, 3)
            eng.load_lwe_linear_weights(0, wc)
            xc = LC.uniform_inputs(37, 2, 4, W)
            assert np.array_equal(eng.lwe_linear(0, xc), LC.linear_ref(xc, wc))
            with pytest.raises(spf_amd.SpfError):
                eng.lwe_linear(0, xa)                                                         # the old shape is gone
            eng.load_lwe_linear_weights(0, wa, ba)
            assert np.array_equal(eng.lwe_linear(0, xa), LC.linear_ref(xa, wa, ba))
        # a failed load leaves the slot empty
        assert lib.spf_load_lwe_linear_weights(h, 0, 2, 2, wp, None) == 0
        assert lib.spf_load_lwe_linear_weights(h, 0, 0, 2, wp, None) == INVALID
        assert lib.spf_lwe_linear_batch(h, 0, LWE0, 1, xp, op) == 0                           # (refused before the slot was touched)
    finally:
        eng.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which,kind", [("tuned", LWE0), ("n128k2", LWE1)])
def test_group_over_one_device_twice_is_word_equal_to_one_context(engines, monkeypatch, which, kind, path):
    eng, W = engines(which), words(which, kind)
    monkeypatch.setenv("SPF_LWE_LINEAR_PATH", path)
    M, Kk, B = 4, 6, 5
    w, bias = LC.class_weights(38, M, Kk, 2), np.arange(7, 7 + M, dtype=np.uint64)
    x = LC.uniform_inputs(39, B, Kk, W)
    eng.load_lwe_linear_weights(8, w, bias)
    want = eng.lwe_linear(8, x, kind)
    assert np.array_equal(want, LC.linear_ref(x, w, bias))
    grp = spf_amd.Group(engine_params(which), devices=[0, 0])
    try:
        with pytest.raises(spf_amd.SpfError) as e:
            grp.lwe_linear(8, x, kind)                                                         # no weights yet
        assert e.value.status == NO_KEY
        grp.load_lwe_linear_weights(8, w, bias)
        assert np.array_equal(grp.lwe_linear(8, x, kind), want)                                # ragged: 3 + 2
        for i in range(2):                                                                     # every member ran its shard
            assert grp.member(i).last_lwe_linear_kernel() == (LC.VALU if path == "valu" else LC.kernel_name(w)), i
        with pytest.raises(spf_amd.SpfError):
            grp.lwe_linear(9, x, kind)
    finally:
        grp.close()


# ---- composition ------------------------------------------------------------------------------------------------------------

def test_linear_map_then_table_bootstrap_on_one_stream():
    """lwe_linear_enqueue (lwe0, K = 3, M = 2) then spf_pbs_univariate_dev on its output, on one stream with no host copy between:
    word-equal to the oracle's univariate bootstrap of linear_ref's rows"""
    P, ks, _, _ = K.keys_of("tuned")
    eng = K.make_engine("tuned")
    try:
        B, M, Kk, W = 2, 2, 3, P.lwe_n + 1
        w = np.array([[4, 1, 0], [1, -1, 2]], dtype=np.int64)
        bias = np.array([0, 1 << 60], dtype=np.uint64)
        x = K.random_lwe_batch(41, B * Kk, P.lwe_n).reshape(B, Kk, W)
        lut = spf_amd.generate_lut([lambda v: (3 * v + 1) % 8], 3, eng.params)
        eng.load_lwe_linear_weights(0, w, bias)
        rows = LC.linear_ref(x, w, bias).reshape(B * M, W)
        out_words = P.k * P.N + 1
        bufs = [eng.device_alloc(n) for n in (x.nbytes, rows.nbytes, lut.nbytes, B * M * out_words * 8)]
        d_in, d_mid, d_lut, d_out = bufs
        try:
            eng.device_upload(d_in, x)
            eng.device_upload(d_lut, lut)
            with HR.streams(1) as (S,):
                eng.lwe_linear_enqueue(S.handle, 0, LWE0, B, d_in, d_mid)
                eng.pbs_univariate_dev(S.handle, B * M, d_mid, d_lut, 0, d_out)
                S.synchronize()
            got = np.empty((B * M, out_words), dtype=np.uint64)
            eng.device_download(None, got, d_out)
            mid = np.empty_like(rows)
            eng.device_download(None, mid, d_mid)
            assert np.array_equal(mid, rows)
            for i in range(B * M):
                assert K.same_words(got[i], O.pbs_univariate(rows[i], lut, ks.bsk_fft, P)), i
        finally:
            for p in bufs:
                eng.device_free(p)
    finally:
        eng.close()
