"""The hand-written kernels' f64 -> torus conversions (`torus_bits16`, `torus_bits16_mantissa`, `untwist_sub_from_negated`:
a wave-voted fast path each, with its own magnitude window and quirk detector, and the literal sequence behind it) on the
inputs of tests/conversion_cases.py, which tests/test_conversion_regimes.py shows to sit on the chosen side of every window.
Every output word of every launch against the oracle, the kernel of every launch asserted.  DEFAULT_128 throughout, one
generic parameter set as a control."""
import functools

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import conversion_cases as C
from tests.decomp_ref import M64
from tests.polyref_cases import N128K2, key_fft
from tests.test_gpu_parity import EDGE_BATCHES, _const_key_engine, _edge_kernel
from tests.util import dev_bootstrap, random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu

P = C.P
CMUX4, CMUX2, CMUX2S = "cmux4_kernel<4,4>", "cmux_kernel<4,4,2>", "cmux_kernel<4,4,2,stream>"


@functools.lru_cache(maxsize=None)
def engine():
    ep = to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count, ss_radix_log=P.ss_radix_log,
                                     ss_radix_count=P.ss_count)
    return spf_amd.Engine(ep)


@functools.lru_cache(maxsize=None)
def cmux_cases():
    return C.cmux_cases()


@functools.lru_cache(maxsize=None)
def expected_cmux(i: int) -> np.ndarray:
    c = cmux_cases()[i]
    return O.cmux(c.d0.reshape(-1), c.d1.reshape(-1), c.ggsw, P.N, P.k, P.cbs_radix_log, P.cbs_count)


class Device:
    """device buffers through the library's own helpers, freed on exit"""

    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.eng.device_free(p)

    def alloc(self, nbytes):
        p = self.eng.device_alloc(nbytes)
        self.bufs.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        self.eng.device_upload(p, a)
        return p


def dev_cmux(eng, sel, a, b) -> np.ndarray:
    """ONE launch of spf_cmux_dev over the whole batch, a selector buffer per gate"""
    B = a.shape[0]
    out = np.empty((B, P.glwe_len), dtype=np.uint64)
    with Device(eng) as d:
        d_out = d.alloc(out.nbytes)
        eng.cmux_dev(None, B, d.up(sel), d.up(a), d.up(b), d_out)
        eng.device_download(None, out, d_out)
    return out


def first_bad(got, exp, names):
    bad = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0]
    return f"{bad.size} of {got.shape[0]} differ, first: " + ", ".join(f"{i}={names[i]}" for i in bad[:6]) if bad.size else ""


# ----------------------------------------------------------------------------------------------- CMUX


def test_cmux_every_case_in_a_launch_of_its_own():
    """B = 1: the latency shape with nothing else in the launch"""
    eng = engine()
    bad = []
    for i, c in enumerate(cmux_cases()):
        got = dev_cmux(eng, c.ggsw[None], c.d0.reshape(1, -1), c.d1.reshape(1, -1))
        assert eng.last_cmux_kernel() == CMUX4
        if not np.array_equal(got[0], expected_cmux(i)):
            bad.append(c.name)
    assert not bad, f"{len(bad)} cases differ from the oracle: {bad[:10]}"


@pytest.mark.parametrize("B,kernel", [(256, CMUX4), (257, CMUX2), (301, CMUX2), (896, CMUX2S)])
def test_cmux_classes_spread_through_every_batch_shape(B, kernel):
    """one gate per workgroup (256), two per workgroup with a half-empty last one (257, 301), and the streaming-load
    instantiation (selectors of the launch >= 224 MiB).  Every batch holds every case; the case list has an even length and
    the second cycle is shifted by one, so a case sits in both gate slots of a workgroup.  The last two gates - in the odd
    batches the full last pair's second slot and the gate alone in the ragged workgroup - are `quirk_in_window` and `mixed`"""
    eng = engine()
    cases = cmux_cases()
    m = len(cases)
    assert m <= 256
    idx = np.array([(i + i // m) % m for i in range(B)])
    name_at = {c.name: j for j, c in enumerate(cases)}
    idx[-2], idx[-1] = name_at["quirk_in_window@row1-level0-poly1"], name_at["mixed@row0-level3-poly0"]
    sel = np.stack([cases[j].ggsw for j in idx])
    a = np.stack([cases[j].d0.reshape(-1) for j in idx])
    b = np.stack([cases[j].d1.reshape(-1) for j in idx])
    got = dev_cmux(eng, sel, a, b)
    assert eng.last_cmux_kernel() == kernel, eng.last_cmux_kernel()
    assert set(idx.tolist()) == set(range(m))
    msg = first_bad(got, np.stack([expected_cmux(j) for j in idx]), [cases[j].name for j in idx])
    assert not msg, msg


@functools.lru_cache(maxsize=None)
def door_cases():
    return C.door_cases()


def oracle_cmux(c, d0, d1):
    return O.cmux(d0.reshape(-1), d1.reshape(-1), c.ggsw, P.N, P.k, P.cbs_radix_log, P.cbs_count)


@pytest.mark.parametrize("B,kernel", [(7, CMUX4), (301, CMUX2)])
def test_multiply_glwe_ggsw_door(B, kernel):
    """`d0_zero`: the product alone"""
    eng = engine()
    cases = door_cases()
    idx = np.arange(B) % len(cases)
    diff = np.stack([cases[j].diff().reshape(-1) for j in idx])
    got = eng.multiply_glwe_ggsw(diff, np.stack([cases[j].ggsw for j in idx]))
    assert eng.last_cmux_kernel() == kernel
    exp = [oracle_cmux(c, np.zeros_like(c.d0), c.diff()) for c in cases]
    msg = first_bad(got, np.stack([exp[j] for j in idx]), [cases[j].name for j in idx])
    assert not msg, msg


@pytest.mark.parametrize("B,kernel", [(7, CMUX4), (77, CMUX2)])
def test_glev_cmux_door(B, kernel):
    """`per_ggsw` = 4: the four GLWEs of a GLEV share a selector; each carries the case's digit pattern on its own d0"""
    eng = engine()
    cases = door_cases()
    idx = np.arange(B) % len(cases)
    rng = np.random.default_rng(0x61E7)
    a = {j: rng.integers(0, 1 << 64, (P.cbs_count, P.k + 1, P.N), dtype=np.uint64) for j in range(len(cases))}
    b = {j: a[j] + cases[j].diff()[None] for j in a}
    got = eng.glev_cmux(np.stack([cases[j].ggsw for j in idx]), np.stack([a[j].reshape(-1) for j in idx]),
                        np.stack([b[j].reshape(-1) for j in idx]))
    assert eng.last_cmux_kernel() == kernel
    exp = {j: np.concatenate([oracle_cmux(cases[j], a[j][l], b[j][l]) for l in range(P.cbs_count)]) for j in a}
    msg = first_bad(got, np.stack([exp[j] for j in idx]), [cases[j].name for j in idx])
    assert not msg, msg


@pytest.mark.parametrize("null_a", [False, True])
@pytest.mark.parametrize("units,kernel", [(7, CMUX4), (301, CMUX2)])
def test_cmux_scattered_door(units, kernel, null_a):
    """a table of four pointers per gate {selector, a, b, out}; a NULL `a` is the zero ciphertext.  Gates share the seven
    selector and operand buffers; outputs are laid out in reverse order"""
    eng = engine()
    cases = door_cases()
    idx = np.arange(units) % len(cases)
    out = np.empty((units, P.glwe_len), dtype=np.uint64)
    with Device(eng) as d:
        sel = [d.up(c.ggsw) for c in cases]
        a = [d.up(c.d0) for c in cases]
        b = [d.up(c.diff() if null_a else c.d1) for c in cases]
        d_out = d.alloc(out.nbytes)
        rows = P.glwe_len * 8
        table = np.array([[sel[j], 0 if null_a else a[j], b[j], d_out + (units - 1 - i) * rows] for i, j in enumerate(idx)],
                         dtype=np.uint64)
        eng.cmux_scattered_dev(None, units, d.up(table))
        eng.device_download(None, out, d_out)
    assert eng.last_cmux_kernel() == kernel
    exp = [oracle_cmux(c, np.zeros_like(c.d0), c.diff()) if null_a else oracle_cmux(c, c.d0, c.d1) for c in cases]
    msg = first_bad(out[::-1], np.stack([exp[j] for j in idx]), [cases[j].name for j in idx])
    assert not msg, msg


def test_gate_graph_level_of_cmux_nodes():
    eng = engine()
    cases = door_cases()
    g = spf_amd.FheCircuit(eng)
    outs = []
    for c in cases:
        sel = g.add_input(ValueKind.GGSW1, np.ascontiguousarray(c.ggsw))
        a, b = g.add_input(ValueKind.GLWE1, c.d0.reshape(-1)), g.add_input(ValueKind.GLWE1, c.d1.reshape(-1))
        outs.append(g.add_output(g.add_op(FheOp.CMux, [sel, a, b]), ValueKind.GLWE1))
    g.run()
    assert eng.last_cmux_kernel() == CMUX4
    for c, got in zip(cases, outs):
        assert np.array_equal(got, oracle_cmux(c, c.d0, c.d1)), c.name
    g.close()


# ----------------------------------------------------------------------------------------------- trace


@functools.lru_cache(maxsize=None)
def trace_groups():
    """the cases that share a key (same constant, round, level, polynomial): a launch takes one automorphism key"""
    groups = {}
    for c in C.trace_cases():
        groups.setdefault((c.cls.c, c.cls.scale_log2, c.rnd, c.at), []).append(c)
    return list(groups.values())


@functools.lru_cache(maxsize=None)
def trace_expected(gi: int):
    """(inputs, oracle outputs) of group gi: its cases' ciphertexts and five of uniform words"""
    grp = trace_groups()[gi]
    x = [c.glwe.reshape(-1) for c in grp] + list(random_glwe(0x7AC0 + gi, 5, P.glwe_len))
    return x, [O.mod_switch_trace_and_rotate(v, grp[0].ak, P) for v in x], [c.name for c in grp] + ["uniform"] * 5


@pytest.mark.parametrize("B", [1, 3, 300])
def test_trace_every_class_every_unit(B):
    """`cbs_trace_kernel<6,7>` (the mantissa form: windows at 2^52 and 2^116): 4 B units, several per workgroup.  B = 1: every
    case in a launch of its own; B = 3, 300: the cases of a key and uniform words cycled through the batch"""
    eng = engine()
    bad = []
    assert {c.rnd for g in trace_groups() for c in g} == {0, C.LOG_N - 1}
    # the library names no trace kernel; its launch timing brackets `cbs_trace_kernel<6,7>` alone (the generic family's trace
    # kernel is launched outside it), so exactly one timed "trace" launch per call is the assertion of the kernel reached
    eng.set_timing(True)
    try:
        eng.last_kernel_ms("trace")
        for gi, grp in enumerate(trace_groups()):
            eng.load_automorphism_key(grp[0].ak)
            x, exp, names = trace_expected(gi)
            for first in range(len(grp) if B < len(grp) else 1):
                idx = (np.arange(B) + first) % (len(grp) if B == 1 else len(x))
                got = eng.mod_switch_trace_and_rotate(np.stack([x[j] for j in idx]))
                assert eng.last_kernel_ms("trace")[1] == 1, "the launch did not go to cbs_trace_kernel<6,7>"
                msg = first_bad(got, np.stack([exp[j] for j in idx]), [names[j] for j in idx])
                if msg:
                    bad.append(msg)
    finally:
        eng.set_timing(False)
    assert not bad, f"{len(bad)} launches differ: {bad[:6]}"


# ----------------------------------------------------------------------------------------------- blind rotation


@pytest.mark.parametrize("B", EDGE_BATCHES)
@pytest.mark.parametrize("const", sorted({C.by_name(C.PBS_CLASSES, n).c for n in C.PBS_EDGE_CLASSES}))
def test_blind_rotation_mixed_outlier_and_lookalike_every_shape(B, const):
    """`test_saturating_cast_quirk_every_shape`'s rig with per-coefficient digit patterns: every third ciphertext is a vector
    of the classes that use this key constant (-2^63: mixed and one_outlier; -3 * 2^48: quirk_lookalike), the others uniform
    words with a LUT of their own"""
    P1, bsk, eng = _const_key_engine(const & M64)
    vectors = [C.pbs_vector(C.by_name(C.PBS_CLASSES, n)) for n in C.PBS_EDGE_CLASSES if C.by_name(C.PBS_CLASSES, n).c == const]
    lwe = random_lwe_batch(0xC5A7 + B, B, 1)
    luts = random_glwe(0xC5A8 + B, B, P1.glwe_len)
    for n, i in enumerate(range(0, B, 3)):
        lwe[i], luts[i] = vectors[n % len(vectors)]
    for log_v in (0, 1):
        _, exp = O.bench_generalized_pbs(lwe, luts, bsk, P1, 8, 0, log_v)
        got = dev_bootstrap(eng, lwe, luts, 0, log_v, 0)
        assert eng.last_blind_rotate_kernel() == _edge_kernel(B, bool(log_v))
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, f"log_v {log_v}: {bad.size} ciphertexts differ, first {bad[:8]}"


# ----------------------------------------------------------------------------------------------- generic family (control)


@pytest.mark.parametrize("name", ["mixed", "minus_2_63", "quirk_in_window"])
def test_generic_family_control(name):
    """N = 128, k = 2, CMUX radix 3 x 4 bits: `f64_round_to_torus` only, no fast path"""
    G = N128K2
    cls = C.by_name(C.CMUX_CLASSES, name)
    rows = np.zeros((G.k + 1, G.cbs_count, G.k + 1, G.N), dtype=np.uint64)
    rows[G.k, 0, G.k, 0] = cls.c & M64
    g = key_fft(rows)
    rng = np.random.default_rng(0x6E)
    d0 = rng.integers(0, 1 << 64, (G.k + 1, G.N), dtype=np.uint64)
    diff = rng.integers(0, 1 << 64, (G.k + 1, G.N), dtype=np.uint64)
    diff[G.k] = C.digit_words(cls.d[:G.N], G.cbs_radix_log, G.cbs_count, G.cbs_count - 1)
    d0f, d1f = d0.reshape(-1), (d0 + diff).reshape(-1)
    seen = C.classify(O.cmux_conversion_input(d0f, d1f, g, G.N, G.k, G.cbs_radix_log, G.cbs_count)[G.k])
    assert seen["quirk"].sum() > 0, "test vector no longer hits the quirk"
    exp = O.cmux(d0f, d1f, g, G.N, G.k, G.cbs_radix_log, G.cbs_count)
    eng = spf_amd.Engine(to_engine_params(G).replace(tr_radix_log=G.tr_radix_log, tr_radix_count=G.tr_count,
                                                     ss_radix_log=G.ss_radix_log, ss_radix_count=G.ss_count))
    for B in (1, 5):
        got = eng.cmux(np.broadcast_to(g, (B, g.size)), np.broadcast_to(d0f, (B, d0f.size)), np.broadcast_to(d1f, (B, d1f.size)))
        assert eng.last_cmux_kernel() == "generic_cmux_kernel"
        assert np.array_equal(got, np.broadcast_to(exp, got.shape)), (name, B)
