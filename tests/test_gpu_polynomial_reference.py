"""The HIP kernels against tests/poly_ref.py on the inputs of tests/test_polynomial_reference.py: every output word equals the
oracle's, and the distance to exact integer arithmetic, computed from the GPU's own output, meets the same conditions (so the
test still means something on the day oracle and kernel are wrong together).  Batches: B = 1 and one batch for each kernel
shape of the dispatcher, at most 8 ciphertexts of a batch checked exactly, the first and the last among them.  The rotation by an
encrypted shift, poly_fft, the integer-form key loaders and the packed operations: profiles/r14_exact_reference_new_ops.md."""
import numpy as np
import pytest

import oracle as O
import spf_amd
from tests import poly_ref as R
from tests import polyref_cases as C
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu

_ENGINES = {}


def engine(P):
    """one engine per parameter set, trace and scheme-switch radices included"""
    if P not in _ENGINES:
        ep = to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count, ss_radix_log=P.ss_radix_log,
                                         ss_radix_count=P.ss_count)
        _ENGINES[P] = spf_amd.Engine(ep)
    return _ENGINES[P]


def spread(m: int, B: int):
    """batch position -> item, the m items cycled through the batch; and the positions checked exactly: one of every item that the
    batch holds and the last (at most 8: a case has at most 4 items)"""
    idx = np.arange(B) % m
    pos = sorted(set(range(min(m, B))) | {B - 1})
    assert len(pos) <= 8
    return idx, pos


def hand_written(P, radix) -> bool:
    """N = 2048, k = 1 at the shipped radix runs the hand-written kernels, everything else the generic family's one kernel"""
    return P.N == 2048 and P.k == 1 and radix in ((16, 2), (4, 4))


# B = 1 and one batch for each kernel shape: the hand-written bootstrap has three (<= 256 ciphertexts, <= 512, beyond), its CMUX two
# (<= 256 gates, beyond); the names are asserted, as tests/test_gpu_parity.py does at the boundaries
PBS_KERNEL = {1: "blind_rotate8", 300: "blind_rotate2p2", 600: "blind_rotate2p_"}
CMUX_KERNEL = {1: "cmux4_kernel", 300: "cmux_kernel<"}


@pytest.mark.parametrize("cls", C.CLASSES)
@pytest.mark.parametrize("shape", list(C.PBS_SHAPES))
def test_one_step_pbs_on_the_gpu_against_exact_arithmetic(shape, cls):
    for c in C.pbs_cases(shape, cls):
        P = c.P
        eng = engine(P)
        bsk = C.key_fft(c.key)
        eng.load_bootstrap_key(bsk)
        exp = [C.pbs_oracle(c, it, bsk) for it in c.items]
        ex = [C.pbs_exact(c, it) for it in c.items]
        nf = [C.pbs_exact(c, it, R.NUMPY) for it in c.items]
        hw = hand_written(P, (P.pbs_radix_log, P.pbs_count))
        for B in (1, 300, 600) if hw else (1, 5):
            # one launch takes one (log_chi, log_v, rotation): the items of each log_v form a batch (B = 1: a launch for every item);
            # the launches of a batch size are judged together, over every item of the case, as on the CPU
            seen = {}
            for log_v in (0, 2):
                same = [i for i, it in enumerate(c.items) if it[3] == log_v]
                for first in range(len(same) if B == 1 else 1):
                    sel = same[first:] + same[:first]
                    idx, pos = spread(len(sel), B)
                    lwe = np.stack([c.items[sel[j]][0] for j in idx])
                    rot = c.items[sel[0]][4]
                    # the rotation argument is one per launch: fold each item's own rotation into its body word
                    lwe[:, -1] += np.array([(c.items[sel[j]][4] - rot) % (1 << 64) for j in idx], dtype=np.uint64)
                    lut = np.stack([c.items[sel[j]][1].reshape(-1) for j in idx])
                    got = eng.generalized_pbs(lwe, lut, 0, log_v, rot).reshape(B, P.k + 1, P.N)
                    name = eng.last_blind_rotate_kernel()
                    assert name.startswith(PBS_KERNEL[B] if hw else "generic_pbs_kernel"), (c.name, B, name)
                    assert np.array_equal(got, np.stack([exp[sel[j]] for j in idx])), (c.name, log_v, B)
                    seen.update({sel[idx[p]]: got[p] for p in pos})
            assert sorted(seen) == list(range(len(c.items)))
            C.check_tier_a(c, [seen[i] for i in sorted(seen)], ex, nf, f"gpu{B}")


def oracle_cmux(P, d0, d1, g):
    return O.cmux(d0.reshape(-1), d1.reshape(-1), g, P.N, P.k, P.cbs_radix_log, P.cbs_count).reshape(d0.shape)


@pytest.mark.parametrize("cls", C.CLASSES)
@pytest.mark.parametrize("shape", list(C.CMUX_SHAPES))
def test_cmux_family_on_the_gpu_against_exact_arithmetic(shape, cls):
    for c in C.cmux_cases(shape, cls):
        P = c.P
        eng = engine(P)
        g, lb, cnt = C.key_fft(c.key), P.cbs_radix_log, P.cbs_count
        m = len(c.items)
        exp_c = [oracle_cmux(P, d0, d1, g) for d0, d1 in c.items]
        exp_m = [oracle_cmux(P, np.zeros_like(d0), d1 - d0, g) for d0, d1 in c.items]
        ex_c = [R.cmux(d0, d1, c.key, lb, cnt) for d0, d1 in c.items]
        ex_m = [R.multiply_glwe_ggsw(d1 - d0, c.key, lb, cnt) for d0, d1 in c.items]
        nf_c = [R.cmux(d0, d1, c.key, lb, cnt, R.NUMPY) for d0, d1 in c.items]
        nf_m = [R.multiply_glwe_ggsw(d1 - d0, c.key, lb, cnt, R.NUMPY) for d0, d1 in c.items]
        a, b = C.glev_of(c)
        exp_g = np.stack([oracle_cmux(P, a[i], b[i], g) for i in range(cnt)])
        ex_g, nf_g = R.glev_cmux(a, b, c.key, lb, cnt), R.glev_cmux(a, b, c.key, lb, cnt, R.NUMPY)
        hw = hand_written(P, (lb, cnt))
        order = list(range(m))
        for B in (1, 300) if hw else (1, 5):
            seen_c, seen_m = {}, {}
            for first in range(m if B == 1 else 1):           # B = 1: a launch for every item
                idx, pos = spread(m, B)
                idx = (idx + first) % m
                gg = np.broadcast_to(g, (B, g.size))
                d0 = np.stack([c.items[j][0].reshape(-1) for j in idx])
                d1 = np.stack([c.items[j][1].reshape(-1) for j in idx])
                got_c = eng.cmux(gg, d0, d1).reshape(B, P.k + 1, P.N)
                name = eng.last_cmux_kernel()
                assert name.startswith(CMUX_KERNEL[B] if hw else "generic_cmux_kernel"), (c.name, B, name)
                got_m = eng.multiply_glwe_ggsw(d1 - d0, gg).reshape(B, P.k + 1, P.N)
                assert np.array_equal(got_c, np.stack([exp_c[j] for j in idx])), (c.name, "cmux", B)
                assert np.array_equal(got_m, np.stack([exp_m[j] for j in idx])), (c.name, "multiply", B)
                seen_c.update({int(idx[p]): got_c[p] for p in pos})
                seen_m.update({int(idx[p]): got_m[p] for p in pos})
            Bg = max(1, B // cnt)
            got_g = eng.glev_cmux(np.broadcast_to(g, (Bg, g.size)), np.broadcast_to(a.reshape(-1), (Bg, a.size)),
                                  np.broadcast_to(b.reshape(-1), (Bg, b.size))).reshape(Bg, cnt, P.k + 1, P.N)
            assert np.array_equal(got_g, np.broadcast_to(exp_g, got_g.shape)), (c.name, "glev_cmux", Bg)
            assert sorted(seen_c) == order and sorted(seen_m) == order
            C.check_tier_a(c, [seen_c[i] for i in order] + [seen_m[i] for i in order] + [got_g[0], got_g[-1]],
                           ex_c + ex_m + [ex_g, ex_g], nf_c + nf_m + [nf_g, nf_g], f"gpu{B}")


@pytest.mark.parametrize("cls", C.CLASSES)
@pytest.mark.parametrize("shape", list(C.SS_SHAPES))
def test_scheme_switch_on_the_gpu_every_row_against_exact_arithmetic(shape, cls):
    for c in C.ss_cases(shape, cls):
        P = c.P
        eng = engine(P)
        ssk = C.key_fft(c.key)
        eng.load_scheme_switch_key(ssk)
        m = len(c.items)
        exp = [O.scheme_switch_fft(glev.reshape(-1), ssk, P) for glev in c.items]
        ex = [R.scheme_switch(glev, c.key, P.ss_radix_log, P.ss_count) for glev in c.items]
        nf = [R.scheme_switch(glev, c.key, P.ss_radix_log, P.ss_count, R.NUMPY) for glev in c.items]
        for B in (1, 5, 300) if P.N == 2048 else (1, 5):
            idx, pos = spread(m, B)
            got = eng.scheme_switch(np.stack([c.items[j].reshape(-1) for j in idx]))
            assert np.array_equal(got.view(np.float64), np.stack([exp[j] for j in idx]).view(np.float64)), (c.name, B)
            if B == 1:                                      # every item in a launch of its own
                got = np.concatenate([got] + [eng.scheme_switch(c.items[j].reshape(1, -1)) for j in range(1, m)])
                assert np.array_equal(got.view(np.float64), np.stack(exp).view(np.float64)), (c.name, B)
                idx, pos = np.arange(m), list(range(m))
            C.check_scheme_switch(c, [C.ggsw_bins_to_words(got[p], P) for p in pos], [ex[idx[p]] for p in pos],
                                [nf[idx[p]] for p in pos], f"gpu{B}")


# ----------------------------------------------------------------------------------------------- tier B

TIER_B_BATCH = 300      # with B = 1; 4 of the batch checked against the exact chain
CHECKED = (0, 1, 150, 299)


@pytest.mark.parametrize("shape", list(C.TRACE_SHAPES))
def test_mod_switch_trace_and_rotate_on_the_gpu_against_the_exact_chain(shape):
    P = C.TRACE_SHAPES[shape]
    hk = C.honest_keys(P, 1, ak=True)
    ak = C.key_fft(hk.ak)
    eng = engine(P)
    eng.load_automorphism_key(ak)
    x = C.honest_glwes(P, hk, 1, TIER_B_BATCH)
    args = (P.tr_radix_log, P.tr_count, P.cbs_radix_log, P.cbs_count)
    one = eng.mod_switch_trace_and_rotate(x[:1].reshape(1, -1))
    got = eng.mod_switch_trace_and_rotate(x.reshape(TIER_B_BATCH, -1))
    assert np.array_equal(one[0], got[0])
    for i in range(TIER_B_BATCH):
        assert np.array_equal(got[i], O.mod_switch_trace_and_rotate(x[i].reshape(-1), ak, P)), i
    ph = lambda g: R.glwe_phase(np.asarray(g).reshape(-1, P.cbs_count, P.k + 1, P.N), hk.glwe_sk)  # noqa: E731
    ex = ph([R.mod_switch_trace_and_rotate(x[i], hk.ak, *args) for i in CHECKED])
    nf = ph([R.mod_switch_trace_and_rotate(x[i], hk.ak, *args, R.NUMPY) for i in CHECKED])
    C.check_tier_b(f"trace-{shape}", ph(got[list(CHECKED)]), ex, nf, "gpu300")


@pytest.mark.parametrize("shape", list(C.ROTATION_SHAPES))
def test_blind_rotation_on_the_gpu_against_the_exact_chain(shape):
    P = C.ROTATION_SHAPES[shape]
    hk = C.honest_keys(P, 2, bsk=True)
    bsk = C.key_fft(hk.bsk)
    eng = engine(P)
    eng.load_bootstrap_key(bsk)
    lwe, lut = C.rotation_inputs(P, 2, TIER_B_BATCH)
    flat = lut.reshape(TIER_B_BATCH, -1)
    one = eng.generalized_pbs(lwe[:1], flat[:1], 0, 0, 0)
    got = eng.generalized_pbs(lwe, flat, 0, 0, 0)
    assert np.array_equal(one[0], got[0])
    _, exp = O.bench_generalized_pbs(lwe, flat, bsk, P, 16, 0, 0)
    assert np.array_equal(got, exp)
    ph = lambda g: R.glwe_phase(np.asarray(g).reshape(-1, P.k + 1, P.N), hk.glwe_sk)  # noqa: E731
    ex = ph([R.generalized_pbs(lwe[i], lut[i], hk.bsk, P.pbs_radix_log, P.pbs_count) for i in CHECKED])
    nf = ph([R.generalized_pbs(lwe[i], lut[i], hk.bsk, P.pbs_radix_log, P.pbs_count, be=R.NUMPY) for i in CHECKED])
    C.check_tier_b(f"rotation-{shape}", ph(got[list(CHECKED)]), ex, nf, "gpu300", mean_test=False)   # see the CPU test


def test_circuit_bootstrap_on_the_gpu_feeding_an_exact_cmux():
    P = C.CBS_SHAPE
    hk = C.honest_keys(P, 3, bsk=True, ak=True, ssk=True)
    bsk, ak, ssk = C.key_fft(hk.bsk), C.key_fft(hk.ak), C.key_fft(hk.ssk)
    eng = engine(P)
    eng.load_bootstrap_key(bsk)
    eng.load_automorphism_key(ak)
    eng.load_scheme_switch_key(ssk)
    d = C.honest_glwes(P, hk, 3, 2)
    rng = np.random.default_rng(33)
    lwe = np.stack([R.lwe_encrypt(rng, hk.lwe_sk, (i % 2) << 63, 1 << 50) for i in range(TIER_B_BATCH)])
    one = eng.circuit_bootstrap(lwe[:1])
    got = eng.circuit_bootstrap(lwe)
    assert np.array_equal(one[0].view(np.float64), got[0].view(np.float64))
    for i in range(TIER_B_BATCH):
        assert np.array_equal(got[i].view(np.float64), O.circuit_bootstrap(lwe[i], bsk, ak, ssk, P).view(np.float64)), i
    phases = [C.cbs_cmux_phases(hk, lwe[i], d, lambda x, i=i: C.ggsw_bins_to_words(got[i], P)) for i in CHECKED]
    ex, nf, mine = (np.stack([p[j] for p in phases]) for j in range(3))
    C.check_tier_b("cbs-cmux", mine, ex, nf, "gpu300", mean_test=False)


# ----------------------------------------------------------------------------------------------- rotation by an encrypted shift

ROT_KERNEL = {1: "cmux4_kernel<4,4,rot>", 300: "cmux_kernel<4,4,2,rot>", 896: "cmux_kernel<4,4,2,stream,rot>"}


def rot_launch(eng, c, g, items, B):
    """one blind_rotation launch of n_bits = 1: the items (all of one r) cycled through the batch, the case's key as every
    selector.  Word equality with the oracle at every position; returns the batch and spread's positions."""
    r = items[0][1]
    assert all(it[1] == r for it in items) and r & (r - 1) == 0
    idx, pos = spread(len(items), B)
    glwe = np.stack([items[j][0].reshape(-1) for j in idx])
    sel = np.ascontiguousarray(np.broadcast_to(g, (B, 1, g.size)))
    got = eng.blind_rotation(sel, glwe, r.bit_length() - 1)
    assert eng.last_cmux_kernel() == ROT_KERNEL[B], (c.name, B, eng.last_cmux_kernel())
    exp = [C.rot_oracle(c, it, g).reshape(-1) for it in items]
    assert np.array_equal(got, np.stack([exp[j] for j in idx])), (c.name, r, B)
    return got.reshape(B, c.P.k + 1, c.P.N), idx, pos


@pytest.mark.parametrize("cls", C.CLASSES)
def test_rotate_cmux_step_on_the_gpu_against_exact_arithmetic(cls):
    for c in C.rot_cases(cls):
        eng = engine(c.P)
        g = C.key_fft(c.key)
        ex = [C.rot_exact(c, it) for it in c.items]
        nf = [C.rot_exact(c, it, R.NUMPY) for it in c.items]
        by_r = {}
        for i, it in enumerate(c.items):
            by_r.setdefault(it[1], []).append(i)
        for B in (1, 300):
            seen = {}
            for r, members in by_r.items():                     # a launch takes one r
                for first in range(len(members) if B == 1 else 1):   # B = 1: a launch for every item
                    sel = members[first:] + members[:first]
                    got, idx, pos = rot_launch(eng, c, g, [c.items[i] for i in sel], B)
                    seen.update({sel[idx[p]]: got[p] for p in pos})
            assert sorted(seen) == list(range(len(c.items)))
            C.check_tier_a(c, [seen[i] for i in sorted(seen)], ex, nf, f"gpu{B}")
        if cls == "uniform":                                    # the streaming shape: 896 selectors of 256 KiB, r = N/2
            members = by_r[c.P.N // 2]
            got, idx, _ = rot_launch(eng, c, g, [c.items[i] for i in members], 896)
            pos = (0, 447, 895)
            at = [members[idx[p]] for p in pos]
            C.check_tier_a(c, [got[p] for p in pos], [ex[i] for i in at], [nf[i] for i in at], "gpu896")


FOUR_DISTINCT = {4: (0, 1, 2, 3), 257: (1, 2, 3, 256)}     # batch -> positions checked against the exact chain: every item once, the last


@pytest.mark.parametrize("shape", list(C.ENC_SHIFT_SHAPES))
def test_encrypted_shift_rotation_on_the_gpu_against_the_exact_chain(shape):
    c = C.enc_shift_case(shape)
    P, m = c.P, len(c.shifts)
    eng = engine(P)
    sel = C.key_fft(c.sel).reshape(m, c.n_bits, -1)
    exp = np.stack([C.enc_shift_oracle(c, i, sel[i]).reshape(-1) for i in range(m)])
    first = None
    # 11 bits: the four-wave kernel.  4 bits: also B = 257, the smallest batch of the per-workgroup kernel, its last workgroup ragged
    for B in (4,) if c.n_bits == 11 else (4, 257):
        idx = np.arange(B) % m
        got = eng.blind_rotation(np.ascontiguousarray(sel[idx]), c.glwe.reshape(m, -1)[idx], c.log_stride)
        assert eng.last_cmux_kernel() == (ROT_KERNEL[1] if B == 4 else ROT_KERNEL[300]), (shape, B, eng.last_cmux_kernel())
        assert np.array_equal(got, exp[idx]), (shape, B)
        if first is None:
            first = got
        assert np.array_equal(got[:4], first)
        pos = FOUR_DISTINCT[B]
        assert sorted(idx[list(pos)]) == list(range(m))
        order = np.argsort(idx[list(pos)])
        ph = R.glwe_phase(got.reshape(B, P.k + 1, P.N)[list(pos)][order], c.hk.glwe_sk)
        C.check_tier_b(c.name, ph, c.exact, c.numpy, f"gpu{B}")
        C.check_rotated_phase(c, ph, f"gpu{B}")
    # the bias on words: every step of every item as a launch of its own from the exact accumulator
    one = lambda i, j, acc, r: eng.blind_rotation(sel[i, j][None, None], acc.reshape(1, -1), r.bit_length() - 1).reshape(acc.shape)  # noqa: E731
    C.check_step_bias(c, one, "gpu1")


# ----------------------------------------------------------------------------------------------- the forward transform

FFT_PARAMS = {2048: C.D128, 256: C.N256K3, 16: C.N16}      # N = 2048 runs poly_fft2048_kernel, any other N generic_poly_fft_kernel


@pytest.mark.parametrize("n", C.FFT_SIZES)
def test_poly_fft_on_the_gpu_against_the_long_double_dft(n):
    """the launch picks its kernel by N alone (launch_poly_fft) and records no name: the shape is what reaches each kernel"""
    eng = engine(FFT_PARAMS[n])
    assert eng.params.polynomial_degree == n
    cases = C.fft_cases(n)
    refs = C.fft_references(n)
    polys = np.concatenate([p for _, p in cases])
    assert polys.shape[0] == 23                                 # at N = 2048: a ragged last workgroup of kPolyFftWaves = 4
    exp = np.stack([O.poly_fft(p) for p in polys])
    batch = eng.poly_fft(polys)
    single = np.stack([eng.poly_fft(p[None])[0] for p in polys])
    at = 0
    for name, p in cases:
        for got, who in ((batch[at:at + len(p)], "gpu23"), (single[at:at + len(p)], "gpu1")):
            assert np.array_equal(got.view(np.uint64), exp[at:at + len(p)].view(np.uint64)), (name, who)
            C.check_forward(name, got, *refs[name], who)
        at += len(p)


def test_std_loaded_key_drives_an_exact_step():
    """keys that reach the kernels with no oracle transform on the path: the rotation's selector through eng.poly_fft, a bootstrap
    key through load_bootstrap_key_std"""
    c = C.rot_cases("uniform")[0]
    eng = engine(c.P)
    g = eng.poly_fft(c.key.reshape(-1, c.P.N)).reshape(-1)
    assert np.array_equal(g.view(np.uint64), C.key_fft(c.key).view(np.uint64))
    items = c.items[::5]                                        # each r once, each accumulator once
    got = [rot_launch(eng, c, g, [it], 1)[0][0] for it in items]
    C.check_tier_a(c, got, [C.rot_exact(c, it) for it in items], [C.rot_exact(c, it, R.NUMPY) for it in items], "gpustd")

    c = C.pbs_cases("default128", "uniform")[0]
    eng = engine(c.P)
    eng.load_bootstrap_key_std(np.ascontiguousarray(c.key).reshape(-1))
    bsk = C.key_fft(c.key)
    got = []
    for it in c.items:
        lwe, lut, log_chi, log_v, rot = it
        out = eng.generalized_pbs(lwe[None], lut.reshape(1, -1), log_chi, log_v, rot).reshape(lut.shape)
        assert np.array_equal(out, C.pbs_oracle(c, it, bsk)), c.name
        got.append(out)
    C.check_tier_a(c, got, [C.pbs_exact(c, it) for it in c.items], [C.pbs_exact(c, it, R.NUMPY) for it in c.items], "gpustd")


# ----------------------------------------------------------------------------------------------- packed integers


def lwe_phase(lwe, sk) -> np.ndarray:
    lwe = np.asarray(lwe, dtype=np.uint64)
    return lwe[..., -1] - (lwe[..., :-1] * sk).sum(axis=-1, dtype=np.uint64)


@pytest.mark.parametrize("part", ["pack_unpack", "table_lookup", "bivariate"])
def test_pack_unpack_table_lookup_and_bivariate_on_the_gpu(part):
    {"pack_unpack": pack_unpack_part, "table_lookup": table_lookup_part, "bivariate": bivariate_part}[part]()


def pack_unpack_part():
    """pack and unpack move words and add them: exact"""
    for P, B, n_bits in ((C.D128, 1, 1), (C.D128, 5, 16), (C.D128, 3, C.D128.N), (C.N128K2, 3, 16)):
        eng = engine(P)
        rng = np.random.default_rng([0xA8, P.N, B, n_bits])
        bits = rng.integers(0, 1 << 64, (B, n_bits, P.k + 1, P.N), dtype=np.uint64)
        packed = eng.glwe_pack(bits.reshape(B, n_bits, -1)).reshape(B, P.k + 1, P.N)
        assert np.array_equal(packed, np.stack([R.pack(b) for b in bits])), (P.N, B, n_bits)
        lwes = eng.glwe_unpack_l1(packed.reshape(B, -1), n_bits)
        assert np.array_equal(lwes, np.stack([R.unpack(p, n_bits) for p in packed])), (P.N, B, n_bits)


def table_lookup_part():
    """16 entries of 8 bits at stride 8 is the second rotation shape: its honest selectors pick entries 0, 5, 10 and 15"""
    c = C.enc_shift_case("default128_4bit_stride8")
    P, m = c.P, len(c.shifts)
    eng = engine(P)
    entries = [int(v) for v in np.random.default_rng(8).integers(0, 256, 16)]
    table, log_stride = spf_amd.packed.trivial_table_glwe(entries, 8, eng.params)
    assert log_stride == c.log_stride and c.n_bits == 4
    tab = table.reshape(P.k + 1, P.N)
    sel = C.key_fft(c.sel).reshape(m, c.n_bits, -1)
    out = eng.blind_rotation(sel, np.tile(table, (m, 1)), log_stride)
    for i in range(m):
        assert np.array_equal(out[i], C.enc_shift_oracle(c, i, sel[i], tab).reshape(-1)), i
    lwes = eng.glwe_unpack_l1(out, 8)
    chain = lambda be: np.stack([R.unpack(R.blind_rotation_by_shift(tab, c.sel[i], log_stride, P.cbs_radix_log, P.cbs_count, be), 8)  # noqa: E731
                                 for i in range(m)])
    got, ex, nf = (lwe_phase(x, c.hk.glwe_sk) for x in (lwes, chain(R.EXACT), chain(R.NUMPY)))     # k = 1: the GLWE key is the LWE key
    for i, s in enumerate(c.shifts):
        assert [int(t) >> 63 for t in got[i] + np.uint64(1 << 62)] == [(entries[s] >> j) & 1 for j in range(8)], s
    C.check_tier_b("table-lookup-16x8", got, ex, nf, "gpu4", mean_test=False)     # 32 phases: no statistic of a mean


def bivariate_part():
    """the packing left * 2^p + right happens on the device; the words of a bootstrap's output under honest keys are no
    measure (a rounding in the accumulator moves a digit, and with it every mask word): the LWE phases are"""
    P = C.ROTATION_SHAPES["default128_S64"]
    hk = C.honest_keys(P, 2, bsk=True)
    eng = engine(P)
    bsk = C.key_fft(hk.bsk)
    eng.load_bootstrap_key(bsk)
    p = 2
    left, lut = C.rotation_inputs(P, 6, TIER_B_BATCH)
    right, _ = C.rotation_inputs(P, 7, TIER_B_BATCH)
    flat = lut.reshape(TIER_B_BATCH, -1)
    packed = R.bivariate_pack(left, right, p)
    for B in (1, TIER_B_BATCH):
        got = eng.pbs_bivariate(left[:B], right[:B], flat[:B], p)
        for i in sorted({0, B - 1}):
            assert np.array_equal(got[i], O.pbs_univariate(packed[i], flat[i], bsk, P)), (B, i)
    assert np.array_equal(got, eng.pbs_univariate(packed, flat))           # ... itself held to the oracle at every position elsewhere
    chain = lambda be: np.stack([R.sample_extract(R.generalized_pbs(packed[i], lut[i], hk.bsk, P.pbs_radix_log, P.pbs_count, be=be), 0)  # noqa: E731
                                 for i in CHECKED])
    ph = lambda x: lwe_phase(x, hk.glwe_sk)  # noqa: E731
    C.check_tier_b("bivariate-default128_S64", ph(got[list(CHECKED)]), ph(chain(R.EXACT)), ph(chain(R.NUMPY)), "gpu300", mean_test=False)
