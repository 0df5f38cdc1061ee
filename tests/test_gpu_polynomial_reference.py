"""The HIP kernels against tests/poly_ref.py on the inputs of tests/test_polynomial_reference.py: every output word equals the
oracle's, and the distance to exact integer arithmetic, computed from the GPU's own output, meets the same conditions (so the
test still means something on the day oracle and kernel are wrong together).  Batches: B = 1 and one batch for each kernel
shape of the dispatcher, at most 8 ciphertexts of a batch checked exactly, the first and the last among them."""
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
