"""Gadget decompositions on the GPU at every radix the ABI accepts.

The keyswitch L1 -> L0 has two formulations (spf_hip.hip `launch_keyswitch`): the int8 matrix-core block GEMM when the
radix fits it (radix_log <= 8 in the tuned context) and the scalar `keyswitch_kernel` otherwise.  Every output word is held
to the independent restatement of tests/decomp_ref.py and to the oracle, over the whole keyswitch domain (0 < l * logB <= 32),
at the LWE dimensions and batch sizes where the two kernels' tiles end, with keys that drive the GEMM's int32 accumulators to
their bound; with a noiseless key the output must also decrypt to the rounded phase.  The other decompositions (PBS, CMUX,
trace, scheme switch, the circuit bootstrap's LUT) are checked at their edges against the oracle.
"""
import functools

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests.decomp_ref import M64, extreme_words, keyswitch_ref, lwe_phase, noiseless_keyswitch_phase
from tests.util import dev_bootstrap, keyset, random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu

N_IN = 2048                                     # tuned context: N = 2048, k = 1
BATCHES = (1, 31, 32, 33, 127, 128, 129, 257)   # scalar kernel: groups of 32 ciphertexts; GEMM: 128-row tiles


def _grid():
    """every radix_log with count 1 and count floor(32 / logB), and DEFAULT_128's 2 x 6"""
    out = {(2, 6)}
    for lg in range(1, 33):
        out.add((lg, 1))
        out.add((lg, 32 // lg))
    return sorted(out)


def _expected_kernel(lg):
    return "ks_gemm_lds_kernel" if lg <= 8 else "keyswitch_kernel"


@functools.lru_cache(maxsize=4)
def _l1_key(seed=0xDEC0):
    return O.gen_binary_key(O.Rng(seed), N_IN)


@functools.lru_cache(maxsize=8)
def _l0_key(n):
    return O.gen_binary_key(O.Rng(0xDEC1 + n), n)


def _inputs(lg, c, B, n_in=N_IN, seed=0):
    """uniform rows, with rows of extreme words (0, 2^63, 2^64 - 1, words recomposed from digit vectors at the ends of the
    digit range) at the start of the batch and at the edges of the kernels' tiles"""
    rng = np.random.default_rng(0xBA7C0 + 64 * lg + c + seed)
    x = rng.integers(0, 1 << 64, size=(B, n_in + 1), dtype=np.uint64)
    ext = np.array(extreme_words(lg, c), dtype=np.uint64)
    special = [np.full(n_in + 1, w, dtype=np.uint64) for w in ext]
    special.append(ext[np.arange(n_in + 1) % ext.size])
    special.append(ext[rng.integers(0, ext.size, size=n_in + 1)])
    rows = list(range(len(special))) + [30, 31, 32, 126, 127, 128, 255, 256]
    for k, r in enumerate(rows):
        if r < B:
            x[r] = special[k % len(special)]
    return x


def _keys(lg, c, n, which=("noiseless", "zero", "ones", "alternating", "00FF")):
    """KSKs [N_IN][c][n + 1]: a real noiseless encryption (first) and synthetic words.  The all-zero key with digits at
    -2^(logB-1) puts every byte plane at -128 against every digit at its largest magnitude: the GEMM's accumulator bound."""
    size = N_IN * c * (n + 1)
    for name in which:
        if name == "noiseless":
            k = O.gen_ksk(O.Rng(0x5EED + 64 * lg + c + 4096 * n), _l1_key(), _l0_key(n), lg, c, 0.0)
        elif name == "noisy":
            k = O.gen_ksk(O.Rng(0x5EEE + 64 * lg + c + 4096 * n), _l1_key(), _l0_key(n), lg, c, O.DEFAULT_128.lwe_std)
        elif name == "zero":
            k = np.zeros(size, dtype=np.uint64)
        elif name == "ones":
            k = np.full(size, M64, dtype=np.uint64)
        elif name == "alternating":
            k = np.where(np.arange(size) % 2 == 0, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555).astype(np.uint64)
        else:
            k = np.where(np.arange(size) % 3 == 0, 0, M64).astype(np.uint64)
        yield name, k


def _engine(n, lg, c):
    return spf_amd.Engine(spf_amd.DEFAULT_128.replace(lwe_dimension=n, ks_radix_log=lg, ks_radix_count=c))


def _check_keyswitch(eng, lg, c, n, x, keys, batches, oracle_rows):
    """for every key: each batch prefix through the host-pointer entry point against keyswitch_ref, the oracle on
    `oracle_rows`, and the noiseless identity"""
    for name, ksk in keys:
        eng.load_keyswitch_key(ksk)
        want = keyswitch_ref(x, ksk, N_IN, n, lg, c)
        for B in batches:
            got = eng.keyswitch_lwe_l1_lwe_l0(x[:B])
            assert eng.last_keyswitch_kernel() == _expected_kernel(lg), (lg, c, n)
            bad = np.nonzero((got != want[:B]).any(axis=1))[0]
            assert bad.size == 0, (f"{c} x {lg} n={n} key={name} B={B}: {bad.size} ciphertexts differ, first {bad[0]}: "
                                   f"got {got[bad[0]][-3:]} want {want[bad[0]][-3:]}")
        for r in oracle_rows:
            if r < x.shape[0]:
                assert np.array_equal(O.keyswitch_lwe(x[r], ksk, N_IN, n, lg, c), want[r]), (lg, c, n, name, r)
        if name == "noiseless":
            assert np.array_equal(lwe_phase(want, _l0_key(n)), noiseless_keyswitch_phase(x, _l1_key(), lg, c)), (lg, c, n)


@pytest.mark.parametrize("n", [12, 15, 16])
@pytest.mark.parametrize("lg", range(1, 33))
def test_keyswitch_every_radix_tuned_context(lg, n):
    """n = 15: the 8 byte planes of the 16 output words fill one 128-column GEMM tile exactly; n = 16 spills into a second"""
    for c in sorted({c for g, c in _grid() if g == lg}):
        x = _inputs(lg, c, 33)
        eng = _engine(n, lg, c)
        try:
            _check_keyswitch(eng, lg, c, n, x, _keys(lg, c, n), (1, 31, 32, 33), range(33))
        finally:
            eng.close()


@pytest.mark.parametrize("lg,c", [(2, 6), (8, 4), (5, 6), (1, 32), (9, 3), (16, 2), (32, 1)])
@pytest.mark.parametrize("n", [15, 16])
def test_keyswitch_batch_edges(lg, c, n):
    x = _inputs(lg, c, max(BATCHES), seed=1)
    eng = _engine(n, lg, c)
    try:
        _check_keyswitch(eng, lg, c, n, x, _keys(lg, c, n, ("noiseless", "zero", "ones")), BATCHES,
                         list(range(10)) + [30, 31, 32, 126, 127, 128, 255, 256])
    finally:
        eng.close()


@pytest.mark.parametrize("lg,c", [(2, 6), (8, 4), (11, 2), (16, 2), (32, 1)])
def test_keyswitch_at_lwe_dimension_637(lg, c):
    n = 637
    x = _inputs(lg, c, 33, seed=2)
    eng = _engine(n, lg, c)
    try:
        _check_keyswitch(eng, lg, c, n, x, _keys(lg, c, n, ("noisy", "zero", "ones")), (1, 33), (0, 1, 2, 3, 4, 5, 6, 7, 32))
    finally:
        eng.close()


@pytest.mark.parametrize("lg,c", [(8, 4), (32, 1)])
def test_keyswitch_through_every_path(lg, c):
    """the largest GEMM radix and the scalar kernel at 32 bits through the device-pointer entry point, the fused gate
    bootstrap (keyswitch -> circuit-bootstrap PBS), the fused keyswitch + circuit bootstrap, a pool submit and a gate graph"""
    n = 12
    P = O.DEFAULT_128.replace(lwe_n=n, ks_radix_log=lg, ks_count=c)
    ks = O.gen_keyset(0x5EED00D0 + lg, P)
    r = O.Rng(0x7AD0 + lg)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, P), O.gen_ssk_fft(r, ks.glwe_sk, P)
    eng = spf_amd.Engine(to_engine_params(P))
    eng.load_bootstrap_key(ks.bsk_fft)
    eng.load_keyswitch_key(ks.ksk)
    eng.load_automorphism_key(ak)
    eng.load_scheme_switch_key(ssk)
    kname = _expected_kernel(lg)
    x = _inputs(lg, c, 12, seed=3)
    want = keyswitch_ref(x, ks.ksk, N_IN, n, lg, c)
    for i in range(x.shape[0]):
        assert np.array_equal(O.keyswitch_lwe(x[i], ks.ksk, N_IN, n, lg, c), want[i]), i
    try:
        # device pointers, one launch
        out = np.empty_like(want)
        d_in, d_out = eng.device_alloc(x.nbytes), eng.device_alloc(out.nbytes)
        try:
            eng.device_upload(d_in, x)
            eng.keyswitch_dev(None, x.shape[0], d_in, d_out)
            eng.device_download(None, out, d_out)
        finally:
            eng.device_free(d_in)
            eng.device_free(d_out)
        assert eng.last_keyswitch_kernel() == kname
        assert np.array_equal(out, want)
        # keyswitch -> circuit-bootstrap PBS
        gate = eng.gate_bootstrap(x[:4])
        assert eng.last_keyswitch_kernel() == kname
        for i in range(4):
            assert np.array_equal(gate[i], O.cbs_pbs(want[i], ks.bsk_fft, P)), i
        # keyswitch -> circuit bootstrap (L1 GGSW)
        kcb = eng.keyswitch_circuit_bootstrap(x[:2])
        assert eng.last_keyswitch_kernel() == kname
        for i in range(2):
            assert np.array_equal(kcb[i].view(np.float64),
                                  O.circuit_bootstrap(want[i], ks.bsk_fft, ak, ssk, P).view(np.float64)), i
        # one pool submit
        pool = spf_amd.Pool(eng, max_batch=16, max_wait_us=200)
        try:
            o = np.zeros(n + 1, dtype=np.uint64)
            pool.keyswitch_lwe_l1_lwe_l0(o, x[3])
        finally:
            pool.close()
        assert eng.last_keyswitch_kernel() == kname
        assert np.array_equal(o, want[3])
        # one gate graph
        g = spf_amd.FheCircuit(eng)
        outs = [g.add_output(g.add_op(FheOp.KeyswitchL1toL0, [g.add_input(ValueKind.LWE1, x[i])]), ValueKind.LWE0)
                for i in (0, 5)]
        g.run()
        assert eng.last_keyswitch_kernel() == kname
        assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[5])
        g.close()
    finally:
        eng.close()


@pytest.mark.parametrize("lg,c", [(9, 3), (16, 2), (32, 1)])
def test_keyswitch_generic_family(lg, c):
    """N = 128, k = 2: the generic family always runs the scalar kernel"""
    N, k, n = 128, 2, 5
    n_in = k * N
    P = O.DEFAULT_128.replace(lwe_n=n, N=N, k=k, pbs_radix_log=4, pbs_count=3, cbs_radix_log=4, cbs_count=3,
                              ks_radix_log=lg, ks_count=c)
    r = O.Rng(0x6E0 + lg)
    s_in, s_out = O.gen_binary_key(r, n_in), O.gen_binary_key(r, n)
    eng = spf_amd.Engine(to_engine_params(P))
    try:
        x = _inputs(lg, c, 33, n_in=n_in, seed=4)
        for std in (0.0, 1e-5):
            ksk = O.gen_ksk(r, s_in, s_out, lg, c, std)
            eng.load_keyswitch_key(ksk)
            want = keyswitch_ref(x, ksk, n_in, n, lg, c)
            for B in (1, 32, 33):
                assert np.array_equal(eng.keyswitch_lwe_l1_lwe_l0(x[:B]), want[:B]), (lg, c, std, B)
                assert eng.last_keyswitch_kernel() == "keyswitch_kernel"
            for i in range(33):
                assert np.array_equal(O.keyswitch_lwe(x[i], ksk, n_in, n, lg, c), want[i]), (lg, c, std, i)
            if std == 0.0:
                assert np.array_equal(lwe_phase(want, s_out), noiseless_keyswitch_phase(x, s_in, lg, c))
    finally:
        eng.close()


# ----------------------------------------------------------------------------- the other decompositions at their edges

# generic parameter sets with radix_logs 17, 21, 31, 32, 63 and l * logB = 63 in the PBS, CBS, trace and scheme switch
GENERIC_EDGES = [
    O.DEFAULT_128.replace(lwe_n=4, N=64, k=1, pbs_radix_log=21, pbs_count=3, cbs_radix_log=31, cbs_count=2,
                          tr_radix_log=63, tr_count=1, ss_radix_log=32, ss_count=1, ks_radix_log=32, ks_count=1),
    O.DEFAULT_128.replace(lwe_n=3, N=128, k=2, pbs_radix_log=63, pbs_count=1, cbs_radix_log=21, cbs_count=3,
                          tr_radix_log=17, tr_count=3, ss_radix_log=31, ss_count=2, ks_radix_log=16, ks_count=2),
    O.DEFAULT_128.replace(lwe_n=5, N=64, k=2, pbs_radix_log=32, pbs_count=1, cbs_radix_log=63, cbs_count=1,
                          tr_radix_log=21, tr_count=3, ss_radix_log=9, ss_count=7, ks_radix_log=9, ks_count=3),
    O.DEFAULT_128.replace(lwe_n=6, N=128, k=1, pbs_radix_log=17, pbs_count=3, cbs_radix_log=9, cbs_count=7,
                          tr_radix_log=7, tr_count=9, ss_radix_log=21, ss_count=3, ks_radix_log=8, ks_count=4),
]


def _generic_engine_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count,
                                       ss_radix_log=P.ss_radix_log, ss_radix_count=P.ss_count)


@pytest.mark.parametrize("P", GENERIC_EDGES, ids=["N64k1-pbs21x3", "N128k2-pbs63x1", "N64k2-pbs32x1", "N128k1-pbs17x3"])
def test_generic_decompositions_at_their_edges(P):
    """PBS (generalized, univariate, circuit-bootstrap), CMUX, trace and scheme switch at radix_logs up to 63: every word
    against the oracle; the whole circuit bootstrap once"""
    ks = O.gen_keyset(0x5EED00E0 + P.N + P.k, P)
    r = O.Rng(0x7AE0 + P.N)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, P), O.gen_ssk_fft(r, ks.glwe_sk, P)
    eng = spf_amd.Engine(_generic_engine_params(P))
    try:
        eng.load_bootstrap_key(ks.bsk_fft)
        eng.load_keyswitch_key(ks.ksk)
        eng.load_automorphism_key(ak)
        eng.load_scheme_switch_key(ssk)
        B = 4
        lwe = random_lwe_batch(0x6F00 + P.N, B, P.lwe_n)
        lwe[0, :] = M64
        lwe[1, :] = 1 << 63
        luts = random_glwe(0x6F10 + P.N, B, P.glwe_len)
        luts[0, :] = M64
        got = eng.generalized_pbs(lwe, luts, 1, 1, 0)
        assert eng.last_blind_rotate_kernel() == "generic_pbs_kernel"
        for i in range(B):
            assert np.array_equal(got[i], O.generalized_pbs(lwe[i], luts[i], ks.bsk_fft, P, 1, 1)), i
        u = eng.pbs_univariate(lwe, luts[1])
        c = eng.circuit_bootstrap_pbs(lwe)
        for i in range(B):
            assert np.array_equal(u[i], O.pbs_univariate(lwe[i], luts[1], ks.bsk_fft, P)), i
            assert np.array_equal(c[i], O.cbs_pbs(lwe[i], ks.bsk_fft, P)), i
        # CMUX over a GGSW of the cbs radix, with extreme operand words
        rng = np.random.default_rng(0x6F20 + P.N)
        sel = np.stack([O.encrypt_ggsw_fft(r, ks.glwe_sk, b, P.N, P.k, P.cbs_radix_log, P.cbs_count, P.glwe_std)
                        for b in (0, 1, 1, 0)])
        a = rng.integers(0, 1 << 64, size=(B, P.glwe_len), dtype=np.uint64)
        b = rng.integers(0, 1 << 64, size=(B, P.glwe_len), dtype=np.uint64)
        a[0, :], b[1, :] = M64, 1 << 63
        mux = eng.cmux(sel, a, b)
        assert eng.last_cmux_kernel() == "generic_cmux_kernel"
        for i in range(B):
            assert np.array_equal(mux[i], O.cmux(a[i], b[i], sel[i], P.N, P.k, P.cbs_radix_log, P.cbs_count)), i
        # trace (mod switch, trace, rotate) and scheme switch
        glwe = random_glwe(0x6F30 + P.N, 2, P.glwe_len)
        glwe[1, :] = M64
        tr = eng.mod_switch_trace_and_rotate(glwe)
        for i in range(2):
            assert np.array_equal(tr[i], O.mod_switch_trace_and_rotate(glwe[i], ak, P)), i
        glev = random_glwe(0x6F40 + P.N, 2 * P.cbs_count, P.glwe_len).reshape(2, P.cbs_count, P.glwe_len)
        glev[1, 0, :] = M64
        gg = eng.scheme_switch(glev)
        for i in range(2):
            assert np.array_equal(gg[i].view(np.float64), O.scheme_switch_fft(glev[i], ssk, P).view(np.float64)), i
        # the whole circuit bootstrap, once
        cb = eng.circuit_bootstrap(lwe[2:3])
        assert np.array_equal(cb[0].view(np.float64), O.circuit_bootstrap(lwe[2], ks.bsk_fft, ak, ssk, P).view(np.float64))
    finally:
        eng.close()


@pytest.mark.parametrize("cbs_log,cbs_count", [(4, 1), (4, 2), (4, 3), (5, 4), (4, 5), (4, 6), (4, 7), (9, 7), (21, 3),
                                               (16, 4), (31, 2), (63, 1)])
def test_tuned_circuit_bootstrap_pbs_cbs_radix(cbs_log, cbs_count):
    """the cbs LUT spf_create builds: counts 1 .. 7 (log_v 0 .. 3), and radices whose top levels reach 64 plaintext bits and
    are zeroed (9 x 7, 21 x 3, 16 x 4); B = 1, 5 and 33, host pointers and one device-pointer launch"""
    n = 8
    ks = keyset(0x5EED00F0, n, with_ksk=False)
    P = O.DEFAULT_128.replace(lwe_n=n, cbs_radix_log=cbs_log, cbs_count=cbs_count)
    eng = spf_amd.Engine(to_engine_params(P))
    try:
        eng.load_bootstrap_key(ks.bsk_fft)
        lwe = random_lwe_batch(0x6F50 + 64 * cbs_count + cbs_log, 33, n)
        lwe[0, :] = M64
        lwe[1, :] = 0
        lwe[2, -1] = 1 << 63
        want = np.stack([O.cbs_pbs(lwe[i], ks.bsk_fft, P) for i in range(33)])
        for B in (1, 5, 33):
            assert np.array_equal(eng.circuit_bootstrap_pbs(lwe[:B]), want[:B]), B
        assert np.array_equal(dev_bootstrap(eng, lwe), want)
    finally:
        eng.close()
