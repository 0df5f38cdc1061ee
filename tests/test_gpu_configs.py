"""GPU parity at the sizes BASELINE.json's configs name (task 1): the kernels the bench runs
must meet the oracle at DEFAULT_128 inside the -m gpu suite, not only inside bench.py.

  config 2  "Batch of 4096 independent programmable bootstraps, default params, 1xMI355X":
            B = 4096 at n = 637 through spf_circuit_bootstrap_pbs_batch (throughput kernel), every
            ciphertext compared with the oracle; ragged B = 1031 on a sample; keyswitch at B = 4096
            (int8-MFMA path, 32 row tiles); streaming cmux_kernel at B > 256.
  noise     SURVEY §8(c)(ii): one external product at the PBS shape on the GPU against the exact
            integer negacyclic product, normalised torus distance bounded (method of
            parasol_runtime/examples/op_noise/noise.rs:15-38).
  golden    a DEFAULT_128 fixture (tests/golden/pbs_default128.npz: inputs + expected outputs, key
            re-derived from the seed recipe stored beside them).
"""
import os

import numpy as np
import pytest

import oracle as O
from tests import poly_ref as R
import spf_amd
from tests.util import M64, dev_bootstrap, keyset, random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu

HOST_THREADS = max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def full():
    ks = keyset(0x5EED0001, 637)
    eng = spf_amd.Engine(to_engine_params(ks.params))
    eng.load_bootstrap_key(ks.bsk_fft)
    eng.load_keyswitch_key(ks.ksk)
    return ks, eng


def test_config2_batch_4096_pbs_default128_every_ciphertext(full):
    """BASELINE configs[1]: all 4096 outputs of the throughput kernel equal the oracle's, word for word."""
    ks, eng = full
    B = 4096
    lwe = random_lwe_batch(0xC0F2, B, 637)
    got = eng.circuit_bootstrap_pbs(lwe)
    _, exp = O.bench_cbs_pbs(lwe, ks.bsk_fft, ks.params, HOST_THREADS, native=False)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} ciphertexts differ, first {bad[:8]}"


def test_config2_ragged_batch_1031_default128(full):
    """Ragged last workgroup (1031 = 257 workgroups of four + 3) at n = 637, as ONE launch through the device-pointer
    entry point (the host-pointer form would cut it into 1024 + 7): first / last ciphertext of a workgroup and the tail
    against the oracle."""
    ks, eng = full
    B = 1031
    lwe = random_lwe_batch(0xC0F3, B, 637)
    got = dev_bootstrap(eng, lwe)
    assert eng.last_blind_rotate_kernel() == "blind_rotate2p_kernel<2,16,6,even>"
    for i in (0, 3, 4, 515, 1023, 1027, 1028, 1029, 1030):
        assert np.array_equal(got[i], O.cbs_pbs(lwe[i], ks.bsk_fft, ks.params)), i
    assert np.array_equal(got, eng.circuit_bootstrap_pbs(lwe))   # the sliced host-pointer form: same words


def test_config2_keyswitch_4096_default128(full):
    """The int8-MFMA keyswitch over 32 row tiles x 5 column tiles: sampled rows against the oracle, and the
    whole batch against the same rows keyswitched 100 at a time (other tile boundaries)."""
    ks, eng = full
    P = ks.params
    B = 4096
    lwe1 = random_lwe_batch(0xC0F4, B, P.N)
    got = eng.keyswitch_lwe_l1_lwe_l0(lwe1)
    for i in (0, 1, 127, 128, 129, 2047, 2048, 4000, 4094, 4095):
        exp = O.keyswitch_lwe(lwe1[i], ks.ksk, P.N, P.lwe_n, P.ks_radix_log, P.ks_count)
        assert np.array_equal(got[i], exp), i
    ref = np.concatenate([eng.keyswitch_lwe_l1_lwe_l0(lwe1[i:i + 100]) for i in range(0, B, 100)])
    assert np.array_equal(got, ref)


def test_config3_streaming_cmux_515(full):
    """cmux_kernel (the streaming shape, B > #CU) with a ragged tail: a sample against the oracle."""
    ks, eng = full
    P = ks.params
    B = 515
    nrng = np.random.default_rng(515)
    a = random_glwe(31, B, P.glwe_len)
    b = random_glwe(32, B, P.glwe_len)
    n = 2 * 4 * 2 * 1024
    g = ((nrng.standard_normal((B, n)) + 1j * nrng.standard_normal((B, n))) * 2.0 ** 60).astype(np.complex128)
    got = eng.cmux(g, a, b)
    for i in (0, 3, 4, 257, 511, 512, 513, 514):
        assert np.array_equal(got[i], O.cmux(a[i], b[i], g[i], P.N, P.k, P.cbs_radix_log, P.cbs_count)), i


def test_streaming_cmux_large_launch_uses_streaming_loads_and_same_words(full):
    """From 224 MB of selectors in one launch (896 gates) the streaming shape reads its selector rows with streaming
    (non-temporal) loads — another instantiation, `cmux_kernel<4,4,2,true>`: 1024 gates in ONE call against the same gates in
    two calls of 512 (plain loads), word for word, and a sample against the oracle."""
    ks, eng = full
    P = ks.params
    B = 1024
    nrng = np.random.default_rng(1024)
    a = random_glwe(41, B, P.glwe_len)
    b = random_glwe(42, B, P.glwe_len)
    n = 2 * 4 * 2 * 1024
    g = np.empty((B, n), dtype=np.complex128)
    for lo in range(0, B, 128):  # (in slices: the normal deviates of all 1024 selectors at once are 0.5 GB of temporaries)
        g[lo:lo + 128] = (nrng.standard_normal((128, n)) + 1j * nrng.standard_normal((128, n))) * 2.0 ** 60
    whole = eng.cmux(g, a, b)
    halves = np.concatenate([eng.cmux(g[:512], a[:512], b[:512]), eng.cmux(g[512:], a[512:], b[512:])])
    assert np.array_equal(whole, halves)
    for i in (0, 511, 512, 1023):
        assert np.array_equal(whole[i], O.cmux(a[i], b[i], g[i], P.N, P.k, P.cbs_radix_log, P.cbs_count)), i


# ---- the plain / univariate PBS (log_v = 0) at config-2 size.  `programmable_bootstrap_univariate`
# (programmable_bootstrapping.rs:291-318) is the unit of the reference's own bench (sunscreen_tfhe/benches/ops.rs:86-123);
# with log_v = 0 the rotation amounts are odd as often as even, so the dispatch takes the OTHER instantiation of every
# blind-rotation kernel (the one that keeps the hand-overs around the rotation gather): it gets the same evidence as the
# circuit-bootstrap variant above.


@pytest.fixture(scope="module")
def plain_pbs_4096(full):
    """4096 LWE words vectors, one shared random LUT, the oracle's GLWE outputs for (log_chi, log_v) = (0, 0)."""
    ks, _ = full
    lwe = random_lwe_batch(0xC0FA, 4096, 637)
    lut = random_glwe(0xC0FB, 1, ks.params.glwe_len)[0]
    _, exp = O.bench_generalized_pbs(lwe, lut, ks.bsk_fft, ks.params, HOST_THREADS, 0, 0)
    return lwe, lut, exp


def test_config2_batch_4096_generalized_pbs_log_v0_every_ciphertext(full, plain_pbs_4096):
    """generalized_programmable_bootstrap(log_chi = 0, log_v = 0) at B = 4096, n = 637 through the throughput shape
    (`blind_rotate2p_kernel<2,16,10>`, nine barriers a step): all 4096 GLWE outputs against the oracle."""
    ks, eng = full
    lwe, lut, exp = plain_pbs_4096
    got = eng.generalized_pbs(lwe, lut, 0, 0, 0)
    assert eng.last_blind_rotate_kernel() == "blind_rotate2p_kernel<2,16,10>"
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} ciphertexts differ, first {bad[:8]}"


def test_config2_batch_4096_pbs_univariate_every_ciphertext(full, plain_pbs_4096):
    """programmable_bootstrap_univariate at B = 4096, n = 637 (fused sample_extract(., 0) epilogue): all 4096 LWE outputs
    against sample_extract of the oracle's GLWE (glwe_ciphertext_ops.rs:31-76), and a sample against the oracle's own
    univariate entry point."""
    ks, eng = full
    P = ks.params
    lwe, lut, exp_glwe = plain_pbs_4096
    got = eng.pbs_univariate(lwe, lut)
    assert eng.last_blind_rotate_kernel() == "blind_rotate2p_kernel<2,16,10>"
    exp = np.stack([O.sample_extract(g, 0, P.N, P.k) for g in exp_glwe])
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} ciphertexts differ, first {bad[:8]}"
    for i in (0, 4095):
        assert np.array_equal(got[i], O.pbs_univariate(lwe[i], lut, ks.bsk_fft, P)), i


def test_config2_plain_pbs_512_and_ragged_1031(full, plain_pbs_4096):
    """The same ciphertexts through the two-ciphertexts-per-workgroup shape (B = 512: `blind_rotate2p2_kernel<2,16,6>`,
    every output against the oracle), the latency shape (B = 200) and a ragged throughput launch (B = 1031 =
    257 workgroups of four + 3)."""
    ks, eng = full
    lwe, lut, exp = plain_pbs_4096
    got = eng.generalized_pbs(lwe[:512], lut, 0, 0, 0)
    assert eng.last_blind_rotate_kernel() == "blind_rotate2p2_kernel<2,16,6>"
    assert np.array_equal(got, exp[:512])
    got = eng.generalized_pbs(lwe[3000:3200], lut, 0, 0, 0)
    assert eng.last_blind_rotate_kernel() == "blind_rotate8_kernel<2,16>"
    assert np.array_equal(got, exp[3000:3200])
    got = dev_bootstrap(eng, lwe[1000:2031], lut, 0, 0, 0)        # one launch: 257 workgroups of four + 3
    assert eng.last_blind_rotate_kernel() == "blind_rotate2p_kernel<2,16,10>"
    assert np.array_equal(got, exp[1000:2031])
    u = dev_bootstrap(eng, lwe[1000:2031], lut, extract=True)
    P = ks.params
    assert np.array_equal(u, np.stack([O.sample_extract(g, 0, P.N, P.k) for g in exp[1000:2031]]))
    got = dev_bootstrap(eng, lwe[:4096], lut, 0, 0, 0)            # and the whole batch as one 1024-workgroup launch
    assert np.array_equal(got, exp)


def test_golden_default128_fixture_plain_pbs(golden_dir):
    """The log_v = 0 entries of the DEFAULT_128 fixture: generalized PBS (GLWE out) and univariate PBS (LWE out)."""
    z = np.load(os.path.join(golden_dir, "pbs_default128.npz"))
    ks = keyset(int(z["key_seed"]), int(z["lwe_n"]))
    eng = spf_amd.Engine(to_engine_params(ks.params))
    eng.load_bootstrap_key(ks.bsk_fft)
    assert np.array_equal(eng.generalized_pbs(z["plain_lwe"], z["plain_lut"], 0, 0, 0), z["gen_out_chi0_v0"])
    assert np.array_equal(eng.pbs_univariate(z["plain_lwe"], z["plain_lut"]), z["univariate_out"])


def _torus_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    d = (a.astype(np.uint64) - b.astype(np.uint64)).astype(np.int64)
    return np.abs(d.astype(np.float64)) / 2.0 ** 64


def test_external_product_fft_noise_at_pbs_shape():
    """One GGSW (x) GLWE external product at the PBS shape (N = 2048, k = 1, 2 x 16 bits) on the GPU — a
    one-step blind rotation — against the EXACT integer result: digits x time-domain GGSW rows by the
    u64 negacyclic product (spfo_negacyclic_mul_exact).  The only difference is the f64 FFT round trip;
    its normalised torus distance must stay at the reference's FFT error scale (53-bit mantissa against
    products of magnitude 2^15 * 2^64 * sqrt(4 * 2048) ~ 2^85.5: error ~ 2^-31 of the torus)."""
    P = O.DEFAULT_128.replace(lwe_n=1)
    rng = np.random.default_rng(0xE47)
    N = P.N
    # time-domain GGSW rows, uniform torus words (what an encrypted GGSW looks like): [row p][level][q][N]
    G = rng.integers(0, 1 << 64, (2, 2, 2, N), dtype=np.uint64)
    bsk = np.stack([O.poly_fft(G[p, lvl, q]) for p in range(2) for lvl in range(2) for q in range(2)]).reshape(-1)
    eng = spf_amd.Engine(to_engine_params(P))
    eng.load_bootstrap_key(bsk)
    a_t = 37
    lwe = np.array([[np.uint64(a_t << 52), 0]], dtype=np.uint64)     # a~ = 37, b~ = 0
    d0 = rng.integers(0, 1 << 64, 2 * N, dtype=np.uint64)
    got = eng.generalized_pbs(lwe, d0)[0]
    assert np.array_equal(got, O.generalized_pbs(lwe[0], d0, bsk, P))  # the oracle computes the same words
    # exact: acc + sum_p sum_j digit_j(X^a acc_p - acc_p) * G[p][L-1-j][q]   (fft_ops.rs:23-98, radix.rs:157-162)
    rot = np.concatenate([O.poly_mul_pos_monomial(d0[:N], a_t), O.poly_mul_pos_monomial(d0[N:], a_t)])
    diff = rot - d0
    exact = d0.copy()
    for p in range(2):
        digs = O.decompose_poly(diff[p * N:(p + 1) * N], P.pbs_radix_log, P.pbs_count)  # least significant first
        for j in range(2):
            for q in range(2):
                exact[q * N:(q + 1) * N] += O.negacyclic_mul_exact(digs[j], G[p, 1 - j, q])
    # the exact side no longer rests on the oracle alone: tests/poly_ref.py states the same step independently
    assert np.array_equal(exact.reshape(2, N), R.generalized_pbs(lwe[0], d0.reshape(2, N), G[None], P.pbs_radix_log, P.pbs_count))
    dist = _torus_distance(got, exact)
    assert dist.max() < 2.0 ** -26, dist.max()
    assert dist.max() > 0.0          # it IS a floating-point transform: not exact, just small
    assert np.sqrt((dist ** 2).mean()) < 2.0 ** -29


def test_golden_default128_fixture(golden_dir):
    """DEFAULT_128 fixture: ciphertexts in / out as committed data, key re-derived from the stored seed."""
    z = np.load(os.path.join(golden_dir, "pbs_default128.npz"))
    ks = keyset(int(z["key_seed"]), int(z["lwe_n"]))
    eng = spf_amd.Engine(to_engine_params(ks.params))
    eng.load_bootstrap_key(ks.bsk_fft)
    assert np.array_equal(eng.circuit_bootstrap_pbs(z["lwe"]), z["cbs_out"])
    assert int(ks.bsk_fft.view(np.uint64).sum(dtype=np.uint64)) == int(z["bsk_checksum"]), "key recipe drifted"


def test_config4_shard_8192_default128(full):
    """BASELINE configs[3] ("65536 PBS sharded across 8xMI355X"): the per-GPU shard, B = 8192 at n = 637, through
    spf_circuit_bootstrap_pbs_batch.  Sampled ciphertexts (first / last of a host slice of 1024, of a workgroup
    of four, of a chip round, the tail) against the oracle, and the whole batch against the same inputs sent
    1024 at a time (other slice / workgroup boundaries; generalized_programmable_bootstrap has no cross-
    ciphertext state, programmable_bootstrapping.rs:342-410)."""
    ks, eng = full
    B = 8192
    lwe = random_lwe_batch(0xC0F8, B, 637)
    got = eng.circuit_bootstrap_pbs(lwe)
    sample = (0, 1, 3, 4, 1023, 1024, 1027, 2047, 2048, 4095, 4096, 4099, 6143, 7168, 8188, 8189, 8190, 8191)
    _, exp = O.bench_cbs_pbs(lwe[list(sample)], ks.bsk_fft, ks.params, HOST_THREADS, native=False)
    for k, i in enumerate(sample):
        assert np.array_equal(got[i], exp[k]), i
    ref = np.concatenate([eng.circuit_bootstrap_pbs(lwe[i:i + 1024]) for i in range(0, B, 1024)])
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} ciphertexts differ between one 8192-launch and eight 1024-launches, first {bad[:8]}"


def test_big_batches_are_bit_stable_run_to_run(full):
    """Determinism at bench sizes (r03): a hazard that shows as ONE wrong register in one unit out of a thousand — a
    register reused while a load into it is still in flight, as r02's cmux_kernel allowed for the dead selector-row
    loads of a gate's last round — passes every small parity test.  Same inputs, three runs, every word equal, for the
    streaming CMUX at 4096 gates (2048 workgroups) and for the whole circuit bootstrap (blind rotation, trace with its
    parked accumulator half, scheme switch) at 2048 ciphertexts; plus every sixteenth of them (and every workgroup slot, both sides of
    a chip round) against the oracle."""
    ks, eng = full
    P = ks.params
    rng = np.random.default_rng(0xD37)
    B = 4096
    a = random_glwe(41, B, P.glwe_len)
    b = random_glwe(42, B, P.glwe_len)
    n = 2 * 4 * 2 * 1024
    g = ((rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))) * 2.0 ** 60).astype(np.complex128)
    first = eng.cmux(g, a, b)
    for _ in range(2):
        again = eng.cmux(g, a, b)
        bad = np.nonzero((again != first).any(axis=1))[0]
        assert bad.size == 0, f"cmux: {bad.size} gates differ between two runs on the same inputs, first {bad[:8]}"
    for i in (0, B - 1):
        assert np.array_equal(first[i], O.cmux(a[i], b[i], g[i], P.N, P.k, P.cbs_radix_log, P.cbs_count)), i
    del first, again, g

    r = O.Rng(0x7A11)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, P), O.gen_ssk_fft(r, ks.glwe_sk, P)
    eng.load_automorphism_key(ak)
    eng.load_scheme_switch_key(ssk)
    B = 2048
    lwe = random_lwe_batch(0xD38, B, 637)
    first = eng.circuit_bootstrap(lwe)
    again = eng.circuit_bootstrap(lwe)
    bad = np.nonzero((again.reshape(B, -1).view(np.uint64) != first.reshape(B, -1).view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"circuit bootstrap: {bad.size} ciphertexts differ between two runs, first {bad[:8]}"
    # against the oracle: every slot of a bootstrap workgroup (4 ciphertexts) and of a trace / scheme-switch workgroup (4 units =
    # one ciphertext), both sides of a chip round of the bootstrap (1024), the last ciphertexts
    for i in sorted(set(range(0, B, 16)) | {1, 2, 3, 517, 1022, 1023, 1025, 1538, B - 2, B - 1}):
        exp = O.circuit_bootstrap(lwe[i], ks.bsk_fft, ak, ssk, P)
        assert np.array_equal(first[i].view(np.float64).reshape(-1), exp.view(np.float64).reshape(-1)), i


_SOAK = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["SPF_ROOT"])
import torch
import oracle as O
import spf_amd

P = spf_amd.DEFAULT_128
OP = O.DEFAULT_128
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
g = torch.Generator(device=dev).manual_seed(0x50A4)
LAUNCH, LAUNCHES = 4096, 256           # 256 launches x 4096 gates = 1 048 576 gates per pass
POOL = LAUNCH + LAUNCHES               # launch l takes gates l .. l + 4095 of the pool: every launch pairs the gates with
                                       # other workgroup slots, neighbours and addresses
sel = torch.randn((POOL, P.cbs_ggsw_complex * 2), generator=g, device=dev, dtype=torch.float64) * (2.0 ** 60)
da = torch.randint(-(2 ** 63), 2 ** 63 - 1, (POOL, P.glwe_words), generator=g, device=dev, dtype=torch.int64)
db = torch.randint(-(2 ** 63), 2 ** 63 - 1, (POOL, P.glwe_words), generator=g, device=dev, dtype=torch.int64)
out = torch.empty((LAUNCH, P.glwe_words), device=dev, dtype=torch.int64)
stream = torch.cuda.current_stream().cuda_stream
w = torch.arange(LAUNCH * P.glwe_words, device=dev, dtype=torch.int64).reshape(LAUNCH, -1) * 2654435761 + 12345


def one_pass(keep):
    sums = []
    for l in range(LAUNCHES):
        eng.cmux_dev(stream, LAUNCH, sel[l].data_ptr(), da[l].data_ptr(), db[l].data_ptr(), out.data_ptr())
        sums.append(torch.stack([out.sum(), (out * w).sum(), out[0].sum(), out[-1].sum()]))
        if l in keep:
            keep[l] = (out[0].cpu().numpy().view(np.uint64).copy(), out[-1].cpu().numpy().view(np.uint64).copy())
    return torch.stack(sums).cpu().numpy()


keep = {l: None for l in (0, 1, 7, 100, 255)}
first = one_pass(keep)
second = one_pass({})
bad = np.nonzero((first != second).any(axis=1))[0]
assert bad.size == 0, f"launches {bad[:8]} differ between two passes over the same 1 048 576 gates"
# a gate's result does not depend on the launch it is in: gate l + 4095 is the last gate of launch l and gate 4095 - ... of
# later ones; first / last gate of sampled launches against the oracle
sel_h = lambda i: sel[i].cpu().numpy().view(np.complex128)
u = lambda t, i: t[i].cpu().numpy().view(np.uint64)
for l, (o_first, o_last) in keep.items():
    for i, got in ((l, o_first), (l + LAUNCH - 1, o_last)):
        exp = O.cmux(u(da, i), u(db, i), sel_h(i), OP.N, OP.k, OP.cbs_radix_log, OP.cbs_count)
        assert np.array_equal(got, exp), (l, i)
assert eng.last_cmux_kernel() == "cmux_kernel<4,4,2,stream>", eng.last_cmux_kernel()
print("CMUX_SOAK_OK", LAUNCHES * LAUNCH * 2)
'''


@pytest.mark.timeout(900)
def test_cmux_soak_one_million_gates_two_passes():
    """VERDICT r3 task 4: >= 1 M gates through spf_cmux_dev in launches of 4096, two passes, every launch's output
    checksums equal between the passes (a register hit by a load landing late shows as a launch that differs from run to
    run), plus the first and last gate of sampled launches against the oracle.  The kernels no longer issue a load nobody
    consumes (the last round / last step is its own copy without requests).  In a child process: torch holds the 1.5 GB
    gate pool on the device and must be imported before the library's HIP runtime."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SPF_ROOT=root)
    r = subprocess.run([sys.executable, "-c", _SOAK], capture_output=True, text=True, timeout=840, cwd=root, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "CMUX_SOAK_OK 2097152" in r.stdout, r.stdout[-1500:]
