"""Keys and polynomials in standard (integer) form on the GPU: `spf_poly_fft_*` against the oracle's `PolynomialRef::fft`, the
`_std` key loaders and the `ComputeKeyNonFft` bincode loader against the float loaders fed with the oracle's transform of the
same words, single context and device group, and the C++ mirror.  Everything is compared as uint64 words: no tolerance anywhere."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd.keys import ComputeKeyNonFft, serialize_compute_key_nonfft
from tests import polyref_cases as C
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def engine_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count, ss_radix_log=P.ss_radix_log,
                                       ss_radix_count=P.ss_count)


def u64(a) -> np.ndarray:
    return np.ascontiguousarray(a).reshape(-1).view(np.uint64)


def key_blob(eng, which: int) -> np.ndarray:
    ptr, nbytes = eng.key_blob(which)
    out = np.empty(nbytes // 8, dtype=np.uint64)
    eng.device_download(None, out, ptr)
    return out


# ----------------------------------------------------------------------------------------------- the primitive


def tie_words(rng, count: int) -> np.ndarray:
    """words whose i64 -> f64 conversion is an exact tie, both signs: for 2^(53+j) <= |v| < 2^(54+j) doubles are 2^(j+1) apart, so
    the odd multiples of 2^j lie half-way (j = 0 .. 9; even and odd upper neighbours alike, so ties-to-even goes both ways) —
    and the odd multiples of 2^10 above 2^53, which an i64 holds exactly but which are ties in the top binade for code that
    converts the word as unsigned (2^63 + odd * 2^10)"""
    out = []
    for j in range(10):
        m = rng.integers(1 << 53, 1 << 54, count, dtype=np.uint64) | np.uint64(1)   # odd, in [2^53, 2^54)
        v = m << np.uint64(j)
        out += [v, np.uint64(0) - v]
    m = rng.integers(1 << 43, 1 << 52, count, dtype=np.uint64) | np.uint64(1)
    v = m << np.uint64(10)                                                                           # odd * 2^10 in [2^53, 2^62)
    out += [v, np.uint64(0) - v, v | np.uint64(1 << 63)]
    return np.concatenate(out)


def operand_rows(n: int, rng):
    """the special polynomials (rows of N words) every shape is run on"""
    rows = [np.zeros(n, dtype=np.uint64), np.full(n, 1 << 63, dtype=np.uint64), np.full(n, M64, dtype=np.uint64),
            np.where(np.arange(n) % 2 == 0, np.uint64(1 << 63), np.uint64((1 << 63) - 1))]
    rows += [C.cos_poly(n, m, (1 << 63) - 1) for m in (0, 3, n // 2 - 1)]
    ties = tie_words(rng, max(8, n // 8))
    ties = np.resize(rng.permutation(ties), (-(-ties.size // n), n))
    rows += list(ties)
    rows += list(rng.integers(0, 1 << 64, (4, n), dtype=np.uint64))
    return np.stack(rows)


def poly_fft_dev(eng, x: np.ndarray, in_place: bool) -> np.ndarray:
    n_polys, n = x.shape
    d_in = eng.device_alloc(x.nbytes)
    d_out = d_in if in_place else eng.device_alloc(x.nbytes)
    try:
        eng.device_upload(d_in, x)
        eng.poly_fft_dev(None, n_polys, d_in, d_out)
        out = np.empty((n_polys, n // 2), dtype=np.complex128)
        eng.device_download(None, out, d_out)
        if not in_place:                       # the input is left as it was
            back = np.empty_like(x)
            eng.device_download(None, back, d_in)
            assert np.array_equal(back, x)
    finally:
        eng.device_free(d_in)
        if not in_place:
            eng.device_free(d_out)
    return out


@pytest.mark.parametrize("shape", list(C.PBS_SHAPES))
def test_poly_fft_is_the_oracles_transform_bit_for_bit(shape):
    P = C.PBS_SHAPES[shape]
    n = P.N
    eng = spf_amd.Engine(engine_params(P))
    rng = np.random.default_rng([0x57D, n, P.k])
    special = operand_rows(n, rng)
    polys = np.concatenate([special, rng.integers(0, 1 << 64, (5096 - special.shape[0], n), dtype=np.uint64)])
    exp = np.stack([O.poly_fft(p) for p in polys]).view(np.uint64)
    one_ggsw = (P.k + 1) * P.pbs_count * (P.k + 1)
    for in_place in (False, True):
        for n_polys in (1, 3, one_ggsw, 5096):
            # the small batches slide over every special polynomial
            starts = [0] if n_polys == 5096 else range(0, special.shape[0], n_polys)
            for at in starts:
                got = poly_fft_dev(eng, polys[at:at + n_polys], in_place).view(np.uint64)
                bad = np.flatnonzero((got != exp[at:at + n_polys]).any(axis=1))
                assert bad.size == 0, (shape, "in place" if in_place else "out of place", n_polys, at, bad[:8])
    # the host-pointer form equals the device-pointer form
    for n_polys in (1, 3, one_ggsw, 5096):
        assert np.array_equal(eng.poly_fft(polys[:n_polys]).view(np.uint64), exp[:n_polys]), (shape, n_polys)
    assert eng.poly_fft(polys[:0]).shape == (0, n // 2)
    # a partial overlap is refused; so is a null operand
    d = eng.device_alloc(3 * n * 8)
    try:
        with pytest.raises(spf_amd.SpfError) as e:
            eng.poly_fft_dev(None, 2, d, d + n * 8)
        assert e.value.status == 1
        with pytest.raises(spf_amd.SpfError):
            eng.poly_fft_dev(None, 2, d, None)
    finally:
        eng.device_free(d)
    eng.close()


# ----------------------------------------------------------------------------------------------- keys


class Keys:
    def __init__(self, P, seed: int, ksk: bool = False):
        self.P = P
        hk = C.honest_keys(P, seed, bsk=True, ak=True, ssk=True)
        self.std = {0: u64(hk.bsk), 2: u64(hk.ak), 3: u64(hk.ssk)}
        self.fft = {w: C.key_fft(rows) for w, rows in ((0, hk.bsk), (2, hk.ak), (3, hk.ssk))}
        self.ksk = (O.gen_ksk(O.Rng(0x4B5 + seed), hk.glwe_sk, hk.lwe_sk, P.ks_radix_log, P.ks_count, P.lwe_std) if ksk else None)

    def load_std(self, eng):
        eng.load_bootstrap_key_std(self.std[0])
        eng.load_automorphism_key_std(self.std[2])
        eng.load_scheme_switch_key_std(self.std[3])
        if self.ksk is not None:
            eng.load_keyswitch_key(self.ksk)

    def load_fft(self, eng):
        eng.load_bootstrap_key(self.fft[0])
        eng.load_automorphism_key(self.fft[2])
        eng.load_scheme_switch_key(self.fft[3])
        if self.ksk is not None:
            eng.load_keyswitch_key(self.ksk)

    def nonfft_blob(self) -> bytes:
        return serialize_compute_key_nonfft(ComputeKeyNonFft(self.std[0], u64(self.ksk), self.std[2], self.std[3]))


@pytest.fixture(scope="module")
def d128():
    return Keys(C.D128, 0x51D, ksk=True)


def same_outputs(std_eng, fft_eng, P, batches, seed):
    """circuit_bootstrap_pbs, pbs_univariate, a full circuit bootstrap and a cmux on its result: word-equal between the contexts"""
    rng = np.random.default_rng([0x5A3E, seed, P.N])
    lut = spf_amd.generate_lut([lambda x: (3 * x + 1) % 4], 2, std_eng.params) if P.N >= 8 else None
    for B in batches:
        lwe = rng.integers(0, 1 << 64, (B, P.lwe_n + 1), dtype=np.uint64)
        a = std_eng.circuit_bootstrap_pbs(lwe)
        assert np.array_equal(a, fft_eng.circuit_bootstrap_pbs(lwe)), ("circuit_bootstrap_pbs", B)
        kernel = std_eng.last_blind_rotate_kernel()
        assert kernel == fft_eng.last_blind_rotate_kernel()
        assert np.array_equal(std_eng.pbs_univariate(lwe, lut), fft_eng.pbs_univariate(lwe, lut)), ("pbs_univariate", B)
        g = std_eng.circuit_bootstrap(lwe)
        assert np.array_equal(g.view(np.uint64), fft_eng.circuit_bootstrap(lwe).view(np.uint64)), ("circuit_bootstrap", B)
        d0, d1 = rng.integers(0, 1 << 64, (2, B, (P.k + 1) * P.N), dtype=np.uint64)
        assert np.array_equal(std_eng.cmux(g, d0, d1), fft_eng.cmux(g, d0, d1)), ("cmux", B)
        yield B, kernel


def test_std_loaders_at_default128_hold_the_oracles_spectra_and_bootstrap_alike(d128):
    P = d128.P
    assert P.lwe_n == 637
    std_eng, fft_eng = spf_amd.Engine(engine_params(P)), spf_amd.Engine(engine_params(P))
    # wrong lengths are refused (status 1) and leave the context without the key
    lib, h = std_eng._lib, std_eng._h
    w = d128.std[0]
    for bad in (w.size - 1, w.size + 1, w.size // 2, 0):
        assert lib.spf_load_bootstrap_key_std(h, w.ctypes.data, bad) == 1
    assert lib.spf_load_automorphism_key_std(h, w.ctypes.data, d128.std[3].size) == 1
    assert lib.spf_load_scheme_switch_key_std(h, w.ctypes.data, d128.std[2].size) == 1
    assert lib.spf_load_bootstrap_key_std(h, None, w.size) == 1
    with pytest.raises(spf_amd.SpfError) as e:
        std_eng.circuit_bootstrap_pbs(np.zeros((1, P.lwe_n + 1), dtype=np.uint64))
    assert e.value.status == 3
    for which, load in ((0, std_eng.load_bootstrap_key_std), (2, std_eng.load_automorphism_key_std), (3, std_eng.load_scheme_switch_key_std)):
        load(d128.std[which])
        assert np.array_equal(key_blob(std_eng, which), u64(d128.fft[which])), which
    d128.load_fft(fft_eng)
    seen = dict(same_outputs(std_eng, fft_eng, P, (3, 600), 1))   # a latency shape and the throughput shape
    assert seen[3].startswith("blind_rotate8") and seen[600].startswith("blind_rotate2p_"), seen
    # loading again over a loaded key (the blob holds spectra when the words arrive) gives the same blob
    std_eng.load_bootstrap_key_std(d128.std[0])
    assert np.array_equal(key_blob(std_eng, 0), u64(d128.fft[0]))
    std_eng.close()
    fft_eng.close()


@pytest.mark.parametrize("name,P", [("N128K2", C.N128K2), ("N2048R", C.N2048R)])
def test_std_loaders_at_a_generic_shape_and_at_another_radix(name, P):
    keys = Keys(P, 0x6E0)
    std_eng, fft_eng = spf_amd.Engine(engine_params(P)), spf_amd.Engine(engine_params(P))
    keys.load_std(std_eng)
    keys.load_fft(fft_eng)
    for which in (0, 2, 3):
        assert np.array_equal(key_blob(std_eng, which), u64(keys.fft[which])), (name, which)
    assert [B for B, _ in same_outputs(std_eng, fft_eng, P, (1, 5), 2)] == [1, 5]
    std_eng.close()
    fft_eng.close()


def test_nonfft_bincode_loads_what_the_per_key_loaders_load(d128):
    P = d128.P
    blob = d128.nonfft_blob()
    ref, eng = spf_amd.Engine(engine_params(P)), spf_amd.Engine(engine_params(P))
    d128.load_std(ref)
    eng.load_compute_key_nonfft_bincode(blob + b"trailing bytes are allowed")
    want = [key_blob(ref, w) for w in range(4)]
    for w in range(4):
        assert np.array_equal(key_blob(eng, w), want[w]), w
    assert np.array_equal(want[1], u64(d128.ksk))
    # malformed blobs: a wrong count in every field (the last one included: nothing before it may have been loaded), truncations,
    # and a ComputeKey-order blob
    counts = [d128.std[0].size, u64(d128.ksk).size, d128.std[2].size, d128.std[3].size]
    def broken():   # (one at a time: each is 149 MB)
        off = 0
        for n in counts:
            yield blob[:off] + struct.pack("<Q", n + 1) + blob[off + 8:]
            yield blob[:off + 4]
            yield blob[:off + 8 + 8 * (n // 2)]
            off += 8 + 8 * n
        yield serialize_compute_key_nonfft(ComputeKeyNonFft(d128.std[0], u64(d128.ksk), d128.std[3], d128.std[2]))

    fresh = spf_amd.Engine(engine_params(P))
    lwe = np.random.default_rng(5).integers(0, 1 << 64, (2, P.lwe_n + 1), dtype=np.uint64)
    lwe1 = np.random.default_rng(6).integers(0, 1 << 64, (2, P.k * P.N + 1), dtype=np.uint64)
    before = eng.keyswitch_circuit_bootstrap(lwe1).view(np.uint64)
    for bad in broken():
        for e in (eng, fresh):
            with pytest.raises(spf_amd.SpfError) as err:
                e.load_compute_key_nonfft_bincode(bad)
            assert err.value.status == 1
    for w in range(4):                                            # the keys that were there are untouched and usable
        assert np.array_equal(key_blob(eng, w), want[w]), w
    assert np.array_equal(eng.keyswitch_circuit_bootstrap(lwe1).view(np.uint64), before)
    for call in (lambda: fresh.circuit_bootstrap_pbs(lwe), lambda: fresh.keyswitch_lwe_l1_lwe_l0(lwe1), lambda: fresh.circuit_bootstrap(lwe)):
        with pytest.raises(spf_amd.SpfError) as err:              # ... and nothing was loaded partially
            call()
        assert err.value.status == 3
    for e in (ref, eng, fresh):
        e.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_group_std_loaders_replicate_member_zeros_spectra(d128, devices):
    P = d128.P
    single = spf_amd.Engine(engine_params(P))
    d128.load_std(single)
    want = [key_blob(single, w) for w in range(4)]
    grp = spf_amd.Group(engine_params(P), devices=devices)
    before = grp.replication_stats()["bytes_per_member"]
    if len(devices) == 1:
        grp.load_compute_key_nonfft_bincode(d128.nonfft_blob())
    else:
        d128.load_std(grp)
    assert len(grp) == len(devices)
    for i in range(len(devices)):
        for w in range(4):
            assert np.array_equal(key_blob(grp.member(i), w), want[w]), (devices, i, w)
    if len(devices) > 1:   # the wire carried the four blobs once, as it does for the float loaders
        assert grp.replication_stats()["bytes_per_member"] - before == sum(b.nbytes for b in want)
    lwe = np.random.default_rng(9).integers(0, 1 << 64, (6, P.lwe_n + 1), dtype=np.uint64)
    assert np.array_equal(grp.circuit_bootstrap(lwe).view(np.uint64), single.circuit_bootstrap(lwe).view(np.uint64))
    with pytest.raises(spf_amd.SpfError) as e:                    # validated before a device is touched, the keys stay
        grp.load_bootstrap_key_std(d128.std[0][:-1])
    assert e.value.status == -2
    short = d128.std[0][:-1]
    assert grp._raw.spf_group_load_bootstrap_key_std(grp._h, short.ctypes.data, short.size) == 1
    assert grp._raw.spf_group_load_compute_key_nonfft_bincode(grp._h, short.ctypes.data, 64) == 1
    assert np.array_equal(key_blob(grp.member(0), 0), want[0])
    grp.close()
    single.close()


def test_cpp_evaluation_with_standard_keys_matches_the_float_form(tmp_path):
    """tests/cpp/standard_keys_parity.cpp, built and run as tests/test_gpu_cpp_host.py builds its program"""
    libdir = os.path.dirname(spf_amd.lib_path())
    oracle_so = O.library_path()
    exe = tmp_path / "standard_keys_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "cpp", "standard_keys_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", oracle_so,
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.dirname(oracle_so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
