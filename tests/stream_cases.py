"""The case table of the stream-contract tests: one entry per `_dev` entry point and launch line of spf_hip.hip.

A case names its entry point, its context, its batch size, its operands (inputs, the output, pointer tables), the arguments of
the call and the kernel the library must report afterwards.  Every operand has REAL contents and DECOY contents: a second,
different, valid operand of the same kind (selectors are finite doubles of the same scale; a decoy pointer table holds valid
pointers to decoy operands and a decoy output).  A kernel that runs on the wrong stream therefore reads decoys, or writes
beside the output, and produces a wrong word; it can never fault.

No GPU and no library here: tests/test_stream_cases.py holds the table to the header on the CPU,
tests/test_gpu_stream_contract.py runs it.  The comparison is always with the same library on the null stream, so the keys are
random words and doubles (`context_keys`); no oracle key generation is paid for."""
import re
import zlib
from dataclasses import dataclass
from typing import Callable, Optional, Tuple, Union

import numpy as np

import spf_amd
from tests.blind_rotation_graph_cases import TEST1, engine_params

SENTINEL = 0x5E5E5E5E5E5E5E5E

# ---- contexts -------------------------------------------------------------------------------------------------------------
T = spf_amd.DEFAULT_128.replace(lwe_dimension=3)
CONTEXTS = {
    "T": T,                                                   # the tuned kernels, int8 matrix-core keyswitch
    "T16": T.replace(ks_radix_log=16, ks_radix_count=2),      # a radix the int8 formulation cannot take: keyswitch_kernel
    "G": engine_params(TEST1),                                # N 128, k 2: the generic family
}


def _doubles(seed: int, n_complex: int) -> np.ndarray:
    """random complex values at 2^58, the scale of blind_rotation_graph_cases.random_selectors"""
    out = np.empty(n_complex, dtype=np.complex128)
    v = out.view(np.float64)
    v[...] = np.random.default_rng(seed).standard_normal(v.shape)
    v *= 2.0 ** 58
    return out


def context_keys(name: str, salt: int = 0):
    """(bootstrap, keyswitch, automorphism, scheme-switch) key of context `name`: random, a function of (name, salt) only"""
    P = CONTEXTS[name]
    seed = zlib.crc32(f"keys/{name}/{salt}".encode())
    ksk = np.random.default_rng(seed + 1).integers(0, 1 << 64, size=P.ksk_words, dtype=np.uint64)
    return _doubles(seed, P.bsk_complex), ksk, _doubles(seed + 2, P.ak_complex), _doubles(seed + 3, P.ssk_complex)


# ---- operands -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Operand:
    name: str
    role: str                 # "in", "out", "inout" (poly_fft in place) or "table" (a device array of device pointers: an input)
    rows: int
    row_words: int            # 64-bit words per row (a complex bin is two)
    kind: str = "words"       # "words": uniform u64; "doubles": finite doubles at 2^58 (selectors); tables: unused
    entries: tuple = ()       # table: one (operand name, row) or None (a null pointer) per pointer

    @property
    def words(self) -> int:
        return len(self.entries) if self.role == "table" else self.rows * self.row_words

    @property
    def nbytes(self) -> int:
        return 8 * self.words


_TILE = 16   # rows generated at random; row r is row r % _TILE of them, changed by a function of r // _TILE


def operand_data(case_id: str, op: Operand, which: str, first_row: int = 0, rows: Optional[int] = None) -> np.ndarray:
    """contents of rows [first_row, first_row + rows) of `op` as u64 words, shape (rows, row_words).  which: "real" | "decoy".
    A function of (case id, operand name, which, row) only, so a slice equals the same rows of the whole."""
    assert op.role != "table" and which in ("real", "decoy")
    rows = op.rows - first_row if rows is None else rows
    rng = np.random.default_rng(zlib.crc32(f"{case_id}/{op.name}/{which}".encode()))
    r = np.arange(first_row, first_row + rows)
    if op.kind == "doubles":
        base = rng.standard_normal((_TILE, op.row_words)) * 2.0 ** 58
        out = base[r % _TILE] * (1.0 + (r // _TILE)[:, None] / 64.0)    # finite, same scale, every row different
        return out.view(np.uint64)
    base = rng.integers(0, 1 << 64, size=(_TILE, op.row_words), dtype=np.uint64)
    return base[r % _TILE] + ((r // _TILE).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))[:, None]


def table_pointers(case: "ResolvedCase", op: Operand, base: dict) -> np.ndarray:
    """the pointer table `op` over the buffers `base` (operand name -> device address)"""
    by_name = {o.name: o for o in case.operands}
    out = np.zeros(len(op.entries), dtype=np.uint64)
    for i, e in enumerate(op.entries):
        if e is not None:
            name, row = e
            out[i] = base[name] + 8 * row * by_name[name].row_words
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    ctx: str
    entry: str                                   # the C symbol
    B: Union[int, str]                           # a batch size, or the blind-rotation shape whose smallest batch is wanted
    build: Callable                              # (P, B) -> (operands, args(ptrs) -> the C arguments after (ctx, stream))
    kernels: Tuple[Tuple[str, str], ...] = ()    # (("pbs" | "cmux" | "keyswitch", regular expression of the reported name), ...)

    def resolve(self, B: Optional[int] = None) -> "ResolvedCase":
        B = B if B is not None else (self.B if isinstance(self.B, int) else NOMINAL_B[self.B])
        operands, args = self.build(CONTEXTS[self.ctx], B)
        return ResolvedCase(self, B, tuple(operands), args)


@dataclass(frozen=True)
class ResolvedCase:
    case: Case
    B: int
    operands: Tuple[Operand, ...]
    args: Callable

    @property
    def id(self) -> str:
        return self.case.id

    @property
    def inputs(self):
        return [o for o in self.operands if o.role in ("in", "inout", "table")]

    @property
    def output(self) -> Operand:
        (out,) = [o for o in self.operands if o.role in ("out", "inout")]
        return out


# The blind-rotation shape is picked from the batch size and the device's CU count.  The GPU test finds the smallest batch of
# each shape from the REPORTED kernel name; these are the batches of a 256-CU part, for the checks that run without a GPU.
NOMINAL_B = {"blind_rotate8": 2, "blind_rotate2p2": 257, "blind_rotate2p": 513}
PBS_SHAPES = tuple(NOMINAL_B)


def pbs_kernel(shape: str, even: bool, ctx: str = "T"):
    """log_v >= 1 makes every rotation even: the kernels report ",even"; the 2p shapes carry a build knob before it"""
    if ctx == "G":
        return (("pbs", re.escape("generic_pbs_kernel")),)
    knob = "" if shape == "blind_rotate8" else r",\d+"
    return (("pbs", re.escape(shape + "_kernel<2,16") + knob + (",even>" if even else ">")),)


def ks_kernel(ctx: str):
    return (("keyswitch", "ks_gemm_lds_kernel" if ctx == "T" else "keyswitch_kernel"),)


def cmux_kernel(name: str, ctx: str = "T"):
    return (("cmux", re.escape("generic_cmux_kernel" if ctx == "G" else name)),)


def _in(name, rows, row_words, kind="words"):
    return Operand(name, "in", rows, row_words, kind)


def _out(name, rows, row_words):
    return Operand(name, "out", rows, row_words)


def _ggsw_words(P):
    return 2 * P.cbs_ggsw_complex


def _glev_words(P):
    return P.cbs_radix_count * P.glwe_words


def _keyswitch(P, B):
    return [_in("lwe1", B, P.lwe1_words), _out("lwe0", B, P.lwe0_words)], lambda p: (B, p["lwe1"], p["lwe0"])


def _generalized(log_v, per_item):
    def build(P, B):
        ops = [_in("lwe0", B, P.lwe0_words), _in("lut", B if per_item else 1, P.glwe_words), _out("glwe", B, P.glwe_words)]
        return ops, lambda p: (B, p["lwe0"], p["lut"], P.glwe_words if per_item else 0, 0, log_v, 1 << 61, p["glwe"])
    return build


def _univariate(per_item):
    def build(P, B):
        ops = [_in("lwe0", B, P.lwe0_words), _in("lut", B if per_item else 1, P.glwe_words), _out("lwe1", B, P.lwe1_words)]
        return ops, lambda p: (B, p["lwe0"], p["lut"], P.glwe_words if per_item else 0, p["lwe1"])
    return build


def _bivariate(P, B):
    ops = [_in("left", B, P.lwe0_words), _in("right", B, P.lwe0_words), _in("lut", 1, P.glwe_words), _out("lwe1", B, P.lwe1_words)]
    return ops, lambda p: (B, p["left"], p["right"], p["lut"], 0, 2, p["lwe1"])


def _cbs_pbs(P, B):
    return [_in("lwe0", B, P.lwe0_words), _out("glwe", B, P.glwe_words)], lambda p: (B, p["lwe0"], p["glwe"])


def _circuit_bootstrap(P, B):
    return [_in("lwe0", B, P.lwe0_words), _out("ggsw", B, _ggsw_words(P))], lambda p: (B, p["lwe0"], p["ggsw"])


def _trace(P, B):
    return [_in("glwe", B, P.glwe_words), _out("glev", B, _glev_words(P))], lambda p: (B, p["glwe"], p["glev"])


def _scheme_switch(P, B):
    return [_in("glev", B, _glev_words(P)), _out("ggsw", B, _ggsw_words(P))], lambda p: (B, p["glev"], p["ggsw"])


def _sample_extract(P, B):
    return [_in("glwe", B, P.glwe_words), _out("lwe1", B, P.lwe1_words)], lambda p: (B, p["glwe"], 5, p["lwe1"])


def _not(P, B):
    return [_in("a", B, P.glwe_words), _out("out", B, P.glwe_words)], lambda p: (B, p["a"], p["out"])


def _xor(P, B):
    ops = [_in("a", B, P.glwe_words), _in("b", B, P.glwe_words), _out("out", B, P.glwe_words)]
    return ops, lambda p: (B, p["a"], p["b"], p["out"])


def _mul_xn(P, B):
    return [_in("a", B, P.glwe_words), _out("out", B, P.glwe_words)], lambda p: (B, p["a"], P.polynomial_degree + 3, p["out"])


def _cmux(P, B):
    ops = [_in("sel", B, _ggsw_words(P), "doubles"), _in("a", B, P.glwe_words), _in("b", B, P.glwe_words), _out("out", B, P.glwe_words)]
    return ops, lambda p: (B, p["sel"], p["a"], p["b"], p["out"])


def _glev_cmux(P, B):
    ops = [_in("sel", B, _ggsw_words(P), "doubles"), _in("a", B, _glev_words(P)), _in("b", B, _glev_words(P)), _out("out", B, _glev_words(P))]
    return ops, lambda p: (B, p["sel"], p["a"], p["b"], p["out"])


def _multiply(P, B):
    ops = [_in("glwe", B, P.glwe_words), _in("ggsw", B, _ggsw_words(P), "doubles"), _out("out", B, P.glwe_words)]
    return ops, lambda p: (B, p["glwe"], p["ggsw"], p["out"])


def _cmux_scattered(P, units):
    """units in reverse order of their operands; the last one multiplies by the zero ciphertext (a null `a`)"""
    entries = []
    for u in range(units):
        r = units - 1 - u
        entries += [("sel", r), ("a", r) if u < units - 1 else None, ("b", r), ("out", u)]
    ops = [_in("sel", units, _ggsw_words(P), "doubles"), _in("a", units, P.glwe_words), _in("b", units, P.glwe_words),
           Operand("ptrs", "table", 0, 0, entries=tuple(entries)), _out("out", units, P.glwe_words)]
    return ops, lambda p: (units, p["ptrs"])


def _gather_rows(P, rows):
    words = P.glwe_words
    entries = tuple(("src", 2 * (rows - 1 - r)) for r in range(rows))   # every other row, last first
    ops = [_in("src", 2 * rows, words), Operand("ptrs", "table", 0, 0, entries=entries), _out("dst", rows, words)]
    return ops, lambda p: (rows, words, p["ptrs"], p["dst"])


def _pack(n_bits):
    def build(P, B):
        return [_in("bits", B * n_bits, P.glwe_words), _out("packed", B, P.glwe_words)], lambda p: (B, n_bits, p["bits"], p["packed"])
    return build


def _unpack_l1(n_bits):
    def build(P, B):
        return [_in("packed", B, P.glwe_words), _out("lwe1", B * n_bits, P.lwe1_words)], lambda p: (B, n_bits, p["packed"], p["lwe1"])
    return build


def _unpack_cbs(n_bits):
    def build(P, B):
        return [_in("packed", B, P.glwe_words), _out("ggsw", B * n_bits, _ggsw_words(P))], lambda p: (B, n_bits, p["packed"], p["ggsw"])
    return build


def _blind_rotation(n_bits, log_stride=1):
    def build(P, B):
        ops = [_in("shift", B * n_bits, _ggsw_words(P), "doubles"), _in("glwe", B, P.glwe_words), _out("out", B, P.glwe_words)]
        return ops, lambda p: (B, n_bits, log_stride, p["shift"], p["glwe"], p["out"])
    return build


def _poly_fft(in_place):
    def build(P, n):
        N = P.polynomial_degree
        if in_place:
            return [Operand("polys", "inout", n, N)], lambda p: (n, p["polys"], p["polys"])
        return [_in("polys", n, N), _out("spectra", n, N)], lambda p: (n, p["polys"], p["spectra"])
    return build


def _table():
    c = []

    def add(id_, ctx, entry, B, build, kernels=()):
        c.append(Case(id_, ctx, entry, B, build, tuple(kernels)))

    # LWE keyswitch: ks_rowsum memset + ks_digits + ks_gemm_lds (one and two row tiles); keyswitch_kernel on T16 and G
    for ctx, B in (("T", 3), ("T", 130), ("T16", 3), ("G", 3)):
        add(f"keyswitch-{ctx}-B{B}", ctx, "spf_keyswitch_lwe_l1_lwe_l0_dev", B, _keyswitch, ks_kernel(ctx))
    # the bootstraps: every blind-rotation shape, log_v 0 and 2, one LUT for the batch and one per item
    for i, shape in enumerate(PBS_SHAPES):
        for log_v in (0, 2):
            per_item = (i + log_v // 2) % 2 == 1
            add(f"generalized_pbs-T-{shape}-logv{log_v}-{'lut_each' if per_item else 'lut_shared'}", "T", "spf_generalized_pbs_dev",
                shape, _generalized(log_v, per_item), pbs_kernel(shape, log_v > 0))
        add(f"pbs_univariate-T-{shape}-{'lut_each' if i == 1 else 'lut_shared'}", "T", "spf_pbs_univariate_dev", shape, _univariate(i == 1),
            pbs_kernel(shape, False))
        add(f"circuit_bootstrap_pbs-T-{shape}", "T", "spf_circuit_bootstrap_pbs_dev", shape, _cbs_pbs, pbs_kernel(shape, True))
    add("generalized_pbs-G-B2", "G", "spf_generalized_pbs_dev", 2, _generalized(1, True), pbs_kernel("", True, "G"))
    add("pbs_univariate-G-B2", "G", "spf_pbs_univariate_dev", 2, _univariate(False), pbs_kernel("", False, "G"))
    add("circuit_bootstrap_pbs-G-B2", "G", "spf_circuit_bootstrap_pbs_dev", 2, _cbs_pbs, pbs_kernel("", True, "G"))
    for ctx in ("T", "G"):   # the packing kernel, then the bootstrap of the packed input in the context
        add(f"pbs_bivariate-{ctx}-B5", ctx, "spf_pbs_bivariate_dev", 5, _bivariate, pbs_kernel("blind_rotate8", False, ctx))
    for ctx, B in (("T", 1), ("T", 5), ("G", 2)):
        add(f"mod_switch_trace_and_rotate-{ctx}-B{B}", ctx, "spf_mod_switch_trace_and_rotate_dev", B, _trace)
        add(f"scheme_switch-{ctx}-B{B}", ctx, "spf_scheme_switch_dev", B, _scheme_switch)
    for ctx in ("T", "G"):
        add(f"circuit_bootstrap-{ctx}-B5", ctx, "spf_circuit_bootstrap_dev", 5, _circuit_bootstrap, pbs_kernel("blind_rotate8", True, ctx))
        for name, build in (("sample_extract_l1", _sample_extract), ("glwe_not", _not), ("glwe_xor", _xor), ("glwe_mul_xn", _mul_xn)):
            add(f"{name}-{ctx}-B3", ctx, f"spf_{name}_dev", 3, build)
    # CMUX: four waves per gate, two gates per workgroup, streaming selector loads (896 x 256 KiB = 224 MiB of selectors)
    for B, name in ((1, "cmux4_kernel<4,4>"), (300, "cmux_kernel<4,4,2>"), (896, "cmux_kernel<4,4,2,stream>")):
        add(f"cmux-T-B{B}", "T", "spf_cmux_dev", B, _cmux, cmux_kernel(name))
    add("cmux-G-B2", "G", "spf_cmux_dev", 2, _cmux, cmux_kernel("", "G"))
    for ctx in ("T", "G"):
        add(f"glev_cmux-{ctx}-B2", ctx, "spf_glev_cmux_dev", 2, _glev_cmux, cmux_kernel("cmux4_kernel<4,4>", ctx))
        add(f"multiply_glwe_ggsw-{ctx}-B2", ctx, "spf_multiply_glwe_ggsw_dev", 2, _multiply, cmux_kernel("cmux4_kernel<4,4>", ctx))
    add("cmux_scattered-T-3", "T", "spf_cmux_scattered_dev", 3, _cmux_scattered, cmux_kernel("cmux4_kernel<4,4>"))
    add("gather_rows-T-3", "T", "spf_gather_rows_dev", 3, _gather_rows)
    for ctx in ("T", "G"):
        add(f"glwe_pack-{ctx}-B2x3", ctx, "spf_glwe_pack_dev", 2, _pack(3))
        add(f"glwe_unpack_l1-{ctx}-B2x3", ctx, "spf_glwe_unpack_l1_dev", 2, _unpack_l1(3))
        add(f"unpack_circuit_bootstrap-{ctx}-B2x3", ctx, "spf_unpack_circuit_bootstrap_dev", 2, _unpack_cbs(3),
            ks_kernel(ctx) + pbs_kernel("blind_rotate8", True, ctx))
    # blind rotation by an encrypted shift: the ping-pong between the context's buffer and the output ends in the output for
    # either parity; every shape of the rotate-fused CMUX; the generic family's mul_xn into the context, one CMUX per item
    for B, name in ((1, "cmux4_kernel<4,4,rot>"), (300, "cmux_kernel<4,4,2,rot>")):
        for n_bits in (1, 2, 3):
            add(f"blind_rotation-T-B{B}-bits{n_bits}", "T", "spf_blind_rotation_dev", B, _blind_rotation(n_bits), cmux_kernel(name))
    add("blind_rotation-T-B896-bits1", "T", "spf_blind_rotation_dev", 896, _blind_rotation(1), cmux_kernel("cmux_kernel<4,4,2,stream,rot>"))
    add("blind_rotation-G-B2-bits3", "G", "spf_blind_rotation_dev", 2, _blind_rotation(3), cmux_kernel("", "G"))
    add("poly_fft-T-5", "T", "spf_poly_fft_dev", 5, _poly_fft(False))
    add("poly_fft-T-5-in_place", "T", "spf_poly_fft_dev", 5, _poly_fft(True))
    add("poly_fft-G-3", "G", "spf_poly_fft_dev", 3, _poly_fft(False))
    return tuple(c)


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# `_dev` prototypes of the header that have no case, each with its reason (tests/test_stream_cases.py closes the list)
EXCLUDED = {}

# The multi-step entry points, whose intermediates live in buffers of the context, as (case id, first batch, second batch):
# two calls back to back on one stream, and a second call that has to grow those buffers (tests (b) and (c)).  The batch sizes
# differ, the second is the larger; each call has its own operands (`operand_data` is seeded by the id the test gives it).
MULTI_STEP = (
    ("circuit_bootstrap-T-B5", 3, 7),
    ("circuit_bootstrap-G-B5", 2, 5),
    ("unpack_circuit_bootstrap-T-B2x3", 1, 3),
    ("unpack_circuit_bootstrap-G-B2x3", 1, 2),
    ("pbs_bivariate-T-B5", 4, 9),
    ("pbs_bivariate-G-B5", 2, 3),
    ("blind_rotation-T-B1-bits2", 2, 5),
    ("blind_rotation-T-B1-bits3", 3, 4),
    ("blind_rotation-G-B2-bits3", 1, 3),
    ("keyswitch-T-B3", 5, 131),
)
