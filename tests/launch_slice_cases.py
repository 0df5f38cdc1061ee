"""Every place where the host code of spf_amd/csrc/spf_hip.hip cuts one call into several kernel launches (`for (size_t at = 0;
at < B; at += ...)`, and the `m0` loop over the rows of a linear map), each with the count one launch takes restated in Python and
the GPU case that takes the loop past its first launch.  Shared by tests/test_launch_slice_cases.py (CPU: every loop of the source
has an entry, every case crosses, no case is too large) and tests/test_gpu_launch_slices.py.  No GPU, no oracle and no library
here: the constants are read from the sources, never copied.

A case counts in the loop's own units (items, rows, outputs): `total` of them, `step` per launch, `wg` per workgroup; `items_step`
is the step in items of the output, the period with which a dropped offset repeats."""
import os
import re
from dataclasses import dataclass, field
from typing import Callable, Optional

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spf_amd", "csrc")
DISTINCT = 7                    # distinct items a batch repeats; must divide no launch size
HOST_LIMIT = 300 * 10 ** 6      # bytes of the largest host array of a case
HBM_LIMIT = 4 << 30             # bytes on the device, scratch included

# the two contexts, as plain numbers (tests/test_gpu_launch_slices.py holds them to K.SMALL16 and O.DEFAULT_128)
CONTEXTS = {"small16": dict(N=16, k=1, lwe_n=5, cbs_count=3), "default128": dict(N=2048, k=1, lwe_n=637, cbs_count=4)}


def words(ctx: str, kind: str) -> int:
    c = CONTEXTS[ctx]
    return {"lwe0": c["lwe_n"] + 1, "lwe1": c["k"] * c["N"] + 1, "glwe": (c["k"] + 1) * c["N"],
            "ggsw": (c["k"] + 1) * c["cbs_count"] * (c["k"] + 1) * c["N"]}[kind]


def source(name: str = "spf_hip.hip") -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern: str, text: str, what: str, places: int = 1) -> int:
    """the number `pattern` captures, stated in `places` places of the text that agree"""
    found = re.findall(pattern, text)
    assert len(found) == places and len(set(found)) == 1, f"{what}: matches {found} of {pattern!r}"
    return int(found[0])


def constants() -> dict:
    """the limits the launch loops are written in, parsed out of the sources"""
    hip, pfks, lin, ker = source(), source("spf_pfks.hpp"), source("spf_lwe_linear.hpp"), source("spf_kernels.hpp")
    C = {
        "kMaxGridRows": _one(r"constexpr size_t kMaxGridRows = (\d+);", hip, "kMaxGridRows"),
        "kPfksDigitCap": 1 << _one(r"constexpr size_t kPfksDigitCap = \(size_t\)1 << (\d+);", hip, "kPfksDigitCap"),
        "kLweLinearImageCap": 1 << _one(r"constexpr size_t kLweLinearImageCap = \(size_t\)1 << (\d+);", hip, "kLweLinearImageCap"),
        "PFKS_TILE": _one(r"constexpr int PFKS_TILE = (\d+);", pfks, "PFKS_TILE"),
        "PFKS_VT": _one(r"constexpr int PFKS_VT = (\d+);", pfks, "PFKS_VT"),
        "LWE_LINEAR_VT": _one(r"constexpr int LWE_LINEAR_VT = (\d+);", lin, "LWE_LINEAR_VT"),
        "KS_CT": _one(r"constexpr int KS_CT = (\d+);", ker, "KS_CT"),
        "KSG_TILE": _one(r"constexpr int KSG_TILE = (\d+);", ker, "KSG_TILE"),
        # the literals: grid.y / grid.z of the linear maps, the outputs of one launch of the tuned public functional keyswitch and
        # the bytes of digits it may hold, the polynomials of one launch of a key transform
        "lin_items": _one(r"for \(size_t at = 0; at < B; at \+= (\d+)\) \{", hip, "items per launch of lwe_linear_valu_kernel"),
        "lin_rows": _one(r"const size_t rows_step = \(size_t\)(\d+) \* LWE_LINEAR_VT;", hip, "row groups per launch"),
        "lin_per": _one(r"per = std::min\(\{per, B, \(size_t\)(\d+),", hip, "items per launch of the matrix-core path"),
        # (launch_pufks_tuned, and launch_pufks_rows where it counts the launches of a graph level)
        "pufks_outputs": _one(r"size_t chunk = std::max<size_t>\(4, std::min<size_t>\((\d+), \(\(\(size_t\)\d+ << 30\) / per_output\)", hip,
                              "outputs per launch of the tuned public functional keyswitch", 2),
        "pufks_digit_bytes": _one(r"std::min<size_t>\(\d+, \(\(\(size_t\)(\d+) << 30\) / per_output\)", hip, "GiB of digits per launch", 2) << 30,
        "fft_polys": 1 << _one(r"step = \(size_t\)1 << (\d+); // \(a grid dimension holds", hip, "polynomials per key-transform launch"),
        "grid_y": _one(r"grid\.y is limited to (\d+),", hip, "the grid.y limit the source states"),
    }
    return C


# ---- the loops of the source ------------------------------------------------------------------------------------------------

LOOP = re.compile(r"^\s*for \(size_t (at|m0) = 0; \1 < [^;]+; \1 \+= (.+)\) \{\s*$")
FUNCTION = re.compile(r"^(?:static )?spf_status (\w+)\(")


def loops_in_source() -> list:
    """(function, loop variable, step expression, n-th such loop of the function) of every launch loop, in source order"""
    out, fn, seen = [], None, {}
    for line in source().split("\n"):
        m = FUNCTION.match(line)
        if m:
            fn = m.group(1)
        m = LOOP.match(line)
        if m:
            key = (fn, m.group(1), m.group(2))
            seen[key] = seen.get(key, -1) + 1
            out.append(key + (seen[key],))
    return out


def any_launch_loop_lines() -> int:
    """every line that steps `at` or `m0` at all, whatever its shape: LOOP must have understood each of them"""
    return len(re.findall(r"\b(?:at|m0) \+= ", source()))


# ---- cases ------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Plan:
    total: int                  # units the loop runs over
    step: int                   # units per launch
    wg: Optional[int]           # units one workgroup takes; None: the formula leaves no room for more than one
    items_step: int             # output items (or rows compared one by one) of a full launch
    host_bytes: int             # the largest host array
    hbm_bytes: int              # device buffers and scratch together

    @property
    def launches(self) -> int:
        return -(-self.total // self.step)

    @property
    def last(self) -> int:
        return self.total - (self.launches - 1) * self.step


@dataclass(frozen=True)
class Case:
    id: str
    ctx: str
    count: int                  # the batch, as a literal: items (rows for the gather; output rows M for the `m0` loop)
    shape: dict
    formula: Callable           # (constants, count) -> Plan
    test: str = "tests/test_gpu_launch_slices.py"
    # a case of a test older than this table, run on the array that test builds: its bytes are reported, not bounded
    older: bool = False

    def plan(self, C) -> Plan:
        return self.formula(C, self.count)


@dataclass(frozen=True)
class Entry:
    function: str
    var: Optional[str]          # None: the function has no loop (launch_keyswitch puts the whole batch into one grid)
    step_text: Optional[str]
    nth: int
    kernels: tuple
    limit: str
    cases: tuple = ()
    unreachable: str = ""       # why no case can exist
    guards: dict = field(default_factory=dict)   # terms of the step that never bind, and why


S, T = "small16", "default128"
GW, L1, L0 = words(S, "glwe"), words(S, "lwe1"), words(S, "lwe0")
# The batches are literals, worked out from the formulas at today's limits: a limit that changes leaves them where they are, and
# tests/test_launch_slice_cases.py fails for every case that no longer crosses.
B_ROWS = 32768 + 3              # one launch of kMaxGridRows grid rows and three more
B_GATHER = 32768 + 5
B_OLDER = 33000                 # tests/test_gpu_keyless_ops.py::test_batches_beyond_one_grid_slice
B_PUFKS_TUNED = 4096 + 1        # tests/test_gpu_public_functional_keyswitch.py, "two_launches"
B_COMPONENTS = 32768 // 3 + 3   # whole items of L = 3 rows: 10 922 per launch
M_PFKS_GEMM = 131072 + 128 + 1  # 2^30 bytes of limbs / 8192 a row, then one full row tile and one row
B_LIN_GRID = 65535 + 3
M_LIN_ROWS = 65535 * 8 + 3
B_LIN_CAP = 1643 + 2            # 2^30 bytes of planes / (8 * 638 * 128) an item
B_KEYSWITCH = 65535 * 32 + 1


def _rows(w_in, w_out, n_in=1):
    """one grid row per item of `w_in` words in (n_in operands) and `w_out` out, kMaxGridRows per launch"""
    def formula(C, B):
        step = C["kMaxGridRows"]
        return Plan(B, step, 1, step, B * max(w_in, w_out) * 8, B * (n_in * w_in + w_out) * 8)
    return formula


def _gather(w):
    def formula(C, rows):
        return Plan(rows, C["kMaxGridRows"], 1, C["kMaxGridRows"], rows * w * 8, rows * (w + w + 1) * 8)
    return formula


# public functional keyswitch, generic: key n = 2, 2 digits of 4 bits, p = 1
PUFKS = dict(n=2, log=4, count=2, p=1)
# tuned, tests/test_gpu_public_functional_keyswitch.py::test_both_sides_of_every_dispatcher_boundary[two_launches-*]
PUFKS_TUNED = dict(n=5, log=4, p=65)


def _pufks_tuned(count):
    def formula(C, B):
        n, p = PUFKS_TUNED["n"], PUFKS_TUNED["p"]
        pstride = (p + 31) & ~31
        per_output = n * pstride * 4
        chunk = max(4, min(C["pufks_outputs"], (C["pufks_digit_bytes"] // per_output) & ~3))
        chunk = min(chunk, (B + 3) & ~3)
        gw = words(T, "glwe")
        return Plan(B, chunk, 4, chunk, B * gw * 8, B * (p * (n + 1) + gw) * 8 + chunk * per_output + n * count * gw * 8)
    return formula


# private functional keyswitch: the VALU kernel (24-bit digits: no limbs), and one-bit digits on the matrix cores past the cap
PFKS_VALU = dict(log=24, count=2, p=1, n=4)
PFKS_COMPONENTS = dict(log=24, count=2, p=1, n=CONTEXTS[S]["k"] * CONTEXTS[S]["N"])     # the GGSW components need n = k N
PFKS_GEMM = dict(log=1, count=63, p=1, n=129)
# circuit bootstrap via PFKS with keys on the matrix cores: launch_pfks is one launch there, only the extract loop slices
CBS_KEYS = dict(log=4, count=3, p=1, n=CONTEXTS[S]["k"] * CONTEXTS[S]["N"])


def pfks_limbs(log: int) -> int:
    """spf_pfks.hpp: one limb up to 8 bits, ceil((log + 1) / 8) up to 23, none from 24"""
    return 0 if log >= 24 else 1 if log <= 8 else -(-(log + 1) // 8)


def pfks_chunk(C, key, rows_per_item, M):
    """launch_pfks: rows per launch of the matrix-core path -> (chunk, whether the grid.y clamp bound it, Kpad, limbs)"""
    K = key["p"] * (key["n"] + 1) * key["count"]
    Kpad, U = (K + 127) & ~127, pfks_limbs(key["log"])
    unit = C["PFKS_TILE"] * rows_per_item
    chunk = max(1, C["kPfksDigitCap"] // (Kpad * U) // unit) * unit
    clamped = chunk > C["kMaxGridRows"] * C["PFKS_TILE"]
    if clamped:
        chunk = max(1, C["kMaxGridRows"] * C["PFKS_TILE"] // unit) * unit
    return min(chunk, -(-M // C["PFKS_TILE"]) * C["PFKS_TILE"]), clamped, Kpad, U


def _pfks_valu(key, rows_per_item):
    def formula(C, items):
        assert pfks_limbs(key["log"]) == 0
        step = C["kMaxGridRows"] // rows_per_item * rows_per_item
        rw = key["p"] * (key["n"] + 1)
        n_keys = 1 if rows_per_item == 1 else CONTEXTS[S]["k"] + 1
        out_w = GW if rows_per_item == 1 else words(S, "ggsw")
        return Plan(items * rows_per_item, step, C["PFKS_VT"], step // rows_per_item, items * max(rows_per_item * rw, out_w) * 8,
                    items * (rows_per_item * rw + out_w) * 8 + n_keys * rw * key["count"] * GW * 8)
    return formula


def _pfks_gemm(C, M):
    key = PFKS_GEMM
    rw = key["p"] * (key["n"] + 1)
    chunk, clamped, Kpad, U = pfks_chunk(C, key, 1, M)
    assert U == 1 and not clamped
    K = rw * key["count"]
    return Plan(M, chunk, C["PFKS_TILE"], chunk, M * rw * 8, M * (rw + GW) * 8 + chunk * Kpad * U + 2 * K * GW * 8 + 8 * GW * Kpad)


def _cbs(C, B):
    L = CONTEXTS[S]["cbs_count"]
    step = C["kMaxGridRows"] // L * L
    chunk, _, Kpad, U = pfks_chunk(C, CBS_KEYS, L, B * L)
    assert U and chunk >= B * L, "launch_pfks must be ONE launch here: only the extract loop is under test"
    ggsw = words(S, "ggsw")
    return Plan(B * L, step, 1, step // L, B * ggsw * 8, B * (L0 + GW + L * L1 + ggsw) * 8 + chunk * Kpad * U)


# linear maps
LIN_ITEMS = dict(M=2, K=2, kind="lwe0")
LIN_ROWS = dict(K=1, B=2, kind="lwe0")
LIN_CAP = dict(M=2, K=3, kind="lwe0")       # on default128; see the entry below for why not lwe1
LIN_GRID = dict(M=1, K=2, kind="lwe0")


def _lin_items(C, B):
    W, s = L0, LIN_ITEMS
    return Plan(B, C["lin_items"], 1, C["lin_items"], B * max(s["M"], s["K"]) * W * 8, B * (s["M"] + s["K"]) * W * 8)


def _lin_rows(C, M):
    W, s = L0, LIN_ROWS
    step = C["lin_rows"] * C["LWE_LINEAR_VT"]
    return Plan(M, step, C["LWE_LINEAR_VT"], step, s["B"] * M * W * 8, s["B"] * (M + s["K"]) * W * 8 + M * (s["K"] + 1) * 8)


def lin_per(C, W, K, B):
    """spf_lwe_linear_enqueue: items per launch of the matrix-core path -> (per, its cap term, its grid term, its index term)"""
    Kpad = (K + 127) & ~127
    cap = max(1, C["kLweLinearImageCap"] // (8 * W * Kpad))
    index = max(1, (1 << 28) // W)
    return min(cap, B, C["lin_per"], index), cap, C["lin_per"], index


def _lin_mfma(ctx, s):
    def formula(C, B):
        W = words(ctx, s["kind"])
        per = lin_per(C, W, s["K"], B)[0]
        Kpad = (s["K"] + 127) & ~127
        planes = -(-8 * per * W // C["PFKS_TILE"]) * C["PFKS_TILE"] * Kpad
        return Plan(B, per, 1, per, B * max(s["M"], s["K"]) * W * 8, B * (s["M"] + s["K"]) * W * 8 + planes)
    return formula


def _keyswitch(C, B):
    step = C["grid_y"] * C["KS_CT"]
    return Plan(B, step, C["KS_CT"], step, B * L1 * 8, B * (L1 + L0) * 8)


KEYLESS = "tests/test_gpu_keyless_ops.py::test_batches_beyond_one_grid_slice"
PUFKS_TEST = "tests/test_gpu_public_functional_keyswitch.py::test_both_sides_of_every_dispatcher_boundary[two_launches-%d]"
ENTRIES = [
    Entry("spf_sample_extract_l1_dev", "at", "kMaxGridRows", 0, ("generic_sample_extract_kernel",), "kMaxGridRows grid rows",
          (Case("generic_sample_extract", S, B_ROWS, dict(idx=5), _rows(GW, L1)),)),
    Entry("spf_sample_extract_l1_dev", "at", "kMaxGridRows", 1, ("sample_extract_kernel",), "kMaxGridRows grid rows",
          (Case("tuned_sample_extract", T, B_OLDER, dict(idx=5), _rows(words(T, "glwe"), words(T, "lwe1")), KEYLESS, older=True),)),
    Entry("glwe_linear_dev", "at", "kMaxGridRows", 0, ("generic_linear_kernel",), "kMaxGridRows grid rows",
          (Case("generic_not", S, B_ROWS, dict(op="not"), _rows(GW, GW)),
           Case("generic_xor", S, B_ROWS, dict(op="xor"), _rows(GW, GW, 2)),
           Case("generic_mul_xn", S, B_ROWS, dict(op="mul_xn", n=CONTEXTS[S]["N"] + 5), _rows(GW, GW)))),
    Entry("glwe_linear_dev", "at", "kMaxGridRows", 1, ("glwe_linear_kernel<NOT>", "glwe_linear_kernel<XOR>", "glwe_linear_kernel<MUL_XN>"),
          "kMaxGridRows grid rows",
          (Case("tuned_not_xor_mul_xn", T, B_OLDER, dict(n=CONTEXTS[T]["N"] + 5), _rows(words(T, "glwe"), words(T, "glwe"), 2), KEYLESS,
                older=True),)),
    Entry("spf_gather_rows_dev", "at", "kMaxGridRows", 0, ("gather_rows_kernel",), "kMaxGridRows grid rows",
          (Case("gather_rows", S, B_GATHER, dict(words=3), _gather(3)),)),
    Entry("spf_load_public_functional_keyswitch_key_std", "at", "step", 0, ("poly_fft kernels",), "2^30 polynomials (a grid dimension)",
          unreachable="a second launch needs more than 2^30 polynomials of the key; at the smallest degree the library admits, N = 16, "
                      "that is 2^30 * 16 words * 8 bytes = 137 GB of key on the host and again on the device"),
    Entry("launch_pufks_tuned", "at", "chunk", 0, ("pufks_digits_kernel", "pufks_kernel<4,8,4>", "pufks_kernel<4,4,4>"),
          "4096 outputs, or 8 GiB of digits",
          (Case("tuned_pufks_8", T, B_PUFKS_TUNED, dict(PUFKS_TUNED, count=8), _pufks_tuned(8), PUFKS_TEST % 8, older=True),
           Case("tuned_pufks_4", T, B_PUFKS_TUNED, dict(PUFKS_TUNED, count=4), _pufks_tuned(4), PUFKS_TEST % 4, older=True))),
    Entry("spf_public_functional_keyswitch_enqueue", "at", "kMaxGridRows", 0, ("generic_pufks_kernel",), "kMaxGridRows workgroups",
          (Case("generic_pufks", S, B_ROWS, PUFKS, _rows(PUFKS["p"] * (PUFKS["n"] + 1), GW)),)),
    Entry("launch_pfks", "at", "step", 0, ("pfks_valu_kernel",), "kMaxGridRows rows, in whole items",
          (Case("pfks_valu_single", S, B_ROWS, PFKS_VALU, _pfks_valu(PFKS_VALU, 1)),
           Case("pfks_valu_components", S, B_COMPONENTS, PFKS_COMPONENTS, _pfks_valu(PFKS_COMPONENTS, CONTEXTS[S]["cbs_count"])))),
    Entry("launch_pfks", "at", "chunk", 0, ("pfks_digits_kernel", "pfks_rowsum_kernel", "pfks_gemm_kernel<1>"), "kPfksDigitCap bytes of limbs",
          (Case("pfks_gemm_cap", S, M_PFKS_GEMM, PFKS_GEMM, _pfks_gemm),),
          guards={"kMaxGridRows * PFKS_TILE": "the clamp binds only where a row has 128 limb bytes (Kpad * U = 128), and then a second launch "
                  "needs more than kMaxGridRows * PFKS_TILE = 4 194 304 rows: with the smallest GLWE the library admits (32 words) the "
                  "output alone is 4 194 305 * 32 * 8 bytes = 1.07 GB, past the bound on a host array of this table"}),
    Entry("spf_circuit_bootstrap_via_pfks_enqueue", "at", "kMaxGridRows / L * L", 0, ("pfks_extract_rotate_kernel",),
          "kMaxGridRows rows, in whole items", (Case("cbs_via_pfks_extract", S, B_COMPONENTS, CBS_KEYS, _cbs),)),
    Entry("spf_lwe_linear_enqueue", "at", "65535", 0, ("lwe_linear_valu_kernel",), "65535 items (grid.z)",
          (Case("lin_valu_items", S, B_LIN_GRID, LIN_ITEMS, _lin_items),)),
    Entry("spf_lwe_linear_enqueue", "m0", "rows_step", 0, ("lwe_linear_valu_kernel",), "65535 row groups of LWE_LINEAR_VT (grid.y)",
          (Case("lin_valu_rows", S, M_LIN_ROWS, LIN_ROWS, _lin_rows),)),
    # The cap case runs on level-0 ciphertexts (638 words: 1643 items per launch), not on level-1 ones: 8 * 2049 * 128 bytes per item
    # give 511 = 7 * 73 items per launch, and in a batch that repeats seven items a second launch that read the first
    # launch's inputs would find the same words there.
    Entry("spf_lwe_linear_enqueue", "at", "per", 0, ("lwe_linear_planes_kernel", "pfks_gemm_kernel<2>", "lwe_linear_bias_kernel"),
          "kLweLinearImageCap bytes of planes, or 65535 items (grid.z of the planes pass)",
          (Case("lin_mfma_cap", T, B_LIN_CAP, LIN_CAP, _lin_mfma(T, LIN_CAP)),
           Case("lin_mfma_grid", S, B_LIN_GRID, LIN_GRID, _lin_mfma(S, LIN_GRID))),
          guards={"((size_t)1 << 28) / W": "never the smallest term: an item's planes are 8 * W * Kpad >= 1024 W bytes, so the cap term is at "
                  "most kLweLinearImageCap / (1024 W) = 2^20 / W, 256 times below 2^28 / W, for every W"}),
    Entry("launch_keyswitch", None, None, 0, ("keyswitch_kernel",), "none in the code: ceil(B / KS_CT) goes into grid.y as it is",
          (Case("keyswitch_grid_y", S, B_KEYSWITCH, dict(), _keyswitch),)),
]
CASES = [c for e in ENTRIES for c in e.cases]
BY_ID = {c.id: c for c in CASES}
NEW_CASES = [c for c in CASES if not c.older]
