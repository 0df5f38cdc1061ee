"""The launch-slice table (tests/launch_slice_cases.py) against the sources, without a GPU: every loop that cuts a call into
several launches has exactly one entry, every case goes past the first launch with a ragged last one under the limits as the
sources state them today, and no case is too large.  A loop added without an entry, or a cap changed so that a case falls back
into one launch, fails here."""
import os
import re

import pytest

from tests import launch_slice_cases as LS

C = LS.constants()


def test_the_constants_are_the_sources():
    print(C)
    assert C["kMaxGridRows"] <= C["grid_y"] == C["lin_items"] == C["lin_rows"] == C["lin_per"]
    assert C["kMaxGridRows"] % LS.DISTINCT and C["grid_y"] % LS.DISTINCT
    for name in ("PFKS_TILE", "PFKS_VT", "LWE_LINEAR_VT", "KS_CT", "KSG_TILE"):
        assert C[name] > 1 and C[name] & (C[name] - 1) == 0, name


def test_every_launch_loop_of_the_source_belongs_to_exactly_one_entry():
    found = LS.loops_in_source()
    print("\n".join(map(str, found)))
    assert len(found) == LS.any_launch_loop_lines(), "a line steps `at` or `m0` in a form the table's pattern does not read"
    assert len(found) >= 14 and len(set(found)) == len(found)
    claimed = [(e.function, e.var, e.step_text, e.nth) for e in LS.ENTRIES if e.var is not None]
    assert len(set(claimed)) == len(claimed), "two entries claim one loop"
    missing = [f for f in found if f not in claimed]
    assert not missing, f"launch loops without an entry (tests/launch_slice_cases.py): {missing}"
    gone = [c for c in claimed if c not in found]
    assert not gone, f"entries for loops the source does not have: {gone}"
    # an entry without a loop stands for a function that has none: the day it gets one, the entry has to name it
    with_loops = {f[0] for f in found}
    src = LS.source()
    for e in LS.ENTRIES:
        if e.var is None:
            assert e.function not in with_loops, e.function
            assert re.search(r"^spf_status " + e.function + r"\(", src, re.M), e.function


def test_every_entry_has_a_case_or_a_written_reason():
    ids = [c.id for c in LS.CASES]
    assert len(set(ids)) == len(ids)
    unreachable = [e for e in LS.ENTRIES if not e.cases]
    for e in LS.ENTRIES:
        assert e.kernels and e.limit.strip()
        assert bool(e.cases) != bool(e.unreachable.strip()), (e.function, e.step_text)
        assert all(isinstance(r, str) and len(r) > 40 for r in e.guards.values())
    # three terms may be listed as out of reach: the key transform's loop, the grid.y clamp of the GEMM, the index term of `per`
    assert [e.function for e in unreachable] == ["spf_load_public_functional_keyswitch_key_std"]
    assert sorted(g for e in LS.ENTRIES for g in e.guards) == ["((size_t)1 << 28) / W", "kMaxGridRows * PFKS_TILE"]
    for e in LS.ENTRIES:
        for g in e.guards:
            assert g in LS.source(), f"the guard term `{g}` is no longer in the source"
    assert {c.test.split("::")[0] for c in LS.CASES} == {"tests/test_gpu_launch_slices.py", "tests/test_gpu_keyless_ops.py",
                                                         "tests/test_gpu_public_functional_keyswitch.py"}


def test_the_unreachable_arithmetic():
    # the key transform: 2^30 polynomials of at least 16 words
    assert C["fft_polys"] * 16 * 8 > 137 * 10 ** 9
    # the clamp of launch_pfks binds for 128 limb bytes a row only, and then a launch holds kMaxGridRows * PFKS_TILE rows
    for Kpad_U, binds in ((128, True), (256, False), (384, False)):
        chunk = C["kPfksDigitCap"] // Kpad_U // C["PFKS_TILE"] * C["PFKS_TILE"]
        assert (chunk > C["kMaxGridRows"] * C["PFKS_TILE"]) == binds
    rows = C["kMaxGridRows"] * C["PFKS_TILE"]
    assert rows == 4194304 and (rows + 1) * 32 * 8 > LS.HOST_LIMIT
    # the index term of `per` is 256 times the largest value the cap term can take, whatever W
    for W in (2, 6, 17, 638, 2049, 4097, 16385):
        per, cap, grid, index = LS.lin_per(C, W, 1, 1 << 40)
        assert cap <= (1 << 20) // W < index and per == min(cap, grid)


@pytest.mark.parametrize("case", LS.CASES, ids=lambda c: c.id)
def test_the_case_crosses_its_limit_with_a_ragged_last_launch(case):
    p = case.plan(C)
    print(case.id, p, "launches", p.launches, "last", p.last)
    assert p.launches >= 2, "the case fits one launch"
    assert 0 < p.last < p.step, "the last launch is full or empty"
    if p.wg is not None:
        assert p.step > p.wg, "the first launch is one workgroup"
    assert p.items_step % LS.DISTINCT, f"{LS.DISTINCT} distinct items repeat with the launch size: a dropped offset reads the same words"


@pytest.mark.parametrize("case", LS.CASES, ids=lambda c: c.id)
def test_the_case_is_small_enough(case):
    p = case.plan(C)
    print(f"{case.id}: host {p.host_bytes / 1e6:.1f} MB, HBM {p.hbm_bytes / 1e6:.1f} MB")
    assert p.hbm_bytes <= LS.HBM_LIMIT
    if not case.older:
        assert p.host_bytes <= LS.HOST_LIMIT


def test_the_older_tests_still_have_the_shapes_the_table_gives_them():
    """three entries are served by tests older than the table: their batches are read out of those tests' text"""
    tests = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(tests, "test_gpu_keyless_ops.py")) as f:
        keyless = f.read().split("def test_batches_beyond_one_grid_slice")[1]
    assert re.search(r"\n    B, h = (\d+), 5\n", keyless).group(1) == str(LS.B_OLDER)
    for op in ("sample_extract_l1", "glwe_not", "glwe_xor", "glwe_mul_xn"):
        assert f"eng.{op}(glwe" in keyless, op
    with open(os.path.join(tests, "test_gpu_public_functional_keyswitch.py")) as f:
        pufks = f.read()
    assert re.search(r"\nPER_LAUNCH = (\d+) ", pufks).group(1) == str(C["pufks_outputs"])
    body = pufks.split("def test_both_sides_of_every_dispatcher_boundary")[1].split("\ndef ")[0]
    assert '"two_launches": (PER_LAUNCH + 1, 4)' in body and LS.B_PUFKS_TUNED == C["pufks_outputs"] + 1
    assert f'n, p = {LS.PUFKS_TUNED["n"]}, {LS.PUFKS_TUNED["p"]}\n' in body


def test_the_literal_batches_are_what_the_formulas_give_today():
    """each batch of the table is a literal; here is where each comes from.  A limit that changes fails this test and, for every
    case that then fits one launch, the crossing test above: the GPU case cannot quietly fall back into one launch."""
    L = LS.CONTEXTS["small16"]["cbs_count"]
    assert LS.B_ROWS == C["kMaxGridRows"] + 3 and LS.B_GATHER == C["kMaxGridRows"] + 5
    assert LS.B_COMPONENTS == C["kMaxGridRows"] // L * L // L + 3
    first = LS.pfks_chunk(C, LS.PFKS_GEMM, 1, 1 << 40)
    assert first[0] == C["kPfksDigitCap"] // 8192 and first[2] == 8192 and LS.M_PFKS_GEMM == first[0] + C["PFKS_TILE"] + 1
    assert LS.B_LIN_GRID == C["lin_items"] + 3 == C["lin_per"] + 3
    assert LS.M_LIN_ROWS == C["lin_rows"] * C["LWE_LINEAR_VT"] + 3
    assert LS.B_LIN_CAP == C["kLweLinearImageCap"] // (8 * LS.words("default128", "lwe0") * 128) + 2
    assert LS.lin_per(C, LS.words("small16", "lwe0"), 2, 1 << 40)[:3] == (C["lin_per"], 174762, C["lin_per"])
    assert LS.B_KEYSWITCH == C["grid_y"] * C["KS_CT"] + 1
