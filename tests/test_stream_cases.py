"""The stream-contract case table (tests/stream_cases.py) against the header, without a GPU: every `_dev` prototype of
include/spf_hip.h has a case or a stated reason to have none, every decoy differs from the real operand it stands in for, and
every pointer table, real or decoy, points into operands the case owns."""
import os
import re

import numpy as np
import pytest

from tests import stream_cases as SC

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spf_hip.h")
RESOLVED = [c.resolve() for c in SC.CASES]


def dev_prototypes():
    with open(HEADER) as f:
        return sorted(set(re.findall(r"\b(spf_\w+_dev)\s*\(", f.read())))


def test_every_dev_prototype_has_a_stream_case_or_a_reason():
    protos = dev_prototypes()
    print("\n".join(protos))
    assert len(protos) >= 22 and {"spf_poly_fft_dev", "spf_blind_rotation_dev", "spf_gather_rows_dev"} <= set(protos), protos
    covered = {c.entry for c in SC.CASES}
    assert covered.isdisjoint(SC.EXCLUDED), "excluded and covered at once"
    missing = [p for p in protos if p not in covered and p not in SC.EXCLUDED]
    assert not missing, f"`_dev` entry points without a stream case (tests/stream_cases.py): {missing}"
    unknown = sorted((covered | set(SC.EXCLUDED)) - set(protos))
    assert not unknown, f"cases or exclusions for symbols the header does not declare: {unknown}"
    assert all(isinstance(r, str) and r.strip() for r in SC.EXCLUDED.values())


def test_the_binding_declares_every_entry_point_of_the_table():
    from spf_amd._ffi import SYMBOLS
    argc = {name: len(args) for name, _, args in SYMBOLS}
    for r in RESOLVED:
        ptrs = {o.name: 0x1000 for o in r.operands}
        assert len(r.args(ptrs)) + 2 == argc[r.case.entry], r.id   # (ctx, stream) first


def test_the_table_has_the_cases_the_contract_names():
    ids = set(SC.BY_ID)
    assert len(ids) == len(SC.CASES)
    for ctx in ("T", "T16", "G"):
        assert any(c.ctx == ctx and c.entry == "spf_keyswitch_lwe_l1_lwe_l0_dev" for c in SC.CASES)
    for shape in SC.PBS_SHAPES:   # each blind-rotation shape through each of the three bootstraps, both log_v through the generalized one
        for entry in ("spf_generalized_pbs_dev", "spf_pbs_univariate_dev", "spf_circuit_bootstrap_pbs_dev"):
            assert any(c.B == shape and c.entry == entry for c in SC.CASES), (shape, entry)
        assert {f"generalized_pbs-T-{shape}-logv0", f"generalized_pbs-T-{shape}-logv2"} <= {i.rsplit("-", 1)[0] for i in ids}
    reported = {k for c in SC.CASES for _, k in c.kernels}
    for name in ("cmux4_kernel<4,4>", "cmux_kernel<4,4,2>", "cmux_kernel<4,4,2,stream>", "cmux4_kernel<4,4,rot>",
                 "cmux_kernel<4,4,2,rot>", "cmux_kernel<4,4,2,stream,rot>", "generic_cmux_kernel", "generic_pbs_kernel",
                 "ks_gemm_lds_kernel", "keyswitch_kernel"):
        assert re.escape(name) in reported or name in reported, name
    for case_id, first, second in SC.MULTI_STEP:
        assert case_id in ids and 0 < first < second, case_id
    assert {SC.BY_ID[i].entry for i, _, _ in SC.MULTI_STEP} == {
        "spf_circuit_bootstrap_dev", "spf_unpack_circuit_bootstrap_dev", "spf_pbs_bivariate_dev", "spf_blind_rotation_dev",
        "spf_keyswitch_lwe_l1_lwe_l0_dev"}


@pytest.mark.parametrize("r", RESOLVED, ids=lambda r: r.id)
def test_decoys_differ_and_tables_stay_inside_the_case(r):
    assert r.output.role in ("out", "inout") and r.inputs
    names = [o.name for o in r.operands]
    assert len(set(names)) == len(names)
    # operands: every decoy row differs from the real row it replaces (the first rows, the tile seam and the last row)
    for op in r.operands:
        if op.role == "table" or op.role == "out":
            continue
        assert op.rows > 0 and op.row_words > 0
        for first, rows in ((0, min(op.rows, SC._TILE + 2)), (op.rows - 1, 1)):
            real, decoy = SC.operand_data(r.id, op, "real", first, rows), SC.operand_data(r.id, op, "decoy", first, rows)
            assert real.shape == decoy.shape == (rows, op.row_words) and real.dtype == np.uint64
            assert (real != decoy).any(axis=1).all(), op.name
            if op.kind == "doubles":
                for x in (real.view(np.float64), decoy.view(np.float64)):
                    assert np.isfinite(x).all() and 2.0 ** 40 < np.abs(x).mean() < 2.0 ** 70, op.name
        whole = SC.operand_data(r.id, op, "real", 0, min(op.rows, 40))
        assert np.array_equal(whole[-1:], SC.operand_data(r.id, op, "real", whole.shape[0] - 1, 1))   # a slice is the same rows
        assert len({row.tobytes() for row in whole}) == whole.shape[0], "rows of one operand repeat"
    # pointer tables over two disjoint sets of buffers: the working buffers and the decoy operands
    at, work, decoys = 1 << 20, {}, {}
    for base in (work, decoys):
        for op in r.operands:
            if op.role != "table":
                base[op.name] = at
                at += op.nbytes + 4096
    by_name = {o.name: o for o in r.operands}
    for op in r.operands:
        if op.role != "table":
            continue
        assert op.entries and all(e is None or e[0] in by_name for e in op.entries), "a pointer to an operand of another case"
        real, decoy = SC.table_pointers(r, op, work), SC.table_pointers(r, op, decoys)
        assert real.shape == decoy.shape == (len(op.entries),)
        for e, pr, pd in zip(op.entries, real, decoy):
            if e is None:
                assert pr == 0 and pd == 0
                continue
            target = by_name[e[0]]
            assert 0 <= e[1] < target.rows
            for p, base in ((int(pr), work), (int(pd), decoys)):
                assert base[e[0]] <= p and p + 8 * target.row_words <= base[e[0]] + target.nbytes, (op.name, e)
            assert pr != pd
        written = [e for e in op.entries if e is not None and by_name[e[0]].role == "out"]
        assert len(set(written)) == len(written), "two units write one row"
