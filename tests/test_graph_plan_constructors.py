"""The plans of graphs with node constructors (the kinds 64 .. 72 of spf_amd/csrc/spf_graph_plan.hpp), held to the planner as it
was before the kinds were described by one table: tests/golden/graph_plans_constructors.json holds the `digest()` of
tests/test_graph_plan.py of every circuit below under both values of `pufks_stage`, recorded from the header that still spelled
every kind out in `has_list`, `key_of` and `plan_access` (tests/golden/graph_plans.json stops at kind 68).  The circuits:
  * the six drawn circuits of tests/golden/graph_fuzz_circuits.json;
  * the case circuits of tests/glwe_poly_graph_cases.py (`pool_graph` at every scattered shape) and of
    tests/glwe_keyswitch_graph_cases.py (`Scattered` in every mode at every batch of both contexts' shapes), recorded;
  * one hand-made circuit that holds all nine kinds, each over consecutive operands and over scattered ones.
Every plan is also checked by tests/cpp/graph_plan.cpp itself (under the sanitizers) while it is printed.  No circuit and no
digest may be missing on either side."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, RecordedCircuit, ValueKind
from spf_amd import graph as G
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as GKG
from tests import glwe_poly_graph_cases as GPG
from tests.blind_rotation_graph_cases import TEST1
from tests.test_graph_plan import GOLDEN_CASES, ROOT, digest, parse, program, run, sizes_of, write_circuit  # noqa: F401 (program: a fixture)

GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_plans_constructors.json")
FUZZ_CIRCUITS = os.path.join(ROOT, "tests", "golden", "graph_fuzz_circuits.json")
L1, GL, GG = ValueKind.LWE1, ValueKind.GLWE1, ValueKind.GGSW1
CONSTRUCTOR_KINDS = set(range(64, 73))
# the kinds that read rows in place when they lie consecutively; a pack always reads through the table, a rotate-CMUX reads units
IN_PLACE_KINDS = CONSTRUCTOR_KINDS - {G.NODE_PACK, G.NODE_ROT_CMUX}


class _Recorded(RecordedCircuit):
    """a recording in the place of an FheCircuit: add_output gives the node back, where a graph gives the array it fills"""

    def add_output(self, node, kind):
        super().add_output(node, kind)
        return node


def all_nine(P) -> RecordedCircuit:
    """every constructor kind twice on one level, under two keys: once over operands that lie consecutively in their order, once
    over the same rows out of order (with a repeat where the kind takes a list)"""
    rec = RecordedCircuit(P.N)
    nothing = np.zeros(1, dtype=np.uint64)      # (a plan looks at no value)
    g = [rec.add_input(GL, nothing) for _ in range(3)]
    l1 = [rec.add_input(L1, nothing) for _ in range(3)]
    sel = [rec.add_input(GG, nothing) for _ in range(2)]
    n = [rec.add_op(FheOp.Not, [x]) for x in g]                           # three consecutive GLWE rows of one group
    r = [rec.add_op(FheOp.KeyswitchL1toL0, [x]) for x in l1]              # three consecutive LWE0 rows of one group
    out = []
    out += rec.add_unpack(n[0], 2) + rec.add_unpack(n[1], 2) + rec.add_unpack(n[2], 3) + rec.add_unpack(n[0], 3)
    out += [rec.add_pack([n[0], n[1]]), rec.add_pack([n[2], n[0], n[2]])]
    out += [rec.add_blind_rotation(n[0], sel, 0), rec.add_blind_rotation(n[1], sel[::-1], 2)]
    out += [rec.add_public_functional_keyswitch(r[:2]), rec.add_public_functional_keyswitch([r[2], r[0], r[2]] * 40)]   # (more bytes than any unpack gathers)
    out += rec.add_lwe_linear(1, r, 2) + rec.add_lwe_linear(2, [r[1], r[0]], 2)
    out += rec.add_glwe_poly_linear(1, n, 2) + rec.add_glwe_poly_linear(2, [n[1], n[0]], 2)
    ks = [rec.add_glwe_keyswitch(3, x) for x in n]
    out += ks + [rec.add_glwe_keyswitch(4, x) for x in (n[2], n[0])]
    out += [rec.add_glwe_automorphism(1, x) for x in n] + [rec.add_glwe_automorphism(2, x) for x in (n[1], n[0], n[1])]
    out += [rec.add_glwe_trace(x) for x in n] + [rec.add_glwe_trace(x) for x in ks[::-1]]      # (one key: the second group a level up)
    for node in out:
        rec.add_output(node, ValueKind(rec.kind[node]))
    return rec


def cases() -> dict:
    """name -> (circuit, parameter set)"""
    out = {}
    with open(FUZZ_CIRCUITS) as f:
        for name in json.load(f):
            rec, P, _ = GOLDEN_CASES[name]()
            out[f"fuzz_{name}"] = (rec, P)
    with pytest.MonkeyPatch.context() as mp:    # the case modules build on `spf_amd.FheCircuit(engine)`: a recording instead
        for M, K in GPG.SCATTERED_SHAPES:
            mp.setattr(spf_amd, "FheCircuit", lambda eng: _Recorded(TEST1.N))
            out[f"poly_pool_{M}x{K}"] = (GPG.pool_graph(None, TEST1, 3, GPG.LAYERS, K, M, 0xC0)[0], TEST1)
        for shape, batches in GKG.BATCHES.items():
            P = KC.SHAPES[shape]
            c = SimpleNamespace(P=P, x=np.zeros((KC.ITEMS, P.k + 1, P.N), dtype=np.uint64))     # (a case without its keys)
            mp.setattr(spf_amd, "FheCircuit", lambda eng, P=P: _Recorded(P.N))
            for name, kind, param in GKG.modes():
                for B in batches:
                    out[f"ks_{shape}_{name}_{B}"] = (GKG.Scattered(None, c, 0xC1, kind, param, B).g, P)
    out["all_nine"] = (all_nine(TEST1), TEST1)
    return out


def plans_of(exe, tmp) -> dict:
    """name -> {"0" / "1" (pufks_stage): printed plan}, each planned and checked by the program"""
    out = {}
    for name, (rec, P) in cases().items():
        sizes, radix = sizes_of(P)
        out[name] = {}
        for stage in (0, 1):
            path = os.path.join(str(tmp), f"{name}_{stage}.circuit")
            write_circuit(path, rec, sizes, radix, bool(stage))
            out[name][str(stage)] = run([exe, path])
    return out


@pytest.fixture(scope="module")
def plans(program, tmp_path_factory):  # noqa: F811
    return plans_of(program, tmp_path_factory.mktemp("constructor_circuits"))


def test_the_cases_are_the_ones_the_digests_were_recorded_for(plans):
    assert len(plans) == 6 + len(GPG.SCATTERED_SHAPES) + 3 * sum(len(b) for b in GKG.BATCHES.values()) + 1
    assert sum(name.startswith("fuzz_") for name in plans) == 6 and "all_nine" in plans
    kinds = set()
    for rec, _ in cases().values():
        kinds |= set(rec.op)
    assert CONSTRUCTOR_KINDS <= kinds


def test_the_hand_made_circuit_reads_every_kind_both_ways(plans):
    for stage in ("0", "1"):
        ways = {}
        for g in parse(plans["all_nine"][stage])["groups"]:
            ways.setdefault(g["op"], []).append(bool(g["contiguous"][0]))
        assert CONSTRUCTOR_KINDS <= set(ways)
        assert all(sorted(ways[op]) == [False, True] for op in IN_PLACE_KINDS), ways
        assert ways[G.NODE_PACK] == [False, False] and len(ways[G.NODE_ROT_CMUX]) >= 2, ways
    # the gathered rows of the public functional keyswitch are the one thing pufks_stage changes
    assert parse(plans["all_nine"]["0"])["stage_bytes"] < parse(plans["all_nine"]["1"])["stage_bytes"]


def test_every_plan_is_the_one_recorded_before_the_table_of_kinds(plans):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden) == set(plans), set(golden) ^ set(plans)
    for name, by_stage in plans.items():
        assert set(golden[name]) == {"0", "1"}, name
        for stage, text in by_stage.items():
            assert digest(text) == golden[name][stage], (name, stage)
