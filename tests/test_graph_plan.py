"""The planner of the gate graphs (spf_amd/csrc/spf_graph_plan.hpp: levels, groups and their order, arena offsets, in place or
through a pointer row, the order of the CMUX units, the stage size) on the CPU.  tests/cpp/graph_plan.cpp is a stand-alone program
built from the HIP-free header alone with the system g++ and AddressSanitizer + UndefinedBehaviorSanitizer, and run as a child
process (nothing is loaded into python).  It takes a `RecordedCircuit` as a file of numbers, builds the graph through the header,
plans it, checks every invariant of the plan by brute force and prints the plan.  The plan is then held to
  * the Python model: `circuit_model.planned_levels`, `graph_fuzz_cases.groups_of` sorted by its packed key (the independent
    statement of the group order), and the offsets that follow from the two alignment rules;
  * the executor as it was before the planner moved into the header: tests/golden/graph_plans.json holds a SHA-256 of the
    complete plan of eight circuits, recorded from that executor's plan();
  * itself: planning the append of two graphs is planning their concatenation."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, RecordedCircuit, TableOp, ValueKind
from spf_amd import graph as G
from tests import arena_cases
from tests import graph_fuzz_cases as F
from tests.blind_rotation_graph_cases import SMALL16, TEST1
from tests.circuit_model import planned_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_plans.json")
TUNED = O.DEFAULT_128.replace(lwe_n=12)         # the tuned context of the graph tests (pbs_graph_cases.keys_of)
L0, L1, GL, GG, GV = ValueKind.LWE0, ValueKind.LWE1, ValueKind.GLWE1, ValueKind.GGSW1, ValueKind.GLEV1
CMUX_FAMILY = {int(FheOp.CMux), int(FheOp.GlevCMux), int(FheOp.MultiplyGgswGlwe), G.NODE_ROT_CMUX}
TABLE_OPS = {int(op) for op in list(FheOp) + list(TableOp)} - CMUX_FAMILY      # read their operands as rows, slot by slot
ARITY = {int(FheOp.GlweAdd): 2, int(TableOp.PBS_UNIVARIATE): 2, int(TableOp.PBS_BIVARIATE): 3}     # (of TABLE_OPS; else 1)
NODE_KINDS = {int(op) for op in list(FheOp) + list(TableOp)} | {v for k, v in vars(G).items() if k.startswith("NODE_")} | {-1, -2}
# ... as it was when the golden plans were recorded (the executor before the planner moved knew these): written out, so that the
# golden test keeps every member whatever spf_amd.graph names
GOLDEN_NODE_KINDS = set(range(12)) | {64, 65, 66, 67, 68} | {-1, -2}
GLWE_KS_KINDS = (G.NODE_GLWE_KEYSWITCH, G.NODE_GLWE_AUTOMORPHISM, G.NODE_GLWE_TRACE)


def sizes_of(P):
    """(bytes of a value of each kind, cbs_radix_count) of an oracle parameter set or of an engine's"""
    if hasattr(P, "lwe_n"):
        return [8 * F.words_of(P, k) for k in ValueKind], P.cbs_count
    return [arena_cases.value_bytes(P, k) for k in ValueKind], P.cbs_radix_count


def write_circuit(path, rec, sizes, radix, pufks_stage):
    with open(path, "w") as f:
        f.write("sizes " + " ".join(map(str, sizes)) + f" {radix} {int(pufks_stage)}\nnodes {len(rec.op)}\n")
        for i, op in enumerate(rec.op):
            width = rec._unpack_width[i] if op == G.NODE_UNPACK else 0
            slot, rows = rec.linear_of(i) if op in (G.NODE_LWE_LINEAR, G.NODE_GLWE_POLY_LINEAR) else (0, 0)
            ins = rec.inputs[i]
            f.write(f"{op} {rec.kind[i]} {rec.param[i] if op not in (G.NODE_PACK, G.NODE_PUFKS) else 0} {width} {slot} {rows} {len(ins)} "
                    + " ".join(map(str, ins)) + "\n")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("graph_plan") / "graph_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "graph_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout and r.stdout.rstrip().endswith("graph_plan ok"), r.stdout[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout[:r.stdout.rstrip().rfind("\n") + 1]     # the plan, without the last line


def digest(plan_text) -> str:
    """SHA-256 of the printed plan without its member lists (their count is in the group's line)"""
    kept = [line for line in plan_text.splitlines() if not line.startswith("members")]
    return hashlib.sha256(("\n".join(kept) + "\n").encode()).hexdigest()


def parse(plan_text) -> dict:
    plan = {"groups": []}
    for line in plan_text.splitlines():
        w = line.split()
        if w[0] in ("levels", "offsets", "table"):
            plan[w[0]] = [int(x) for x in w[2:]]
            assert len(plan[w[0]]) == int(w[1])
        elif w[0] == "group":
            level, op, kind, slot, rows, n = (int(x) for x in w[1:7])
            access = [int(x) for x in w[11:20]]
            plan["groups"].append({"level": level, "op": op, "kind": kind, "slot": slot, "rows": rows, "n": n, "count": int(w[8]),
                                   "out_off": int(w[9]), "contiguous": access[0::3], "one_lut": int(w[21])})
        elif w[0] == "members":
            plan["groups"][-1]["members"] = [int(x) for x in w[1:]]
        elif w[0] == "sizes":
            plan["inputs_bytes"], plan["arena_bytes"], plan["stage_bytes"], plan["n_levels"] = (int(x) for x in w[1:])
    return plan


def packed_key(g):
    """a printed group's key as `graph_fuzz_cases.group_key` packs it"""
    if g["op"] == G.NODE_PUFKS:
        return g["level"], g["op"], g["n"] | g["kind"] << 32
    if g["op"] in (G.NODE_LWE_LINEAR, G.NODE_GLWE_POLY_LINEAR):
        return g["level"], g["op"], g["n"] | g["rows"] << 32 | g["slot"] << 48 | g["kind"] << 56
    return g["level"], g["op"], g["n"]


def model_plan(rec, sizes):
    """levels, [(packed key, members)] in group order, offsets, inputs_bytes, arena_bytes: inputs and constants first, each on 256
    bytes; then one block per group on 256 bytes, rows in member order"""
    up = lambda v: -(-v // 256) * 256
    levels = planned_levels(rec)
    groups = sorted(F.groups_of(rec, levels).items())
    offsets, off = [0] * len(rec.op), 0
    for i, op in enumerate(rec.op):
        if op < 0:
            offsets[i] = off
            off = up(off + sizes[rec.kind[i]])
    inputs_bytes = off
    for _, members in groups:
        for r, i in enumerate(members):
            offsets[i] = off + r * sizes[rec.kind[i]]
        off = up(off + len(members) * sizes[rec.kind[members[0]]])
    return levels, groups, offsets, inputs_bytes, off


def both_ways(P, scattered) -> RecordedCircuit:
    """every operation that reads its operands as rows, in pairs: over two successive rows of one group in their order (read in
    place; the bootstraps by table with one table for both), or in the opposite order (each slot through a pointer row)"""
    rec = RecordedCircuit(P.N)
    nothing = np.zeros(1, dtype=np.uint64)      # (a plan looks at no value)
    g = [rec.add_input(GL, nothing) for _ in range(2)]
    l1 = [rec.add_input(L1, nothing) for _ in range(4)]
    v = [rec.add_input(GV, nothing) for _ in range(2)]
    sel = rec.add_input(GG, nothing)
    pick = lambda rows: [rows[1], rows[0]] if scattered else [rows[0], rows[1]]
    nots = [rec.add_op(FheOp.Not, [x]) for x in g]
    se = [rec.add_op(FheOp.SampleExtract, [x], 3) for x in pick(nots)]
    ks = [rec.add_op(FheOp.KeyswitchL1toL0, [x]) for x in pick(se)]
    out = [rec.add_op(FheOp.CircuitBootstrap, [x]) for x in pick(ks)]
    out += [rec.add_op(FheOp.Not, [x]) for x in pick(nots)] + [rec.add_op(FheOp.MulXN, [x], 5) for x in pick(nots)]
    out += [rec.add_op(FheOp.GlweAdd, [x, y]) for x, y in zip(pick(nots), pick(nots))]
    glev = [rec.add_op(FheOp.GlevCMux, [sel, v[0], v[1]]), rec.add_op(FheOp.GlevCMux, [sel, v[1], v[0]])]
    out += [rec.add_op(FheOp.SchemeSwitch, [x]) for x in pick(glev)]
    rows = [rec.add_op(FheOp.KeyswitchL1toL0, [x]) for x in l1]
    tables = pick(nots) if scattered else [nots[0], nots[0]]
    out += [rec.add_op(TableOp.PBS_UNIVARIATE, [x, t]) for x, t in zip(pick(rows[:2]), tables)]
    out += [rec.add_op(TableOp.PBS_BIVARIATE, [x, y, t], 2) for x, y, t in zip(pick(rows[:2]), pick(rows[2:]), tables)]
    # the polynomial linear map (layers of two rows over two operands) and the GLWE keyswitch family, a pair of each
    out += rec.add_glwe_poly_linear(7, pick(nots), 2)
    out += [rec.add_glwe_keyswitch(3, x) for x in pick(nots)] + [rec.add_glwe_automorphism(2, x) for x in pick(nots)]
    out += [rec.add_glwe_trace(x) for x in pick(nots)]
    for n in out:
        rec.add_output(n, ValueKind(rec.kind[n]))
    return rec


def concatenation(a, b) -> RecordedCircuit:
    """the circuit recorded as `a`, then `b` with its node ids behind a's"""
    rec, base = RecordedCircuit(a.polynomial_degree), len(a.op)
    for src, shift in ((a, 0), (b, base)):
        for i in range(len(src.op)):
            rec._add(src.op[i], src.kind[i], src.param[i], [j + shift for j in src.inputs[i]], src.host[i])
        rec._unpack_width.update({i + shift: w for i, w in src._unpack_width.items()})
        rec._linear.update({i + shift: x for i, x in src._linear.items()})
        rec.outputs += [o + shift for o in src.outputs]
    return rec


# the circuits whose plans are held to the executor before the planner moved: name -> (circuit, parameter set, pufks_stage).
# Between them every node kind that executor knew; the drawn ones with public functional keyswitch operands of both kinds and
# without such nodes, and without the GLWE section the generator has learned since (`glwe=False`: the circuits as recorded)
GOLDEN_CASES = {
    "add32": lambda: (arena_cases.record("add32"), spf_amd.DEFAULT_128, False),
    "mul8": lambda: (arena_cases.record("mul8"), spf_amd.DEFAULT_128, False),
    "full_0_tuned_lwe0": lambda: (F.draw_circuit(0, TUNED, "full", L0, glwe=False)[0], TUNED, False),
    "full_1_tuned_lwe1_gathered": lambda: (F.draw_circuit(1, TUNED, "full", L1, glwe=False)[0], TUNED, True),
    "full_2_n128k2_lwe0": lambda: (F.draw_circuit(2, TEST1, "full", L0, glwe=False)[0], TEST1, True),
    "pushable_3_n128k2": lambda: (F.draw_circuit(3, TEST1, "pushable", glwe=False)[0], TEST1, True),
    "small_4_n16k1_lwe1": lambda: (F.draw_circuit(4, SMALL16, "small", L1, glwe=False)[0], SMALL16, True),
    "small_5_tuned_lwe0": lambda: (F.draw_circuit(5, TUNED, "small", L0, glwe=False)[0], TUNED, False),
}


def other_cases():
    """60 drawn circuits (20 seeds of each profile, over the three parameter sets, both operand kinds of the public functional
    keyswitch, both pufks_stage values, every third with a linear seed of its own; all with the polynomial linear maps and the GLWE
    keyswitch family), the two hand-made ones, mul32"""
    for seed in range(100, 120):
        for at, profile in enumerate(F.PROFILES):
            P = (TUNED, TEST1, SMALL16)[(seed + at) % 3]
            kind = None if profile == "pushable" else (L0, L1)[(seed // 3) % 2]
            yield (f"{profile}_{seed}", lambda seed=seed, P=P, profile=profile, kind=kind:
                   (F.draw_circuit(seed, P, profile, kind, linear_seed=7 if seed % 3 == 0 else None, glwe=True)[0], P, bool(seed & 1)))
    yield "in_place", lambda: (both_ways(TEST1, False), TEST1, True)
    yield "scattered", lambda: (both_ways(TEST1, True), TEST1, False)
    yield "mul32", lambda: (arena_cases.record("mul32"), spf_amd.DEFAULT_128, False)


def plan_of(program, tmp_path, name, make):
    rec, P, stage = make()
    sizes, radix = sizes_of(P)
    path = str(tmp_path / f"{name}.circuit")
    write_circuit(path, rec, sizes, radix, stage)
    return rec, sizes, stage, run([program, path])


@pytest.fixture(scope="module")
def plans(program, tmp_path_factory):
    """name -> (circuit, sizes, pufks_stage, printed plan) of every case, each planned (and checked by the program) once"""
    tmp = tmp_path_factory.mktemp("circuits")
    cases = list(GOLDEN_CASES.items()) + list(other_cases())
    return {name: plan_of(program, tmp, name, make) for name, make in cases}


def test_every_plan_equals_the_python_model(plans):
    assert sum(name.split("_")[0] in F.PROFILES for name in plans) >= 60 and {"add32", "mul8", "mul32"} <= set(plans)
    for name, (rec, sizes, _, text) in plans.items():
        got = parse(text)
        levels, groups, offsets, inputs_bytes, arena_bytes = model_plan(rec, sizes)
        assert got["levels"] == levels, name
        assert [(packed_key(g), g["members"]) for g in got["groups"]] == groups, name
        assert all(g["count"] == len(g["members"]) for g in got["groups"]), name
        assert got["offsets"] == offsets, name
        assert (got["inputs_bytes"], got["arena_bytes"], got["n_levels"]) == (inputs_bytes, arena_bytes, max(levels)), name


def test_the_cases_reach_every_node_kind_and_both_ways_of_reading_every_operand(plans):
    kinds, stages, ways = set(), set(), {}
    pufks_kinds, linear_seen = set(), False
    for name, (rec, _, stage, text) in plans.items():
        kinds |= set(rec.op)
        if G.NODE_PUFKS in rec.op:
            stages.add(stage)
            pufks_kinds |= {rec.kind[rec.inputs[i][0]] for i, op in enumerate(rec.op) if op == G.NODE_PUFKS}
        for g in parse(text)["groups"]:
            listed = (G.NODE_UNPACK, G.NODE_PUFKS, G.NODE_LWE_LINEAR, G.NODE_GLWE_POLY_LINEAR) + GLWE_KS_KINDS
            slots = ARITY.get(g["op"], 1) if g["op"] in TABLE_OPS else 1 if g["op"] in listed else 0
            for s in range(slots):
                ways.setdefault((g["op"], s), set()).add(bool(g["contiguous"][s]))
    assert kinds == NODE_KINDS, NODE_KINDS ^ kinds
    assert stages == {False, True} and pufks_kinds == {int(L0), int(L1)}
    want = {(op, s) for op in TABLE_OPS for s in range(ARITY.get(op, 1))} | {(op, 0) for op in (G.NODE_UNPACK, G.NODE_PUFKS, G.NODE_LWE_LINEAR)}
    want |= {(69, 0), (70, 0), (71, 0), (72, 0)}
    assert {69, 70, 71, 72} <= NODE_KINDS and NODE_KINDS == GOLDEN_NODE_KINDS | {69, 70, 71, 72}
    assert set(ways) == want, set(ways) ^ want
    assert all(w == {False, True} for w in ways.values()), {k: w for k, w in ways.items() if w != {False, True}}


def test_golden_plans_are_those_of_the_executor_before_the_planner_moved(plans):
    golden = json.load(open(GOLDEN))
    assert set(golden) == set(GOLDEN_CASES) and len(golden) == 8
    kinds = set()
    for name, want in golden.items():
        rec, _, _, text = plans[name]
        kinds |= set(rec.op)
        got = parse(text)
        numbers = {k: got[k] for k in ("inputs_bytes", "arena_bytes", "stage_bytes", "n_levels")}
        assert numbers == {k: want[k] for k in numbers}, name
        assert digest(text) == want["sha256"], name
    assert kinds == GOLDEN_NODE_KINDS, GOLDEN_NODE_KINDS ^ kinds


def test_planning_an_append_is_planning_the_concatenation(program, tmp_path):
    """circuits with pack, public functional keyswitch and linear nodes, so that the positions in the side list move too"""
    a, b = F.draw_circuit(31, TEST1, "small", L0)[0], F.draw_circuit(32, TEST1, "full", L0)[0]
    for rec in (a, b):
        assert {G.NODE_PACK, G.NODE_PUFKS, G.NODE_LWE_LINEAR, G.NODE_UNPACK, G.NODE_ROT_CMUX, G.NODE_GLWE_POLY_LINEAR, *GLWE_KS_KINDS} <= set(rec.op)
    sizes, radix = sizes_of(TEST1)
    paths = {}
    for name, rec in (("a", a), ("b", b), ("ab", concatenation(a, b)), ("ba", concatenation(b, a))):
        paths[name] = str(tmp_path / f"{name}.circuit")
        write_circuit(paths[name], rec, sizes, radix, True)
    assert run([program, "--append", paths["a"], paths["b"]]) == run([program, paths["ab"]])
    assert run([program, "--append", paths["b"], paths["a"]]) == run([program, paths["ba"]])
    assert run([program, paths["ab"]]) != run([program, paths["ba"]])
