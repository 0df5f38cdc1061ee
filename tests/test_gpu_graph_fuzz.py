"""Randomised differential tests of gate graphs with every node kind mixed (r23): circuits of tests/graph_fuzz_cases.py, lowered
into a gate graph, pushed node by node through the pool by handle, run as jobs of a device group, and drawn on random parameter
sets.  Since r29 the plaintext linear maps are among the node kinds: their weight slots (`graph_fuzz_cases.draw_linear_slots`)
are loaded before a circuit is lowered and handed to the model with the keys.  Since r37 the plaintext polynomial linear maps over
GLWEs and the GLWE keyswitch, automorphism round and trace are among them too: their polynomial weight slots and keyswitch-key slots
(`draw_glwe_poly_slots`, `draw_glwe_ksk_slots`) are loaded the same way; the automorphism key is the context's own.  The only expectation is
`circuit_model.evaluate`, the oracle walking the same circuit on the CPU; the only comparison is `same_words`.  The default
suite runs a few circuits per context; `SPF_FUZZ_CASES=N` (and `SPF_FUZZ_SEED`) turn it into a soak and `SPF_FUZZ_REPORT=path`
collects one JSON line per circuit — profiles/r23_graph_fuzz.md records the r23 run, profiles/r29_graph_fuzz_linear.md the one
with linear nodes, profiles/r37_graph_fuzz_glwe.md the one with the polynomial and GLWE keyswitch nodes."""
import gc
import json
import os

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from spf_amd.graph import (NODE_GLWE_AUTOMORPHISM, NODE_GLWE_KEYSWITCH, NODE_GLWE_POLY_LINEAR, NODE_GLWE_TRACE, NODE_LWE_LINEAR, NODE_PACK,
                           NODE_PUFKS, NODE_ROT_CMUX, NODE_UNPACK)
from tests import circuit_model as M
from tests import glwe_keyswitch_graph_cases as GKG
from tests import glwe_poly_cases as GC
from tests import graph_fuzz_cases as F
from tests import lwe_linear_cases as LC
from tests import pbs_graph_cases as K
from tests.util import to_engine_params

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("SPF_FUZZ_CASES", str(F.DEFAULT_CASES)))
SEED = int(os.environ.get("SPF_FUZZ_SEED", str(F.DEFAULT_SEED)))
_CONVERSIONS = (int(FheOp.SampleExtract), int(FheOp.KeyswitchL1toL0), int(FheOp.CircuitBootstrap), NODE_UNPACK)
_GLWE_NAMES = {"GlwePolyLinear": "poly_linear", "GlweKeyswitch": "keyswitch", "GlweAutomorphism": "automorphism", "GlweTrace": "trace"}
# the submits by handle of the GLWE keyswitch family (the nodes keep the kinds of their constructors, the pool takes the FheOp values)
_PUSH_OP = {NODE_GLWE_KEYSWITCH: FheOp.GLWE_KEYSWITCH, NODE_GLWE_AUTOMORPHISM: FheOp.GLWE_AUTOMORPHISM, NODE_GLWE_TRACE: FheOp.GLWE_TRACE}


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(which):
        if which not in made:
            made[which] = K.make_engine(which)
        return K.keys_of(which)[0], made[which]

    yield get
    for e in made.values():
        e.close()


def report(test, which, facts, **more):
    path = os.environ.get("SPF_FUZZ_REPORT")
    if path:
        line = {"test": test, "context": which, "seed": facts["seed"], "profile": facts["profile"], "nodes": facts["nodes"],
                "groups": facts["groups"], "levels": facts["levels"], "pufks_kind": None if facts["pufks_kind"] is None else facts["pufks_kind"].name,
                "linear_nodes": facts["nodes"].get("LweLinear", 0), "linear_groups": facts["groups"].get("LweLinear", 0),
                "glwe_nodes": {short: facts["nodes"].get(name, 0) for name, short in _GLWE_NAMES.items()},
                "glwe_groups": {short: facts["groups"].get(name, 0) for name, short in _GLWE_NAMES.items()}}
        line.update(more)
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def check(rec, got, want, tag):
    """every output against the model; the message names the seed, the case and the lowest differing output node"""
    message = M.first_difference(rec, got, want)
    assert message is None, f"{tag}: {message}"


def load_linear_slots(eng, slots):
    """every weight slot of the table into an engine or a group: before lower() (a graph may also be built first; run() checks)"""
    for slot, (w, b) in slots.items():
        eng.load_lwe_linear_weights(slot, w, b)
    return slots


def load_glwe_slots(eng, ksk, poly):
    """every keyswitch-key slot and every polynomial weight slot of the two tables (`poly` None: a circuit without polynomial
    layers) into an engine or a group, before lower(); -> (ksk, poly) as the model takes them"""
    for slot, (words, lg, cnt) in ksk.items():
        eng.load_glwe_keyswitch_key_std(slot, words, lg, cnt)
    for slot, (triple, bias, shape) in (poly or {}).items():
        eng.load_glwe_poly_weights(slot, triple, bias, shape=shape)
    return ksk, poly


def glwe_group_keys(rec):
    """plan()'s keys of the polynomial linear groups (level, 69, K | M << 32 | slot << 48 | kind << 56) and of the GLWE keyswitch,
    automorphism and trace groups (level, kind, parameter) of a circuit run alone"""
    levels = M.planned_levels(rec)
    poly = {F.group_key(rec, levels, i) for i, op in enumerate(rec.op) if op == NODE_GLWE_POLY_LINEAR}
    return poly, {F.group_key(rec, levels, i) for i, op in enumerate(rec.op) if op in F.GLWE_KS_KINDS}


def pufks_key_of(which, case, P, kind):
    """(key words, log, count): the tuned context draws its radix per case; the key's dimension is the operand kind's"""
    if which == "tuned":
        # (cases 0, 1, 2 take the three radices in turn; a soak shifts the turn by one every three cases, so that the case that
        # changes the key between its runs starts under each radix)
        log, count = (4, 4) if kind == ValueKind.LWE1 else F.PUFKS_RADICES[(case + case // 3) % 3]
    else:
        log, count = 4, 3
    return K.pufks_key(P.N, P.k, K.dimension(P, kind), count, seed=log), log, count


@pytest.mark.parametrize("which", K.CONTEXTS)
def test_random_graphs_of_every_node_kind_equal_the_oracle(rigs, which, monkeypatch):
    """profile `full` lowered into one gate graph; run, the inputs refilled and run again; on the tuned context every third case
    then loads a key of the other radix family and runs a third time (the keyswitch nodes' rows are planned again).  One case in
    three loads other weights of the same shapes into every slot between its first and second run — the polynomial weight slots and
    the GLWE keyswitch-key slots (the same shapes and radices, other contents) with them.  On case 0 the last launch of the GLWE
    keyswitch family is the rows kernel (`glwe_last_keyswitch_group_scattered`: the hand-written one on the tuned context, the generic
    one elsewhere) and the last polynomial launch the in-place LDS kernel (`poly_last_group_in_place_general`); the per-kernel timing
    record does not split the rows kernels from the in-place ones, so the last launches stand for the rest.  Case 0 is then lowered a
    second time with the matrix cores forced on every in-place linear group they can serve: the same words, and the last linear
    launch (in place, one-limb weights: `linear_last_group_in_place_with_one_limb_weights`) is theirs"""
    P, eng = rigs(which)
    monkeypatch.delenv("SPF_LWE_LINEAR_PATH", raising=False)
    for case in range(CASES):
        seed = F.case_seed(SEED, 0, case)
        rec, facts = F.draw_circuit(seed, P, "full", F.tuned_pufks_kind(case) if which == "tuned" else None)
        key = pufks_key_of(which, case, P, facts["pufks_kind"])
        runs = [key, key]
        if which == "tuned" and case % 3 == 0:
            log, count = (5, 3) if key[1:] != (5, 3) else (4, 4)
            runs.append((K.pufks_key(P.N, P.k, key[0].shape[0], count, seed=log), log, count))
        slots = load_linear_slots(eng, facts["linear_slots"])
        ksk, poly = load_glwe_slots(eng, facts["glwe_ksk_slots"], facts["glwe_poly_slots"])
        g, outs = rec.lower(eng)
        launches = []
        try:
            for run, loaded in enumerate(runs):
                tag = f"seed {seed} case {case} ({which}, keyswitch key {loaded[2]}x{loaded[1]} of {facts['pufks_kind'].name}) run {run}"
                if run == 0 or loaded is not runs[run - 1]:
                    eng.load_public_functional_keyswitch_key_std(*loaded)
                if run:
                    F.refill_inputs(rec, P, seed + run)
                if run == 1 and case % 3 == 1:
                    slots = load_linear_slots(eng, F.draw_linear_slots(facts["linear_seed"] + 1))
                    ksk, poly = load_glwe_slots(eng, F.draw_glwe_ksk_slots(facts["glwe_key_seed"] + 1, P), F.draw_glwe_poly_slots(facts["glwe_poly_seed"] + 1, P.N))
                g.run()
                launches.append(g.stats()["launches"])
                want = M.evaluate(rec, P, M.keys_of(which, loaded, slots, ksk, poly))
                check(rec, outs, want, tag)
            assert g.stats()["nodes"] == len(rec.op)
            kernels = [eng.last_lwe_linear_kernel()]
            glwe_kernels = [eng.last_glwe_keyswitch_kernel(), eng.last_glwe_poly_kernel()]
            if case == 0:
                assert {"glwe_last_keyswitch_group_scattered", "poly_last_group_in_place_general"} <= set(facts["patterns"]), tag
                assert glwe_kernels == [GKG.ROWS[which == "tuned"], GC.LDS], (tag, glwe_kernels)
                assert kernels[0] == LC.VALU, tag      # (the cost rule takes the matrix cores from K = 512 on; in place, so not the rows kernel)
                monkeypatch.setenv("SPF_LWE_LINEAR_PATH", "mfma")
                forced, forced_outs = rec.lower(eng)
                try:
                    forced.run()
                    kernels.append(eng.last_lwe_linear_kernel())
                finally:
                    forced.close()
                    monkeypatch.delenv("SPF_LWE_LINEAR_PATH")
                check(rec, forced_outs, want, tag + " lowered again with SPF_LWE_LINEAR_PATH=mfma")
                assert all(K.same_words(a, b) for a, b in zip(forced_outs, outs)), tag
                assert kernels[1] == "pfks_gemm_kernel<1>", (tag, kernels)
            report("lowered", which, facts, launches=launches, outputs=len(outs), linear_kernels=kernels, linear_reloaded=case % 3 == 1,
                   glwe_kernels=glwe_kernels, rounds=sorted({rec.param[i] for i, op in enumerate(rec.op) if op == NODE_GLWE_AUTOMORPHISM}),
                   radix=[list(r[1:]) for r in runs], kernel=eng.last_public_functional_keyswitch_kernel())
        finally:
            g.close()


# ---- the same circuits pushed through the pool by handle --------------------------------------------------------------------

def conversions_first(rec):
    """a second topological order of the operation nodes: whenever a conversion (SampleExtract, unpack bit, KeyswitchL1toL0,
    CircuitBootstrap) is ready it goes before everything else"""
    n = len(rec.op)
    waiting = [len({j for j in rec.inputs[i] if rec.op[j] >= 0}) for i in range(n)]
    users = [[] for _ in range(n)]
    for i in range(n):
        for j in {j for j in rec.inputs[i] if rec.op[j] >= 0}:
            users[j].append(i)
    ready = sorted(i for i in range(n) if rec.op[i] >= 0 and not waiting[i])
    order = []
    while ready:
        at = next((k for k, i in enumerate(ready) if rec.op[i] in _CONVERSIONS), 0)
        i = ready.pop(at)
        order.append(i)
        for u in users[i]:
            waiting[u] -= 1
            if not waiting[u]:
                ready.append(u)
        ready.sort()
    assert len(order) == sum(op >= 0 for op in rec.op)
    return order


def whole_chains(rec):
    """{first step: [steps]} of the blind rotations whose middle steps nobody else reads: pushed as ONE call"""
    used = [0] * len(rec.op)
    for ins in rec.inputs:
        for j in set(ins):
            used[j] += 1
    chains, i = {}, 0
    while i < len(rec.op):
        if rec.op[i] != NODE_ROT_CMUX:
            i += 1
            continue
        run = [i]
        while (run[-1] + 1 < len(rec.op) and rec.op[run[-1] + 1] == NODE_ROT_CMUX and rec.inputs[run[-1] + 1][1] == run[-1]
               and rec.param[run[-1] + 1] == 2 * rec.param[run[-1]]):
            run.append(run[-1] + 1)
        if len(run) > 1 and all(used[m] == 1 and m not in rec.outputs for m in run[:-1]):
            chains[run[0]] = run
        i = run[-1] + 1
    return chains


def push_circuit(pool, rec, order):
    """every node through Pool.push_v / push_blind_rotation_v in `order`, nothing waited for but the outputs.  An unpack bit is a
    SampleExtract with its index, a pack the GlweAdd of MulXN results, a whole rotation one call, a broken one a call per step, a
    GLWE keyswitch, automorphism round or trace node the FheOp value of its mode with its slot or round.
    -> the outputs' arrays; every value is released again"""
    import tools.driver as drv
    vals = drv.upload_circuit_inputs(pool, rec)
    temps, chains, in_chain = [], whole_chains(rec), {}
    try:
        for i in order:
            op, ins, par = rec.op[i], rec.inputs[i], rec.param[i]
            if i in in_chain:
                continue                                   # pushed with the first step of its rotation
            if op == NODE_UNPACK:
                vals[i] = pool.push_v(FheOp.SampleExtract, [vals[ins[0]]], par)
            elif op == NODE_PACK:
                acc = None
                for at, j in enumerate(ins):
                    term = pool.push_v(FheOp.MulXN, [vals[j]], at)
                    temps.append(term)
                    if acc is not None:
                        term = pool.push_v(FheOp.GlweAdd, [acc, term])
                        temps.append(term)
                    acc = term
                vals[i] = temps.pop()
            elif op == NODE_ROT_CMUX:
                run = chains.get(i)
                if run is not None and all(vals[rec.inputs[m][0]] is not None for m in run):
                    last = pool.push_blind_rotation_v(vals[ins[1]], [vals[rec.inputs[m][0]] for m in run], par.bit_length() - 1)
                    for m in run[1:]:
                        in_chain[m] = True
                    vals[run[-1]] = last
                    if len(run) > 1:
                        continue
                vals[i] = pool.push_blind_rotation_v(vals[ins[1]], [vals[ins[0]]], par.bit_length() - 1)
            elif op in _PUSH_OP:
                vals[i] = pool.push_v(_PUSH_OP[op], [vals[ins[0]]], par)
            else:
                assert op not in (NODE_PUFKS, NODE_LWE_LINEAR, NODE_GLWE_POLY_LINEAR), "public functional keyswitch, linear and polynomial linear nodes have no submit by handle"
                vals[i] = pool.push_v(op, [vals[j] for j in ins], par)
        return [vals[node].wait().download() for node in rec.outputs]
    finally:
        for v in temps + vals:
            if v is not None:
                v.release()


@pytest.mark.parametrize("which", K.CONTEXTS)
def test_random_graphs_pushed_by_handle_equal_the_oracle(rigs, which):
    """profile `pushable` through the pool's deferred scheduler, in creation order and with the conversions first, and a third time
    through a second pool with mixed parameters, where the SampleExtract indices, MulXN amounts, keyswitch slots and rounds of one
    level share launches; afterwards the pools hold no value of the case.  The three modes of the GLWE keyswitch family are among
    the pushed nodes (their keyswitch-key slots are the engine's)"""
    P, eng = rigs(which)
    rng = np.random.default_rng(SEED + 1)
    pool = spf_amd.Pool(eng, max_batch=4096, max_wait_us=int(rng.choice((20, 200, 2000))))
    mixed = None
    try:
        mixed = spf_amd.Pool(eng, max_batch=4096, max_wait_us=int(rng.choice((20, 200, 2000))))
        mixed.set_mixed_parameters(True)
        for case in range(CASES):
            seed = F.case_seed(SEED, 1, case)
            rec, facts = F.draw_circuit(seed, P, "pushable")
            assert set(F.GLWE_KS_KINDS) <= set(rec.op) and NODE_GLWE_POLY_LINEAR not in rec.op and facts["glwe_poly_slots"] is None
            ksk, _ = load_glwe_slots(eng, facts["glwe_ksk_slots"], None)
            want = M.evaluate(rec, P, M.keys_of(which, glwe_ksk=ksk))
            whole = whole_chains(rec)
            assert whole and any(op == NODE_ROT_CMUX and i not in {m for r in whole.values() for m in r} for i, op in enumerate(rec.op))
            creation = [i for i, op in enumerate(rec.op) if op >= 0]
            for through, name, order in ((pool, "creation", creation), (pool, "conversions first", conversions_first(rec)),
                                         (mixed, "creation", creation)):
                live = through.value_stats()["live_values"]
                got = push_circuit(through, rec, order)
                check(rec, got, want, f"seed {seed} case {case} ({which}) pushed in {name} order" + (" with mixed parameters" if through is mixed else ""))
                del got
                gc.collect()
                assert through.value_stats()["live_values"] == live, (seed, name, through is mixed)
            report("pushed", which, facts, whole_rotations=len(whole), counters={k: v for k, v in pool.counters().items() if isinstance(v, int)},
                   mixed_counters={k: v for k, v in mixed.counters().items() if isinstance(v, int)})
    finally:
        if mixed is not None:
            mixed.close()
        pool.close()


# ---- jobs of a device group ---------------------------------------------------------------------------------------------------

def linear_group_keys(rec):
    """plan()'s keys (level, kind, K | M << 32 | slot << 48 | operand kind << 56) of the linear groups of a circuit run alone"""
    levels = M.planned_levels(rec)
    return {F.group_key(rec, levels, i) for i, op in enumerate(rec.op) if op == NODE_LWE_LINEAR}


def test_random_graphs_as_group_jobs_equal_the_oracle():
    """four circuits of the (128, 2) context and two of the tuned one as jobs of Group(devices=[0, 0]): a member that is dealt two
    jobs runs them merged into one graph (nodes and pack / keyswitch / linear operand lists renumbered).  All jobs of a group are
    drawn with ONE linear_seed and the group holds one table of weight slots, so layers of two jobs that share a slot and a level
    become one group of the merged graph; likewise ONE seed for the polynomial weight slots and ONE for the keyswitch-key slots, so
    that polynomial layers and keyswitch-family nodes of two jobs become one group too"""
    for round_ in range(max(1, CASES // 3)):
        for which, n_jobs in (("n128k2", 4), ("tuned", 2)):
            P = K.keys_of(which)[0]
            key, log, count = pufks_key_of(which, 1 + round_, P, ValueKind.LWE0)
            seeds = [F.case_seed(SEED, 2, 100 * round_ + 10 * K.CONTEXTS.index(which) + j) for j in range(n_jobs)]
            recs = [F.draw_circuit(s, P, "full", ValueKind.LWE0, linear_seed=seeds[0], glwe_key_seed=seeds[0], glwe_poly_seed=seeds[0]) for s in seeds]
            slots, ksk, poly = (recs[0][1][name] for name in ("linear_slots", "glwe_ksk_slots", "glwe_poly_slots"))
            grp = spf_amd.Group(K.engine_params(P), devices=[0, 0])
            jobs = []
            try:
                K.load_keys(grp, which)
                grp.load_public_functional_keyswitch_key_std(key, log, count)
                load_linear_slots(grp, slots)
                load_glwe_slots(grp, ksk, poly)
                jobs = [rec.lower(grp) for rec, _ in recs]
                grp.run_graphs([g for g, _ in jobs])
                members = [g.member() for g, _ in jobs]
                if n_jobs > 2:
                    assert max(members.count(m) for m in set(members)) >= 2, members       # at least one merge of two
                for m in set(members):      # two circuits dealt to one member: layers of one slot, shape, kind and level in both
                    dealt = [recs[j][0] for j in range(n_jobs) if members[j] == m]
                    assert all(linear_group_keys(a) & linear_group_keys(b) for a, b in zip(dealt, dealt[1:])), (m, members)
                    for a, b in zip(dealt, dealt[1:]):      # ... and polynomial layers and keyswitch-family nodes of one key in both
                        (poly_a, ks_a), (poly_b, ks_b) = glwe_group_keys(a), glwe_group_keys(b)
                        assert poly_a & poly_b and all({key for key in ks_a & ks_b if key[1] == kind} for kind in F.GLWE_KS_KINDS), (m, members)
                for j, ((rec, facts), (g, outs)) in enumerate(zip(recs, jobs)):
                    want = M.evaluate(rec, P, M.keys_of(which, (key, log, count), slots, ksk, poly))
                    check(rec, outs, want, f"seed {seeds[j]} job {j} of {n_jobs} ({which}) on member {members[j]} of {members}")
                    report("group", which, facts, member=members[j], members=members)
            finally:
                for g, _ in jobs:
                    g.close()
                grp.close()


# ---- random parameter sets ------------------------------------------------------------------------------------------------------

def test_random_parameter_sets_with_random_graphs():
    """parameter sets drawn as test_gpu_fuzz.py::test_random_parameter_sets_through_the_generic_family draws them (the same
    bounds), a random radix of the public-functional-keyswitch key, one `small` circuit per set: its two linear layers (nine rows
    over scattered operands, two rows in place) work on rows of 2 words up to kN + 1.  Its polynomial layers (five rows scattered,
    one row in place; the slots drawn for the set's N) and its node of each GLWE keyswitch mode run under the drawn trace radix;
    the other-radix keyswitch-key slot takes a radix drawn with the same bounds"""
    rng = np.random.default_rng(SEED + 3)
    for case in range(max(4, CASES)):
        if rng.random() < 0.2:
            N, k = 2048, 1
        else:
            N, k = int(rng.choice((16, 32, 64, 128, 256, 512, 1024))), int(rng.integers(1, 4))
        if (k + 1) * N > 4096:      # keeps the oracle fast and the polynomials inside one CU's LDS
            k = 1

        def radix(max_bits=40):
            lg = int(rng.integers(1, 17))
            return lg, int(rng.integers(1, max(2, min(8, max_bits // lg) + 1)))
        pl, pc = radix()
        if N == 2048 and (pl, pc) == (16, 2):
            pl, pc = 8, 3
        cl, cc = radix(24)
        cc = min(cc, 7)
        tl, tc = radix()
        sl, sc = radix()
        kl = int(rng.integers(1, 9))
        kc = int(rng.integers(1, max(2, 32 // kl + 1)))
        fl, fc = radix()
        n = int(rng.integers(1, 9))
        # the other-radix keyswitch-key slot: radix()'s bounds, from a generator of its own (the draws above and below stay as they were)
        own = np.random.default_rng([SEED + 3, case, 0x6AA])
        lg = int(own.integers(1, 17))
        other = lg, int(own.integers(1, max(2, min(8, 40 // lg) + 1)))
        if other == (tl, tc):       # (the slot is there for a radix that is not the trace's)
            other = (tl % 16 + 1, 1)
        P = O.DEFAULT_128.replace(lwe_n=n, N=N, k=k, pbs_radix_log=pl, pbs_count=pc, cbs_radix_log=cl, cbs_count=cc,
                                  ks_radix_log=kl, ks_count=kc, tr_radix_log=tl, tr_count=tc, ss_radix_log=sl, ss_count=sc)
        seed = F.case_seed(SEED, 3, case)
        rec, facts = F.draw_circuit(seed, P, "small", glwe_other_radix=other)
        dim = K.dimension(P, facts["pufks_kind"])
        fc = max(1, min(fc, (1 << 23) // (dim * (k + 1) * N)))     # (a key of at most 64 MB: the oracle transforms it row by row)
        tag = (f"seed {seed} case {case}: N={N} k={k} n={n} pbs={pc}x{pl} cbs={cc}x{cl} ks={kc}x{kl} tr={tc}x{tl} ss={sc}x{sl} "
               f"pufks={fc}x{fl} of {facts['pufks_kind'].name} glwe ksk other={other[1]}x{other[0]}")
        ks = O.gen_keyset(int(rng.integers(1 << 30)), P)
        r = O.Rng(int(rng.integers(1 << 30)))
        ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, P), O.gen_ssk_fft(r, ks.glwe_sk, P)
        key = rng.integers(0, 1 << 64, (dim, fc, k + 1, N), dtype=np.uint64)
        EP = to_engine_params(P).replace(tr_radix_log=tl, tr_radix_count=tc, ss_radix_log=sl, ss_radix_count=sc)
        eng = spf_amd.Engine(EP)
        try:
            eng.load_bootstrap_key(ks.bsk_fft)
            eng.load_keyswitch_key(ks.ksk)
            eng.load_automorphism_key(ak)
            eng.load_scheme_switch_key(ssk)
            eng.load_public_functional_keyswitch_key_std(key, fl, fc)
            slots = load_linear_slots(eng, facts["linear_slots"])
            ksk, poly = load_glwe_slots(eng, facts["glwe_ksk_slots"], facts["glwe_poly_slots"])
            assert ksk[F.K_OTHER][1:] == other and ksk[F.K_A][1:] == (tl, tc)
            g, outs = rec.lower(eng)
            try:
                g.run()
                check(rec, outs, M.evaluate(rec, P, M.Keys(ks, ak, ssk, (key, fl, fc), slots, ksk, poly)), tag)
                report("parameter sets", f"N{N}k{k}", facts, launches=[g.stats()["launches"]], tag=tag,
                       glwe_kernels=[eng.last_glwe_keyswitch_kernel(), eng.last_glwe_poly_kernel()])
            finally:
                g.close()
        finally:
            eng.close()
