#!/usr/bin/env python3
"""The GLWE keyswitch, one automorphism round and the homomorphic trace as gate-graph nodes (spf_graph_add_glwe_keyswitch /
_automorphism / _trace), on DEFAULT_128 with synthetic keys and uniform inputs (fixed seeds: timing only; the words are tested in
tests/test_gpu_glwe_keyswitch_graph.py).  Two tables, one JSON line.  Forms alternate in one process on one build: one warm-up run
of each, then `repeats` timed runs per form; median (min - max); two forms are level when each median lies inside the other's
min - max.

rows: the rows kernels (operands through the pointer table) against the in-place kernels on the same GLWEs, by device events around
  the launch (spf_last_kernel_ms "glwe_keyswitch"): B nodes of one mode over B input GLWEs in order (consecutive: in place) and in
  reverse order (not consecutive: the rows kernel, the same rows), B = 256 and 4096, the three modes.
chain: public functional keyswitch of 8 level-0 LWEs -> X^-j (a 1 x 1 polynomial slot) -> trace -> SampleExtract(0) -> keyswitch ->
  one univariate table, as
  g  ONE gate graph: the GLWE never leaves the arena;
  c  today's route without the node: a graph up to X^-j, its GLWE fetched, spf_glwe_trace_enqueue on a device buffer, the result
     fed into a second graph (sample extract, keyswitch, table).
  Both take the same inputs from host memory and leave the same LWE there; a run ends in a device synchronise, so the host clock
  around it is the time of the whole run.

usage: python tools/glwe_keyswitch_graph_bench.py [repeats]      (default 7; at least 5)"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (device memory for the synthetic keys only)

import spf_amd  # noqa: E402
from spf_amd import FheCircuit, FheOp, ValueKind  # noqa: E402

repeats = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
P = spf_amd.DEFAULT_128
N = P.polynomial_degree
BATCHES = (256, 4096)
KS_SLOT, POLY_SLOT, WIDTH, SHIFT, BITS = 2, 4, 8, 3, 3
GLWE = ValueKind.GLWE1


class _DevArray:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def synthetic_keys(eng, rng):
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev)
    g0.manual_seed(1)
    for which in range(3):       # bootstrap key (spectra), keyswitch key (words), automorphism key (spectra)
        ptr, nbytes = eng.key_blob(which)
        t = torch.as_tensor(_DevArray(ptr, nbytes), device=dev)
        if which == 1:
            t.copy_(torch.randint(-(2 ** 63), 2 ** 63 - 1, (nbytes // 8,), generator=g0, device=dev, dtype=torch.int64).view(torch.uint8))
        else:
            t.copy_((torch.randn(nbytes // 8, generator=g0, device=dev, dtype=torch.float64) * 2.0 ** 67).view(torch.uint8))
        torch.cuda.synchronize()
        eng.key_blob_commit(which)
    count = 4                    # public functional keyswitch key from the level-0 dimension: uniform words
    key = rng.integers(0, 1 << 64, (P.lwe_dimension, count, P.glwe_size + 1, N), dtype=np.uint64)
    eng.load_public_functional_keyswitch_key_std(key, 4, count)
    lg, cnt = P.tr_radix_log, P.tr_radix_count                       # a GLWE keyswitch key at the trace radix: the tuned kernel
    eng.load_glwe_keyswitch_key_std(KS_SLOT, rng.integers(0, 1 << 64, (P.glwe_size, cnt, P.glwe_size + 1, N), dtype=np.uint64), lg, cnt)
    # X^-SHIFT = -X^(N - SHIFT), 1 x 1
    eng.load_glwe_poly_weights(POLY_SLOT, (np.array([0, 1], dtype=np.uint32), np.array([N - SHIFT], dtype=np.uint32), np.array([-1], dtype=np.int64)),
                               shape=(1, 1))


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def level(a, b) -> bool:
    """each median lies inside the other's min - max"""
    return b["min_ms"] <= a["median_ms"] <= b["max_ms"] and a["min_ms"] <= b["median_ms"] <= a["max_ms"]


def add_node(g, mode, node):
    if mode == "keyswitch":
        return g.add_glwe_keyswitch(KS_SLOT, node)
    if mode == "automorphism":
        return g.add_glwe_automorphism(2, node)
    return g.add_glwe_trace(node)


def rows(eng, x, mode):
    B = len(x)
    forms = {}
    for form in ("in_place", "rows_kernel"):
        g = FheCircuit(eng)
        ins = [g.add_input(GLWE, v) for v in x]
        nodes = [add_node(g, mode, n) for n in (ins if form == "in_place" else ins[::-1])]
        forms[form] = (g, [g.add_output(nodes[0], GLWE), g.add_output(nodes[-1], GLWE)])
    eng.set_timing(True)
    ms, names, words = {f: [] for f in forms}, {}, {}
    try:
        for f, (g, outs) in forms.items():     # warm-up: plans the graph
            g.run()
            names[f] = eng.last_glwe_keyswitch_kernel()
            words[f] = np.stack(outs)
            eng.last_kernel_ms("glwe_keyswitch")
        for _ in range(repeats):
            for f, (g, _) in forms.items():
                g.run()
                t, n = eng.last_kernel_ms("glwe_keyswitch")
                assert n == 1, n
                ms[f].append(t)
    finally:
        eng.set_timing(False)
        for g, _ in forms.values():
            g.close()
    a, b = summary(ms["in_place"]), summary(ms["rows_kernel"])
    # (the rows form runs over the inputs in reverse: its first node is the in-place form's last)
    return {"mode": mode, "B": B, "in_place": {**a, "kernel": names["in_place"]}, "rows_kernel": {**b, "kernel": names["rows_kernel"]},
            "rows_over_in_place": round(b["median_ms"] / a["median_ms"], 3), "level": level(a, b),
            "outputs_equal": bool(np.array_equal(words["in_place"], words["rows_kernel"][::-1]) and words["in_place"].any())}


def tail(g, traced, table):
    low = g.add_op(FheOp.KeyswitchL1toL0, [g.add_op(FheOp.SampleExtract, [traced], 0)])
    return g.add_output(g.add_op(FheOp.PBS_UNIVARIATE, [low, table]), ValueKind.LWE1)


def head(g, x):
    packed = g.add_public_functional_keyswitch([g.add_input(ValueKind.LWE0, row) for row in x])
    return g.add_glwe_poly_linear(POLY_SLOT, [packed], 1)[0]


def one_graph(eng, x, table):
    g = FheCircuit(eng)
    t = g.add_input(GLWE, table)
    return g, tail(g, g.add_glwe_trace(head(g, x)), t)


class Route:
    """graph, fetch, spf_glwe_trace_enqueue on a device buffer, second graph"""

    def __init__(self, eng, x, table):
        self.eng = eng
        self.g1 = FheCircuit(eng)
        self.shifted = self.g1.add_output(head(self.g1, x), GLWE)
        self.traced = np.zeros(P.glwe_words, dtype=np.uint64)
        self.d_in, self.d_out = eng.device_alloc(P.glwe_words * 8), eng.device_alloc(P.glwe_words * 8)
        self.g2 = FheCircuit(eng)
        t = self.g2.add_input(GLWE, table)
        self.out = tail(self.g2, self.g2.add_input(GLWE, self.traced), t)

    def run(self):
        self.g1.run()
        self.eng.device_upload(self.d_in, self.shifted)
        self.eng.glwe_trace_enqueue(None, 1, self.d_in, self.d_out)
        self.eng.device_download(None, self.traced, self.d_out)
        self.g2.run()

    def close(self):
        self.g1.close()
        self.g2.close()
        self.eng.device_free(self.d_in)
        self.eng.device_free(self.d_out)


def chain(eng, rng):
    x = rng.integers(0, 1 << 64, size=(WIDTH, P.lwe0_words), dtype=np.uint64)
    table = spf_amd.generate_lut([lambda v: (3 * v + 1) % 8], BITS)
    g, out = one_graph(eng, x, table)
    c = Route(eng, x, table)
    g.run()
    c.run()
    ms = {"g": [], "c": []}
    for _ in range(repeats):
        for f, run in (("g", g.run), ("c", c.run)):
            t0 = time.perf_counter()
            run()
            ms[f].append((time.perf_counter() - t0) * 1e3)
    st = g.stats()
    one, route = summary(ms["g"]), summary(ms["c"])
    row = {"lwes": WIDTH, "shift": SHIFT, "one_graph": {**one, "levels": st["levels"], "launches": st["launches"]},
           "route": {**route, "graphs": 2, "enqueue_calls": 1}, "one_graph_over_route": round(one["median_ms"] / route["median_ms"], 3),
           "level": level(one, route), "outputs_equal": bool(np.array_equal(out, c.out) and out.any())}
    g.close()
    c.close()
    return row


def main():
    eng = spf_amd.Engine(P, device=0)
    rng = np.random.default_rng(33)
    synthetic_keys(eng, rng)
    table_rows = []
    for B in BATCHES:
        x = rng.integers(0, 1 << 64, size=(B, P.glwe_words), dtype=np.uint64)
        table_rows += [rows(eng, x, mode) for mode in ("keyswitch", "automorphism", "trace")]
    print(json.dumps({"tool": "glwe_keyswitch_graph_bench", "repeats": repeats, "library": spf_amd.lib_path(), "rows": table_rows,
                      "chain": [chain(eng, rng)]}))
    eng.close()


if __name__ == "__main__":
    main()
