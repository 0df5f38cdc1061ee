#!/usr/bin/env python3
""""layer -> activation table -> layer -> keyswitch -> activation table" over R level-0 LWEs, two ways, on DEFAULT_128 with
synthetic keys and uniform weights of one int8 limb (a fixed seed: the words are reproducible, the arithmetic is the real one):

    R inputs (lwe0) -> linear map R x R -> univariate table -> linear map R x R (on the level-1 results) -> keyswitch
                    -> univariate table -> R outputs (lwe1)

  g  ONE gate graph (spf_graph_add_lwe_linear between the SPF_OP_PBS_UNIVARIATE nodes): the LWE rows never leave the arena;
  c  today's composition without the node: spf_lwe_linear_batch through host pointers, a graph for the first table, its results
     downloaded, spf_lwe_linear_batch again, the rows uploaded into a second graph (keyswitch + table).
Both forms take the same inputs from host memory and leave the same R LWEs there.  Per R in {16, 64}: one warm-up run of each
form, then `repeats` timed runs per form, alternating; a run ends in a device synchronise, so the host clock around it is the
time of the whole run.  Medians and min - max are reported, and that the two forms gave the same words.

Second part: lwe_linear_rows_kernel (operands through the pointer table) against the in-place path (the batch dispatcher) on the
same rows, by device events around the product (spf_last_kernel_ms "lwe_linear"), alternating: `layers` layers of 64 x 64 over
the 64 LWE1 rows that one add_unpack makes (consecutive: in place), and over the same rows of each layer in reverse order (not
consecutive: the rows kernel).

usage: python tools/lwe_linear_graph_bench.py [repeats]      (default 7; at least 5)
Prints one JSON line."""
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
ROWS = (16, 64)
LAYERS = (1, 16)
BITS = 3
LWE0, LWE1 = 0, 1


class _DevArray:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def synthetic_keys(eng):
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev)
    g0.manual_seed(1)
    for which in range(2):       # bootstrap key (spectra), keyswitch key (words)
        ptr, nbytes = eng.key_blob(which)
        t = torch.as_tensor(_DevArray(ptr, nbytes), device=dev)
        if which == 1:
            t.copy_(torch.randint(-(2 ** 63), 2 ** 63 - 1, (nbytes // 8,), generator=g0, device=dev, dtype=torch.int64).view(torch.uint8))
        else:
            t.copy_((torch.randn(nbytes // 8, generator=g0, device=dev, dtype=torch.float64) * 2.0 ** 67).view(torch.uint8))
        torch.cuda.synchronize()
        eng.key_blob_commit(which)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def one_graph(eng, x, t1, t2, R):
    g = FheCircuit(eng)
    a, b = g.add_input(ValueKind.GLWE1, t1), g.add_input(ValueKind.GLWE1, t2)
    xs = [g.add_input(ValueKind.LWE0, row) for row in x]
    h = [g.add_op(FheOp.PBS_UNIVARIATE, [n, a]) for n in g.add_lwe_linear(0, xs, R)]
    low = [g.add_op(FheOp.KeyswitchL1toL0, [n]) for n in g.add_lwe_linear(1, h, R)]
    return g, [g.add_output(g.add_op(FheOp.PBS_UNIVARIATE, [n, b]), ValueKind.LWE1) for n in low]


class Composition:
    """batch call, graph, download, batch call, upload, second graph"""

    def __init__(self, eng, x, t1, t2, R):
        self.eng, self.x = eng, x
        self.a = np.zeros((R, P.lwe0_words), dtype=np.uint64)
        self.b = np.zeros((R, P.lwe1_words), dtype=np.uint64)
        self.g1 = FheCircuit(eng)
        t = self.g1.add_input(ValueKind.GLWE1, t1)
        self.h = [self.g1.add_output(self.g1.add_op(FheOp.PBS_UNIVARIATE, [self.g1.add_input(ValueKind.LWE0, row), t]), ValueKind.LWE1)
                  for row in self.a]
        self.g2 = FheCircuit(eng)
        t = self.g2.add_input(ValueKind.GLWE1, t2)
        low = [self.g2.add_op(FheOp.KeyswitchL1toL0, [self.g2.add_input(ValueKind.LWE1, row)]) for row in self.b]
        self.outs = [self.g2.add_output(self.g2.add_op(FheOp.PBS_UNIVARIATE, [n, t]), ValueKind.LWE1) for n in low]

    def run(self):
        self.a[...] = self.eng.lwe_linear(0, self.x[None], LWE0)[0]
        self.g1.run()
        self.b[...] = self.eng.lwe_linear(1, np.stack(self.h)[None], LWE1)[0]
        self.g2.run()

    def close(self):
        self.g1.close()
        self.g2.close()


def chain(eng, rng, R):
    for slot in (0, 1):
        eng.load_lwe_linear_weights(slot, rng.integers(-127, 128, (R, R), dtype=np.int64, endpoint=True), rng.integers(0, 1 << 64, R, dtype=np.uint64))
    x = rng.integers(0, 1 << 64, size=(R, P.lwe0_words), dtype=np.uint64)
    t1 = spf_amd.generate_lut([lambda v: (3 * v + 1) % 8], BITS)
    t2 = spf_amd.generate_lut([lambda v: (7 - v) % 8], BITS)
    g, outs = one_graph(eng, x, t1, t2, R)
    c = Composition(eng, x, t1, t2, R)
    g.run()
    c.run()
    ms = {"g": [], "c": []}
    for _ in range(repeats):
        for f, run in (("g", g.run), ("c", c.run)):
            t0 = time.perf_counter()
            run()
            ms[f].append((time.perf_counter() - t0) * 1e3)
    st = g.stats()
    row = {"rows_per_layer": R, "one_graph": {**summary(ms["g"]), "levels": st["levels"], "launches": st["launches"]},
           "composition": {**summary(ms["c"]), "graphs": 2, "batch_calls": 2},
           "one_graph_over_composition": round(statistics.median(ms["g"]) / statistics.median(ms["c"]), 3),
           "outputs_equal": bool(np.array_equal(np.stack(outs), np.stack(c.outs)) and np.stack(outs).any())}
    g.close()
    c.close()
    return row


def product(eng, rng, layers, size=64):
    eng.load_lwe_linear_weights(2, rng.integers(-127, 128, (size, size), dtype=np.int64, endpoint=True), rng.integers(0, 1 << 64, size, dtype=np.uint64))
    glwe = rng.integers(0, 1 << 64, size=(layers, P.glwe_words), dtype=np.uint64)
    forms = {}
    for form in ("in_place", "rows_kernel"):
        g = FheCircuit(eng)
        bits = [g.add_unpack(g.add_input(ValueKind.GLWE1, v), size) for v in glwe]
        outs = [g.add_output(n, ValueKind.LWE1) for b in bits for n in g.add_lwe_linear(2, b if form == "in_place" else b[::-1], size)]
        forms[form] = (g, outs)
    eng.set_timing(True)
    ms, names, words = {f: [] for f in forms}, {}, {}
    try:
        for f, (g, outs) in forms.items():     # warm-up: plans the graph
            g.run()
            names[f] = eng.last_lwe_linear_kernel()
            words[f] = np.stack(outs)
            eng.last_kernel_ms("lwe_linear")
            eng.last_kernel_ms("lwe_linear_planes")
        for _ in range(repeats):
            for f, (g, _) in forms.items():
                g.run()
                t, n = eng.last_kernel_ms("lwe_linear")
                tp, np_ = eng.last_kernel_ms("lwe_linear_planes")   # (the matrix-core path: its planes pass belongs to the product)
                assert n >= 1, n
                ms[f].append(t * n + tp * np_)
    finally:
        eng.set_timing(False)
        for g, _ in forms.values():
            g.close()
    a, b = summary(ms["in_place"]), summary(ms["rows_kernel"])
    # (the reversed operands are the same rows under a column-reversed matrix: other words, the same work)
    return {"layers": layers, "M": size, "K": size, "words_per_row": P.lwe1_words, "in_place": {**a, "kernel": names["in_place"]},
            "rows_kernel": {**b, "kernel": names["rows_kernel"]}, "rows_over_in_place": round(b["median_ms"] / a["median_ms"], 3),
            "outputs_nonzero": bool(words["in_place"].any() and words["rows_kernel"].any())}


def main():
    eng = spf_amd.Engine(P, device=0)
    rng = np.random.default_rng(27)
    synthetic_keys(eng)
    rows = [chain(eng, rng, R) for R in ROWS]
    prod = [product(eng, rng, q) for q in LAYERS]
    print(json.dumps({"tool": "lwe_linear_graph_bench", "repeats": repeats, "library": spf_amd.lib_path(), "chain": rows, "product": prod}))
    eng.close()


if __name__ == "__main__":
    main()
