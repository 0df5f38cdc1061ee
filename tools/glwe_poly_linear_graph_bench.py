#!/usr/bin/env python3
"""The plaintext polynomial linear map over GLWE ciphertexts as a gate-graph node (spf_graph_add_glwe_poly_linear), on DEFAULT_128
with synthetic keys and uniform inputs (fixed seeds: timing only; the words are tested in tests/test_gpu_glwe_poly_linear_graph.py).
Two tables, one JSON line.  Forms alternate on one build: one warm-up run of each, then `repeats` timed runs per form; median
(min - max); a difference counts when the medians are apart by more than the spread.

rows: the rows kernels (operands through the pointer table) against the in-place batch kernels on the same GLWEs, by device events
  around the launch (spf_last_kernel_ms "glwe_poly_linear"): `layers` layers of M = K = 8 over layers * 8 input GLWEs, each layer
  over its eight in order (consecutive: in place) and in reverse order (not consecutive: the rows kernel — the same rows under a
  column-reversed matrix: other words, the same work).  A constants-only slot (the stream kernels) and a 3-tap slot (the LDS
  kernels), 1 and 16 layers.
chain: public functional keyswitch of 8 level-0 LWEs -> X^s * a + b (slot M = 1, K = 2) -> unpack of 8 bits -> keyswitch -> 8
  univariate tables, as
  g  ONE gate graph: the GLWEs never leave the arena;
  c  today's composition without the node: a graph for the keyswitch, its GLWE downloaded, spf_glwe_poly_linear_batch through
     host pointers, the result uploaded into a second graph (unpack, keyswitch, tables).
  Both take the same inputs from host memory and leave the same 8 LWEs there; a run ends in a device synchronise, so the host
  clock around it is the time of the whole run.

usage: python tools/glwe_poly_linear_graph_bench.py [repeats]      (default 7; at least 5)"""
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
LAYERS = (1, 16)
SIZE, TAPS, WIDTH, SHIFT, BITS = 8, 3, 8, 3, 3
GLWE = ValueKind.GLWE1


class _DevArray:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def synthetic_keys(eng, rng):
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
    count = 4                    # public functional keyswitch key from the level-0 dimension: uniform words
    key = rng.integers(0, 1 << 64, (P.lwe_dimension, count, P.glwe_size + 1, N), dtype=np.uint64)
    eng.load_public_functional_keyswitch_key_std(key, 4, count)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def apart(a, b) -> bool:
    """the medians are apart by more than the spread of either form"""
    return abs(a["median_ms"] - b["median_ms"]) > max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])


def slot_csr(rng, taps):
    """SIZE x SIZE polynomials of `taps` terms each; taps = 0: one constant per polynomial (a constants-only slot)"""
    T = max(taps, 1)
    off = np.arange(SIZE * SIZE + 1, dtype=np.uint32) * T
    exp = (np.concatenate([rng.permutation(N)[:T] for _ in range(SIZE * SIZE)]) if taps else np.zeros(SIZE * SIZE)).astype(np.uint32)
    return off, exp, rng.integers(-(1 << 63), (1 << 63) - 1, SIZE * SIZE * T, dtype=np.int64, endpoint=True)


def rows(eng, rng, layers, taps):
    eng.load_glwe_poly_weights(2, slot_csr(rng, taps), shape=(SIZE, SIZE))
    x = rng.integers(0, 1 << 64, size=(layers, SIZE, P.glwe_words), dtype=np.uint64)
    forms = {}
    for form in ("in_place", "rows_kernel"):
        g = FheCircuit(eng)
        ins = [[g.add_input(GLWE, v) for v in layer] for layer in x]
        outs = [g.add_output(n, GLWE) for b in ins for n in g.add_glwe_poly_linear(2, b if form == "in_place" else b[::-1], SIZE)]
        forms[form] = (g, outs)
    eng.set_timing(True)
    ms, names, words = {f: [] for f in forms}, {}, {}
    try:
        for f, (g, outs) in forms.items():     # warm-up: plans the graph
            g.run()
            names[f] = eng.last_glwe_poly_kernel()
            words[f] = np.stack(outs)
            eng.last_kernel_ms("glwe_poly_linear")
        for _ in range(repeats):
            for f, (g, _) in forms.items():
                g.run()
                t, n = eng.last_kernel_ms("glwe_poly_linear")
                assert n == 1, n
                ms[f].append(t)
    finally:
        eng.set_timing(False)
        for g, _ in forms.values():
            g.close()
    a, b = summary(ms["in_place"]), summary(ms["rows_kernel"])
    return {"layers": layers, "M": SIZE, "K": SIZE, "taps": taps, "in_place": {**a, "kernel": names["in_place"]},
            "rows_kernel": {**b, "kernel": names["rows_kernel"]}, "rows_over_in_place": round(b["median_ms"] / a["median_ms"], 3),
            "apart_by_more_than_the_spread": apart(a, b), "outputs_nonzero": bool(words["in_place"].any() and words["rows_kernel"].any())}


def tail(g, packed, table):
    low = [g.add_op(FheOp.KeyswitchL1toL0, [n]) for n in g.add_unpack(packed, WIDTH)]
    return [g.add_output(g.add_op(FheOp.PBS_UNIVARIATE, [n, table]), ValueKind.LWE1) for n in low]


def one_graph(eng, x, b, table):
    g = FheCircuit(eng)
    t, other = g.add_input(GLWE, table), g.add_input(GLWE, b)
    a = g.add_public_functional_keyswitch([g.add_input(ValueKind.LWE0, row) for row in x])
    return g, tail(g, g.add_glwe_poly_linear(3, [a, other], 1)[0], t)


class Composition:
    """graph, download, batch call, upload, second graph"""

    def __init__(self, eng, x, b, table):
        self.eng, self.b = eng, b
        self.g1 = FheCircuit(eng)
        self.a = self.g1.add_output(self.g1.add_public_functional_keyswitch([self.g1.add_input(ValueKind.LWE0, row) for row in x]), GLWE)
        self.sum = np.zeros(P.glwe_words, dtype=np.uint64)
        self.g2 = FheCircuit(eng)
        t = self.g2.add_input(GLWE, table)
        self.outs = tail(self.g2, self.g2.add_input(GLWE, self.sum), t)

    def run(self):
        self.g1.run()
        self.sum[...] = self.eng.glwe_poly_linear(3, np.stack([self.a, self.b]).reshape(1, 2, P.glwe_size + 1, N)).reshape(-1)
        self.g2.run()

    def close(self):
        self.g1.close()
        self.g2.close()


def chain(eng, rng):
    eng.load_glwe_poly_weights(3, (np.array([0, 1, 2], dtype=np.uint32), np.array([SHIFT, 0], dtype=np.uint32), np.array([1, 1], dtype=np.int64)),
                               shape=(1, 2))
    x = rng.integers(0, 1 << 64, size=(WIDTH, P.lwe0_words), dtype=np.uint64)
    b = rng.integers(0, 1 << 64, size=P.glwe_words, dtype=np.uint64)
    table = spf_amd.generate_lut([lambda v: (3 * v + 1) % 8], BITS)
    g, outs = one_graph(eng, x, b, table)
    c = Composition(eng, x, b, table)
    g.run()
    c.run()
    ms = {"g": [], "c": []}
    for _ in range(repeats):
        for f, run in (("g", g.run), ("c", c.run)):
            t0 = time.perf_counter()
            run()
            ms[f].append((time.perf_counter() - t0) * 1e3)
    st = g.stats()
    one, comp = summary(ms["g"]), summary(ms["c"])
    row = {"lwes": WIDTH, "shift": SHIFT, "one_graph": {**one, "levels": st["levels"], "launches": st["launches"]},
           "composition": {**comp, "graphs": 2, "batch_calls": 1},
           "one_graph_over_composition": round(one["median_ms"] / comp["median_ms"], 3), "apart_by_more_than_the_spread": apart(one, comp),
           "outputs_equal": bool(np.array_equal(np.stack(outs), np.stack(c.outs)) and np.stack(outs).any())}
    g.close()
    c.close()
    return row


def main():
    os.environ.pop("SPF_GLWE_POLY_PATH", None)
    eng = spf_amd.Engine(P, device=0)
    rng = np.random.default_rng(31)
    synthetic_keys(eng, rng)
    table_rows = [rows(eng, rng, q, taps) for taps in (0, TAPS) for q in LAYERS]
    print(json.dumps({"tool": "glwe_poly_linear_graph_bench", "repeats": repeats, "library": spf_amd.lib_path(), "rows": table_rows,
                      "chain": [chain(eng, rng)]}))
    eng.close()


if __name__ == "__main__":
    main()
