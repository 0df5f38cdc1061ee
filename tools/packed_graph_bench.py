#!/usr/bin/env python3
"""The 32-bit ripple-carry adder graph (tests/test_gpu_graph.py) on DEFAULT_128 with three kinds of input and output, on
synthetic keys and ciphertext words (a fixed seed: the words are reproducible, the arithmetic is the real one):
  a  one GLWE per bit in and out: 64 inputs -> SampleExtract(0) -> KeyswitchL1toL0 -> CircuitBootstrap, 33 outputs;
  b  packed I/O composed from graph operations: 2 packed inputs -> SampleExtract(i), i < 32, of each; the 33 result bits
     through MulXN(i) and a pairwise tree of GlweAdd (dynamic_generic_int_graph_nodes.rs:139-200) -> 1 output;
  c  packed I/O through spf_graph_add_unpack / spf_graph_add_pack: 2 packed inputs, 1 output.
For each form: one warm-up run (plans the graph, sizes the scratch), then windows of `runs` runs, the forms alternating; a
run ends in a stream synchronise inside spf_graph_run, so the host clock around it is the time of the whole run (input copy,
launches, output copy).  Prints milliseconds per run, levels, launches and the bytes of the caller's buffers copied each
way, and whether b and c returned the same words.
usage: python tools/packed_graph_bench.py [runs] [forms]        (default: 50 runs per window, forms abc; a library without
the two calls can run `ab`)
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (device memory for the synthetic keys only)

import spf_amd  # noqa: E402
from spf_amd import FheCircuit, FheOp, ValueKind  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 50
forms = sys.argv[2] if len(sys.argv) > 2 else "abc"
BITS = 32
P = spf_amd.DEFAULT_128


class _DevArray:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def synthetic_keys(eng):
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev)
    g0.manual_seed(1)
    for which in range(4):
        ptr, nbytes = eng.key_blob(which)
        t = torch.as_tensor(_DevArray(ptr, nbytes), device=dev)
        if which == 1:
            t.copy_(torch.randint(-(2 ** 63), 2 ** 63 - 1, (nbytes // 8,), generator=g0, device=dev, dtype=torch.int64).view(torch.uint8))
        else:
            t.copy_((torch.randn(nbytes // 8, generator=g0, device=dev, dtype=torch.float64) * 2.0 ** 67).view(torch.uint8))
        torch.cuda.synchronize()
        eng.key_blob_commit(which)


def adder(g, ga, gb):
    zero, one = g.add_trivial(ValueKind.GLWE1, 0), g.add_trivial(ValueKind.GLWE1, 1)
    carry, sums = zero, []
    for i in range(BITS):
        ncarry = g.add_op(FheOp.Not, [carry])
        l1 = [g.add_op(FheOp.CMux, [gb[i], lo, hi]) for lo, hi in [(carry, ncarry), (ncarry, carry), (zero, carry), (carry, one)]]
        sums.append(g.add_op(FheOp.CMux, [ga[i], l1[0], l1[1]]))
        carry = g.add_op(FheOp.CMux, [ga[i], l1[2], l1[3]])
    return sums + [carry]


def selectors(g, lwe1):
    return [g.add_op(FheOp.CircuitBootstrap, [g.add_op(FheOp.KeyswitchL1toL0, [x])]) for x in lwe1]


def build(form, eng, packed):
    """-> (graph, output arrays, caller bytes up, caller bytes down)"""
    g = FheCircuit(eng)
    if form == "a":
        rng = np.random.default_rng(3)
        ins = [g.add_input(ValueKind.GLWE1, rng.integers(0, 1 << 64, size=P.glwe_words, dtype=np.uint64)) for _ in range(2 * BITS)]
        sel = selectors(g, [g.add_op(FheOp.SampleExtract, [x], 0) for x in ins])
        outs = [g.add_output(x, ValueKind.GLWE1) for x in adder(g, sel[:BITS], sel[BITS:])]
        return g, outs, 2 * BITS * P.glwe_words * 8, (BITS + 1) * P.glwe_words * 8
    xa, xb = (g.add_input(ValueKind.GLWE1, x) for x in packed)
    if form == "b":
        lwe1 = [g.add_op(FheOp.SampleExtract, [x], i) for x in (xa, xb) for i in range(BITS)]
    else:
        lwe1 = g.add_unpack(xa, BITS) + g.add_unpack(xb, BITS)
    sel = selectors(g, lwe1)
    bits = adder(g, sel[:BITS], sel[BITS:])
    if form == "b":
        red = [bits[0]] + [g.add_op(FheOp.MulXN, [x], i) for i, x in enumerate(bits) if i]
        while len(red) > 1:
            red = [g.add_op(FheOp.GlweAdd, red[j:j + 2]) if len(red[j:j + 2]) == 2 else red[j] for j in range(0, len(red), 2)]
        out = red[0]
    else:
        out = g.add_pack(bits)
    return g, [g.add_output(out, ValueKind.GLWE1)], 2 * P.glwe_words * 8, P.glwe_words * 8


def main():
    eng = spf_amd.Engine(P, device=0)
    synthetic_keys(eng)
    packed = np.random.default_rng(2).integers(0, 1 << 64, size=(2, P.glwe_words), dtype=np.uint64)
    built = {f: build(f, eng, packed) for f in forms}
    for g, _, _, _ in built.values():
        g.run()
    windows = {f: [] for f in forms}
    for _ in range(3):
        for f in forms:
            g = built[f][0]
            t0 = time.perf_counter()
            for _ in range(runs):
                g.run()
            windows[f].append((time.perf_counter() - t0) * 1e3 / runs)
    rows = []
    for f in forms:
        g, outs, up, down = built[f]
        st = g.stats()
        rows.append({"form": f, "ms_per_run": round(sum(windows[f]) / len(windows[f]), 4), "windows_ms": [round(t, 4) for t in windows[f]],
                     "nodes": st["nodes"], "levels": st["levels"], "launches": st["launches"], "bytes_up": up, "bytes_down": down})
    equal = None
    if "b" in built and "c" in built:
        equal = bool(np.array_equal(built["b"][1][0], built["c"][1][0]) and built["c"][1][0].any())
    print(json.dumps({"tool": "packed_graph_bench", "runs_per_window": runs, "library": spf_amd.lib_path(), "rows": rows,
                      "b_and_c_outputs_equal": equal}))
    for g, _, _, _ in built.values():
        g.close()
    eng.close()


if __name__ == "__main__":
    main()
