#!/usr/bin/env python3
"""Blind rotation by an encrypted shift inside gate graphs, two ways, on DEFAULT_128 with synthetic keys and ciphertext words
(a fixed seed: the words are reproducible, the arithmetic is the real one):
  c  spf_graph_add_blind_rotation: one rotate-fused CMUX node per bit, one launch per level;
  n  the same words composed from MulXN(2N - r) + CMux nodes: two levels and two launches per bit.
Shapes (items, n_bits): (1, 11), (64, 11), (256, 11), (1024, 5) — one GGSW input per bit shared by all items, every rotated
item an output — and the circuit x >> s for a packed 32-bit x and a packed 5-bit s (unpack, KeyswitchL1toL0 and
CircuitBootstrap per bit of s, the rotation, unpack of the 32 result bits).
For each shape: one warm-up run of each form (plans the graph, sizes the scratch), then three windows of `runs` runs per form,
the forms alternating.  A run ends in a stream synchronise inside spf_graph_run, so the host clock around it is the time of the
whole run: the copy of the caller's inputs, the launches, the copy of the outputs — the copies are the same in both forms.
usage: python tools/blind_rotation_graph_bench.py [runs] [forms]     (default: 20 runs per window, forms cn; a library
without the constructor can run `n`)
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

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
forms = sys.argv[2] if len(sys.argv) > 2 else "cn"
P = spf_amd.DEFAULT_128
N = P.polynomial_degree
SHAPES = [(1, 11), (64, 11), (256, 11), (1024, 5)]


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


def rotate(g, form, acc, sels, log_stride=0):
    if form == "c":
        return g.add_blind_rotation(acc, sels, log_stride)
    for i, sel in enumerate(sels):
        acc = g.add_op(FheOp.CMux, [sel, acc, g.add_op(FheOp.MulXN, [acc], 2 * N - (1 << (i + log_stride)))])
    return acc


def build_shape(form, eng, glwes, sels):
    g = FheCircuit(eng)
    s = [g.add_input(ValueKind.GGSW1, v) for v in sels]
    return g, [g.add_output(rotate(g, form, g.add_input(ValueKind.GLWE1, x), s), ValueKind.GLWE1) for x in glwes]


def build_shift_right(form, eng, packed):
    g = FheCircuit(eng)
    x, s = (g.add_input(ValueKind.GLWE1, v) for v in packed)
    sels = [g.add_op(FheOp.CircuitBootstrap, [g.add_op(FheOp.KeyswitchL1toL0, [b])]) for b in g.add_unpack(s, 5)]
    return g, [g.add_output(b, ValueKind.LWE1) for b in g.add_unpack(rotate(g, form, x, sels), 32)]


def measure(built):
    for g, _ in built.values():
        g.run()
    windows = {f: [] for f in built}
    for _ in range(3):
        for f, (g, _) in built.items():
            t0 = time.perf_counter()
            for _ in range(runs):
                g.run()
            windows[f].append((time.perf_counter() - t0) * 1e3 / runs)
    row = {}
    for f, (g, _) in built.items():
        st = g.stats()
        row[f] = {"ms_per_run": round(sum(windows[f]) / 3, 4), "windows_ms": [round(t, 4) for t in windows[f]],
                  "levels": st["levels"], "launches": st["launches"]}
    if "c" in built and "n" in built:
        row["c_over_n"] = round(row["c"]["ms_per_run"] / row["n"]["ms_per_run"], 3)
        row["outputs_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(built["c"][1], built["n"][1])) and built["c"][1][0].any())
    for g, _ in built.values():
        g.close()
    return row


def main():
    eng = spf_amd.Engine(P, device=0)
    synthetic_keys(eng)
    rng = np.random.default_rng(2)
    glwes = rng.integers(0, 1 << 64, size=(max(i for i, _ in SHAPES), P.glwe_words), dtype=np.uint64)
    sels = (rng.standard_normal((11, 2 * P.cbs_ggsw_complex)) * 2.0 ** 58).view(np.complex128)
    rows = []
    for items, n_bits in SHAPES:
        row = measure({f: build_shape(f, eng, glwes[:items], sels[:n_bits]) for f in forms})
        rows.append({"items": items, "n_bits": n_bits, **row})
    packed = rng.integers(0, 1 << 64, size=(2, P.glwe_words), dtype=np.uint64)
    rows.append({"circuit": "x >> s, 32-bit x, 5-bit s", **measure({f: build_shift_right(f, eng, packed) for f in forms})})
    print(json.dumps({"tool": "blind_rotation_graph_bench", "runs_per_window": runs, "library": spf_amd.lib_path(), "rows": rows,
                      "bytes_per_item_step": {"c": 320 * 1024, "n": 416 * 1024}}))
    eng.close()


if __name__ == "__main__":
    main()
