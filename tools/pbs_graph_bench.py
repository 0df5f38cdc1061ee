#!/usr/bin/env python3
"""A two-stage table pipeline over W independent 2-bit digits, two ways, on DEFAULT_128 with synthetic keys (a fixed seed: the
words are reproducible, the arithmetic is the real one):

    two packed GLWEs -> unpack (2 W LWEs) -> keyswitch -> bivariate table (digit i of one with digit i of the other)
                     -> keyswitch -> univariate table -> public functional keyswitch of the W results into ONE GLWE -> unpack (W)

  g  ONE gate graph (SPF_OP_PBS_BIVARIATE, SPF_OP_PBS_UNIVARIATE, spf_graph_add_public_functional_keyswitch): every
     intermediate stays in the arena;
  d  the same operations through the `_dev` entry points with a host round trip (download, upload) wherever a graph without
     those three nodes ends: after the first keyswitch, after each bootstrap, after the second keyswitch and after the public
     functional keyswitch — the route a library without the nodes offers.  Device buffers are allocated once, outside the clock.
Both forms copy the same inputs up and the same W LWEs down.  Per W in {32, 1024}: one warm-up run of each form, then `repeats`
timed runs per form, alternating; a run ends in a device synchronise, so the host clock around it is the time of the whole
run.  Medians and min - max are reported, and that the two forms gave the same words.

Second part: the transposing pre-pass of the public functional keyswitch over rows from FOUR levels of a graph, read where they
lie (pufks_digits_rows_kernel) against gather_rows_kernel + pufks_digits_kernel (SPF_PUFKS_ROWS_GATHER=1), by device events
around the pre-pass (spf_last_kernel_ms "pufks_prepass"), alternating, at 32 and 1024 rows of dimension 2048.

usage: python tools/pbs_graph_bench.py [repeats]      (default 7; at least 5)
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
WIDTHS = (32, 1024)
BITS = 2


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
    # from_dimension = k N (the bootstraps' results are L1 LWEs), the hand-written radix 4 bits x 4
    key = rng.integers(0, 1 << 64, size=(P.glwe_size * P.polynomial_degree, 4, P.glwe_size + 1, P.polynomial_degree), dtype=np.uint64)
    eng.load_public_functional_keyswitch_key_std(key, 4, 4)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def build_graph(eng, packed, biv_lut, uni_lut, W):
    g = FheCircuit(eng)
    a, b = (g.add_input(ValueKind.GLWE1, v) for v in packed)
    tb, tu = g.add_input(ValueKind.GLWE1, biv_lut), g.add_input(ValueKind.GLWE1, uni_lut)
    da = [g.add_op(FheOp.KeyswitchL1toL0, [x]) for x in g.add_unpack(a, W)]
    db = [g.add_op(FheOp.KeyswitchL1toL0, [x]) for x in g.add_unpack(b, W)]
    sums = [g.add_op(FheOp.KeyswitchL1toL0, [g.add_op(FheOp.PBS_BIVARIATE, [x, y, tb], BITS)]) for x, y in zip(da, db)]
    outs = [g.add_op(FheOp.PBS_UNIVARIATE, [s, tu]) for s in sums]
    together = g.add_public_functional_keyswitch(outs)
    return g, [g.add_output(x, ValueKind.LWE1) for x in g.add_unpack(together, W)]


class DevRoute:
    """the `_dev` calls on the default stream, with a host round trip wherever a graph of the ten FheOps would end"""

    def __init__(self, eng, packed, biv_lut, uni_lut, W):
        self.eng, self.W, self.packed = eng, W, np.ascontiguousarray(packed)
        self.l0w, self.l1w, self.gw = P.lwe0_words, P.lwe1_words, P.glwe_words
        self.bufs = []
        self.d_packed = self._alloc(2 * self.gw * 8)
        self.d_tb, self.d_tu = self._alloc(self.gw * 8), self._alloc(self.gw * 8)
        eng.device_upload(self.d_tb, biv_lut)
        eng.device_upload(self.d_tu, uni_lut)
        self.d_l1 = self._alloc(2 * W * self.l1w * 8)
        self.d_l0 = self._alloc(2 * W * self.l0w * 8)
        self.d_glwe = self._alloc(self.gw * 8)
        self.h_l0 = np.empty((2 * W, self.l0w), dtype=np.uint64)
        self.h_l1 = np.empty((W, self.l1w), dtype=np.uint64)
        self.h_glwe = np.empty(self.gw, dtype=np.uint64)
        self.out = np.empty((W, self.l1w), dtype=np.uint64)

    def _alloc(self, nbytes):
        p = self.eng.device_alloc(nbytes)
        self.bufs.append(p)
        return p

    def _round_trip(self, host, ptr):
        self.eng.device_download(None, host, ptr)     # (waits for what was enqueued)
        self.eng.device_upload(ptr, host)

    def run(self):
        e, W = self.eng, self.W
        e.device_upload(self.d_packed, self.packed)
        e.glwe_unpack_l1_dev(None, 2, W, self.d_packed, self.d_l1)
        e.keyswitch_dev(None, 2 * W, self.d_l1, self.d_l0)
        self._round_trip(self.h_l0, self.d_l0)
        e.pbs_bivariate_dev(None, W, self.d_l0, self.d_l0 + W * self.l0w * 8, self.d_tb, 0, BITS, self.d_l1)
        self._round_trip(self.h_l1, self.d_l1)
        e.keyswitch_dev(None, W, self.d_l1, self.d_l0)
        self._round_trip(self.h_l0[:W], self.d_l0)
        e.pbs_univariate_dev(None, W, self.d_l0, self.d_tu, 0, self.d_l1)
        self._round_trip(self.h_l1, self.d_l1)
        e.public_functional_keyswitch_enqueue(None, 1, W, self.d_l1, self.d_glwe)
        self._round_trip(self.h_glwe, self.d_glwe)
        e.glwe_unpack_l1_dev(None, 1, W, self.d_glwe, self.d_l1)
        e.device_download(None, self.out, self.d_l1)

    def close(self):
        for p in self.bufs:
            self.eng.device_free(p)


def pipeline(eng, rng, W):
    packed = rng.integers(0, 1 << 64, size=(2, P.glwe_words), dtype=np.uint64)
    biv_lut = spf_amd.generate_bivariate_lut(lambda l, r: (l + r) % 4, BITS, BITS)
    uni_lut = spf_amd.generate_lut([lambda x: (3 * x + 1) % 4], BITS)
    g, outs = build_graph(eng, packed, biv_lut, uni_lut, W)
    d = DevRoute(eng, packed, biv_lut, uni_lut, W)
    g.run()
    d.run()
    ms = {"g": [], "d": []}
    for _ in range(repeats):
        for f, run in (("g", g.run), ("d", d.run)):
            t0 = time.perf_counter()
            run()
            ms[f].append((time.perf_counter() - t0) * 1e3)
    st = g.stats()
    row = {"W": W, "graph": {**summary(ms["g"]), "levels": st["levels"], "launches": st["launches"]},
           "dev_with_round_trips": {**summary(ms["d"]), "round_trips": 5},
           "graph_over_dev": round(statistics.median(ms["g"]) / statistics.median(ms["d"]), 3),
           "outputs_equal": bool(np.array_equal(np.stack(outs), d.out) and d.out.any())}
    g.close()
    d.close()
    return row


def prepass(eng, rng, rows):
    """one keyswitch node over `rows` L1 LWEs taken in turn from four levels: inputs, bits unpacked from an input GLWE, from its
    NOT, from the NOT of that"""
    per = rows // 4
    g = FheCircuit(eng)
    x = g.add_input(ValueKind.GLWE1, rng.integers(0, 1 << 64, size=P.glwe_words, dtype=np.uint64))
    n1 = g.add_op(FheOp.Not, [x])
    n2 = g.add_op(FheOp.Not, [n1])
    levels = [[g.add_input(ValueKind.LWE1, v) for v in rng.integers(0, 1 << 64, size=(per, P.lwe1_words), dtype=np.uint64)],
              g.add_unpack(x, per), g.add_unpack(n1, per), g.add_unpack(n2, per)]
    out = g.add_output(g.add_public_functional_keyswitch([levels[j % 4][j // 4] for j in range(rows)]), ValueKind.GLWE1)
    eng.set_timing(True)
    words, ms = {}, {"0": [], "1": []}
    try:
        for form in ("0", "1"):     # warm-up: plans the graph for the form, sizes the scratch
            os.environ["SPF_PUFKS_ROWS_GATHER"] = form
            g.run()
            words[form] = out.copy()
            eng.last_kernel_ms("pufks_prepass")
        for _ in range(repeats):
            for form in ("0", "1"):
                os.environ["SPF_PUFKS_ROWS_GATHER"] = form
                g.run()
                t, n = eng.last_kernel_ms("pufks_prepass")
                assert n == 1, n
                ms[form].append(t)
    finally:
        os.environ.pop("SPF_PUFKS_ROWS_GATHER", None)
        eng.set_timing(False)
        g.close()
    sc, ga = summary(ms["0"]), summary(ms["1"])
    return {"rows": rows, "dimension": P.lwe1_words - 1, "levels": 4, "scattered": sc, "gather_then_contiguous": ga,
            "scattered_over_gather": round(sc["median_ms"] / ga["median_ms"], 3),
            "keep_scattered": bool(sc["median_ms"] <= ga["median_ms"] + (ga["max_ms"] - ga["min_ms"])),
            "outputs_equal": bool(np.array_equal(words["0"], words["1"]) and words["0"].any())}


def main():
    eng = spf_amd.Engine(P, device=0)
    rng = np.random.default_rng(21)
    synthetic_keys(eng, rng)
    rows = [pipeline(eng, rng, W) for W in WIDTHS]
    pre = [prepass(eng, rng, r) for r in WIDTHS]
    print(json.dumps({"tool": "pbs_graph_bench", "repeats": repeats, "library": spf_amd.lib_path(), "pipeline": rows, "prepass": pre}))
    eng.close()


if __name__ == "__main__":
    main()
