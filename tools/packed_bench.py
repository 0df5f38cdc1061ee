#!/usr/bin/env python3
"""Fused packed-integer calls against the single-index calls a caller composes them from, device-resident, on the same
device inputs (a fixed seed):
  unpack: spf_glwe_unpack_l1_dev (one launch, int-major rows [b][i]) against n x spf_sample_extract_l1_dev (bit-major [i][b]);
  pack:   spf_glwe_pack_dev (one launch) against (n - 1) x (spf_glwe_mul_xn_dev + spf_glwe_xor_dev) accumulated left to right.
The composed pack reads each bit's batch contiguously, so its input is the bit-major copy of the fused call's int-major
input (the copy is made once, outside the timed windows).  For each (B, n): one warm-up of each form, then windows of
`calls` calls between synchronises, timed with hipEvents, alternating composed / fused; the mean of each form's windows.
The fused and composed outputs are compared word for word.
usage: python tools/packed_bench.py [calls] [B ...]        (default: 20 calls, B = 1 64 4096; n = 8 16 32)
Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import spf_amd

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(b) for b in sys.argv[2:]] or [1, 64, 4096]
bit_counts = [8, 16, 32]
P = spf_amd.DEFAULT_128
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(7)
GW, LW = P.glwe_words, P.lwe1_words


def window(call) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


def timed(composed, fused):
    composed()
    fused()
    torch.cuda.synchronize()
    tc, tf = [], []
    for _ in range(3):
        tc.append(window(composed))
        tf.append(window(fused))
    return sum(tc) / len(tc), sum(tf) / len(tf), tc, tf


rows = []
for B in sizes:
    for n in bit_counts:
        # unpack
        packed = words(B, GW)
        out_f = torch.empty((B, n, LW), device=dev, dtype=torch.int64)
        out_c = torch.empty((n, B, LW), device=dev, dtype=torch.int64)

        def unpack_composed():
            for i in range(n):
                eng.sample_extract_l1_dev(stream, B, packed.data_ptr(), i, out_c[i].data_ptr())

        unpack_fused = lambda: eng.glwe_unpack_l1_dev(stream, B, n, packed.data_ptr(), out_f.data_ptr())  # noqa: E731
        uc, uf, uwc, uwf = timed(unpack_composed, unpack_fused)
        u_equal = bool(torch.equal(out_f, out_c.transpose(0, 1)))
        del out_f, out_c, packed

        # pack
        bits = words(B, n, GW)
        bits_bm = bits.transpose(0, 1).contiguous()   # [i][b] for the composed calls
        pk_f = torch.empty((B, GW), device=dev, dtype=torch.int64)
        acc = [torch.empty((B, GW), device=dev, dtype=torch.int64) for _ in range(2)]
        tmp = torch.empty((B, GW), device=dev, dtype=torch.int64)

        def pack_composed():
            src = bits_bm[0]
            for i in range(1, n):
                eng.glwe_mul_xn_dev(stream, B, bits_bm[i].data_ptr(), i, tmp.data_ptr())
                eng.glwe_xor_dev(stream, B, src.data_ptr(), tmp.data_ptr(), acc[i % 2].data_ptr())
                src = acc[i % 2]

        pack_fused = lambda: eng.glwe_pack_dev(stream, B, n, bits.data_ptr(), pk_f.data_ptr())  # noqa: E731
        pc, pf, pwc, pwf = timed(pack_composed, pack_fused)
        p_equal = bool(torch.equal(pk_f, acc[(n - 1) % 2]))
        del bits, bits_bm, pk_f, acc, tmp
        torch.cuda.empty_cache()
        gib = 1 << 30
        rows.append({"B": B, "n": n,
                     "unpack_fused_ms": round(uf, 4), "unpack_composed_ms": round(uc, 4), "unpack_speedup": round(uc / uf, 2),
                     "pack_fused_ms": round(pf, 4), "pack_composed_ms": round(pc, 4), "pack_speedup": round(pc / pf, 2),
                     "unpack_launches": [1, n], "pack_launches": [1, 2 * (n - 1)],
                     "unpack_fused_gib": round(B * (GW + n * LW) * 8 / gib, 4), "pack_fused_gib": round(B * (n + 1) * GW * 8 / gib, 4),
                     "windows_ms": {"unpack_fused": [round(t, 4) for t in uwf], "unpack_composed": [round(t, 4) for t in uwc],
                                    "pack_fused": [round(t, 4) for t in pwf], "pack_composed": [round(t, 4) for t in pwc]},
                     "unpack_outputs_equal": u_equal, "pack_outputs_equal": p_equal})
print(json.dumps({"tool": "packed_bench", "calls_per_window": calls, "rows": rows}))
