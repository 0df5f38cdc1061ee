#!/usr/bin/env python3
"""spf_blind_rotation_dev (one rotate-fused CMUX per bit) against the chain a caller composes from spf_glwe_mul_xn_dev +
spf_cmux_dev, device-resident, on the same inputs: B items, n_bits = 11 (the reference's call at N = 2048), distinct selectors
generated on the device from a fixed seed.  The composed chain wants one contiguous selector per item and step, so it reads a
bit-major copy [i][b] of the fused call's int-major selectors [b][i]; the copy is made once, outside the timed windows.
For each B: one warm-up of each form, then three windows per form, alternating composed / fused, each `calls` calls between
stream synchronises under a host clock.  The outputs are compared word for word.  Bytes per item and step are computed
from the shapes (selector + GLWE reads and writes), not measured.
usage: python tools/blind_rotation_bench.py [calls] [B ...]        (default: 5 calls, B = 64 1024)
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import spf_amd

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sizes = [int(b) for b in sys.argv[2:]] or [64, 1024]
n_bits, log_stride = 11, 0
P = spf_amd.DEFAULT_128
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(13)
GW, SEL, N = P.glwe_words, P.cbs_ggsw_complex, P.polynomial_degree


def window(call) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


rows = []
for B in sizes:
    shift = torch.randn((B, n_bits, 2 * SEL), generator=g, device=dev, dtype=torch.float64) * 2.0 ** 58
    shift_bm = shift.transpose(0, 1).contiguous()      # [i][b] for the composed chain
    glwe = torch.randint(-(1 << 63), (1 << 63) - 1, (B, GW), generator=g, device=dev, dtype=torch.int64)
    out_f = torch.empty_like(glwe)
    acc = [torch.empty_like(glwe) for _ in range(2)]
    high = torch.empty_like(glwe)

    def composed():
        src = glwe
        for i in range(n_bits):
            eng.glwe_mul_xn_dev(stream, B, src.data_ptr(), 2 * N - (1 << (i + log_stride)), high.data_ptr())
            eng.cmux_dev(stream, B, shift_bm[i].data_ptr(), src.data_ptr(), high.data_ptr(), acc[i % 2].data_ptr())
            src = acc[i % 2]

    fused = lambda: eng.blind_rotation_dev(stream, B, n_bits, log_stride, shift.data_ptr(), glwe.data_ptr(), out_f.data_ptr())  # noqa: E731
    composed()
    composed_kernel = eng.last_cmux_kernel()
    fused()
    fused_kernel = eng.last_cmux_kernel()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_f, acc[(n_bits - 1) % 2]))
    tc, tf = [], []
    for _ in range(3):
        tc.append(window(composed))
        tf.append(window(fused))
    mc, mf = sum(tc) / 3, sum(tf) / 3
    sel_b, glwe_b = SEL * 16, GW * 8
    rows.append({"B": B, "n_bits": n_bits, "fused_ms": round(mf, 4), "composed_ms": round(mc, 4), "fused_over_composed": round(mf / mc, 3),
                 "windows_ms": {"fused": [round(t, 4) for t in tf], "composed": [round(t, 4) for t in tc]},
                 "composed_spread_ms": round(max(tc) - min(tc), 4),
                 "fused_not_slower": bool(mf <= max(tc)),
                 "kernels": {"fused": fused_kernel, "composed": composed_kernel}, "launches": [n_bits, 2 * n_bits],
                 "bytes_per_item_step": {"fused": sel_b + 2 * glwe_b, "composed": 2 * glwe_b + sel_b + 3 * glwe_b},
                 "outputs_equal": equal})
    del shift, shift_bm, glwe, out_f, acc, high
    torch.cuda.empty_cache()
print(json.dumps({"tool": "blind_rotation_bench", "calls_per_window": calls, "rows": rows}))
