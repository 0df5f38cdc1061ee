#!/usr/bin/env python3
"""Bivariate against univariate PBS, device-resident, on the same inputs: spf_pbs_bivariate_dev(left, right) packs
left * 2^p + right (lwe_pack_kernel) and then runs the univariate bootstrap, so the difference between the two is the
cost of the pack.  For each batch size: one warm-up call of each, then windows of `calls` calls between synchronises,
timed with hipEvents, alternating univariate / bivariate / univariate / bivariate; the mean of each variant's windows.
The outputs of the two are compared word for word (the univariate call gets the input packed on the host).
usage: python tools/bivariate_bench.py [calls] [B ...]        (default: 20 calls, B = 64 256 512 4096)
Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spf_amd
from spf_amd.sharding import _DevArray

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(b) for b in sys.argv[2:]] or [64, 256, 512, 4096]
P, p = spf_amd.DEFAULT_128, 2
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(7)

# a random bootstrap key: the timing does not depend on its values
ptr, nbytes = eng.key_blob(0)
torch.as_tensor(_DevArray(ptr, nbytes), device=dev).copy_(
    (torch.randn(nbytes // 8, generator=g, device=dev, dtype=torch.float64) * 2.0 ** 67).view(torch.uint8))
torch.cuda.synchronize()
eng.key_blob_commit(0)

lut = torch.from_numpy(spf_amd.generate_bivariate_lut(lambda l, r: (l + r) % 4, p, p).view(np.int64)).to(dev)
rng = np.random.default_rng(11)


def window(call) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


rows = []
for B in sizes:
    left = rng.integers(0, 1 << 64, size=(B, P.lwe0_words), dtype=np.uint64)
    right = rng.integers(0, 1 << 64, size=(B, P.lwe0_words), dtype=np.uint64)
    packed = left * np.uint64(1 << p) + right
    d_left, d_right, d_packed = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (left, right, packed))
    out_u = torch.empty((B, P.lwe1_words), device=dev, dtype=torch.int64)
    out_b = torch.empty_like(out_u)
    uni = lambda: eng.pbs_univariate_dev(stream, B, d_packed.data_ptr(), lut.data_ptr(), 0, out_u.data_ptr())  # noqa: E731
    biv = lambda: eng.pbs_bivariate_dev(stream, B, d_left.data_ptr(), d_right.data_ptr(), lut.data_ptr(), 0, p,  # noqa: E731
                                        out_b.data_ptr())
    uni()
    k_uni = eng.last_blind_rotate_kernel()
    biv()
    k_biv = eng.last_blind_rotate_kernel()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_u, out_b))
    t_uni, t_biv = [], []
    for _ in range(2):
        t_uni.append(window(uni))
        t_biv.append(window(biv))
    mu, mb = sum(t_uni) / len(t_uni), sum(t_biv) / len(t_biv)
    rows.append({"B": B, "univariate_ms": round(mu, 4), "bivariate_ms": round(mb, 4), "ratio": round(mb / mu, 4),
                 "windows_univariate_ms": [round(t, 4) for t in t_uni], "windows_bivariate_ms": [round(t, 4) for t in t_biv],
                 "kernel": k_biv, "kernel_univariate": k_uni, "outputs_equal": equal})
print(json.dumps({"tool": "bivariate_bench", "calls_per_window": calls, "plaintext_bits": p, "rows": rows}))
