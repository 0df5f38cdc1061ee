#!/usr/bin/env python3
"""spf_public_functional_keyswitch_enqueue (`public_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/
public_functional_keyswitch.rs:74-148; the reference's leg: benches/ops.rs:395-452) at from_dimension = 2048, device-resident,
timed with events on the launch stream: B outputs of p inputs each, radix 4 bits x `count`.
With --route the route that exists without it is timed in the same run for the same bits: B * p x (keyswitch L1 -> L0, circuit
bootstrap, multiply_glwe_ggsw of a trivial one by the GGSW), then glwe_pack — one bootstrap per bit.  Its keys are random numbers of
a key's magnitudes (timing only); its GGSWs take 256 KiB per bit, so it is run where B * p of them fit (--route-max-bits).
Inputs are uniform words from a fixed seed.  Per shape: one warm-up, then `calls` timed calls between two events.
The flop count per output is stated, not measured: n * count rounds of one 1024-point complex transform (5 * 1024 * 10 flops) and
two rows of 1024 four-FMA complex multiply-adds (2 * 1024 * 8), the inverse pair and the pre-pass left out.
usage: python tools/pufks_bench.py [--calls 3] [--B 1 64 1024] [--p 32 1024] [--count 8 4] [--n 2048] [--route] [--once]
       --once: one call per shape, no warm-up, no route (a counter collection run)
Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spf_amd

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 1024])
ap.add_argument("--p", type=int, nargs="+", default=[32, 1024])
ap.add_argument("--count", type=int, nargs="+", default=[8, 4])
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--route", action="store_true")
ap.add_argument("--route-max-bits", type=int, default=1 << 16)
ap.add_argument("--once", action="store_true")
args = ap.parse_args()

P = spf_amd.DEFAULT_128
N, GW = P.polynomial_degree, P.glwe_words
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(18)
ROOF_TF = 78.6
FLOPS_PER_ROUND = 5 * 1024 * 10 + 2 * 1024 * 8


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


def timed(call, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def fill_blob(which, scale):
    """random spectra / words of a key's size straight into the key blob (timing only)"""
    ptr, nbytes = eng.key_blob(which)
    if which == 1:
        t = words(nbytes // 8)
    else:
        t = torch.randn(nbytes // 8, generator=g, device=dev, dtype=torch.float64) * scale
    torch.cuda.synchronize()
    eng.device_upload(ptr, t.cpu().numpy())
    eng.key_blob_commit(which)


route_ready = False
rows = []
for count in args.count:
    key = np.random.default_rng([18, args.n, count]).integers(0, 1 << 64, (args.n, count, P.glwe_size + 1, N), dtype=np.uint64)
    eng.load_public_functional_keyswitch_key_std(key, 4, count)
    key_bytes = key.nbytes
    del key
    for p in args.p:
        for B in args.B:
            lwes = words(B * p, args.n + 1)
            out = torch.empty((B, GW), device=dev, dtype=torch.int64)
            call = lambda: eng.public_functional_keyswitch_enqueue(stream, B, p, lwes.data_ptr(), out.data_ptr())  # noqa: E731
            if args.once:
                ms = timed(call, 1)
            else:
                call()
                ms = timed(call, args.calls)
            flops = B * args.n * count * FLOPS_PER_ROUND
            row = {"count": count, "p": p, "B": B, "kernel": eng.last_public_functional_keyswitch_kernel(), "ms_per_call": round(ms, 4),
                   "us_per_output": round(ms * 1e3 / B, 2), "flop_per_output": args.n * count * FLOPS_PER_ROUND,
                   "fp64_fraction_of_roof": round(flops / (ms * 1e-3) / (ROOF_TF * 1e12), 4),
                   "key_bytes": key_bytes, "input_bytes": lwes.numel() * 8}
            if args.route and not args.once and B * p <= args.route_max_bits:
                if not route_ready:
                    fill_blob(0, 2.0 ** 40)
                    fill_blob(1, 0)
                    fill_blob(2, 2.0 ** 40)
                    fill_blob(3, 2.0 ** 40)
                    route_ready = True
                bits = B * p
                lwe1 = words(bits, P.lwe1_words)
                lwe0 = torch.empty((bits, P.lwe0_words), device=dev, dtype=torch.int64)
                ggsw = torch.empty((bits, 2 * P.cbs_ggsw_complex), device=dev, dtype=torch.float64)
                one = torch.zeros((bits, GW), device=dev, dtype=torch.int64)
                one[:, P.glwe_size * N] = 1 << 62
                bit_glwe = torch.empty((bits, GW), device=dev, dtype=torch.int64)
                packed = torch.empty((B, GW), device=dev, dtype=torch.int64)

                def route():
                    eng.keyswitch_dev(stream, bits, lwe1.data_ptr(), lwe0.data_ptr())
                    eng.circuit_bootstrap_dev(stream, bits, lwe0.data_ptr(), ggsw.data_ptr())
                    eng._ck(eng._lib.spf_multiply_glwe_ggsw_dev(eng._h, stream, bits, one.data_ptr(), ggsw.data_ptr(), bit_glwe.data_ptr()))
                    eng.glwe_pack_dev(stream, B, p, bit_glwe.data_ptr(), packed.data_ptr())

                route()
                rms = timed(route, max(1, min(args.calls, 2)))
                row["route_ms_per_call"] = round(rms, 3)
                row["route_over_new"] = round(rms / ms, 2)
                del lwe1, lwe0, ggsw, one, bit_glwe, packed
            rows.append(row)
            del lwes, out
            torch.cuda.empty_cache()
print(json.dumps({"tool": "pufks_bench", "from_dimension": args.n, "calls": 1 if args.once else args.calls, "rows": rows}))
