#!/usr/bin/env python3
"""spf_private_functional_keyswitch_enqueue (`private_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/
private_functional_keyswitch.rs:107-142) and spf_circuit_bootstrap_via_pfks_enqueue (`circuit_bootstrap_via_pfks`,
ops/bootstrapping/circuit_bootstrapping.rs:162-219; the reference's leg: benches/ops.rs:172-234) on DEFAULT_128's GLWE at the
reference benchmark's PFKS radix (17 bits x 2, from_dimension = 2048, the k+1 keys of the circuit bootstrap), device-resident,
timed with events on the launch stream.  spf_circuit_bootstrap_dev (trace and scheme switch) runs at the same B in the same run.
Keys are random numbers of a key's magnitudes (timing only); inputs are uniform words from a fixed seed.  Per shape: one warm-up,
then `calls` timed calls between two events.  --radix LOG COUNT may be given several times (24 bits and more time the VALU kernel).
The operation count per row is stated, not measured: (from_dimension + 1) * count * (k+1) * N wrapping 64-bit multiply-adds.
usage: python tools/pfks_bench.py [--calls 3] [--B 64 1024 4096] [--radix 17 2] [--once]
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
ap.add_argument("--B", type=int, nargs="+", default=[64, 1024, 4096])
ap.add_argument("--radix", type=int, nargs=2, action="append")
ap.add_argument("--once", action="store_true")
args = ap.parse_args()
radices = args.radix or [[17, 2]]

P = spf_amd.DEFAULT_128
N, K1, GW, L = P.polynomial_degree, P.glwe_size + 1, P.glwe_words, P.cbs_radix_count
n = P.glwe_size * N
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(19)


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


def timed(call):
    if not args.once:
        call()
    calls = 1 if args.once else args.calls
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def fill_blob(which, scale):
    """random spectra of a key's size straight into the key blob (timing only)"""
    ptr, nbytes = eng.key_blob(which)
    t = torch.randn(nbytes // 8, generator=g, device=dev, dtype=torch.float64) * scale
    torch.cuda.synchronize()
    eng.device_upload(ptr, t.cpu().numpy())
    eng.key_blob_commit(which)


for which in (0, 2, 3):
    fill_blob(which, 2.0 ** 40)

rows = []
for log, count in radices:
    keys = np.random.default_rng([19, log, count]).integers(0, 1 << 64, (K1, 1, n + 1, count, K1, N), dtype=np.uint64)
    eng.load_private_functional_keyswitch_keys_std(keys, log, count)
    key_bytes = keys.nbytes
    del keys
    for B in args.B:
        lwe1 = words(B, n + 1)
        glwe = torch.empty((B, GW), device=dev, dtype=torch.int64)
        lwe0 = words(B, P.lwe0_words)
        ggsw = torch.empty((B, 2 * P.cbs_ggsw_complex), device=dev, dtype=torch.float64)
        rows_l = words(B * L, n + 1)
        ggsw_int = torch.empty((B, 2 * P.cbs_ggsw_complex), device=dev, dtype=torch.int64)
        single = timed(lambda: eng.private_functional_keyswitch_enqueue(stream, K1 - 1, B, lwe1.data_ptr(), glwe.data_ptr()))
        comps = timed(lambda: eng.apply_pfks_on_ggsw_components_enqueue(stream, B, rows_l.data_ptr(), ggsw_int.data_ptr()))
        cbs_pfks = timed(lambda: eng.circuit_bootstrap_via_pfks_enqueue(stream, B, lwe0.data_ptr(), ggsw.data_ptr()))
        kernel = eng.last_private_functional_keyswitch_kernel()
        pbs = timed(lambda: eng.circuit_bootstrap_pbs_dev(stream, B, lwe0.data_ptr(), glwe.data_ptr()))
        cbs = timed(lambda: eng.circuit_bootstrap_dev(stream, B, lwe0.data_ptr(), ggsw.data_ptr()))
        mads = (n + 1) * count * GW
        rows.append({"radix_log": log, "radix_count": count, "B": B, "kernel": kernel,
                     "pfks_ms": round(single, 4), "pfks_us_per_output": round(single * 1e3 / B, 3),
                     "pfks_u64_gmad_per_s": round(B * mads / (single * 1e-3) / 1e9, 1),
                     "components_ms": round(comps, 4), "components_u64_gmad_per_s": round(B * L * K1 * mads / (comps * 1e-3) / 1e9, 1),
                     "cbs_via_pfks_ms": round(cbs_pfks, 4), "cbs_pbs_stage_ms": round(pbs, 4), "circuit_bootstrap_dev_ms": round(cbs, 4),
                     "cbs_via_pfks_over_circuit_bootstrap_dev": round(cbs_pfks / cbs, 2), "key_bytes": key_bytes})
        del lwe1, glwe, lwe0, ggsw, rows_l, ggsw_int
        torch.cuda.empty_cache()
print(json.dumps({"tool": "pfks_bench", "from_dimension": n, "calls": 1 if args.once else args.calls, "rows": rows}))
