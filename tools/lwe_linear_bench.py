#!/usr/bin/env python3
"""spf_lwe_linear_enqueue (`scalar_mul_ciphertext_mad` + `add_lwe_inplace`, sunscreen_tfhe ops/ciphertext/lwe_ciphertext_ops.rs:
48-66, :4-18, for an integer matrix) on DEFAULT_128's ciphertexts, device-resident.  Two tables, one JSON line.

throughput: M = K = 1024 (--square), kind lwe1 (2049 words), one weight matrix per limb class U = 1, 2, 3 (uniform over the class's
  range), at each --B: the whole call between two events on the launch stream, and its two parts as the library times them
  (spf_last_kernel_ms "lwe_linear_planes": the per-call byte planes; "lwe_linear": the GEMM and the bias).  The operation count is
  stated, not measured: M * K * B * W wrapping 64-bit multiply-adds; the GEMM runs U limb passes over them.
dispatch: K = 256 (--K), kind lwe1, B = 50 (B W = 102 450 words), M in --M: the VALU kernel and the matrix-core path on the same build,
  forced by SPF_LWE_LINEAR_PATH, forms alternating, one warm-up of each and then --runs timed runs of --reps calls each.  Per M:
  median, min and max of each form, and whether the matrix-core median is below the VALU median by more than the VALU form's own
  min-max spread (the rule the estimates of lwe_linear_matrix_cores_pay in spf_hip.hip are fitted to).
Weights and inputs are uniform numbers from fixed seeds (timing only; the words are tested in tests/test_gpu_lwe_linear.py).
usage: python tools/lwe_linear_bench.py [--B 1 32] [--square 1024] [--M 1 8 32 64 128] [--K 256] [--runs 7] [--reps 5] [--limbs 1 3]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spf_amd

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, nargs="*", default=[1, 32], help="batch sizes of the throughput table (none: skip it)")
ap.add_argument("--square", type=int, default=1024)
ap.add_argument("--M", type=int, nargs="+", default=[1, 8, 32, 64, 128])
ap.add_argument("--K", type=int, nargs="+", default=[256], help="input counts of the dispatch table")
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limbs", type=int, nargs="+", default=[1, 3], help="limb classes of the dispatch table")
args = ap.parse_args()

P = spf_amd.DEFAULT_128
W = P.lwe1_words
LWE1 = 1
RANGES = {1: (-127, 128), 2: (-32639, 32896), 3: (-8355711, 8421504)}
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(24)


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


def class_weights(M, K, U):
    lo, hi = RANGES[U]
    w = np.random.default_rng([24, M, K, U]).integers(lo, hi, (M, K), dtype=np.int64, endpoint=True)
    w.reshape(-1)[:2] = [hi, lo][:w.size]
    return w


def timed(call, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def force(path):
    if path:
        os.environ["SPF_LWE_LINEAR_PATH"] = path
    else:
        os.environ.pop("SPF_LWE_LINEAR_PATH", None)


throughput = []
S = args.square
for U in (1, 2, 3):
    eng.load_lwe_linear_weights(0, class_weights(S, S, U), np.arange(S, dtype=np.uint64))
    for B in args.B:
        x, y = words(B, S, W), torch.empty((B, S, W), device=dev, dtype=torch.int64)
        call = lambda: eng.lwe_linear_enqueue(stream, 0, LWE1, B, x.data_ptr(), y.data_ptr())  # noqa: E731
        force("mfma")
        call()
        whole = statistics.median(timed(call, args.reps) for _ in range(args.runs))
        kernel = eng.last_lwe_linear_kernel()
        eng.set_timing(True)
        for _ in range(args.runs):
            call()
        torch.cuda.synchronize()
        planes_ms, _ = eng.last_kernel_ms("lwe_linear_planes")
        gemm_ms, _ = eng.last_kernel_ms("lwe_linear")
        eng.set_timing(False)
        force("valu")
        call()
        valu = statistics.median(timed(call, args.reps) for _ in range(args.runs))
        mads = S * S * B * W
        throughput.append({"U": U, "M": S, "K": S, "B": B, "kernel": kernel, "call_ms": round(whole, 4), "planes_ms": round(planes_ms, 4),
                           "gemm_and_bias_ms": round(gemm_ms, 4), "planes_share": round(planes_ms / (planes_ms + gemm_ms), 3),
                           "call_u64_gmad_per_s": round(mads / (whole * 1e-3) / 1e9, 1),
                           "gemm_u64_gmad_per_s": round(mads / (gemm_ms * 1e-3) / 1e9, 1),
                           "gemm_u64_gmad_per_s_per_limb_pass": round(U * mads / (gemm_ms * 1e-3) / 1e9, 1),
                           "valu_call_ms": round(valu, 4), "valu_u64_gmad_per_s": round(mads / (valu * 1e-3) / 1e9, 1)})
        del x, y
        torch.cuda.empty_cache()

dispatch = []
B = 50
for K, U, M in [(K, U, M) for K in args.K for U in args.limbs for M in args.M]:
    if True:
        x = words(B, K, W)
        eng.load_lwe_linear_weights(1, class_weights(M, K, U), np.arange(M, dtype=np.uint64))
        y = torch.empty((B, M, W), device=dev, dtype=torch.int64)
        call = lambda: eng.lwe_linear_enqueue(stream, 1, LWE1, B, x.data_ptr(), y.data_ptr())  # noqa: E731
        t = {"valu": [], "mfma": []}
        names = {}
        for path in t:
            force(path)
            call()
            names[path] = eng.last_lwe_linear_kernel()
        for _ in range(args.runs):
            for path in t:
                force(path)
                t[path].append(timed(call, args.reps))
        med = {p: statistics.median(v) for p, v in t.items()}
        spread = max(t["valu"]) - min(t["valu"])
        dispatch.append({"U": U, "M": M, "K": K, "B": B, "words": B * W,
                         **{f"{p}_{s}_ms": round(f(t[p]), 4) for p in t for s, f in (("median", statistics.median), ("min", min), ("max", max))},
                         "kernels": names, "valu_spread_ms": round(spread, 4), "matrix_cores_win": bool(med["mfma"] < med["valu"] - spread)})
        del x, y
        torch.cuda.empty_cache()
force(None)
print(json.dumps({"tool": "lwe_linear_bench", "kind": "lwe1", "W": W, "runs": args.runs, "reps": args.reps, "throughput": throughput,
                  "dispatch": dispatch}))
