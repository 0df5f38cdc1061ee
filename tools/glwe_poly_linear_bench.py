#!/usr/bin/env python3
"""spf_glwe_poly_linear_enqueue (`glwe_polynomial_mad`, `glwe_scalar_mad`, `sub_glwe_ciphertexts`, `glwe_negate_inplace`,
`glwe_rotate`: sunscreen_tfhe ops/ciphertext/glwe_ciphertext_ops.rs:164-183, :189-202, :121-141, :147-156, :285-305, for a matrix of
sparse plaintext polynomials) on DEFAULT_128's GLWEs (4096 words), device-resident.  Three tables, one JSON line.  Every table
times its forms alternating on one build: one warm-up of each, then --runs timed runs of --reps calls each, between two events on
the launch stream; median (min - max) per form.

constants: constants-only slots (every exponent 0: weighted sums), M = K in --square, B in --B.  Both kernels, forced by
  SPF_GLWE_POLY_PATH; each against the bytes it must move (B (K + M) GLWEs, once each) over the 6.29 TB/s copy ceiling DESIGN uses
  for cmux_kernel; `stream_wins` / `lds_wins`: the median below the other median by more than its own min-max spread.  At
  --host-B items also today's route for the same value: download, numpy (one wrapping uint64 matrix product), upload.
fused: X^3 * x0 + x1 (M = 1, K = 2) in one launch against the same value composed today from spf_glwe_mul_xn_dev and
  spf_glwe_xor_dev (two launches and a temporary), B in --B.
taps: t-tap polynomials (t distinct random exponents, random int64 coefficients) at M = K = 8, B = --taps-B, t in --taps: time per
  call, per term and polynomial read (B (k+1) M K t of them), and the LDS read rate reached, 8 N bytes per such read, against the
  ds_read_b64 rate of 150 TB/s with every CU streaming.
Weights and inputs are uniform numbers from fixed seeds (timing only; the words are tested in tests/test_gpu_glwe_poly_linear.py).
usage: python tools/glwe_poly_linear_bench.py [--square 1 8 64] [--B 1 16 256] [--host-B 16] [--taps 1 4 16 64 2048] [--runs 7] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spf_amd

ap = argparse.ArgumentParser()
ap.add_argument("--square", type=int, nargs="*", default=[1, 8, 64])
ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 256])
ap.add_argument("--host-B", type=int, default=16, help="items of the download-numpy-upload route (0: skip it)")
ap.add_argument("--taps", type=int, nargs="*", default=[1, 4, 16, 64, 2048])
ap.add_argument("--taps-B", type=int, default=64)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

P = spf_amd.DEFAULT_128
N, K1 = P.polynomial_degree, P.glwe_size + 1
W = K1 * N
COPY_CEILING, LDS_CEILING = 6.29e12, 150e12
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(28)


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


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
        os.environ["SPF_GLWE_POLY_PATH"] = path
    else:
        os.environ.pop("SPF_GLWE_POLY_PATH", None)


def alternate(forms: dict):
    """forms: name -> (set-up, call).  One warm-up of each, then the timed runs, forms alternating -> name -> list of ms"""
    t = {name: [] for name in forms}
    for name, (setup, call) in forms.items():
        setup()
        call()
    for _ in range(args.runs):
        for name, (setup, call) in forms.items():
            setup()
            t[name].append(timed(call, args.reps))
    return t


def stats(t: dict) -> dict:
    return {f"{n}_{s}_ms": round(f(v), 5) for n, v in t.items() for s, f in (("median", statistics.median), ("min", min), ("max", max))}


def scalar_csr(w):
    """an (M, K) int64 matrix of constants as the CSR triple: one term X^0 per polynomial"""
    M, K = w.shape
    return np.arange(M * K + 1, dtype=np.uint32), np.zeros(M * K, dtype=np.uint32), np.ascontiguousarray(w.reshape(-1))


constants = []
for S in args.square:
    w = np.random.default_rng([28, S]).integers(-(1 << 63), (1 << 63) - 1, (S, S), dtype=np.int64, endpoint=True)
    eng.load_glwe_poly_weights(0, scalar_csr(w), np.zeros((S, N), dtype=np.uint64), shape=(S, S))
    for B in args.B:
        x, y = words(B, S, W), torch.empty((B, S, W), device=dev, dtype=torch.int64)
        call = lambda: eng.glwe_poly_linear_enqueue(stream, 0, B, x.data_ptr(), y.data_ptr())  # noqa: E731
        t = alternate({"stream": (lambda: force("stream"), call), "lds": (lambda: force("lds"), call)})
        med = {n: statistics.median(v) for n, v in t.items()}
        spread = {n: max(v) - min(v) for n, v in t.items()}
        floor_ms = B * 2 * S * W * 8 / COPY_CEILING * 1e3
        row = {"M": S, "K": S, "B": B, **stats(t), "bytes_floor_ms": round(floor_ms, 5),
               "stream_of_floor": round(floor_ms / med["stream"], 3), "lds_of_floor": round(floor_ms / med["lds"], 3),
               "stream_wins": bool(med["stream"] < med["lds"] - spread["stream"]), "lds_wins": bool(med["lds"] < med["stream"] - spread["lds"])}
        if args.host_B and B == args.host_B:
            wu = w.view(np.uint64)

            def host_route():
                h = x.cpu().numpy().view(np.uint64).reshape(B, S, W)
                out = np.stack([wu @ hb for hb in h])
                y.copy_(torch.from_numpy(out.view(np.int64)))
                torch.cuda.synchronize()
            host_route()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                host_route()
                ts.append((time.perf_counter() - t0) * 1e3)
            row.update({"host_route_median_ms": round(statistics.median(ts), 3), "host_route_min_ms": round(min(ts), 3),
                        "host_route_max_ms": round(max(ts), 3), "host_route_runs": 3})
        constants.append(row)
        del x, y
        torch.cuda.empty_cache()

fused = []
off, exp, coef = np.array([0, 1, 2], dtype=np.uint32), np.array([3, 0], dtype=np.uint32), np.array([1, 1], dtype=np.int64)
eng.load_glwe_poly_weights(1, (off, exp, coef), shape=(1, 2))
force(None)
for B in args.B:
    x, y = words(B, 2, W), torch.empty((B, W), device=dev, dtype=torch.int64)
    x0, x1, tmp = x[:, 0].contiguous(), x[:, 1].contiguous(), torch.empty((B, W), device=dev, dtype=torch.int64)

    def composed():
        eng.glwe_mul_xn_dev(stream, B, x0.data_ptr(), 3, tmp.data_ptr())
        eng.glwe_xor_dev(stream, B, tmp.data_ptr(), x1.data_ptr(), y.data_ptr())
    one = lambda: eng.glwe_poly_linear_enqueue(stream, 1, B, x.data_ptr(), y.data_ptr())  # noqa: E731
    t = alternate({"one_launch": (lambda: None, one), "mul_xn_then_xor": (lambda: None, composed)})
    med = {n: statistics.median(v) for n, v in t.items()}
    fused.append({"B": B, **stats(t), "kernel": eng.last_glwe_poly_kernel(),
                  "one_launch_wins": bool(med["one_launch"] < med["mul_xn_then_xor"] - (max(t["one_launch"]) - min(t["one_launch"])))})
    del x, y, x0, x1, tmp
    torch.cuda.empty_cache()

taps = []
M = K = 8
B = args.taps_B
for T in args.taps:
    rng = np.random.default_rng([28, T])
    exps = np.concatenate([rng.permutation(N)[:T] for _ in range(M * K)]).astype(np.uint32)
    coefs = rng.integers(-(1 << 63), (1 << 63) - 1, M * K * T, dtype=np.int64, endpoint=True)
    eng.load_glwe_poly_weights(2, (np.arange(M * K + 1, dtype=np.uint32) * T, exps, coefs), shape=(M, K))
    x, y = words(B, K, W), torch.empty((B, M, W), device=dev, dtype=torch.int64)
    call = lambda: eng.glwe_poly_linear_enqueue(stream, 2, B, x.data_ptr(), y.data_ptr())  # noqa: E731
    t = alternate({"lds": (lambda: None, call)})
    med = statistics.median(t["lds"])
    reads = B * K1 * M * K * T
    taps.append({"taps": T, "M": M, "K": K, "B": B, **stats(t), "kernel": eng.last_glwe_poly_kernel(),
                 "ns_per_term_and_polynomial": round(med * 1e6 / reads, 3), "lds_read_TB_per_s": round(reads * N * 8 / (med * 1e-3) / 1e12, 2),
                 "of_ds_read_b64_rate": round(reads * N * 8 / (med * 1e-3) / LDS_CEILING, 3)})
    del x, y
    torch.cuda.empty_cache()

print(json.dumps({"tool": "glwe_poly_linear_bench", "N": N, "glwe_words": W, "runs": args.runs, "reps": args.reps, "constants": constants,
                  "fused": fused, "taps": taps}))
