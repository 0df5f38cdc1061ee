#!/usr/bin/env python3
"""spf_glwe_keyswitch_enqueue, spf_glwe_automorphism_enqueue and spf_glwe_trace_enqueue (`keyswitch_glwe_to_glwe`, sunscreen_tfhe
ops/fft_ops.rs:457-495; the trace's round and `trace`, ops/automorphisms/mod.rs:53-85) on DEFAULT_128, device events around the one
launch of a call (spf_last_kernel_ms "glwe_keyswitch"; the shipped fused trace: "trace"):

  1  the trace at B = 4096 against spf_mod_switch_trace_and_rotate_dev at 1024 ciphertexts: 4096 units of eleven rounds in both
  2  the keyswitch and one automorphism round at every --B, each against one eleventh of the trace at the same B; and the keyswitch
     under a 4 x 8-bit key, which a DEFAULT_128 context hands to the generic kernel
  3  today's route for the same values at --host-B items: download, the oracle on the host, upload (wall clock)

Forms alternate on one build: one warm-up of each, then --runs timed runs of each in turn; median (min - max).  Keys and inputs are
uniform numbers from fixed seeds (timing only; the words are tested in tests/test_gpu_glwe_keyswitch.py).
usage: python tools/glwe_keyswitch_bench.py [--B 256 4096] [--trace-B 4096] [--host-B 16] [--runs 7]"""
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
ap.add_argument("--B", type=int, nargs="+", default=[256, 4096])
ap.add_argument("--trace-B", type=int, default=4096, help="units of measurement 1 (the fused kernel runs a quarter as many ciphertexts)")
ap.add_argument("--host-B", type=int, default=16, help="items of the download-oracle-upload route (0: skip it)")
ap.add_argument("--runs", type=int, default=7)
args = ap.parse_args()

P = spf_amd.DEFAULT_128
N, K1 = P.polynomial_degree, P.glwe_size + 1
W = K1 * N
LOGN = N.bit_length() - 1
dev = torch.device("cuda", 0)
eng = spf_amd.Engine(P, device=0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(32)
rng = np.random.default_rng(32)

ak = rng.integers(0, 1 << 64, (LOGN, P.glwe_size, P.tr_radix_count, K1, N), dtype=np.uint64)
eng.load_automorphism_key_std(ak)
eng.load_glwe_keyswitch_key_std(0, np.ascontiguousarray(ak[0]), P.tr_radix_log, P.tr_radix_count)
eng.load_glwe_keyswitch_key_std(1, rng.integers(0, 1 << 64, (P.glwe_size, 4, K1, N), dtype=np.uint64), 8, 4)
eng.set_timing(True)


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


def one(call, timer):
    """the device time of the launches `call` makes, by the library's own events"""
    eng.last_kernel_ms(timer)
    call()
    torch.cuda.synchronize()
    ms, n = eng.last_kernel_ms(timer)
    assert n == 1, (timer, n)
    return ms


def alternate(forms: dict):
    """forms: name -> (call, timer).  One warm-up of each, then the timed runs, forms alternating -> name -> list of ms"""
    t = {name: [] for name in forms}
    for call, timer in forms.values():
        one(call, timer)
    for _ in range(args.runs):
        for name, (call, timer) in forms.items():
            t[name].append(one(call, timer))
    return t


def stats(t: dict) -> dict:
    return {f"{n}_{s}_ms": round(f(v), 5) for n, v in t.items() for s, f in (("median", statistics.median), ("min", min), ("max", max))}


# 1: the trace against the fused kernel, 4096 units of eleven rounds in both
B = args.trace_B
x, y = words(B, W), words(B, W)
cts = B // P.cbs_radix_count
glwe, glev = words(cts, W), words(cts * P.cbs_radix_count, W)
t = alternate({"glwe_trace": (lambda: eng.glwe_trace_enqueue(stream, B, x.data_ptr(), y.data_ptr()), "glwe_keyswitch"),
               "fused_trace": (lambda: eng.mod_switch_trace_and_rotate_dev(stream, cts, glwe.data_ptr(), glev.data_ptr()), "trace")})
trace_vs_fused = {"units": B, "fused_ciphertexts": cts, "kernel": eng.last_glwe_keyswitch_kernel(), **stats(t)}
del glwe, glev

# 2: single rounds against one eleventh of the trace
rounds = []
for B in args.B:
    x, y = words(B, W), words(B, W)
    names = {}

    def ks(slot):
        def call():
            eng.glwe_keyswitch_enqueue(stream, slot, B, x.data_ptr(), y.data_ptr())
            names[slot] = eng.last_glwe_keyswitch_kernel()
        return call
    t = alternate({"trace": (lambda: eng.glwe_trace_enqueue(stream, B, x.data_ptr(), y.data_ptr()), "glwe_keyswitch"),
                   "keyswitch": (ks(0), "glwe_keyswitch"),
                   "automorphism_round1": (lambda: eng.glwe_automorphism_enqueue(stream, 1, B, x.data_ptr(), y.data_ptr()), "glwe_keyswitch"),
                   "automorphism_round11": (lambda: eng.glwe_automorphism_enqueue(stream, LOGN, B, x.data_ptr(), y.data_ptr()), "glwe_keyswitch"),
                   "keyswitch_in_place": (lambda: eng.glwe_keyswitch_enqueue(stream, 0, B, y.data_ptr(), y.data_ptr()), "glwe_keyswitch"),
                   "keyswitch_4x8_generic": (ks(1), "glwe_keyswitch")})
    s = stats(t)
    rounds.append({"B": B, "kernels": {"6x7": names[0], "4x8": names[1]}, **s,
                   "trace_over_11_ms": round(s["trace_median_ms"] / LOGN, 5),
                   "keyswitch_over_trace_eleventh": round(s["keyswitch_median_ms"] / (s["trace_median_ms"] / LOGN), 3),
                   "automorphism_over_trace_eleventh": round(s["automorphism_round1_median_ms"] / (s["trace_median_ms"] / LOGN), 3)})

# 3: today's route: download, the oracle on the host, upload
host = None
if args.host_B:
    import oracle as O
    OP = O.DEFAULT_128
    B = args.host_B
    x, y = words(B, W), words(B, W)
    ak_fft = np.stack([O.poly_fft(p) for p in ak.reshape(-1, N)]).reshape(LOGN, -1)
    buf = np.empty((B, W), dtype=np.uint64)

    def route(fn):
        t = []
        for _ in range(args.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.device_download(None, buf, x.data_ptr())
            out = np.stack([fn(row) for row in buf])
            eng.device_upload(y.data_ptr(), out)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return t[1:]
    th = {"host_trace": route(lambda r: O.trace(r, ak_fft.reshape(-1), OP)),
          "host_keyswitch": route(lambda r: O.keyswitch_glwe_to_glwe(r, ak_fft[0], N, P.glwe_size, P.tr_radix_log, P.tr_radix_count))}
    td = alternate({"gpu_trace": (lambda: eng.glwe_trace_enqueue(stream, B, x.data_ptr(), y.data_ptr()), "glwe_keyswitch"),
                    "gpu_keyswitch": (lambda: eng.glwe_keyswitch_enqueue(stream, 0, B, x.data_ptr(), y.data_ptr()), "glwe_keyswitch")})
    host = {"B": B, **stats(th), **stats(td)}

print(json.dumps({"tool": "glwe_keyswitch_bench", "N": N, "glwe_words": W, "runs": args.runs, "device": torch.cuda.get_device_name(0),
                  "library": spf_amd.lib_path(), "trace_vs_fused": trace_vs_fused, "rounds": rounds, "host_route": host}))
eng.close()
