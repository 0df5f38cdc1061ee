#!/usr/bin/env python3
"""Ring packing (spf_lwe_ring_pack_enqueue; include/spf_hip.h, "ring packing") on DEFAULT_128 against the two other ways to bring
p LWE ciphertexts into one GLWE, device events around a whole call on one stream:

  a  spf_lwe_ring_pack_enqueue on LWE1 leaves; a call whose scratch would pass 1 GiB is issued in slices of B, as
     spf_lwe_ring_pack_batch issues it
  b  spf_public_functional_keyswitch_enqueue on the same leaves under an 8 x 4-bit and a 4 x 4-bit key (message j to coefficient
     j, not j N / p: the operation ring packing competes with, not the same words)
  c  the same composition through the calls that existed before: spf_glwe_mul_xn_dev (X^x and X^(x+N) = -X^x), spf_glwe_xor_dev,
     spf_glwe_automorphism_enqueue, with the strided operands made contiguous by device copies; it starts from c^(0), which no
     earlier entry point makes (shr_round is done here with torch, untimed).  Only where B p <= --c-limit GLWEs fit.  The outputs
     of a (on GLWE1 leaves) and c are compared word for word.

Candidates alternate in one process: one warm-up of each, then --runs timed runs of each in turn; median (min - max).  Keys and
inputs are uniform numbers from fixed seeds (timing only; the words are tested in tests/test_gpu_lwe_ring_pack.py).
usage: python tools/lwe_ring_pack_bench.py [--shapes 1x32 64x32 1024x32 64x1024 1024x1024] [--runs 5] [--no-pufks]"""
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
ap.add_argument("--shapes", nargs="+", default=["1x32", "64x32", "1024x32", "64x1024", "1024x1024"], help="B x p")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--c-limit", type=int, default=65536, help="route c only where B * p is at most this many GLWEs")
ap.add_argument("--no-pufks", action="store_true")
args = ap.parse_args()

P = spf_amd.DEFAULT_128
N, K1 = P.polynomial_degree, P.glwe_size + 1
W, LW = K1 * N, P.glwe_size * N + 1
LOGN = N.bit_length() - 1
LWE1, GLWE1 = 1, 2
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(36)
rng = np.random.default_rng(36)


def words(*shape):
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, device=dev, dtype=torch.int64)


def make_engine():
    e = spf_amd.Engine(P, device=0)
    e.load_automorphism_key_std(rng.integers(0, 1 << 64, (LOGN, P.glwe_size, P.tr_radix_count, K1, N), dtype=np.uint64))
    return e


eng = make_engine()
pufks = {}
if not args.no_pufks:
    for count in (8, 4):
        e = spf_amd.Engine(P, device=0)
        e.load_public_functional_keyswitch_key_std(rng.integers(0, 1 << 64, (P.glwe_size * N, count, K1, N), dtype=np.uint64), 4, count)
        pufks[f"pufks_{count}x4"] = e


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(forms: dict):
    t = {name: [] for name in forms}
    for call in forms.values():
        timed(call)
    for _ in range(args.runs):
        for name, call in forms.items():
            t[name].append(timed(call))
    return {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for n, v in t.items()}


def ring_pack(kind, p, B, leaves, lw, scratch, out):
    """route a: slices of B under 1 GiB of scratch"""
    per = eng.lwe_ring_pack_scratch_words(p, 1)
    chunk = B if per == 0 else max(1, min(B, (1 << 30) // (per * 8)))
    for at in range(0, B, chunk):
        nb = min(chunk, B - at)
        eng.lwe_ring_pack_enqueue(stream, kind, p, nb, leaves.data_ptr() + at * p * lw * 8, scratch.data_ptr(), scratch.numel(),
                                  out.data_ptr() + at * W * 8)
    return chunk


def composition(p, B, c0, out):
    """route c: c0 (B, p, W) holds c^(0); the tree and the tail through the existing calls"""
    m = p.bit_length() - 1
    cur = c0
    for lvl in range(1, m + 1):
        cnt = p >> lvl
        v = cur.view(B, 2, cnt, W)
        E, Od = v[:, 0].contiguous(), v[:, 1].contiguous()
        n = B * cnt
        pos, neg, r = torch.empty_like(Od), torch.empty_like(Od), torch.empty_like(Od)
        S, D, nxt = torch.empty_like(Od), torch.empty_like(Od), torch.empty_like(Od)
        eng.glwe_mul_xn_dev(stream, n, Od.data_ptr(), N >> lvl, pos.data_ptr())
        eng.glwe_mul_xn_dev(stream, n, Od.data_ptr(), (N >> lvl) + N, neg.data_ptr())
        eng.glwe_xor_dev(stream, n, E.data_ptr(), neg.data_ptr(), D.data_ptr())               # D = E - O
        eng.glwe_xor_dev(stream, n, E.data_ptr(), pos.data_ptr(), S.data_ptr())               # S = E + O
        eng.glwe_automorphism_enqueue(stream, LOGN - lvl + 1, n, D.data_ptr(), r.data_ptr())
        eng.glwe_xor_dev(stream, n, S.data_ptr(), r.data_ptr(), nxt.data_ptr())
        cur = nxt
    x = cur.view(B, W)
    r, y = torch.empty_like(x), torch.empty_like(x)
    for rnd in range(1, LOGN - m + 1):
        eng.glwe_automorphism_enqueue(stream, rnd, B, x.data_ptr(), r.data_ptr())
        eng.glwe_xor_dev(stream, B, x.data_ptr(), r.data_ptr(), y.data_ptr())
        x, y = y, x
    out.copy_(x)
    return 6 * m + 2 * (LOGN - m)


results = []
for shape in args.shapes:
    B, p = (int(v) for v in shape.split("x"))
    m = p.bit_length() - 1
    leaves, out = words(B * p, LW), words(B, W)
    per = eng.lwe_ring_pack_scratch_words(p, 1)
    chunk = B if per == 0 else max(1, min(B, (1 << 30) // (per * 8)))
    scratch = torch.empty(max(1, eng.lwe_ring_pack_scratch_words(p, chunk)), dtype=torch.int64, device=dev)
    forms = {"ring_pack": lambda: ring_pack(LWE1, p, B, leaves, LW, scratch, out)}
    outs = {}
    for name, e in pufks.items():
        outs[name] = torch.empty(B, W, dtype=torch.int64, device=dev)
        forms[name] = (lambda e=e, o=outs[name]: e.public_functional_keyswitch_enqueue(stream, B, p, leaves.data_ptr(), o.data_ptr()))
    row = {"B": B, "p": p, "slices": -(-B // chunk), "scratch_bytes": scratch.numel() * 8}
    with_c = B * p <= args.c_limit
    if with_c:
        gl = words(B, p, W)
        c0 = ((gl >> LOGN) & ((1 << (64 - LOGN)) - 1)) + ((gl >> (LOGN - 1)) & 1)             # polynomial_shr_round on u64 words
        out_a, out_c = torch.empty(B, W, dtype=torch.int64, device=dev), torch.empty(B, W, dtype=torch.int64, device=dev)
        forms["ring_pack_glwe_leaves"] = lambda: ring_pack(GLWE1, p, B, gl, W, scratch, out_a)
        forms["composition_existing_calls"] = lambda: composition(p, B, c0, out_c)
    row["ms"] = alternate(forms)
    eng.set_timing(True)
    eng.last_kernel_ms("lwe_ring_pack")
    ring_pack(LWE1, p, B, leaves, LW, scratch, out)
    torch.cuda.synchronize()
    ms, n = eng.last_kernel_ms("lwe_ring_pack")
    eng.set_timing(False)
    row.update(launches=n, mean_launch_ms=round(ms, 4), kernel=eng.last_lwe_ring_pack_kernel())
    if with_c:
        row["composition_launches"] = composition(p, B, c0, out_c) + 2 * m
        torch.cuda.synchronize()
        row["a_equals_c"] = bool(torch.equal(out_a, out_c))
        row["checksum_a"] = int(out_a.sum().item())
        row["checksum_c"] = int(out_c.sum().item())
        del gl, c0, out_a, out_c
    results.append(row)
    del leaves, out, scratch, outs, forms
    torch.cuda.empty_cache()

print(json.dumps({"tool": "lwe_ring_pack_bench", "N": N, "runs": args.runs, "device": torch.cuda.get_device_name(0),
                  "library": spf_amd.lib_path(), "results": results}))
eng.close()
for e in pufks.values():
    e.close()
