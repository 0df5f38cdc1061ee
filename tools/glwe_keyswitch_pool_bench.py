#!/usr/bin/env python3
"""The GLWE keyswitch, one automorphism round and the trace in the pool (spf_pool_submit_glwe_*_v, spf_pool_submit_glwe_*) on
DEFAULT_128 with keys of uniform words from a fixed seed (timing only; the words are tested in tests/test_gpu_glwe_keyswitch_pool.py).

  1  by handle, SCATTERED operands, B = 64 and 256, the three operations: the rows route (one launch_glwe_ks_rows over the pointer
     table) against the gather route of the same build (gather_rows_kernel into the set's rows, then the in-place kernel:
     SPF_GLWE_KS_ROWS_GATHER=1 when the pool is made) — two pools on one engine.  One thread pushes the B operations; the clock runs
     from the wait for the last value, which closes the batch, to its return: table, launches, kernels, completion.
  2  blocking callers: 64 and 256 native threads (tools/glwe_keyswitch_pool_driver.cpp), each submit + wait on one ciphertext,
     of the trace and of a keyswitch, by handle and by host pointer, against spf_glwe_*_enqueue + synchronise on as many
     device-resident rows; operations per second, and the operations per launch the pool reached.
  3  the same callers of a keyswitch by handle over FOUR slots (caller t: slot t mod 4): a launch holds one slot, so a pool cycle is
     four launches — their count per cycle and the time per launch.  Beside it the MIXED leg: a second pool with
     spf_pool_set_mixed_parameters, the same callers over one slot and over four — the four slots of a cycle are then one launch of
     glwe_ks_each_kernel.  At 64 callers also a 32-index SampleExtract cycle (caller t: index t mod 32) on both pools.
  4  trace batches by handle: ms per batch of the size a pool cycle holds (the `heavy` decision of spf_ops.hpp).

Forms alternate in one process: one warm-up of each, then `repeats` timed runs of each in turn; median (min - max).
usage: python tools/glwe_keyswitch_pool_bench.py [repeats] [seconds per run of part 2 and 3] [slots]      (default 7, 0.3; "slots":
part 3 alone)
Prints one JSON line."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (device rows of the enqueue forms)

import spf_amd  # noqa: E402
from spf_amd import FheOp, ValueKind  # noqa: E402

repeats = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.3
only_slots = len(sys.argv) > 3 and sys.argv[3] == "slots"
P = spf_amd.DEFAULT_128
N, K1 = P.polynomial_degree, P.glwe_size + 1
W = K1 * N
LOGN = N.bit_length() - 1
OPS = {"keyswitch": (FheOp.GLWE_KEYSWITCH, 0), "automorphism": (FheOp.GLWE_AUTOMORPHISM, 2), "trace": (FheOp.GLWE_TRACE, 0)}


def summary(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def driver():
    libdir = os.path.dirname(spf_amd.lib_path())
    out = os.path.join(ROOT, "tools", "bin", "libglwe_keyswitch_pool_driver.so")
    src = os.path.join(ROOT, "tools", "glwe_keyswitch_pool_driver.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "include", "spf_hip.h"))):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", tmp, src,
                        "-L", libdir, "-lspf_hip", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, out)
    spf_amd.load_library()
    d = C.CDLL(out)
    U32P, D = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    d.glwe_ks_drive_v.restype = d.glwe_ks_drive.restype = C.c_long
    d.glwe_ks_drive_v.argtypes = [C.c_void_p, C.c_int, U32P, C.c_size_t, C.c_int, C.c_double, C.POINTER(C.c_void_p), D]
    d.glwe_ks_drive.argtypes = [C.c_void_p, C.c_int, U32P, C.c_size_t, C.c_int, C.c_double, C.c_void_p, C.c_size_t, D]
    return d


def load_keys(eng, rng):
    eng.load_automorphism_key_std(rng.integers(0, 1 << 64, size=(LOGN, P.glwe_size, P.tr_radix_count, K1, N), dtype=np.uint64))
    for slot in range(4):
        eng.load_glwe_keyswitch_key_std(slot, rng.integers(0, 1 << 64, size=(P.glwe_size, 6, K1, N), dtype=np.uint64), 7, 6)


def scattered_values(pool, rows):
    """every row its own upload with another upload in between, taken by descending address: no row lies behind the one before"""
    vals, between = [], []
    for r in rows:
        vals.append(pool.upload(ValueKind.GLWE1, r))
        between.append(pool.upload(ValueKind.GLWE1, r))
    vals.sort(key=lambda v: -v.device_ptr())
    ptrs = [v.device_ptr() for v in vals]
    assert all(ptrs[i + 1] != ptrs[i] + 8 * W for i in range(len(ptrs) - 1))
    return vals, between


def one_batch(pool, op, param, vals):
    """push one operation per value, then the clock around the wait that closes and runs the batch: ms"""
    outs = [pool.push_v(op, [v], param) for v in vals]
    t0 = time.perf_counter()
    outs[-1].wait()
    ms = (time.perf_counter() - t0) * 1e3
    for o in outs:
        o.release()
    return ms


def part1(eng, rng):
    os.environ.pop("SPF_GLWE_KS_ROWS_GATHER", None)
    pools = {"rows": spf_amd.Pool(eng, max_batch=1024, max_wait_us=1_000_000)}
    os.environ["SPF_GLWE_KS_ROWS_GATHER"] = "1"
    pools["gather"] = spf_amd.Pool(eng, max_batch=1024, max_wait_us=1_000_000)
    os.environ.pop("SPF_GLWE_KS_ROWS_GATHER", None)
    out = []
    for B in (64, 256):
        rows = rng.integers(0, 1 << 64, size=(B, W), dtype=np.uint64)
        held = {f: scattered_values(p, rows) for f, p in pools.items()}
        for name, (op, param) in OPS.items():
            ms, kernels = {"rows": [], "gather": []}, {}
            for f, p in pools.items():      # warm-up: sets and tables sized, and which kernel the route runs
                one_batch(p, op, param, held[f][0])
                one_batch(p, op, param, held[f][0])
                kernels[f] = eng.last_glwe_keyswitch_kernel()
            before = {f: p.counters() for f, p in pools.items()}
            for _ in range(repeats):
                for f, p in pools.items():
                    ms[f].append(one_batch(p, op, param, held[f][0]))
            launches = {f: p.counters()["handle_launches"] - before[f]["handle_launches"] for f, p in pools.items()}
            r, g = summary(ms["rows"]), summary(ms["gather"])
            out.append({"op": name, "B": B, "rows_ms": r, "gather_ms": g, "kernels": kernels, "pool_batches": launches,
                        "rows_over_gather": round(r["median"] / g["median"], 3),
                        # the rule of the issue: rows stays the default unless its median is above gather's by more than the ranges overlap
                        "keep_rows": bool(r["median"] <= g["median"] or r["min"] <= g["max"])})
        for vals, between in held.values():
            for v in vals + between:
                v.release()
    for p in pools.values():
        p.close()
    return out


def part2_3_4(eng, rng, d):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    glwe = rng.integers(0, 1 << 64, size=W, dtype=np.uint64)
    one = (C.c_uint32 * 1)(0)
    four = (C.c_uint32 * 4)(0, 1, 2, 3)
    thirty_two = (C.c_uint32 * 32)(*range(32))
    callers_out, slots_out, batch_out = [], [], []
    for T in (64, 256):
        pool = spf_amd.Pool(eng, max_batch=4096, max_wait_us=200)
        vals = pool.upload_batch(ValueKind.GLWE1, rng.integers(0, 1 << 64, size=(T, W), dtype=np.uint64))
        arr = (C.c_void_p * T)(*[v._h for v in vals])
        x = torch.zeros(T * W, dtype=torch.int64, device=dev)
        y = torch.zeros(T * W, dtype=torch.int64, device=dev)
        el = C.c_double()

        def by_handle(op, params, n, pool=pool, arr=arr):
            before = pool.counters()
            done = d.glwe_ks_drive_v(pool._h, int(op), params, n, T, seconds, arr, C.byref(el))
            assert done > 0, done
            after = pool.counters()
            ops, launches = after["handle_ops"] - before["handle_ops"], after["handle_launches"] - before["handle_launches"]
            return {"ops_per_s": done / el.value, "ops_per_launch": ops / max(launches, 1), "launches": launches, "ops": ops, "elapsed_s": el.value}

        def by_pointer(op, params, n):
            before = pool.counters()
            done = d.glwe_ks_drive(pool._h, int(op), params, n, T, seconds, glwe.ctypes.data_as(C.c_void_p), W, C.byref(el))
            assert done > 0, done
            after = pool.counters()
            ops = after["ops"] - before["ops"]
            return {"ops_per_s": done / el.value, "ops_per_launch": ops / max(after["launches"] - before["launches"], 1)}

        def resident(op):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            while time.perf_counter() - t0 < seconds / 4:
                if op == FheOp.GLWE_TRACE:
                    eng.glwe_trace_enqueue(stream, T, x.data_ptr(), y.data_ptr())
                else:
                    eng.glwe_keyswitch_enqueue(stream, 0, T, x.data_ptr(), y.data_ptr())
                torch.cuda.synchronize()
                n += 1
            return {"ops_per_s": n * T / (time.perf_counter() - t0)}

        for name in () if only_slots else ("trace", "keyswitch"):
            op, _ = OPS[name]
            forms = {"by_handle": lambda: by_handle(op, one, 1), "by_host_pointer": lambda: by_pointer(op, one, 1), "device_resident_enqueue": lambda: resident(op)}
            got = {f: [] for f in forms}
            for f, run in forms.items():
                run()
            for _ in range(repeats):
                for f, run in forms.items():
                    got[f].append(run())
            row = {"op": name, "callers": T}
            for f in forms:
                row[f] = {"ops_per_s": summary([g["ops_per_s"] for g in got[f]], 0)}
                if f != "device_resident_enqueue":
                    row[f]["ops_per_launch"] = round(statistics.median(g["ops_per_launch"] for g in got[f]), 1)
            res = row["device_resident_enqueue"]["ops_per_s"]["median"]
            row["by_handle_over_resident"] = round(row["by_handle"]["ops_per_s"]["median"] / res, 3)
            row["by_host_pointer_over_resident"] = round(row["by_host_pointer"]["ops_per_s"]["median"] / res, 3)
            callers_out.append(row)
        # part 3: four slots against one
        mixed = spf_amd.Pool(eng, max_batch=4096, max_wait_us=200)
        mixed.set_mixed_parameters(True)
        mvals = mixed.upload_batch(ValueKind.GLWE1, rng.integers(0, 1 << 64, size=(T, W), dtype=np.uint64))
        marr = (C.c_void_p * T)(*[v._h for v in mvals])
        forms = {"one_slot": lambda: by_handle(FheOp.GLWE_KEYSWITCH, one, 1), "four_slots": lambda: by_handle(FheOp.GLWE_KEYSWITCH, four, 4),
                 "one_slot_mixed": lambda: by_handle(FheOp.GLWE_KEYSWITCH, one, 1, mixed, marr),
                 "four_slots_mixed": lambda: by_handle(FheOp.GLWE_KEYSWITCH, four, 4, mixed, marr)}
        if T == 64:   # the 32 SampleExtract(i) of a 32-bit unpack (caller t: index t mod 32), without mixing and with it
            forms["sample_extract_32"] = lambda: by_handle(FheOp.SampleExtract, thirty_two, 32)
            forms["sample_extract_32_mixed"] = lambda: by_handle(FheOp.SampleExtract, thirty_two, 32, mixed, marr)
        got = {f: [] for f in forms}
        for f, run in forms.items():
            run()
        for _ in range(repeats):
            for f, run in forms.items():
                got[f].append(run())
        row = {"callers": T}
        for f in forms:
            row[f] = {"ops_per_s": summary([g["ops_per_s"] for g in got[f]], 0),
                      # a cycle: every caller served once
                      "launches_per_cycle": summary([g["launches"] / (g["ops"] / T) for g in got[f]], 2),
                      "ms_per_launch": summary([1e3 * g["elapsed_s"] / g["launches"] for g in got[f]], 4),
                      "ms_per_cycle": summary([1e3 * g["elapsed_s"] / (g["ops"] / T) for g in got[f]], 4)}
        row["four_over_one_ops_per_s"] = round(row["four_slots"]["ops_per_s"]["median"] / row["one_slot"]["ops_per_s"]["median"], 3)
        row["four_mixed_over_one_ops_per_s"] = round(row["four_slots_mixed"]["ops_per_s"]["median"] / row["one_slot"]["ops_per_s"]["median"], 3)
        row["one_mixed_over_one_ops_per_s"] = round(row["one_slot_mixed"]["ops_per_s"]["median"] / row["one_slot"]["ops_per_s"]["median"], 3)
        slots_out.append(row)
        for v in vals + mvals:
            v.release()
        pool.close()
        mixed.close()
        if only_slots:
            continue
        # part 4: a trace batch of T by handle, consecutive operands (close -> done), and the kernel alone by device events
        pool = spf_amd.Pool(eng, max_batch=4096, max_wait_us=1_000_000)
        vals = pool.upload_batch(ValueKind.GLWE1, rng.integers(0, 1 << 64, size=(T, W), dtype=np.uint64))
        one_batch(pool, FheOp.GLWE_TRACE, 0, vals)
        ms = [one_batch(pool, FheOp.GLWE_TRACE, 0, vals) for _ in range(repeats)]
        eng.set_timing(True)
        eng.glwe_trace_enqueue(stream, T, x.data_ptr(), y.data_ptr())
        torch.cuda.synchronize()
        eng.last_kernel_ms("glwe_keyswitch")
        kernel = []
        for _ in range(repeats):
            eng.glwe_trace_enqueue(stream, T, x.data_ptr(), y.data_ptr())
            torch.cuda.synchronize()
            kernel.append(eng.last_kernel_ms("glwe_keyswitch")[0])
        eng.set_timing(False)
        batch_out.append({"B": T, "pool_batch_close_to_done_ms": summary(ms), "trace_kernel_ms": summary(kernel)})
        for v in vals:
            v.release()
        pool.close()
    return callers_out, slots_out, batch_out


def main():
    eng = spf_amd.Engine(P, device=0)
    rng = np.random.default_rng(34)
    load_keys(eng, rng)
    d = driver()
    scattered = [] if only_slots else part1(eng, rng)
    callers, slots, batches = part2_3_4(eng, rng, d)
    print(json.dumps({"tool": "glwe_keyswitch_pool_bench", "repeats": repeats, "seconds_per_run": seconds, "library": spf_amd.lib_path(),
                      "scattered_rows_against_gather": scattered, "blocking_callers": callers, "four_slots": slots, "trace_batches": batches}))
    eng.close()


if __name__ == "__main__":
    main()
