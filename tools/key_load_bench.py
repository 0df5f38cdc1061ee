"""Loading the DEFAULT_128 bootstrap key in float form against standard (integer) form, in one process on one key:

  float   wall time of spf_load_bootstrap_key (host spectra -> HBM, scaled copy): unchanged code, the baseline
  std     wall time of spf_load_bootstrap_key_std (host words -> HBM, transform in place, scaled copy)
  kernel  the transform alone (spf_poly_fft_dev in place over the key blob), hipEvents on the launch stream
  h2d     the host-to-device copy of the key's 83.5 MB alone (spf_device_upload into a scratch buffer)

five repeats each, interleaved; prints a markdown table (kept in profiles/r07_standard_keys.md) with the kernel's achieved bytes
per second (the key is read once and written once).  The key words are uniform: timing does not need an honest key, and the
transform's work does not depend on the values.

usage: python tools/key_load_bench.py [--repeats 5] [--device 0]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import spf_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch

    P = spf_amd.DEFAULT_128
    eng = spf_amd.Engine(P, device=args.device)
    rng = np.random.default_rng(0x10AD)
    words = rng.integers(0, 1 << 64, 2 * P.bsk_complex, dtype=np.uint64)
    n_polys = words.size // P.polynomial_degree
    eng.load_bootstrap_key_std(words)                      # the spectra of these words, for the float loader
    ptr, nbytes = eng.key_blob(0)
    spectra = np.empty(P.bsk_complex, dtype=np.complex128)
    eng.device_download(None, spectra, ptr)
    scratch = eng.device_alloc(nbytes)
    stream = torch.cuda.current_stream(args.device).cuda_stream
    rows = {"float": [], "std": [], "kernel": [], "h2d": []}
    for _ in range(args.repeats + 1):                      # the first round warms up and is dropped
        t = time.perf_counter(); eng.load_bootstrap_key(spectra); rows["float"].append(time.perf_counter() - t)       # noqa: E702
        t = time.perf_counter(); eng.load_bootstrap_key_std(words); rows["std"].append(time.perf_counter() - t)        # noqa: E702
        t = time.perf_counter(); eng.device_upload(scratch, words); rows["h2d"].append(time.perf_counter() - t)        # noqa: E702
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.device_upload(scratch, words)                  # (integer words again: the transform of spectra read as words is as much work)
        torch.cuda.synchronize(args.device)
        e0.record()
        eng.poly_fft_dev(stream, n_polys, scratch, scratch)
        e1.record()
        torch.cuda.synchronize(args.device)
        rows["kernel"].append(e0.elapsed_time(e1) * 1e-3)
    eng.device_free(scratch)
    print(f"device: {torch.cuda.get_device_name(args.device)}; key: {nbytes} bytes, {n_polys} polynomials; {args.repeats} repeats after one warm-up\n")
    print("| step | " + " | ".join(f"run {i + 1} (ms)" for i in range(args.repeats)) + " | min | median | spread (max - min) |")
    print("|---|" + "---|" * (args.repeats + 3))
    for name in ("float", "std", "kernel", "h2d"):
        v = np.array(rows[name][1:]) * 1e3
        print(f"| {name} | " + " | ".join(f"{x:.3f}" for x in v) + f" | {v.min():.3f} | {np.median(v):.3f} | {v.max() - v.min():.3f} |")
    k = np.median(rows["kernel"][1:])
    print(f"\nkernel: {2 * nbytes / k / 1e9:.1f} GB/s (reads {nbytes} bytes, writes {nbytes} bytes in {k * 1e3:.3f} ms)")
    print(f"h2d copy: {nbytes / np.median(rows['h2d'][1:]) / 1e9:.2f} GB/s from pageable host memory")
    d = (np.median(rows["std"][1:]) - np.median(rows["float"][1:])) * 1e3
    print(f"std - float (medians): {d:+.3f} ms; kernel median {k * 1e3:.3f} ms")
    eng.close()


if __name__ == "__main__":
    main()
