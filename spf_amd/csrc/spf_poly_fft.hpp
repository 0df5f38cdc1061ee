// spf_poly_fft.hpp — the forward transform of batches of full-range torus polynomials: `PolynomialRef::fft`
// (sunscreen_tfhe/src/entities/polynomial.rs:257-274) for every polynomial of a key or ciphertext in standard (integer) form,
// which is all that `BootstrapKey::fft` (entities/bootstrap_key.rs:92-105), `GgswCiphertext::fft` (ggsw_ciphertext.rs:98),
// `AutomorphismKey::fft` (automorphism_key.rs:68) and `SchemeSwitchKey::fft` (scheme_switch_key.rs:174) do: a flat map over the
// polynomials, output block i (N/2 complex bins) from input block i (N words).
//
// A polynomial and its spectrum have the same size (N * 8 = N/2 * 16 bytes) and both kernels hold a whole polynomial in registers
// or LDS before their first store, so `out == in` is allowed: a key is transformed where it was copied to.
//
// N = 2048 (poly_fft2048_kernel): ONE WAVE PER POLYNOMIAL.  The two 512-point transforms of DAG-I (even / odd complex samples) are
// the two members of one `fft512_pair1` on the wave's 8 KiB image; the radix-2 stage X[k] = E[k] +- W1024^k O[k] that the
// two-waves-per-ciphertext kernels spread over a pair of waves stays inside the wave.  Conversion and prologue as in
// scheme_switch_body's `y.a[j] = FFT(x.b)` step: words are (double)(int64_t)w (round to nearest even: key words use all 64 bits),
// then the non-fused twist product.  Memory: lane l reads the 16 bytes of coefficients (128 n1 + 2 l, + 1) — one sample of each
// parity — and writes bin l + 64 r as 16 bytes: every access of a wave is 1 KiB, contiguous.  16 KiB in and 16 KiB out per
// polynomial against ~10 k cycles of arithmetic: the kernel is bound by memory, nothing here schedules arithmetic.
//
// Any other N (generic_poly_fft_kernel): one workgroup per polynomial through generic_poly_fft (spf_generic.hpp), the oracle's
// radix-2 transform for those sizes.
//
// Compiled with -ffp-contract=off like everything else: the only fused operations are DAG-I's own (cmul_tw).
#pragma once

#include "spf_generic.hpp"
#include "spf_kernels.hpp"

namespace spf {

struct PolyFftArgs {
    const uint64_t* in; // n_polys x N words (may alias `out`)
    c64* out;           // n_polys x N/2 bins, canonical order
    const c64* tables;  // kTableEntries
    uint32_t n_polys;
};

constexpr int kPolyFftWaves = 4; // waves (= polynomials in flight) per workgroup
constexpr int kPolyFftLds = kTableBytes + kPolyFftWaves * 8192;

__global__ __launch_bounds__(64 * kPolyFftWaves) void poly_fft2048_kernel(PolyFftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const c64* tab = reinterpret_cast<const c64*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* image = smem + kTableBytes + wv * 8192;
    {
        const double2* src = reinterpret_cast<const double2*>(a.tables);
        double2* dst = reinterpret_cast<double2*>(smem);
        for (int i = tid; i < kTableEntries; i += 64 * kPolyFftWaves) dst[i] = src[i];
    }
    __syncthreads();
    const c64* twist = tab + kTWOff + lane; // TW[par][64 n1 + lane]
    const c64* wc = tab + kWCOff + lane;    // W1024^{lane + 64 r}
    for (uint32_t poly = blockIdx.x * kPolyFftWaves + wv; poly < a.n_polys; poly += gridDim.x * kPolyFftWaves) {
        // (no __restrict__: the two may be the same memory; every load below feeds every store)
        const ulonglong2* x = reinterpret_cast<const ulonglong2*>(a.in + (size_t)poly * kN) + lane;
        c64* y = a.out + (size_t)poly * kHalf + lane;
        // complex sample j = 2 n' + par, n' = 64 n1 + lane: (coefficient j, coefficient j + 1024), twisted
        ulonglong2 lo[8], hi[8];
#pragma unroll
        for (int n1 = 0; n1 < 8; n1++) {
            lo[n1] = x[64 * n1];
            hi[n1] = x[512 + 64 * n1];
        }
        c64 E[8], O[8];
#pragma unroll
        for (int n1 = 0; n1 < 8; n1++) {
            E[n1] = cmul_nf({(double)(long long)lo[n1].x, (double)(long long)hi[n1].x}, twist[64 * n1]);
            O[n1] = cmul_nf({(double)(long long)lo[n1].y, (double)(long long)hi[n1].y}, twist[512 + 64 * n1]);
        }
        fft512_pair1<+1>(E, O, image, tab, lane);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const c64 t = cmul_tw<+1>(O[r], wc[64 * r]);
            y[64 * r] = cadd(E[r], t);
            y[512 + 64 * r] = csub(E[r], t);
        }
    }
}

struct GenericPolyFftArgs {
    GenericShape g;
    const uint64_t* in; // n_polys x N words (may alias `out`)
    c64* out;           // n_polys x N/2 bins
};

// spectrum N/2 c64, and as much again for DAG-I's second image (used at N = 2048 only)
__host__ __device__ inline size_t generic_poly_fft_lds_bytes(uint32_t N) { return (size_t)N * 16; }

__global__ __launch_bounds__(kGenericThreads) void generic_poly_fft_kernel(GenericPolyFftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GenericShape& g = a.g;
    const uint32_t N = g.N, h = N / 2;
    c64* spec = reinterpret_cast<c64*>(smem);
    const uint64_t* x = a.in + (size_t)blockIdx.x * N;
    c64* y = a.out + (size_t)blockIdx.x * h;
    generic_poly_fft(g, spec, spec + h, [&](uint32_t i) { return x[i]; }); // (ends behind a barrier: every word has been read)
    for (uint32_t t = threadIdx.x; t < h; t += kGenericThreads) y[t] = spec[t];
}

} // namespace spf
