// spf_glwe_poly.hpp — plaintext polynomial linear maps over GLWE ciphertexts: `glwe_polynomial_mad`, `glwe_scalar_mad`,
// `sub_glwe_ciphertexts`, `glwe_negate_inplace` and `glwe_rotate` (sunscreen_tfhe ops/ciphertext/glwe_ciphertext_ops.rs:164-183,
// :189-202, :121-141, :147-156, :285-305; the product is `polynomial_external_mad`, math/polynomial.rs:114-197) for ANY matrix of
// sparse plaintext polynomials, in R = Z_2^64[X]/(X^N + 1):
//
//   out[b][m][p] = sum_{k < K} w[m][k] * in[b][k][p]      p = 0 .. glwe_size (the mask polynomials, then the body)
//   out[b][m][glwe_size] += bias[m]                        bias[m] a plaintext polynomial of N words, optional
//
// in [B][K][(k+1) N], out [B][M][(k+1) N]; w[m][k] = sum of coefficient * X^exponent over its terms, the matrix in CSR form over
// the M K polynomials (spf_glwe_poly_plan.hpp: offsets [M K + 1], terms of 16 bytes).  Wrapping 64-bit integers, no floating point.
// A term c X^e sends coefficient i of the operand to coefficient i + e, negated once it passes N:
//   (c X^e * x)[j] = c x[j - e] for j >= e,   -c x[N + j - e] for j < e       (e < N)
//
// Runtime-generic in N (a power of two, 16 .. 2048) and glwe_size: one code path for the tuned and the generic parameter sets.
//
// Two kernels for a batch of contiguous items (glwe_poly_lds_kernel, glwe_poly_stream_kernel) and their two twins for operands
// where they lie, through a pointer table (glwe_poly_lds_rows_kernel, glwe_poly_stream_rows_kernel: a level of a gate graph).
#pragma once

#include "spf_glwe_poly_plan.hpp"

#include <hip/hip_runtime.h>

namespace spf {

constexpr int GLWE_POLY_VT = 4;       // output rows per workgroup, of both kernels
constexpr int GLWE_POLY_MAX_N = 2048; // the LDS image of one operand polynomial: 16 KiB
constexpr int GLWE_POLY_CPT = GLWE_POLY_MAX_N / 256; // coefficients a thread holds of one output polynomial
struct GlwePolyArgs {
    const uint64_t* in;                // [items][K][(k+1) N]
    const uint32_t* offsets;           // [M K + 1]
    const spf_glwe_poly::Term* terms;  // [T]
    const uint64_t* scalars;           // [M][K], constants-only slots (the stream kernel); else null
    const uint64_t* bias;              // [M][N], or null
    uint64_t* out;                     // [items][M][(k+1) N]
    uint32_t M, K, N, glwe_size;
};

// ---- the general kernel.  A workgroup owns GLWE_POLY_VT output rows of ONE polynomial p of one item; thread t holds their
// coefficients j = t + 256 i.  For each k the operand polynomial in[b][k][p] is staged into LDS once (16-byte global loads and
// LDS stores where the caller's pointer allows) and read by every term of the VT polynomials w[m][k]: lanes read consecutive
// 8-byte words whatever e is ((j - e) mod N is consecutive in j), so the reads are conflict-free.  Offsets, exponents and
// coefficients depend on the workgroup and the loop counters only: scalar loads.  A k at which every polynomial of the tile is
// empty is not staged (a uniform test).  The bias rides along in the body's workgroups.
// grid (items, ceil(M / GLWE_POLY_VT), glwe_size + 1)
__global__ __launch_bounds__(256) void glwe_poly_lds_kernel(GlwePolyArgs a)
{
    __shared__ __attribute__((aligned(16))) uint64_t x[GLWE_POLY_MAX_N];
    const uint32_t tid = threadIdx.x, m0 = blockIdx.y * GLWE_POLY_VT, p = blockIdx.z, N = a.N, mask = N - 1;
    const size_t b = blockIdx.x, W = (size_t)(a.glwe_size + 1) * N;
    const uint64_t* src = a.in + b * a.K * W + (size_t)p * N;
    const bool wide = ((uintptr_t)src & 15) == 0; // W is a multiple of 16 words: the same for every k
    uint64_t acc[GLWE_POLY_VT][GLWE_POLY_CPT];
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++)
#pragma unroll
        for (int i = 0; i < GLWE_POLY_CPT; i++) acc[t][i] = 0;

    for (uint32_t k = 0; k < a.K; k++) {
        uint32_t beg[GLWE_POLY_VT], end[GLWE_POLY_VT];
        bool any = false;
#pragma unroll
        for (int t = 0; t < GLWE_POLY_VT; t++) {
            const uint32_t m = m0 + t < a.M ? m0 + t : a.M - 1;
            beg[t] = a.offsets[(size_t)m * a.K + k];
            end[t] = m0 + t < a.M ? a.offsets[(size_t)m * a.K + k + 1] : beg[t];
            any |= end[t] > beg[t];
        }
        if (!any) continue;
        __syncthreads(); // the reads of the previous operand are done
        const uint64_t* xk = src + (size_t)k * W;
        if (wide) {
            for (uint32_t j = 2 * tid; j < N; j += 512)
                *reinterpret_cast<ulonglong2*>(x + j) = *reinterpret_cast<const ulonglong2*>(xk + j);
        } else {
            for (uint32_t j = tid; j < N; j += 256) x[j] = xk[j];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < GLWE_POLY_VT; t++) {
            // (fetching four terms a round ahead of their products was measured and is no faster: profiles/r28_glwe_poly_linear.md)
            for (uint32_t q = beg[t]; q < end[t]; q++) {
                const spf_glwe_poly::Term term = a.terms[q];
                const uint64_t c = term.coefficient;
                const uint32_t e = term.exponent;
#pragma unroll
                for (int i = 0; i < GLWE_POLY_CPT; i++) {
                    const uint32_t j = tid + 256u * i;
                    if (256u * i < N) { // (uniform; lanes j >= N of a degree below 256 compute on words of the image and store nothing)
                        const uint64_t v = c * x[(j - e) & mask];
                        acc[t][i] += j < e ? 0 - v : v;
                    }
                }
            }
        }
    }
    const bool body = p == a.glwe_size && a.bias != nullptr;
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++) {
        const uint32_t m = m0 + t;
        uint64_t* dst = a.out + (b * a.M + m) * W + (size_t)p * N;
#pragma unroll
        for (int i = 0; i < GLWE_POLY_CPT; i++) {
            const uint32_t j = tid + 256u * i;
            if (m < a.M && j < N) dst[j] = acc[t][i] + (body ? a.bias[(size_t)m * N + j] : 0);
        }
    }
}

// ---- slots whose every exponent is 0 (scalar weights: weighted sums, subtraction, negation, and `glwe_rotate` through the
// bias): no rotation, so no LDS.  A workgroup owns GLWE_POLY_VT output rows x 256 words of one item; every input word fetched
// (coalesced across the 256 columns) is used for all its rows, as in lwe_linear_valu_kernel; the weights are the dense [M][K] words
// the load summed out of the terms, workgroup-uniform.  The bias polynomial is added to the body's words.
// grid (items, ceil(M / GLWE_POLY_VT), ceil((k+1) N / 256))
__global__ __launch_bounds__(256) void glwe_poly_stream_kernel(GlwePolyArgs a)
{
    const uint32_t m0 = blockIdx.y * GLWE_POLY_VT, W = (a.glwe_size + 1) * a.N, col = blockIdx.z * 256 + threadIdx.x;
    const size_t b = blockIdx.x;
    const bool live = col < W;
    const uint64_t* x = a.in + b * a.K * W + (live ? col : 0);
    const uint64_t* wr[GLWE_POLY_VT];
    uint64_t sum[GLWE_POLY_VT];
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++) {
        wr[t] = a.scalars + (size_t)(m0 + t < a.M ? m0 + t : a.M - 1) * a.K;
        sum[t] = 0;
    }
#pragma unroll 4
    for (uint32_t k = 0; k < a.K; k++) {
        const uint64_t xv = x[(size_t)k * W];
#pragma unroll
        for (int t = 0; t < GLWE_POLY_VT; t++) sum[t] += xv * wr[t][k];
    }
    if (!live) return;
    const uint32_t body0 = a.glwe_size * a.N;
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++)
        if (m0 + t < a.M) {
            if (a.bias && col >= body0) sum[t] += a.bias[(size_t)(m0 + t) * a.N + (col - body0)];
            a.out[(b * a.M + m0 + t) * W + col] = sum[t];
        }
}

// ---- the same two products over operands where they lie (a level of a gate graph, spf_graph.hpp): layer b reads its K GLWEs
// through row b of a pointer table and writes its M GLWEs contiguously.  The pointer of step k is workgroup-uniform like the
// offsets and the weights (a scalar load), as in lwe_linear_rows_kernel.  The GLWEs of a graph's arena start on 16 bytes (its
// blocks on 256, a GLWE is a multiple of 128 bytes at N >= 16; the host checks the base): the 16-byte staging only.
struct GlwePolyRowsArgs {
    const uint64_t* const* rows;       // [layers][K] device pointers to GLWEs of (k+1) N words, 16-byte aligned
    const uint32_t* offsets;           // [M K + 1]
    const spf_glwe_poly::Term* terms;  // [T]
    const uint64_t* scalars;           // [M][K], constants-only slots (the stream kernel); else null
    const uint64_t* bias;              // [M][N], or null
    uint64_t* out;                     // [layers][M][(k+1) N]
    uint32_t M, K, N, glwe_size;
};

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
typedef const u64x2_t __attribute__((address_space(1))) GlwePolyPair; // two coefficients of an operand, in global memory

// The body of glwe_poly_lds_kernel; the operand polynomial of step k is rows[layer K + k] + p N.  The pointer is loaded only for a
// k that is staged: a tile that is empty at k does not touch the table.
// grid (layers, ceil(M / GLWE_POLY_VT), glwe_size + 1)
__global__ __launch_bounds__(256) void glwe_poly_lds_rows_kernel(GlwePolyRowsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint64_t x[GLWE_POLY_MAX_N];
    const uint32_t tid = threadIdx.x, m0 = blockIdx.y * GLWE_POLY_VT, p = blockIdx.z, N = a.N, mask = N - 1;
    const size_t b = blockIdx.x, W = (size_t)(a.glwe_size + 1) * N;
    const uint64_t* const* rows = a.rows + b * a.K;
    uint64_t acc[GLWE_POLY_VT][GLWE_POLY_CPT];
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++)
#pragma unroll
        for (int i = 0; i < GLWE_POLY_CPT; i++) acc[t][i] = 0;

    for (uint32_t k = 0; k < a.K; k++) {
        uint32_t beg[GLWE_POLY_VT], end[GLWE_POLY_VT];
        bool any = false;
#pragma unroll
        for (int t = 0; t < GLWE_POLY_VT; t++) {
            const uint32_t m = m0 + t < a.M ? m0 + t : a.M - 1;
            beg[t] = a.offsets[(size_t)m * a.K + k];
            end[t] = m0 + t < a.M ? a.offsets[(size_t)m * a.K + k + 1] : beg[t];
            any |= end[t] > beg[t];
        }
        if (!any) continue;
        __syncthreads(); // the reads of the previous operand are done
        // (a pointer fetched from memory is generic to the compiler: the view pins it to global, a global_load that counts on
        // vmcnt alone where a flat_load would count on lgkmcnt too, under the LDS stores)
        const GlwePolyPair* xk = (const GlwePolyPair*)(uintptr_t)(rows[k] + (size_t)p * N);
        for (uint32_t j = 2 * tid; j < N; j += 512) *reinterpret_cast<u64x2_t*>(x + j) = xk[j >> 1];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < GLWE_POLY_VT; t++) {
            for (uint32_t q = beg[t]; q < end[t]; q++) {
                const spf_glwe_poly::Term term = a.terms[q];
                const uint64_t c = term.coefficient;
                const uint32_t e = term.exponent;
#pragma unroll
                for (int i = 0; i < GLWE_POLY_CPT; i++) {
                    const uint32_t j = tid + 256u * i;
                    if (256u * i < N) { // (uniform, as above)
                        const uint64_t v = c * x[(j - e) & mask];
                        acc[t][i] += j < e ? 0 - v : v;
                    }
                }
            }
        }
    }
    const bool body = p == a.glwe_size && a.bias != nullptr;
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++) {
        const uint32_t m = m0 + t;
        uint64_t* dst = a.out + (b * a.M + m) * W + (size_t)p * N;
#pragma unroll
        for (int i = 0; i < GLWE_POLY_CPT; i++) {
            const uint32_t j = tid + 256u * i;
            if (m < a.M && j < N) dst[j] = acc[t][i] + (body ? a.bias[(size_t)m * N + j] : 0);
        }
    }
}

// The body of glwe_poly_stream_kernel with rows[layer K + k][col]; the k loop is unrolled by 4, so the next pointers are in flight
// under the row load.
// grid (layers, ceil(M / GLWE_POLY_VT), ceil((k+1) N / 256))
__global__ __launch_bounds__(256) void glwe_poly_stream_rows_kernel(GlwePolyRowsArgs a)
{
    const uint32_t m0 = blockIdx.y * GLWE_POLY_VT, W = (a.glwe_size + 1) * a.N, col = blockIdx.z * 256 + threadIdx.x;
    const size_t b = blockIdx.x;
    const bool live = col < W;
    const uint32_t c = live ? col : 0;
    const uint64_t* const* rows = a.rows + b * a.K;
    const uint64_t* wr[GLWE_POLY_VT];
    uint64_t sum[GLWE_POLY_VT];
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++) {
        wr[t] = a.scalars + (size_t)(m0 + t < a.M ? m0 + t : a.M - 1) * a.K;
        sum[t] = 0;
    }
#pragma unroll 4
    for (uint32_t k = 0; k < a.K; k++) {
        const uint64_t xv = rows[k][c];
#pragma unroll
        for (int t = 0; t < GLWE_POLY_VT; t++) sum[t] += xv * wr[t][k];
    }
    if (!live) return;
    const uint32_t body0 = a.glwe_size * a.N;
#pragma unroll
    for (int t = 0; t < GLWE_POLY_VT; t++)
        if (m0 + t < a.M) {
            if (a.bias && col >= body0) sum[t] += a.bias[(size_t)(m0 + t) * a.N + (col - body0)];
            a.out[((size_t)b * a.M + m0 + t) * W + col] = sum[t];
        }
}

} // namespace spf
