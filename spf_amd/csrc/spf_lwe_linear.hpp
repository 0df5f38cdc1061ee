// spf_lwe_linear.hpp — plaintext linear maps over LWE ciphertexts: `scalar_mul_ciphertext_mad` then `add_lwe_inplace`
// (sunscreen_tfhe ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18), the two calls `programmable_bootstrap_bivariate` makes for
// its left * 2^bits + right input, for ANY integer matrix:
//
//   out[b][m][c] = sum_{k < K} (uint64_t)w[m][k] * in[b][k][c]      (every word mod 2^64),      out[b][m][W-1] += bias[m]
//
// in [B][K][W], out [B][M][W], one weight matrix [M][K] of int64 for the whole batch; W = n + 1 or k N + 1 words, the body last.
// A batch is the dense wrapping-u64 product [M x K] . [K x (B W)] with small signed integers on the left: the product of
// spf_pfks.hpp with the roles exchanged.  There the small operand (digits) came with the call and the u64 operand (the key) was
// loaded once; here the small operand (the weights) is loaded once and the u64 operand (the ciphertexts) comes with the call.
//
// Matrix-core path.  pfks_gemm_kernel<U> is reused UNCHANGED: its epilogue writes 0 - v, so it is given the limbs of -w.
//   A   [U][Mpad][Kpad] int8   balanced limbs of -w, -w = sum_u 2^(8u) e_u, e_u in [-128, 127]; rows >= M and columns >= K are
//                              zero                                                       (lwe_linear_limbs_kernel, at load)
//   rs  [nseg][U][Mpad] int32  limb sums per K segment                                     (pfks_rowsum_kernel, at load)
//   Bt  [Npad][Kpad]    int8   byte planes of the call's ciphertexts, row 8*(b*W + c) + t = byte t of in[b][k][c] minus 128,
//                              columns k in [K, Kpad) zero                                 (lwe_linear_planes_kernel, per call)
// U limbs hold d = -w iff d in [-128 S_U, 127 S_U], S_U = 1 + 256 + .. + 256^(U-1), i.e. w in [-127 S_U, 128 S_U]:
//   U = 1: [-127, 128]     U = 2: [-32 639, 32 896]     U = 3: [-8 355 711, 8 421 504]
// and the smallest U whose range holds every weight of the matrix is taken (lwe_linear_limbs).  A matrix with a weight outside
// the three-limb range has no limb image: the VALU kernel reads the int64 matrix, which every slot keeps.
// int32 accumulators: |limb| <= 128 and |plane| <= 128, so a sum over S columns is at most S * 2^14 in magnitude; the GEMM folds
// its accumulators into the 64-bit partial sums every kPfksSegRounds * 128 = 130 944 columns, and 130 944 * 2^14 = 2 145 386 496
// < 2^31 = 2 147 483 648, whatever K is.  (The limb sums of a segment are at most 130 944 * 128 < 2^24.)
// The bias is one word per output row: lwe_linear_bias_kernel adds it after the GEMM (B M words against the GEMM's B M W), which
// leaves pfks_gemm_kernel without a second instantiation and the PFKS code objects what they were.
//
// VALU path (weights beyond three limbs, small M, and whatever the first path declines): lwe_linear_valu_kernel; the same product
// over operands that do not lie consecutively (a level of a gate graph, through a pointer table): lwe_linear_rows_kernel.
#pragma once

#include "spf_pfks.hpp"

namespace spf {

constexpr int LWE_LINEAR_VT = 8; // output rows per workgroup of the VALU kernel

// int8 limbs of a matrix whose weights span [lo, hi]; 0: the matrix-core path does not take this matrix
__host__ __device__ inline uint32_t lwe_linear_limbs(long long lo, long long hi)
{
    long long s = 0;
    for (uint32_t u = 1; u <= 3; u++) {
        s = s * 256 + 1;
        if (lo >= -127 * s && hi <= 128 * s) return u;
    }
    return 0;
}

// ---- weight limbs (at load): one workgroup per row of A, padded rows included; every byte of A is written exactly once, the
// padding as zeros.  Four columns per thread and store.
__global__ __launch_bounds__(256) void lwe_linear_limbs_kernel(const long long* w, int8_t* A, uint32_t M, uint32_t Mpad, uint32_t K,
                                                               uint32_t Kpad, uint32_t U)
{
    const uint32_t row = blockIdx.x;
    if (row >= Mpad) return;
    for (uint32_t k4 = 4 * threadIdx.x; k4 < Kpad; k4 += 1024) {
        uint32_t v[3] = {0, 0, 0};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t k = k4 + b;
            long long d = row < M && k < K ? -w[(size_t)row * K + k] : 0; // within the U-limb range: no overflow
#pragma unroll
            for (uint32_t u = 0; u < 3; u++) {
                if (u >= U) break;
                const int e = (int)(int8_t)(d & 0xff); // balanced: e in [-128, 127], d - e a multiple of 256
                v[u] |= (uint32_t)(e & 0xff) << (8 * b);
                d = (d - e) >> 8;
            }
        }
        for (uint32_t u = 0; u < U; u++) *reinterpret_cast<uint32_t*>(A + ((size_t)u * Mpad + row) * Kpad + k4) = v[u];
    }
}

// ---- ciphertext planes (per call).  One workgroup transposes a tile of 64 inputs k x 32 words c of one batch item through LDS:
// the input is read along c (256 contiguous bytes per row of the tile), the image is written 64 bytes per thread along k, as
// four 16-byte stores (Kpad is a multiple of 128 and k0 of 64).  byte - 128 in int8 is byte ^ 0x80.
// grid (Kpad / 64, ceil(W / 32), items of the launch)
__global__ __launch_bounds__(256) void lwe_linear_planes_kernel(const uint64_t* in, int8_t* bt, uint32_t W, uint32_t K, uint32_t Kpad)
{
    __shared__ uint64_t tile[64][33];
    const uint32_t k0 = blockIdx.x * 64, c0 = blockIdx.y * 32, b = blockIdx.z;
    const uint64_t* src = in + (size_t)b * K * W;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int rr = 0; rr < 8; rr++) {
        const uint32_t kl = ty + 8 * rr, k = k0 + kl, col = c0 + tx;
        tile[kl][tx] = k < K && col < W ? src[(size_t)k * W + col] : 0;
    }
    __syncthreads();
    const uint32_t cl = threadIdx.x >> 3, t = threadIdx.x & 7, col = c0 + cl;
    if (col >= W) return;
    uint4* dst = reinterpret_cast<uint4*>(bt + (((size_t)b * W + col) * 8 + t) * Kpad + k0);
#pragma unroll
    for (int g = 0; g < 4; g++) {
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t x = 0;
#pragma unroll
            for (int bb = 0; bb < 4; bb++) {
                const uint32_t kl = 16 * g + 4 * j + bb;
                const uint32_t plane = k0 + kl < K ? ((uint32_t)(tile[kl][cl] >> (8 * t)) & 0xff) ^ 0x80u : 0u;
                x |= plane << (8 * bb);
            }
            v[j] = x;
        }
        dst[g] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// ---- the bias after the GEMM: out[b][m][W-1] += bias[m], one thread per output row
__global__ __launch_bounds__(256) void lwe_linear_bias_kernel(uint64_t* out, const uint64_t* bias, uint32_t M, uint32_t W, size_t rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) out[i * W + (W - 1)] += bias[i % M];
}

// ---- VALU path: a workgroup owns LWE_LINEAR_VT output rows x 256 words of one batch item; every input word fetched (coalesced
// across the 256 columns) is used for all its rows; the weights are workgroup-uniform; plain wrapping 64-bit multiplies.
// grid (ceil(W / 256), ceil(M / LWE_LINEAR_VT), items of the launch)
struct LweLinearValuArgs {
    const uint64_t* in;   // [items][K][W]
    const long long* w;   // [M][K], the first row of this launch's rows
    const uint64_t* bias; // [M] from the same row on, or null
    uint64_t* out;        // [items][M_total][W], at the first row of this launch's rows
    uint32_t M, M_total, K, W;
};

__global__ __launch_bounds__(256) void lwe_linear_valu_kernel(LweLinearValuArgs a)
{
    const uint32_t col = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    const uint32_t m0 = blockIdx.y * LWE_LINEAR_VT;
    const bool live = col < a.W;
    const uint64_t* x = a.in + (size_t)b * a.K * a.W + (live ? col : 0);
    const long long* wr[LWE_LINEAR_VT];
    uint64_t sum[LWE_LINEAR_VT];
#pragma unroll
    for (int t = 0; t < LWE_LINEAR_VT; t++) {
        wr[t] = a.w + (size_t)(m0 + t < a.M ? m0 + t : a.M - 1) * a.K;
        sum[t] = 0;
    }
#pragma unroll 4
    for (uint32_t k = 0; k < a.K; k++) {
        const uint64_t xv = x[(size_t)k * a.W];
#pragma unroll
        for (int t = 0; t < LWE_LINEAR_VT; t++) sum[t] += xv * (uint64_t)wr[t][k];
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < LWE_LINEAR_VT; t++)
        if (m0 + t < a.M) {
            if (a.bias && col == a.W - 1) sum[t] += a.bias[m0 + t];
            a.out[((size_t)b * a.M_total + m0 + t) * a.W + col] = sum[t];
        }
}

// ---- the same product over operands where they lie (a level of a gate graph, spf_graph.hpp): layer q reads its K rows through
// row q of a pointer table and writes its M rows contiguously.  The row pointer of step k is workgroup-uniform like the weights
// (a scalar load); the k loop is unrolled as above, so the pointer of step k + 1 is fetched before the row load of step k returns.
// Layers in grid.x (2^31 - 1 of them), M <= SPF_GRAPH_LWE_LINEAR_MAX_ROWS in grid.y: any group is one launch.
// grid (layers, ceil(M / LWE_LINEAR_VT), ceil(W / 256))
struct LweLinearRowsArgs {
    const uint64_t* const* in_ptrs; // [layers][K] device pointers to rows of W words
    const long long* w;             // [M][K]
    const uint64_t* bias;           // [M], or null
    uint64_t* out;                  // [layers][M][W]
    uint32_t M, K, W;
};

__global__ __launch_bounds__(256) void lwe_linear_rows_kernel(LweLinearRowsArgs a)
{
    const uint32_t col = blockIdx.z * 256 + threadIdx.x, m0 = blockIdx.y * LWE_LINEAR_VT;
    const size_t q = blockIdx.x;
    const bool live = col < a.W;
    const uint32_t c = live ? col : 0;
    const uint64_t* const* rows = a.in_ptrs + q * a.K;
    const long long* wr[LWE_LINEAR_VT];
    uint64_t sum[LWE_LINEAR_VT];
#pragma unroll
    for (int t = 0; t < LWE_LINEAR_VT; t++) {
        wr[t] = a.w + (size_t)(m0 + t < a.M ? m0 + t : a.M - 1) * a.K;
        sum[t] = 0;
    }
#pragma unroll 4
    for (uint32_t k = 0; k < a.K; k++) {
        const uint64_t xv = rows[k][c];
#pragma unroll
        for (int t = 0; t < LWE_LINEAR_VT; t++) sum[t] += xv * (uint64_t)wr[t][k];
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < LWE_LINEAR_VT; t++)
        if (m0 + t < a.M) {
            if (a.bias && col == a.W - 1) sum[t] += a.bias[m0 + t];
            a.out[(q * a.M + m0 + t) * a.W + col] = sum[t];
        }
}

} // namespace spf
