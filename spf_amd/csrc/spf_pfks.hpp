// spf_pfks.hpp — private functional keyswitch (`private_functional_keyswitch`, sunscreen_tfhe
// ops/keyswitch/private_functional_keyswitch.rs:107-142) and the pieces of `circuit_bootstrap_via_pfks`
// (ops/bootstrapping/circuit_bootstrapping.rs:162-252, :485-514) that it adds.
//
//   out = - sum_z sum_{i <= n} sum_{j < count} digit_j(ct_z[i]) * K[z][i][count-1-j]          (every word mod 2^64)
//
// p = lwe_count inputs of n + 1 words (the body is row i = n, decomposed like the mask words; no body is added afterwards), key
// [lwe_count][n+1][count][k+1][N] words.  A batch is a dense product [M x K] . [K x W] in wrapping u64: M output rows,
// K = lwe_count * (n+1) * count digits per row (digit k = (z*(n+1) + i)*count + j: the inputs of one output are consecutive in
// memory, so k = word * count + j), W = (k+1)*N words per key row.  Nothing depends on N or k beyond W: tuned and generic
// contexts run the same kernels.  Pure integer arithmetic: the words are the reference's, bit for bit.
//
// Matrix-core path (radix_log <= 23).  A digit d in [-2^(log-1), 2^(log-1)) is split into U = 1 (log <= 8) or
// U = ceil((log+1)/8) <= 3 balanced int8 limbs, d = sum_u 2^(8u) e_u, e_u in [-128, 127]; then
//   sum_k d_k w_k = sum_u 2^(8u) sum_k e_{k,u} w_k
// and each inner sum is the keyswitch identity of spf_kernels.hpp (key words as eight signed byte planes, byte - 128, the
// 128 * rowsum correction, recombination in wrapping 64-bit):
//   sum_k e_k w_k = sum_t 2^(8t) ( sum_k e_k (byte_{k,t} - 128) + 128 sum_k e_k ).
// Limb u REUSES the one plane image: the GEMM runs U passes over the same Bt tiles with A = limb u, and the pass is shifted by
// 8 (t + u) bits when its int32 sums are folded into the 64-bit partial sums (a shift of 64 or more contributes nothing and is
// skipped).  The image therefore costs 1 x the key's bytes, not U x.
//   A   [U][Mpad][Kpad] int8   limbs, K-contiguous; rows >= M and columns >= K are zero      (pfks_digits_kernel, per launch)
//   rs  [nseg][U][Mpad] int32  limb sums per K segment                                       (pfks_rowsum_kernel, per launch)
//   Bt  [Npad][Kpad]    int8   byte planes of EVERY key of the set, row n = 8*(key*W + col) + t  (pfks_planes_kernel, per load)
// int32 accumulators: |e| <= 128, |plane| <= 128, so a sum over S columns is at most S * 2^14; the accumulators are folded into the
// 64-bit partial sums every kPfksSegRounds * 128 = 130 944 columns (130 944 * 2^14 < 2^31), whatever K is.
//
// VALU path (every other radix, and whatever the first path declines): pfks_valu_kernel, keyswitch_kernel's shape.
#pragma once

#include "spf_kernels.hpp"

namespace spf {

constexpr int PFKS_TILE = 128;            // block tile of the GEMM (rows and plane columns); 4 waves, each 64 x 64
constexpr uint32_t kPfksSegRounds = 1023; // rounds of 128 limb columns between two folds of the int32 accumulators
constexpr int PFKS_VT = 8;                // output rows per workgroup of the VALU kernel

// int8 limbs of a digit of radix_log bits; 0: the matrix-core path does not take this radix
__host__ __device__ inline uint32_t pfks_limbs(uint32_t radix_log)
{
    if (radix_log <= 8) return 1;
    const uint32_t u = (radix_log + 1 + 7) / 8;
    return u <= 3 ? u : 0;
}

// where output row m (= item * rows_per_item + r) of key q and word `col` goes: the single operation has rows_per_item = 1 and
// one key; the GGSW components call places row (item, level) of key q at [item][q][level][col]
struct PfksDest {
    uint64_t* out;
    uint32_t rows_per_item;
    size_t item_stride, row_stride, key_stride; // in words
};

__device__ __forceinline__ uint64_t* pfks_dest(const PfksDest& d, uint32_t m, uint32_t q, uint32_t col)
{
    const uint32_t item = m / d.rows_per_item, r = m % d.rows_per_item;
    return d.out + (size_t)item * d.item_stride + (size_t)r * d.row_stride + (size_t)q * d.key_stride + col;
}

// ---- digits pre-pass: one workgroup per row of A, padded rows included (they are written as zeros, as are the columns from K
// to Kpad: every byte of the launch's A is written exactly once, no clearing pass).  Digits: round (radix.rs:157-162) then
// vector_next_decomp (scalar.rs:52-71), least significant first.
__global__ __launch_bounds__(256) void pfks_digits_kernel(const uint64_t* in, int8_t* dig, uint32_t row_words, uint32_t M, uint32_t Mpad,
                                                          uint32_t radix_log, uint32_t count, uint32_t U, uint32_t K, uint32_t Kpad)
{
    const uint32_t row = blockIdx.x;
    if (row >= Mpad) return;
    if (row >= M) {
        for (uint32_t u = 0; u < U; u++) {
            uint32_t* z = reinterpret_cast<uint32_t*>(dig + ((size_t)u * Mpad + row) * Kpad);
            for (uint32_t i = threadIdx.x; i < Kpad / 4; i += 256) z[i] = 0;
        }
        return;
    }
    const uint64_t* x = in + (size_t)row * row_words;
    const uint32_t shift = 64 - radix_log * count;
    const uint64_t mask = ((uint64_t)1 << radix_log) - 1;
    for (uint32_t i = threadIdx.x; i < row_words; i += 256) {
        const uint64_t v = x[i];
        uint64_t st = (v >> shift) + ((v >> (shift - 1)) & 1);
        for (uint32_t j = 0; j < count; j++) {
            const uint64_t dg = st & mask;
            st >>= radix_log;
            const uint64_t carry = dg >> (radix_log - 1);
            st += carry;
            int digit = (int)dg - (int)(carry << radix_log); // radix_log <= 23 on this path
            for (uint32_t u = 0; u < U; u++) {
                const int e = (int)(int8_t)(digit & 0xff); // balanced: e in [-128, 127], digit - e a multiple of 256
                dig[((size_t)u * Mpad + row) * Kpad + (size_t)i * count + j] = (int8_t)e;
                digit = (digit - e) >> 8;
            }
        }
    }
    for (uint32_t u = 0; u < U; u++)
        for (uint32_t kk = K + threadIdx.x; kk < Kpad; kk += 256) dig[((size_t)u * Mpad + row) * Kpad + kk] = 0;
}

// limb sums of every (segment, limb, row): grid (Mpad, nseg * U), written directly (no atomics, nothing to clear)
__global__ __launch_bounds__(256) void pfks_rowsum_kernel(const int8_t* dig, int* rowsum, uint32_t Mpad, uint32_t U, uint32_t Kpad,
                                                          uint32_t seg_cols)
{
    __shared__ int part[4];
    const uint32_t row = blockIdx.x, su = blockIdx.y, seg = su / U, u = su % U;
    const uint32_t c0 = seg * seg_cols, c1 = min(Kpad, c0 + seg_cols);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(dig + ((size_t)u * Mpad + row) * Kpad);
    int local = 0;
    for (uint32_t i = c0 / 4 + threadIdx.x; i < c1 / 4; i += 256) {
        const uint32_t v = w[i];
        local += (int)(int8_t)(v & 0xff) + (int)(int8_t)((v >> 8) & 0xff) + (int)(int8_t)((v >> 16) & 0xff) + (int)(int8_t)(v >> 24);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) rowsum[(size_t)su * Mpad + row] = part[0] + part[1] + part[2] + part[3];
}

// ---- planes pass (at key load): Bt[8*(q*W + col) + t][zi*count + j] = byte t of K[q][zi][count-1-j][col], minus 128 (GLEV levels
// are consumed in reverse, glev_ciphertext_ops.rs:48-59).  One workgroup transposes a tile of 32 digit columns x 32 key words
// through LDS: the key is read along `col`, the image is written 32 bytes at a time along k.  Columns k in [K, Kpad) get zeros.
// grid (Kpad / 32, ceil(W / 32), n_keys)
__global__ __launch_bounds__(256) void pfks_planes_kernel(const uint64_t* key, int8_t* bt, uint32_t count, uint32_t W, uint32_t K,
                                                          uint32_t Kpad)
{
    __shared__ uint64_t tile[32][33];
    const uint32_t k0 = blockIdx.x * 32, c0 = blockIdx.y * 32, q = blockIdx.z;
    const uint64_t* kq = key + (size_t)q * K * W;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const uint32_t kl = ty + 8 * rr, k = k0 + kl, col = c0 + tx;
        uint64_t word = 0;
        if (k < K && col < W) {
            const uint32_t zi = k / count, j = k % count;
            word = kq[((size_t)zi * count + (count - 1 - j)) * W + col];
        }
        tile[kl][tx] = word;
    }
    __syncthreads();
    const uint32_t cl = threadIdx.x >> 3, t = threadIdx.x & 7, col = c0 + cl;
    if (col >= W) return;
    uint32_t packed[8];
#pragma unroll
    for (int g = 0; g < 8; g++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t kl = 4 * g + b;
            const int plane = k0 + kl < K ? (int)((tile[kl][cl] >> (8 * t)) & 0xff) - 128 : 0;
            v |= (uint32_t)(plane & 0xff) << (8 * b);
        }
        packed[g] = v;
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(bt + ((size_t)(q * W + col) * 8 + t) * Kpad + k0);
#pragma unroll
    for (int g = 0; g < 8; g++) dst[g] = packed[g];
}

// ---- the block GEMM on v_mfma_i32_32x32x32_i8, operand tiles through LDS
struct PfksGemmArgs {
    const int8_t* A;   // [U][Mpad][Kpad]
    const int8_t* Bt;  // the image from the first plane row of this call's first key on
    const int* rowsum; // [nseg][U][Mpad]
    PfksDest dst;
    uint32_t M, Mpad, Kpad;
    uint32_t W, ncols; // words per key row; words of this call (W, or n_keys * W for the components call)
};

// A workgroup (4 waves, 128 x 128 tile, 64 x 64 per wave) stages each 128-row x 128-byte slab of A and of Bt in LDS once per
// round: the slabs of round i+1 are fetched into registers before the 16 MFMAs per wave of round i and stored after them.
// LDS image as in ks_gemm_lds_kernel: 16-byte slot of (row, chunk) = 8 row + (chunk ^ ((row >> 1) & 7)), conflict-free for the
// 16-lane groups of a ds_read_b128.  Lane (r, h) supplies 16 k values of A row r and of B column r per instruction (chunk
// 2q + h of step q for both operands).  U passes (limb u against the same Bt tiles); the int32 accumulators are folded into 64-bit
// partial sums at the end of every K segment and of every pass.
template <int U>
__global__ __launch_bounds__(256) void pfks_gemm_kernel(PfksGemmArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[2 * PFKS_TILE * 128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const size_t Kpad = a.Kpad;
    const uint32_t tm0 = blockIdx.y * PFKS_TILE, tn0 = blockIdx.x * PFKS_TILE;
    const uint32_t rounds = a.Kpad / 128;
    // staging duty of this thread: rows 32 wave + 8 j + (lane >> 3), chunk lane & 7, of the A slab and of the B slab
    size_t goff[4];
    uint32_t loff[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t row = 32 * wave + 8 * j + (lane >> 3), chunk = lane & 7;
        goff[j] = (size_t)row * Kpad + 16 * chunk;
        loff[j] = row * 128 + 16 * (chunk ^ ((row >> 1) & 7));
    }
    const char* gB = reinterpret_cast<const char*>(a.Bt) + (size_t)tn0 * Kpad;
    v4i32 ga[4], gb[4];
    auto fetch = [&](uint32_t it) {
        const uint32_t u = it / rounds, rd = it % rounds;
        const char* pa = reinterpret_cast<const char*>(a.A) + ((size_t)u * a.Mpad + tm0) * Kpad + (size_t)rd * 128;
        const char* pb = gB + (size_t)rd * 128;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            ga[j] = *reinterpret_cast<const v4i32*>(pa + goff[j]);
            gb[j] = *reinterpret_cast<const v4i32*>(pb + goff[j]);
        }
    };
    uint32_t rdA[2], rdB[2], swA[2], swB[2];
#pragma unroll
    for (int blk = 0; blk < 2; blk++) {
        const uint32_t ra = 64 * wm + 32 * blk + r, rb = 64 * wn + 32 * blk + r;
        rdA[blk] = ra * 128; swA[blk] = (ra >> 1) & 7;
        rdB[blk] = PFKS_TILE * 128 + rb * 128; swB[blk] = (rb >> 1) & 7;
    }
    const uint32_t m0 = tm0 + wm * 64, n0 = tn0 + wn * 64;
    const int t = r & 7; // plane of this lane's column (n0 and the 32-column blocks are multiples of 8)
    v16i32 acc[2][2];
    unsigned long long part[2][2][16];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int reg = 0; reg < 16; reg++) { acc[i][j][reg] = 0; part[i][j][reg] = 0; }

    const uint32_t total = (uint32_t)U * rounds;
    fetch(0);
    for (uint32_t it = 0; it < total; it++) {
        __syncthreads(); // everyone is done reading the previous round's slabs
#pragma unroll
        for (int j = 0; j < 4; j++) {
            *reinterpret_cast<v4i32*>(smem + loff[j]) = ga[j];
            *reinterpret_cast<v4i32*>(smem + PFKS_TILE * 128 + loff[j]) = gb[j];
        }
        __syncthreads();
        if (it + 1 < total) fetch(it + 1);
        v4i32 fa[2][4], fb[2][4];
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                fa[blk][q] = *reinterpret_cast<const v4i32*>(smem + rdA[blk] + 16 * ((2 * q + h) ^ swA[blk]));
                fb[blk][q] = *reinterpret_cast<const v4i32*>(smem + rdB[blk] + 16 * ((2 * q + h) ^ swB[blk]));
            }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[0][q], fb[0][q], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[0][q], fb[1][q], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[1][q], fb[0][q], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[1][q], fb[1][q], acc[1][1], 0, 0, 0);
        }
        const uint32_t u = it / rounds, rd = it % rounds;
        if ((rd + 1) % kPfksSegRounds == 0 || rd + 1 == rounds) {
            // fold: C/D map of the 32x32 forms: row = (reg & 3) + 8 (reg >> 2) + 4 h, column = r
            const uint32_t seg = rd / kPfksSegRounds;
            const int* rs = a.rowsum + ((size_t)seg * U + u) * a.Mpad;
            const int sh = 8 * (t + (int)u);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) {
                        const uint32_t row = m0 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                        const long long s = (long long)acc[i][j][reg] + 128ll * (long long)rs[row];
                        if (sh < 64) part[i][j][reg] += (unsigned long long)s << sh;
                        acc[i][j][reg] = 0;
                    }
        }
    }
    // epilogue: add the 8 planes of a word (8 neighbouring lanes), write -v
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                unsigned long long v = part[i][j][reg];
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                const uint32_t row = m0 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                const uint32_t word = (n0 + 32 * j + r) >> 3;
                if (t == 0 && row < a.M && word < a.ncols) *pfks_dest(a.dst, row, word / a.W, word % a.W) = (uint64_t)0 - v;
            }
}

// ---- VALU path: a workgroup owns PFKS_VT rows x 256 words of one key; every key word fetched (coalesced across the 256 columns)
// is used PFKS_VT times; digits are workgroup-uniform.  grid (ceil(W / 256), ceil(M / PFKS_VT), keys of the call)
struct PfksValuArgs {
    const uint64_t* in;  // M rows of row_words words
    const uint64_t* key; // first key of the call: [keys][row_words][count][W]
    PfksDest dst;
    uint32_t M, W, row_words, radix_log, count;
};

__global__ __launch_bounds__(256) void pfks_valu_kernel(PfksValuArgs a)
{
    const uint32_t col = blockIdx.x * 256 + threadIdx.x, q = blockIdx.z;
    const uint32_t m0 = blockIdx.y * PFKS_VT;
    const bool live = col < a.W;
    const uint32_t colc = live ? col : 0;
    const uint64_t* key = a.key + (size_t)q * a.row_words * a.count * a.W + colc;
    uint64_t sum[PFKS_VT];
#pragma unroll
    for (int t = 0; t < PFKS_VT; t++) sum[t] = 0;
    // state in 64 bits: radix_log may be anything up to 63 (count 1), where the rounded state carries into bit 63
    const uint32_t shift = 64 - a.radix_log * a.count;
    const uint64_t mask = ((uint64_t)1 << a.radix_log) - 1;
    for (uint32_t i = 0; i < a.row_words; i++) {
        const uint64_t* lev = key + (size_t)i * a.count * a.W;
        uint64_t st[PFKS_VT];
#pragma unroll
        for (int t = 0; t < PFKS_VT; t++) {
            const uint32_t m = m0 + t < a.M ? m0 + t : a.M - 1;
            const uint64_t x = a.in[(size_t)m * a.row_words + i];
            st[t] = (x >> shift) + ((x >> (shift - 1)) & 1);
        }
        for (uint32_t j = 0; j < a.count; j++) {
            const uint64_t kv = lev[(size_t)(a.count - 1 - j) * a.W];
#pragma unroll
            for (int t = 0; t < PFKS_VT; t++) {
                const uint64_t d = st[t] & mask;
                st[t] >>= a.radix_log;
                const uint64_t carry = d >> (a.radix_log - 1);
                st[t] += carry;
                sum[t] += kv * (d - (carry << a.radix_log)); // the signed digit, mod 2^64
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < PFKS_VT; t++)
        if (m0 + t < a.M) *pfks_dest(a.dst, m0 + t, q, col) = (uint64_t)0 - sum[t];
}

// ---- `extract_and_rotate_lo_noise_glwe` (circuit_bootstrapping.rs:224-252): for level i < l_cbs, `sample_extract`(i)
// (glwe_ciphertext_ops.rs:31-76) then 2^(64 - (log_cbs (i+1) + 1)) onto the body.  B lo-noise GLWEs -> B * l_cbs LWE rows of
// k N + 1 words; grid (ceil((k N + 1) / 256), rows of the launch)
__global__ __launch_bounds__(256) void pfks_extract_rotate_kernel(const uint64_t* glwe, uint64_t* lwe, uint32_t N, uint32_t k,
                                                                  uint32_t l_cbs, uint32_t log_cbs)
{
    const uint32_t rowi = blockIdx.y, b = rowi / l_cbs, lvl = rowi % l_cbs;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > k * N) return;
    const uint64_t* g = glwe + (size_t)b * (k + 1) * N;
    uint64_t* o = lwe + (size_t)rowi * (k * N + 1);
    if (i == k * N) {
        o[i] = g[k * N + lvl] + ((uint64_t)1 << (64 - (log_cbs * (lvl + 1) + 1)));
        return;
    }
    const uint32_t p = i / N, j = i % N;
    o[i] = j <= lvl ? g[p * N + lvl - j] : (uint64_t)0 - g[p * N + lvl + N - j];
}

} // namespace spf
