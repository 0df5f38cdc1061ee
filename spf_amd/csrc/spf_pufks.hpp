// spf_pufks.hpp — `public_functional_keyswitch` (sunscreen_tfhe/src/ops/keyswitch/public_functional_keyswitch.rs:74-148) with the
// public map "message j to coefficient j": p <= N LWE ciphertexts (a_j, b_j) of dimension n become ONE GLWE,
//   poly_i = sum_{j<p} a_j[i] X^j                                   (i < n; coefficients p .. N-1 are zero)
//   acc_fft = 0;  for i ascending: decomposed_polynomial_glev_mad(acc_fft, Decomp(poly_i), fft(K[i]))   (ops/fft_ops.rs:67-98)
//   out = -(ifft(acc_fft)) wrapping, on every polynomial;  out.body[j] += b_j for j < p
// over the key `PublicFunctionalKeyswitchKey<u64>` (entities/public_functional_keyswitch_key.rs), [n][count][k+1][N], transformed
// polynomial by polynomial on load.  The loop over i is glwe_ggsw_mad (fft_ops.rs:23-56) over consecutive groups of k+1 key rows,
// all into one spectrum: rows ascending, digits within a row least significant first against GLEV entries in reverse, four-FMA
// multiply-add, ONE inverse transform at the end.  That order is the function: no kernel here splits the sum over rows.
//
// pufks_kernel<LOGB, L> (N = 2048, k = 1, radix 4 bits x 8 — the reference benchmark's, benches/ops.rs:395-452 — and 4 x 4): cmux_body
// with the round loop running over n * L rounds.  Two waves per output (sample parity), the two spectrum accumulators of a wave
// in registers across all rows, key rows requested one round ahead, one inverse transform pair and one conversion at the end.
//   Input polynomials.  Coefficient j of poly_i is word i of LWE row j, rows n + 1 words apart: read as they lie that is a
//   16 KiB-strided gather per key row.  pufks_digits_kernel is a transposing PRE-PASS into scratch of the context: 32 x 32 tiles
//   through LDS, LWE rows read along their words, the packed gadget digits (one uint32 per coefficient: L * LOGB <= 32) written
//   along the coefficients, [output][key row][pstride] with pstride = p rounded up to 32.  The main kernel reads one row of packed
//   digits per key row, one row ahead; coefficients >= p are zeros and touch no line of their own.  Half the bytes of the words themselves.
//   pufks_digits_rows_kernel is the same pre-pass over rows that lie anywhere (a gate graph's node): row b * p + c comes from a
//   device pointer table, and the p bodies of an output are copied into a compact array, which the main kernels then read (PufksArgs::body).
//   Key sharing.  G outputs (G = 2 up to two workgroups per CU, G = 4 beyond) share a workgroup whose waves meet at the same
//   barriers every round, so the G wave pairs ask for the same key row within one round of each other: the first request brings
//   the line into L2, the others hit there; workgroups launched together stay within a few rounds of each other and meet in the
//   Infinity Cache (measured: profiles/r18_public_functional_keyswitch.md).
// pufks4_kernel<LOGB, L>: the same arithmetic on four waves per output, for batches of at most one output per CU (below).
// generic_pufks_kernel: every other parameter set — one workgroup per output, generic_glev_mad / generic_poly_ifft of
// spf_generic.hpp with a run-time radix; also N = 2048, k = 1 at radices other than the two above.
#pragma once

#include "spf_generic.hpp"
#include "spf_kernels.hpp"

namespace spf {

struct GenericPufksArgs {
    GenericShape g;
    const uint64_t* lwe_in; // B * p rows of n + 1 words, int-major: input j of output b is row b * p + j
    uint64_t* out;          // B x (k+1) N
    const c64* key;         // [n][count][k+1][N/2]
    uint32_t n, p, radix_log, count;
};

__global__ __launch_bounds__(kGenericThreads) void generic_pufks_kernel(GenericPufksArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GenericShape& g = a.g;
    const uint32_t tid = threadIdx.x, N = g.N, h = N / 2, k = g.k;
    c64* accf = reinterpret_cast<c64*>(smem);
    c64* buf = accf + (size_t)(k + 1) * h;
    uint64_t* state = reinterpret_cast<uint64_t*>(buf + h);
    c64* tmp = reinterpret_cast<c64*>(state + N);
    const size_t row_words = (size_t)a.n + 1;
    const uint64_t* rows = a.lwe_in + (size_t)blockIdx.x * a.p * row_words;
    uint64_t* out = a.out + (size_t)blockIdx.x * (k + 1) * N;
    for (uint32_t i = tid; i < (k + 1) * h; i += kGenericThreads) accf[i] = {0.0, 0.0};
    __syncthreads();
    const size_t glev_len = (size_t)a.count * (k + 1) * h;
    for (uint32_t i = 0; i < a.n; i++)
        generic_glev_mad(g, accf, buf, state, a.key + (size_t)i * glev_len, a.radix_log, a.count,
                         [&](uint32_t c) { return c < a.p ? rows[(size_t)c * row_words + i] : (uint64_t)0; });
    // out = -(ifft(acc_fft)); out.body[j] += b_j (public_functional_keyswitch.rs:132-147)
    for (uint32_t q = 0; q <= k; q++)
        generic_poly_ifft(g, accf + (size_t)q * h, buf, tmp, [&](uint32_t i, uint64_t t) {
            const uint64_t body = (q == k && i < a.p) ? rows[(size_t)i * row_words + a.n] : (uint64_t)0;
            out[q * N + i] = body - t;
        });
}

// ---- N = 2048, k = 1 --------------------------------------------------------------------------

// the transposing pre-pass: dig[b][i][c] = gadget_digits_packed(word i of LWE row b * p + c), c < p, i < n.
// grid (ceil(n / 32), ceil(p / 32), outputs), 256 threads: a 32 x 32 tile, read along i, written along c.
template <int L, int LOGB>
__global__ __launch_bounds__(256) void pufks_digits_kernel(const uint64_t* __restrict__ lwe_in, uint32_t* __restrict__ dig, uint32_t n,
                                                           uint32_t p, uint32_t pstride)
{
    __shared__ uint32_t tile[32][33];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t i0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const size_t row_words = (size_t)n + 1;
    const uint64_t* rows = lwe_in + (size_t)blockIdx.z * p * row_words;
    uint32_t* o = dig + (size_t)blockIdx.z * n * pstride;
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t c = c0 + r, i = i0 + tx;
        if (c < p && i < n) tile[r][tx] = gadget_digits_packed<L, LOGB>(rows[(size_t)c * row_words + i]);
    }
    __syncthreads();
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t i = i0 + r, c = c0 + tx;
        if (i < n && c < p) o[(size_t)i * pstride + c] = tile[tx][r];
    }
}

// The same with row b * p + c read where it lies, through a device pointer table (a gate graph's level: the LWEs of a
// spf_graph_add_public_functional_keyswitch node come from any node of any level).  The main kernels need the p bodies per output
// as well: the blocks of the first tile column copy them into a compact [output][pstride] array, so no row is gathered whole.
template <int L, int LOGB>
__global__ __launch_bounds__(256) void pufks_digits_rows_kernel(const uint64_t* const* __restrict__ rows, uint32_t* __restrict__ dig,
                                                                uint64_t* __restrict__ bodies, uint32_t n, uint32_t p, uint32_t pstride)
{
    __shared__ uint32_t tile[32][33];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t i0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const uint64_t* const* row = rows + (size_t)blockIdx.z * p;
    uint32_t* o = dig + (size_t)blockIdx.z * n * pstride;
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t c = c0 + r, i = i0 + tx;
        if (c < p && i < n) tile[r][tx] = gadget_digits_packed<L, LOGB>(row[c][i]);
    }
    if (blockIdx.x == 0 && threadIdx.x < 32 && c0 + threadIdx.x < p)
        bodies[(size_t)blockIdx.z * pstride + c0 + threadIdx.x] = row[c0 + threadIdx.x][n];
    __syncthreads();
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t i = i0 + r, c = c0 + tx;
        if (i < n && c < p) o[(size_t)i * pstride + c] = tile[tx][r];
    }
}

struct PufksArgs {
    const c64* key;         // [n][L][2][1024]
    const uint32_t* dig;    // [B][n][pstride] (pufks_digits_kernel / pufks_digits_rows_kernel)
    // body of input c of output b = body[b * body_out_stride + c * body_stride]: word n of the contiguous rows (lwe_in + n, strides
    // p * (n + 1) and n + 1), or the compact array of pufks_digits_rows_kernel (strides pstride and 1)
    const uint64_t* body;
    size_t body_out_stride, body_stride;
    uint64_t* out;          // B x 4096
    const c64* tables;
    uint32_t B, n, p, pstride;
};

template <int L, int LOGB, int G, int W>
__device__ __forceinline__ void pufks_body(const PufksArgs& a, char* smem)
{
    static_assert(L * LOGB <= 32, "packed digits need L*LOGB <= 32");
    static_assert((L & (L - 1)) == 0, "the round index splits into (row, digit) by shift and mask");
    c64* tab = reinterpret_cast<c64*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cslot = wv >> 1;
    constexpr int w = W;
    char* tile = smem + kTableBytes + cslot * kWaveBufBytes;
    char* mine = tile + w * 8192;
    char* theirs = tile + (w ^ 1) * 8192;
    auto pair_sync = [&]() { pair_barrier_w(); }; // every wave of the workgroup runs the same sequence of rounds
    table_image_dma<128 * G>(a.tables, smem, tid, wv);
    const uint32_t ct_raw = blockIdx.x * G + cslot;
    const bool owns_output = ct_raw < a.B;
    const uint32_t ct = owns_output ? ct_raw : a.B - 1;
    const uint32_t n = a.n, p = a.p;
    const uint32_t* dig_ct = a.dig + (size_t)ct * n * a.pstride;
    const gu64_ptr gout = global_view(a.out + (size_t)ct * 2 * kN);

    // packed digits of key row i for this wave's 16 coefficients.  Coefficients >= p are zeros: their lanes re-read word p - 1
    // (no branch around a load, no line that is not read anyway) and the zero is put in where the row is taken into use, a row
    // later, so that nothing waits for the loads where they are requested
    auto dig_row = [&](uint32_t i, uint32_t (&d)[16]) {
        const uint32_t* row = dig_ct + (size_t)i * a.pstride;
#pragma unroll
        for (int e = 0; e < 16; e++) d[e] = row[min((uint32_t)coef2(e, lane, w), p - 1)];
    };
    uint32_t cur[16], nxt[16];
    dig_row(0, nxt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // my pieces of the twiddle image have landed (LDS-DMA counts on vmcnt)
    __syncthreads();

    const c64* twist = tab + kTWOff + w * 512 + lane;
    const c64* wc = tab + kWCOff + 256 * w + lane;
    c64 prod[2][8];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int r = 0; r < 8; r++) prod[q][r] = {0.0, 0.0};

    // this wave's bins of key row (i, L-1-j), both output polynomials, requested one round ahead as in cmux_body
    const gc64_ptr gkey = global_view(a.key) + 256 * w + lane;
    auto key_row = [&](uint32_t m) -> gc64_ptr {
        const uint32_t i = m / L, j = m & (L - 1);
        return gkey + ((size_t)i * L + (L - 1 - j)) * 2 * kHalf;
    };
    c64 k0[8], k1[8];
    {
        const gc64_ptr row = key_row(0);
#pragma unroll
        for (int r = 0; r < 8; r++) k0[r] = gload(row + 64 * (r & 3) + 512 * (r >> 2));
#pragma unroll
        for (int r = 0; r < 8; r++) k1[r] = gload(row + kHalf + 64 * (r & 3) + 512 * (r >> 2));
    }
    const uint32_t rounds = n * L;
    auto round = [&](uint32_t m, auto last_c) {
        constexpr bool LAST = decltype(last_c)::value;
        const uint32_t i = m / L, j = m & (L - 1);
        const int sh = (int)j * LOGB;
        if (j == 0) { // a new key row: its digits were requested a row ago; the next row's are requested now
#pragma unroll
            for (int e = 0; e < 16; e++) cur[e] = (uint32_t)coef2(e, lane, w) < p ? nxt[e] : 0u;
            dig_row(min(i + 1, n - 1), nxt); // (the last row asks for itself again: no branch around the requests)
        }
        const gc64_ptr next = key_row(LAST ? m : m + 1);
        c64 V[8];
#pragma unroll
        for (int n1 = 0; n1 < 8; n1++) {
            int dre = ((int)(cur[n1] << (32 - LOGB - sh))) >> (32 - LOGB);
            int dim = ((int)(cur[8 + n1] << (32 - LOGB - sh))) >> (32 - LOGB);
            V[n1] = cmul_nf({(double)dre, (double)dim}, twist[64 * n1]);
        }
        if (m > 0) pair_sync(); // partner is done with my last cross data
        fft512_single<+1>(V, mine, tab, lane);
        cross_put<w>(mine, lane, V);
        pair_sync();
        cross_take<w>(theirs, lane, V); // V[0..3] = E, V[4..7] = O
        c64 X[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            c64 t = cmul_tw<+1>(V[4 + q], wc[64 * q]);
            X[q] = cadd(V[q], t);
            X[q + 4] = csub(V[q], t);
        }
#pragma unroll
        for (int r = 0; r < 8; r++) cmad(prod[0][r], k0[r], X[r]);
        if constexpr (!LAST) {
#pragma unroll
            for (int r = 0; r < 8; r++) k0[r] = gload(next + 64 * (r & 3) + 512 * (r >> 2));
        }
#pragma unroll
        for (int r = 0; r < 8; r++) cmad(prod[1][r], k1[r], X[r]);
        if constexpr (!LAST) {
#pragma unroll
            for (int r = 0; r < 8; r++) k1[r] = gload(next + kHalf + 64 * (r & 3) + 512 * (r >> 2));
        }
    };
#pragma unroll 1
    for (uint32_t m = 0; m + 1 < rounds; m++) round(m, std::false_type{});
    round(rounds - 1, std::true_type{}); // (its own copy without the requests for a next key row, as in cmux_body)

    // ---- both output polynomials back to the torus as ONE transform pair, as cmux_body does
    int lane_late = lane;
    asm volatile("" : "+v"(lane_late));
    c64 WW[2][8];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            WW[q][i] = cadd(prod[q][i], prod[q][i + 4]);
            WW[q][4 + i] = cmul_tw<-1>(csub(prod[q][i], prod[q][i + 4]), wc[64 * i]);
        }
    pair_sync(); // partner is done with my last cross data
    cross_put<w>(mine, lane, WW);
    pair_sync();
    cross_take<w>(theirs, lane, WW);
    pair_sync(); // both cross reads retired before either image is overwritten
    SPF_CMUX_INV_PAIR<-1, 2>(WW[0], WW[1], mine, tab, lane);
    // the bodies b_j of this wave's coefficients j < p (word n of LWE row j): they land under the first polynomial's conversion
    uint64_t body[16];
    {
        const uint64_t* rows = a.body + (size_t)ct * a.body_out_stride;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t c = (uint32_t)coef2(e, lane_late, w);
            body[e] = rows[(size_t)min(c, p - 1) * a.body_stride]; // (coefficients >= p: masked where the body is added)
        }
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        uint64_t t[16];
        untwist_to_torus_bits(WW[q], twist, t);
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const bool has_body = q == 1 && (uint32_t)coef2(e, lane_late, w) < p;
            const uint64_t v = (has_body ? body[e] : (uint64_t)0) - t[e]; // -(ifft), then the body
            if (owns_output) gout[q * kN + coef2(e, lane_late, w)] = v;
        }
    }
}

// ---- the LATENCY shape: four waves per output, one output per workgroup, for batches of at most one output per CU.
// A round of pufks_body is one chain — digit, transform, cross exchange, two multiply-add rows — on one wave per SIMD, and the n * L
// rounds of an output follow each other: 2.3 us a round, 38 ms for n = 2048 at 8 digits whatever the batch.  The transforms of
// different digits do not depend on each other; only the SUMS have an order.  Wave (w, h) = sample parity w x pair h: pair h
// transforms digit 2t + h of the row (one step = two digits), publishes its spectrum in LDS, and runs the whole accumulation
// chain of OUTPUT polynomial h — digit 2t first, then digit 2t + 1, its own transform from registers, the sibling pair's from
// LDS — against the key rows of polynomial h alone.  Every accumulator sees the products in the reference's order: same words.
// Three barriers per step of two digits; one inverse transform per wave at the end, as in cmux4_body.
constexpr int kPufks4Lds = kTableBytes + 2 * kWaveBufBytes + 4 * 8192 + 64;

template <int L, int LOGB, int W>
__device__ __forceinline__ void pufks4_body(const PufksArgs& a, char* smem)
{
    static_assert(L * LOGB <= 32, "packed digits need L*LOGB <= 32");
    static_assert(L >= 2 && (L & (L - 1)) == 0, "two digits a step; the step index splits into (row, digit pair) by shift and mask");
    constexpr uint32_t T = L / 2; // steps per key row
    c64* tab = reinterpret_cast<c64*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = wv >> 1;
    constexpr int w = W;
    char* tile = smem + kTableBytes + h * kWaveBufBytes;
    char* mine = tile + w * 8192;
    char* theirs = tile + (w ^ 1) * 8192;
    char* pub = smem + kTableBytes + 2 * kWaveBufBytes;
    c64* pub_mine = reinterpret_cast<c64*>(pub + (h * 2 + w) * 8192) + lane;
    const c64* pub_sibling = reinterpret_cast<const c64*>(pub + ((h ^ 1) * 2 + w) * 8192) + lane;
    auto wg_sync = [&]() { pair_barrier_w(); };
    table_image_dma<256>(a.tables, smem, tid, wv);
    const uint32_t ct = blockIdx.x; // grid = outputs
    const uint32_t n = a.n, p = a.p;
    const uint32_t* dig_ct = a.dig + (size_t)ct * n * a.pstride;
    const gu64_ptr gout = global_view(a.out + (size_t)ct * 2 * kN + (size_t)h * kN);
    auto dig_row = [&](uint32_t i, uint32_t (&d)[16]) { // as in pufks_body; both pairs read the row
        const uint32_t* row = dig_ct + (size_t)i * a.pstride;
#pragma unroll
        for (int e = 0; e < 16; e++) d[e] = row[min((uint32_t)coef2(e, lane, w), p - 1)];
    };
    uint32_t cur[16], nxt[16];
    dig_row(0, nxt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // my pieces of the twiddle image have landed (LDS-DMA counts on vmcnt)
    __syncthreads();

    const c64* twist = tab + kTWOff + w * 512 + lane;
    const c64* wc = tab + kWCOff + 256 * w + lane;
    c64 acc[8];
#pragma unroll
    for (int r = 0; r < 8; r++) acc[r] = {0.0, 0.0};

    // key row (i, L-1-j), output polynomial h, this wave's bins; the two rows of a step are requested one step ahead
    const gc64_ptr gkey = global_view(a.key) + (size_t)h * kHalf + 256 * w + lane;
    auto key_row = [&](uint32_t s, uint32_t d) -> gc64_ptr {
        const uint32_t i = s / T, j = 2 * (s & (T - 1)) + d;
        return gkey + ((size_t)i * L + (L - 1 - j)) * 2 * kHalf;
    };
    c64 ke[8], ko[8];
    {
        const gc64_ptr re = key_row(0, 0), ro = key_row(0, 1);
#pragma unroll
        for (int r = 0; r < 8; r++) ke[r] = gload(re + 64 * (r & 3) + 512 * (r >> 2));
#pragma unroll
        for (int r = 0; r < 8; r++) ko[r] = gload(ro + 64 * (r & 3) + 512 * (r >> 2));
    }
    const uint32_t steps = n * T;
    auto step = [&](uint32_t s, auto last_c) {
        constexpr bool LAST = decltype(last_c)::value;
        const uint32_t i = s / T, t = s & (T - 1);
        const int sh = (int)(2 * t + (uint32_t)h) * LOGB;
        if (t == 0) {
#pragma unroll
            for (int e = 0; e < 16; e++) cur[e] = (uint32_t)coef2(e, lane, w) < p ? nxt[e] : 0u;
            dig_row(min(i + 1, n - 1), nxt);
        }
        const uint32_t s_next = LAST ? s : s + 1;
        c64 V[8];
#pragma unroll
        for (int n1 = 0; n1 < 8; n1++) {
            int dre = ((int)(cur[n1] << (32 - LOGB - sh))) >> (32 - LOGB);
            int dim = ((int)(cur[8 + n1] << (32 - LOGB - sh))) >> (32 - LOGB);
            V[n1] = cmul_nf({(double)dre, (double)dim}, twist[64 * n1]);
        }
        if (s > 0) wg_sync(); // partner is done with my last cross data, the sibling pair with my last spectrum
        fft512_single<+1>(V, mine, tab, lane);
        cross_put<w>(mine, lane, V);
        wg_sync();
        cross_take<w>(theirs, lane, V); // V[0..3] = E, V[4..7] = O
        c64 X[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            c64 tq = cmul_tw<+1>(V[4 + q], wc[64 * q]);
            X[q] = cadd(V[q], tq);
            X[q + 4] = csub(V[q], tq);
        }
#pragma unroll
        for (int r = 0; r < 8; r++) pub_mine[r * 64] = X[r];
        wg_sync();
        c64 S[8];
#pragma unroll
        for (int r = 0; r < 8; r++) S[r] = pub_sibling[r * 64];
        // digit 2t (pair 0's transform) first, then digit 2t + 1 (pair 1's)
        if (h == 0) {
#pragma unroll
            for (int r = 0; r < 8; r++) cmad(acc[r], ke[r], X[r]);
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) cmad(acc[r], ke[r], S[r]);
        }
        if constexpr (!LAST) {
            const gc64_ptr re = key_row(s_next, 0);
#pragma unroll
            for (int r = 0; r < 8; r++) ke[r] = gload(re + 64 * (r & 3) + 512 * (r >> 2));
        }
        if (h == 0) {
#pragma unroll
            for (int r = 0; r < 8; r++) cmad(acc[r], ko[r], S[r]);
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) cmad(acc[r], ko[r], X[r]);
        }
        if constexpr (!LAST) {
            const gc64_ptr ro = key_row(s_next, 1);
#pragma unroll
            for (int r = 0; r < 8; r++) ko[r] = gload(ro + 64 * (r & 3) + 512 * (r >> 2));
        }
    };
#pragma unroll 1
    for (uint32_t s = 0; s + 1 < steps; s++) step(s, std::false_type{});
    step(steps - 1, std::true_type{});

    // ---- output polynomial h back to the torus: the split, the exchange inside the pair, one inverse transform
    c64 WW[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        WW[i] = cadd(acc[i], acc[i + 4]);
        WW[4 + i] = cmul_tw<-1>(csub(acc[i], acc[i + 4]), wc[64 * i]);
    }
    wg_sync(); // partner is done with my last cross data
    cross_put<w>(mine, lane, WW);
    wg_sync();
    cross_take<w>(theirs, lane, WW);
    wg_sync(); // cross reads retired before the image is overwritten
    uint64_t body[16];
    {
        const uint64_t* rows = a.body + (size_t)ct * a.body_out_stride;
#pragma unroll
        for (int e = 0; e < 16; e++) body[e] = rows[(size_t)min((uint32_t)coef2(e, lane, w), p - 1) * a.body_stride];
    }
    fft512_single<-1, 7>(WW, mine, tab, lane);
    uint64_t tw[16];
    untwist_to_torus_bits(WW, twist, tw);
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const bool has_body = h == 1 && (uint32_t)coef2(e, lane, w) < p;
        gout[coef2(e, lane, w)] = (has_body ? body[e] : (uint64_t)0) - tw[e]; // -(ifft), then the body
    }
}

template <int LOGB, int L>
__global__ __launch_bounds__(256, 1) void pufks4_kernel(PufksArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) pufks4_body<L, LOGB, 1>(a, smem);
    else pufks4_body<L, LOGB, 0>(a, smem);
}

template <int LOGB, int L, int G>
__global__ __launch_bounds__(128 * G, G == 2 ? 2 : 1) void pufks_kernel(PufksArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) pufks_body<L, LOGB, G, 1>(a, smem);
    else pufks_body<L, LOGB, G, 0>(a, smem);
}

} // namespace spf
