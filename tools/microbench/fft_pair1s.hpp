// fft_pair1s.hpp — variant 5 of fft_pair_bench.hip: fft512_pair1 (spf_device.hpp) with the eight LDS stores of one transform
// issued two at a time between the three butterfly stages and the twiddle products of the OTHER transform.  Measured in r04
// (profiles/r04_experiments_blind_rotate.md: 7 397 cycles per pair against 7 877); the library ships the form that also shares the
// pass twiddles between the two transforms (fft512_pair1ts), so this one is kept for the probe only.  Same butterflies on the same
// values as fft512_pair1: same words.
// Include it behind the device header (fft_pair_bench.hip can be pointed at another one): it uses that header's radix-8 stages.
#pragma once

namespace spf {

// radix-8 of X, then its seven twiddle products (table entries tw_base[stride * (k - 1)]), with the eight LDS operations
// op(0) .. op(7) of the caller issued two at a time between the stages
template <int DIR, class OP>
__device__ __forceinline__ void radix8_tw_spread(c64 (&X)[8], const c64* tw_base, int stride, OP op)
{
    c64 s[4], t[4], u[8];
    radix8_stage1<DIR>(X, s, t);
    sched_fence();
    op(0); op(1);
    sched_fence();
    radix8_stage2<DIR>(s, t, u);
    sched_fence();
    op(2); op(3);
    sched_fence();
    radix8_stage3<DIR>(X, u);
    sched_fence();
    op(4); op(5);
    sched_fence();
#pragma unroll
    for (int k = 1; k < 5; k++) X[k] = cmul_tw<DIR>(X[k], tw_base[stride * (k - 1)]);
    sched_fence();
    op(6); op(7);
    sched_fence();
#pragma unroll
    for (int k = 5; k < 8; k++) X[k] = cmul_tw<DIR>(X[k], tw_base[stride * (k - 1)]);
    sched_fence();
}
template <int DIR, int XP = 2, class MID = no_hook>
__device__ __forceinline__ void fft512_pair1s(c64 (&A)[8], c64 (&B)[8], char* buf, const c64* tab, int lane, MID mid = MID())
{
    static_assert(XP == 1 || XP == 2, "exchange 2 of B (XP = 2) or of both transforms (XP = 1) in registers");
    constexpr bool XA = XP == 1;
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const uint32_t rd1 = 16 * (8 * lo3 + (hi3 ^ lo3));
    const uint32_t rd2 = 16 * (8 * hi3 + (hi3 ^ lo3));
    const uint32_t wbase = 16 * (64 * hi3 + lo3);
    char* wr[8];
#pragma unroll
    for (int r = 0; r < 8; r++) wr[r] = buf + ((wbase ^ (16 * r)) + 128 * r);
    const c64* t1 = tab + kT1Off + lane;
    const c64* t2 = tab + kT2Off + hi3;
    // pass 1 of A
    radix8<DIR>(A);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) A[k1] = cmul_tw<DIR>(A[k1], t1[64 * (k1 - 1)]);
    sched_fence();
    // pass 1 of B, A's exchange-1 stores spread through it
    radix8_tw_spread<DIR>(B, t1, 64, [&](int k) { *reinterpret_cast<c64*>(wr[k]) = A[k]; });
    // A's exchange-1 reads (ahead of B's stores to the same image: a wave's DS instructions execute in issue order), then
    // pass 2 of A with B's exchange-1 stores spread through it
#pragma unroll
    for (int a = 0; a < 8; a++) A[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd1);
    sched_fence();
    radix8_tw_spread<DIR>(A, t2, 8, [&](int k) { *reinterpret_cast<c64*>(wr[k]) = B[k]; });
    mid();
#pragma unroll
    for (int a = 0; a < 8; a++) B[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd1);
    sched_fence();
    if constexpr (XA) {
        lane_transpose_hi3(A);
        radix8<DIR>(A); // pass 3 of A
        sched_fence();
        radix8<DIR>(B);
#pragma unroll
        for (int c = 1; c < 8; c++) B[c] = cmul_tw<DIR>(B[c], t2[8 * (c - 1)]);
        sched_fence();
        lane_transpose_hi3(B);
        radix8<DIR>(B);
    } else {
        // pass 2 of B, A's exchange-2 stores spread through it
        radix8_tw_spread<DIR>(B, t2, 8, [&](int k) { *reinterpret_cast<c64*>(wr[k]) = A[k]; });
#pragma unroll
        for (int b = 0; b < 8; b++) A[b] = *reinterpret_cast<const c64*>(buf + 1024 * b + rd2);
        sched_fence();
        lane_transpose_hi3(B);
        radix8<DIR>(A); // pass 3 of A, its exchange-2 reads having travelled under B's transposition
        radix8<DIR>(B);
    }
    sched_fence(); // the image's next writer stays behind these reads
}

} // namespace spf
