// spf_device.hpp — device-side arithmetic of the gfx950 bootstrap engine.
//
// Everything here is wave64 / CDNA4 code: a 512-point complex FFT lives in ONE wavefront
// (64 lanes x 8 complex f64 registers), exchanges go through a per-wave LDS tile with an
// XOR-swizzled, bank-conflict-free image, and no workgroup barrier is ever needed.
//
// The arithmetic follows the canonical operation order "DAG-I" (DESIGN.md §FFT): every add,
// multiply and fma below is performed on the same operands in the same association as the
// build's definition, so results are reproducible bit for bit.  Compile with
// -ffp-contract=off: the only fused operations are the explicit __builtin_fma calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spf {

struct c64 {
    double re, im;
};

// Pointers fetched from a table in memory (per-gate operand tables) are generic to the compiler: it emits
// flat_load, which counts on lgkmcnt as well as vmcnt, so every LDS wait in the transforms also waits for the
// key rows in flight.  These views pin the address space to global (global_load/global_store: vmcnt only).
typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef const f64x2_t __attribute__((address_space(1)))* gc64_ptr;
typedef const uint64_t __attribute__((address_space(1)))* gu64_cptr;
typedef uint64_t __attribute__((address_space(1)))* gu64_ptr;
__device__ __forceinline__ gc64_ptr global_view(const c64* p) { return (gc64_ptr)(uintptr_t)p; }
__device__ __forceinline__ gu64_cptr global_view(const uint64_t* p) { return (gu64_cptr)(uintptr_t)p; }
__device__ __forceinline__ gu64_ptr global_view(uint64_t* p) { return (gu64_ptr)(uintptr_t)p; }
__device__ __forceinline__ c64 gload(gc64_ptr p) { f64x2_t v = *p; return {v.x, v.y}; }
// read-once data (a gate's selector rows): streaming hint, 6.2 -> 7.0 TB/s for the bare read pattern (tools/microbench)
__device__ __forceinline__ c64 gload_stream(gc64_ptr p) { f64x2_t v = __builtin_nontemporal_load(p); return {v.x, v.y}; }

__device__ __forceinline__ c64 cadd(c64 a, c64 b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ c64 csub(c64 a, c64 b) { return {a.re - b.re, a.im - b.im}; }

// Complex product as num-complex defines it (4 mul, 1 sub, 1 add; nothing fused) — what
// complex_twist / complex_untwist / complex_mad use
// (sunscreen_tfhe/src/math/simd/scalar.rs:12-35).
__device__ __forceinline__ c64 cmul_nf(c64 a, c64 b)
{
    c64 o;
    o.re = a.re * b.re - a.im * b.im;
    o.im = a.re * b.im + a.im * b.re;
    return o;
}
// a * conj(b), same association as cmul_nf(a, {b.re, -b.im})
__device__ __forceinline__ c64 cmul_nf_conj(c64 a, c64 b)
{
    c64 o;
    o.re = a.re * b.re + a.im * b.im;
    o.im = a.im * b.re - a.re * b.im;
    return o;
}

// FFT-internal twiddle product of DAG-I: one multiply and one fma per component.
template <int DIR> __device__ __forceinline__ c64 cmul_tw(c64 a, c64 w)
{
    c64 o;
    if (DIR > 0) {
        double t1 = a.im * w.im;
        o.re = __builtin_fma(a.re, w.re, -t1);
        double t2 = a.im * w.re;
        o.im = __builtin_fma(a.re, w.im, t2);
    } else { // multiply by conj(w)
        double t1 = a.im * w.im;
        o.re = __builtin_fma(a.re, w.re, t1);
        double t2 = a.im * w.re;
        o.im = __builtin_fma(-a.re, w.im, t2);
    }
    return o;
}

constexpr double kSqrtHalf = 0.70710678118654752440; // 0x3FE6A09E667F3BCD

// 8-point DFT, decimation in frequency, in place.  DIR=+1: e^{-2 pi i jk/8}, DIR=-1: conjugate.
template <int DIR> __device__ __forceinline__ void radix8(c64 (&v)[8])
{
    c64 s0 = cadd(v[0], v[4]), s1 = cadd(v[1], v[5]), s2 = cadd(v[2], v[6]), s3 = cadd(v[3], v[7]);
    c64 t0 = csub(v[0], v[4]), t1 = csub(v[1], v[5]), t2 = csub(v[2], v[6]), t3 = csub(v[3], v[7]);
    c64 t1w, t3w;
    if (DIR > 0) {
        double p1 = t1.re + t1.im, m1 = t1.im - t1.re;
        t1w.re = p1 * kSqrtHalf; t1w.im = m1 * kSqrtHalf;
        double p3 = t3.re + t3.im, m3 = t3.im - t3.re;
        t3w.re = m3 * kSqrtHalf; t3w.im = -(p3 * kSqrtHalf);
    } else {
        double p1 = t1.re + t1.im, m1 = t1.re - t1.im;
        t1w.re = m1 * kSqrtHalf; t1w.im = p1 * kSqrtHalf;
        double p3 = t3.re + t3.im, m3 = t3.re - t3.im;
        t3w.re = -(p3 * kSqrtHalf); t3w.im = m3 * kSqrtHalf;
    }
    c64 a0 = cadd(s0, s2), a1 = cadd(s1, s3), a2 = csub(s0, s2), d = csub(s1, s3);
    v[0] = cadd(a0, a1);
    v[4] = csub(a0, a1);
    c64 b0, b2;
    if (DIR > 0) {
        v[2] = {a2.re + d.im, a2.im - d.re};
        v[6] = {a2.re - d.im, a2.im + d.re};
        b0 = {t0.re + t2.im, t0.im - t2.re};
        b2 = {t0.re - t2.im, t0.im + t2.re};
    } else {
        v[2] = {a2.re - d.im, a2.im + d.re};
        v[6] = {a2.re + d.im, a2.im - d.re};
        b0 = {t0.re - t2.im, t0.im + t2.re};
        b2 = {t0.re + t2.im, t0.im - t2.re};
    }
    c64 b1 = cadd(t1w, t3w), e = csub(t1w, t3w);
    v[1] = cadd(b0, b1);
    v[5] = csub(b0, b1);
    if (DIR > 0) {
        v[3] = {b2.re + e.im, b2.im - e.re};
        v[7] = {b2.re - e.im, b2.im + e.re};
    } else {
        v[3] = {b2.re - e.im, b2.im + e.re};
        v[7] = {b2.re + e.im, b2.im - e.re};
    }
}

// ---- LDS image of the twiddle tables (one copy per workgroup), in 16-byte complex entries.
//   T1[k1-1][lane]   = W512^{lane*k1}, k1 = 1..7          (7*64 entries)
//   T2[c-1][b]       = W64^{b*c},      c  = 1..7, b < 8   (7*8  entries)
//   WC[k]            = W1024^{k},      k < 512
//   TW[par][n']      = e^{+i pi (2n'+par)/2048}, n' < 512 (negacyclic twist, de-interleaved)
// with W_M = e^{-2 pi i / M}.  The host builds the same image (spf_hip.hip: build_tables).
constexpr int kT1Off = 0;
constexpr int kT2Off = kT1Off + 7 * 64;
constexpr int kWCOff = kT2Off + 7 * 8;
constexpr int kTWOff = kWCOff + 512;
constexpr int kTableEntries = kTWOff + 1024; // 2040 entries = 32640 bytes
constexpr int kTableBytes = kTableEntries * 16;
constexpr int kWaveBufBytes = 16384; // per-wave staging / exchange tile

// wave-local ordering point between LDS writes and the reads of other lanes' data.  DS
// operations of one wave execute in issue order; the asm keeps the compiler from moving
// memory operations across and drains the LDS queue.
__device__ __forceinline__ void wave_lds_fence()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// compiler-only ordering point (no instruction): LDS reads that precede it in program order
// stay ahead of the LDS writes that follow it.  The hardware needs nothing here: a wave's DS
// instructions execute in order and all 64 lanes retire an instruction together.
__device__ __forceinline__ void compiler_fence() { asm volatile("" ::: "memory"); }
// compiler-only as well, and stronger: no instruction of any kind is scheduled across it.  Pins the
// source-level interleave of two transforms (and keeps their temporaries from overlapping).
__device__ __forceinline__ void sched_fence()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// One 512-point DFT, DIF 8x8x8, held by one wave: lane l, register j holds element 64*j + l on entry (time order) and on
// exit (frequency order).  `buf` is the wave's private 8 KiB LDS tile.
//   n' = 64*n1 + n0, n0 = 8a + b;   k' = k1 + 8c + 64d
//   pass 1: radix-8 over n1 -> k1, * W512^{n0 k1} (k1 != 0)     lanes (a,b)  regs k1
//   exchange 1                                                  lanes (b,k1) regs a
//   pass 2: radix-8 over a -> c,  * W64^{b c}   (c != 0)        lanes (b,k1) regs c
//   exchange 2                                                  lanes (c,k1) regs b
//   pass 3: radix-8 over b -> d                                 lanes (c,k1) regs d
// Exchange images (16-byte slots): slot(x, y, z) = 64 x + 8 z + (y ^ z) with (x,y,z) =
// (a,b,k1) resp. (b,c,k1): writes hit 8 distinct slots mod 8 per 8-lane group and reads 16
// distinct slots mod 16 per ds_read_b128 lane group — conflict-free both ways (measured:
// SQ_LDS_BANK_CONFLICT = 0).
// Used where the partner wave on the SIMD hides the LDS round trips (the eight-waves-per-ciphertext kernel, the CMUX gates).
// PRE (0..7): how many of each pass's seven twiddles are fetched from the LDS image BEFORE the
// butterflies that precede their use, so the reads travel under ~56 f64 instructions instead of
// being issued one or two at a time right where they are needed (what the compiler does by itself to
// save registers: about five exposed LDS round trips per pass).  Costs 4 PRE live VGPRs across the
// radix-8; the kernels pick what their register budget allows.
template <int DIR, int PRE = 0>
__device__ __forceinline__ void fft512_single(c64 (&V)[8], char* buf, const c64* tab, int lane)
{
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const int rd = 16 * (8 * lo3 + (hi3 ^ lo3));
    {
        c64 tw[PRE > 0 ? PRE : 1];
#pragma unroll
        for (int k = 0; k < PRE; k++) tw[k] = tab[kT1Off + k * 64 + lane];
        if constexpr (PRE > 0) compiler_fence();
        radix8<DIR>(V);
#pragma unroll
        for (int k1 = 1; k1 < 8; k1++)
            V[k1] = cmul_tw<DIR>(V[k1], (k1 - 1 < PRE) ? tw[k1 - 1 < PRE ? k1 - 1 : 0] : tab[kT1Off + (k1 - 1) * 64 + lane]);
    }
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++)
        *reinterpret_cast<c64*>(buf + 16 * (64 * hi3 + 8 * k1 + (lo3 ^ k1))) = V[k1];
    wave_lds_fence();
    {
        c64 tw[PRE > 0 ? PRE : 1];
#pragma unroll
        for (int k = 0; k < PRE; k++) tw[k] = tab[kT2Off + k * 8 + hi3];
#pragma unroll
        for (int a = 0; a < 8; a++) V[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd);
        if constexpr (PRE > 0) compiler_fence();
        radix8<DIR>(V);
#pragma unroll
        for (int c = 1; c < 8; c++)
            V[c] = cmul_tw<DIR>(V[c], (c - 1 < PRE) ? tw[c - 1 < PRE ? c - 1 : 0] : tab[kT2Off + (c - 1) * 8 + hi3]);
    }
    compiler_fence();
#pragma unroll
    for (int c = 0; c < 8; c++)
        *reinterpret_cast<c64*>(buf + 16 * (64 * hi3 + 8 * lo3 + (c ^ lo3))) = V[c];
    wave_lds_fence();
#pragma unroll
    for (int b = 0; b < 8; b++) V[b] = *reinterpret_cast<const c64*>(buf + 1024 * b + rd);
    radix8<DIR>(V);
    compiler_fence();
}

// ---- register <-> lane transposition without LDS ------------------------------------------------
// Swap the three bits of the register index r (V[r], r = 4 r2 + 2 r1 + r0) with lane bits 5, 4, 3:
// afterwards lane (h2 h1 h0 | lo3) register (r2 r1 r0) holds what lane (r2 r1 r0 | lo3) register
// (h2 h1 h0) held.  Bit 5 and bit 4 are one `v_permlane32_swap` / `v_permlane16_swap` per dword and
// register pair (the instruction IS the 2x2 block transpose: upper half of the first operand <->
// lower half of the second), bit 3 has no swap instruction: a copy and two bank-masked DPP moves
// (row_ror:8 reaches lane ^ 8 inside a row of 16).  16 + 16 + 48 32-bit VALU instructions for the eight
// complex registers, no LDS traffic and no waitcnt.
__device__ __forceinline__ void swap_halves32(double& a, double& b)
{
    uint32_t al = (uint32_t)__double2loint(a), ah = (uint32_t)__double2hiint(a);
    uint32_t bl = (uint32_t)__double2loint(b), bh = (uint32_t)__double2hiint(b);
    auto r0 = __builtin_amdgcn_permlane32_swap(al, bl, false, false);
    auto r1 = __builtin_amdgcn_permlane32_swap(ah, bh, false, false);
    a = __hiloint2double((int)r1[0], (int)r0[0]);
    b = __hiloint2double((int)r1[1], (int)r0[1]);
}
__device__ __forceinline__ void swap_rows16(double& a, double& b)
{
    uint32_t al = (uint32_t)__double2loint(a), ah = (uint32_t)__double2hiint(a);
    uint32_t bl = (uint32_t)__double2loint(b), bh = (uint32_t)__double2hiint(b);
    auto r0 = __builtin_amdgcn_permlane16_swap(al, bl, false, false);
    auto r1 = __builtin_amdgcn_permlane16_swap(ah, bh, false, false);
    a = __hiloint2double((int)r1[0], (int)r0[0]);
    b = __hiloint2double((int)r1[1], (int)r0[1]);
}
__device__ __forceinline__ void swap_lane8(double& a, double& b)
{
    // a: lanes with bit 3 set take b from lane ^ 8; b: lanes with bit 3 clear take (the old) a from lane ^ 8
    constexpr int kRowRor8 = 0x128; // DPP row_ror:8
    int al = __double2loint(a), ah = __double2hiint(a);
    int bl = __double2loint(b), bh = __double2hiint(b);
    int nal = __builtin_amdgcn_update_dpp(al, bl, kRowRor8, 0xF, 0xC, false);
    int nah = __builtin_amdgcn_update_dpp(ah, bh, kRowRor8, 0xF, 0xC, false);
    int nbl = __builtin_amdgcn_update_dpp(bl, al, kRowRor8, 0xF, 0x3, false);
    int nbh = __builtin_amdgcn_update_dpp(bh, ah, kRowRor8, 0xF, 0x3, false);
    a = __hiloint2double(nah, nal);
    b = __hiloint2double(nbh, nbl);
}
__device__ __forceinline__ void lane_transpose_hi3(c64 (&V)[8])
{
#pragma unroll
    for (int r = 0; r < 4; r++) { // register bit 2 <-> lane bit 5
        swap_halves32(V[r].re, V[r + 4].re);
        swap_halves32(V[r].im, V[r + 4].im);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) { // register bit 1 <-> lane bit 4
        if (r & 2) continue;
        swap_rows16(V[r].re, V[r + 2].re);
        swap_rows16(V[r].im, V[r + 2].im);
    }
#pragma unroll
    for (int r = 0; r < 8; r += 2) { // register bit 0 <-> lane bit 3
        swap_lane8(V[r].re, V[r + 1].re);
        swap_lane8(V[r].im, V[r + 1].im);
    }
}

// Two independent 512-point DFTs (the even / odd sample halves of one 1024-point transform; the DAG and exchange images of
// fft512_single, each on its own 8 KiB tile bufE / bufO), software-pipelined for a wave that has its SIMD to itself (the latency
// kernels): there nothing else covers an LDS round trip, and the two advanced in lockstep with the LDS queue drained between
// the passes cost exactly twice one transform (measured 5 774 vs 2 707 cycles).  A wave's DS instructions execute in issue order, so a read issued
// behind the writes of the same image needs no drain: every exchange of one transform is issued and then
// left in flight under a radix-8 pass of the other.  Same butterflies on the same values: same words.
// (Exchange 2 in registers, `lane_transpose_hi3` as in fft512_pair1, trades the LDS store path the four waves of a CU
// share against 80 32-bit VALU instructions per transform: 4.03 -> 3.98 ms on blind_rotate4_kernel, not kept.)
template <int DIR>
__device__ __forceinline__ void fft512_pair_pipelined(c64 (&E)[8], c64 (&O)[8], char* bufE, char* bufO,
                                                      const c64* tab, int lane)
{
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const int rd = 16 * (8 * lo3 + (hi3 ^ lo3));
    c64 tw1[7], tw2[7];
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) tw1[k1 - 1] = tab[kT1Off + (k1 - 1) * 64 + lane];
#pragma unroll
    for (int c = 1; c < 8; c++) tw2[c - 1] = tab[kT2Off + (c - 1) * 8 + hi3];
    compiler_fence(); // all fourteen requested HERE (r04: without the fence hipcc sank them to their uses, two at a time, each
                      // waited for on the spot — at one wave per SIMD every such round trip is lost time)
    // E pass 1 -> exchange-1 image
    radix8<DIR>(E);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) E[k1] = cmul_tw<DIR>(E[k1], tw1[k1 - 1]);
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++)
        *reinterpret_cast<c64*>(bufE + 16 * (64 * hi3 + 8 * k1 + (lo3 ^ k1))) = E[k1];
    compiler_fence();
    // O pass 1, E's exchange-1 reads in flight under it
#pragma unroll
    for (int a = 0; a < 8; a++) E[a] = *reinterpret_cast<const c64*>(bufE + 1024 * a + rd);
    compiler_fence();
    radix8<DIR>(O);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) O[k1] = cmul_tw<DIR>(O[k1], tw1[k1 - 1]);
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++)
        *reinterpret_cast<c64*>(bufO + 16 * (64 * hi3 + 8 * k1 + (lo3 ^ k1))) = O[k1];
    compiler_fence();
#pragma unroll
    for (int a = 0; a < 8; a++) O[a] = *reinterpret_cast<const c64*>(bufO + 1024 * a + rd);
    compiler_fence();
    // E pass 2 (O's reads in flight) -> exchange-2 image
    radix8<DIR>(E);
#pragma unroll
    for (int c = 1; c < 8; c++) E[c] = cmul_tw<DIR>(E[c], tw2[c - 1]);
#pragma unroll
    for (int c = 0; c < 8; c++)
        *reinterpret_cast<c64*>(bufE + 16 * (64 * hi3 + 8 * lo3 + (c ^ lo3))) = E[c];
    compiler_fence();
#pragma unroll
    for (int b = 0; b < 8; b++) E[b] = *reinterpret_cast<const c64*>(bufE + 1024 * b + rd);
    compiler_fence();
    // O pass 2 (E's reads in flight)
    radix8<DIR>(O);
#pragma unroll
    for (int c = 1; c < 8; c++) O[c] = cmul_tw<DIR>(O[c], tw2[c - 1]);
#pragma unroll
    for (int c = 0; c < 8; c++)
        *reinterpret_cast<c64*>(bufO + 16 * (64 * hi3 + 8 * lo3 + (c ^ lo3))) = O[c];
    compiler_fence();
#pragma unroll
    for (int b = 0; b < 8; b++) O[b] = *reinterpret_cast<const c64*>(bufO + 1024 * b + rd);
    compiler_fence();
    // pass 3
    radix8<DIR>(E);
    radix8<DIR>(O);
    compiler_fence(); // the tile's next writer stays behind these reads
}

// A transform pair with ONE 8 KiB exchange image for both transforms — the form that fits two waves per
// SIMD (blind_rotate2p_kernel: 256 registers, 8 KiB of LDS per wave).  A wave's DS instructions execute
// in issue order, so the two transforms can take turns on the same image as long as the program
// order is  A.write, A.read, B.write, B.read, A.write, ...: each read is issued one butterfly pass
// ahead of its use and travels under the OTHER transform's arithmetic, each write drains under it.
// Same DAG as fft512_single.  Exchange images (16-byte slots), chosen so that BOTH exchanges write to
// the same eight lane addresses (8 address registers for the whole transform pair):
//   exchange 1: writer lane (a,b) reg k1 -> 64 a + 8 k1 + (b ^ k1);  reader lane (b,k1) reg a <- 64 a + 8 k1 + (b ^ k1)
//   exchange 2: writer lane (b,k1) reg c -> 64 b + 8 c  + (k1 ^ c);  reader lane (c,k1) reg b <- 64 b + 8 c  + (k1 ^ c)
// i.e. writer (hi3, lo3) reg r -> ((64 hi3 + lo3) ^ r) + 8 r in both; both are conflict-free for
// ds_write_b128 (8 distinct slots mod 8 per 8-lane group) and ds_read_b128 (16 distinct slots mod 16
// per 16-lane group of the b128 read pattern).
// XP = 1: exchange 2 (registers c <-> lane bits 5..3 = b, the lanes are (b, k1) before and (c, k1) after:
// exactly `lane_transpose_hi3`) stays in registers; only exchange 1 goes through the image.
// XP: which transforms keep exchange 2 in registers (registers c <-> lane bits 5..3 = b; the lanes are
// (b, k1) before and (c, k1) after: exactly `lane_transpose_hi3`) instead of sending it through the
// image: 0 none, 1 both, 2 only B (balances the LDS store path against the VALU).
struct no_hook { __device__ __forceinline__ void operator()() const {} };
// `mid` is called once, half-way through the pair (behind pass 2 of A): a hook for the issue-priority schedule of the
// callers, which swap the roles of the two waves of a SIMD in the middle of a long barrier-to-barrier stretch
template <int DIR, int XP = 0, class MID = no_hook>
__device__ __forceinline__ void fft512_pair1(c64 (&A)[8], c64 (&B)[8], char* buf, const c64* tab, int lane, MID mid = MID())
{
    constexpr bool XA = XP == 1, XB = XP == 1 || XP == 2;
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const uint32_t rd1 = 16 * (8 * lo3 + (hi3 ^ lo3));
    const uint32_t rd2 = 16 * (8 * hi3 + (hi3 ^ lo3));
    const uint32_t wbase = 16 * (64 * hi3 + lo3);
    char* wr[8];
#pragma unroll
    for (int r = 0; r < 8; r++) wr[r] = buf + ((wbase ^ (16 * r)) + 128 * r);
    // pass 1
    radix8<DIR>(A);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) A[k1] = cmul_tw<DIR>(A[k1], tab[kT1Off + (k1 - 1) * 64 + lane]);
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++) *reinterpret_cast<c64*>(wr[k1]) = A[k1];
    sched_fence();
    radix8<DIR>(B);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) B[k1] = cmul_tw<DIR>(B[k1], tab[kT1Off + (k1 - 1) * 64 + lane]);
    sched_fence();
#pragma unroll
    for (int a = 0; a < 8; a++) A[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd1);
    sched_fence();
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++) *reinterpret_cast<c64*>(wr[k1]) = B[k1];
    sched_fence();
    // pass 2 of A; B's exchange-1 reads travel under it
    radix8<DIR>(A);
#pragma unroll
    for (int c = 1; c < 8; c++) A[c] = cmul_tw<DIR>(A[c], tab[kT2Off + (c - 1) * 8 + hi3]);
    sched_fence();
    mid();
#pragma unroll
    for (int a = 0; a < 8; a++) B[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd1);
    sched_fence();
    if constexpr (XA) {
        lane_transpose_hi3(A);
        radix8<DIR>(A); // pass 3 of A
    } else {
#pragma unroll
        for (int c = 0; c < 8; c++) *reinterpret_cast<c64*>(wr[c]) = A[c];
    }
    sched_fence();
    radix8<DIR>(B);
#pragma unroll
    for (int c = 1; c < 8; c++) B[c] = cmul_tw<DIR>(B[c], tab[kT2Off + (c - 1) * 8 + hi3]);
    sched_fence();
    if constexpr (!XA) {
#pragma unroll
        for (int b = 0; b < 8; b++) A[b] = *reinterpret_cast<const c64*>(buf + 1024 * b + rd2);
        sched_fence();
    }
    if constexpr (XB) {
        lane_transpose_hi3(B);
        if constexpr (!XA) radix8<DIR>(A); // pass 3 of A, its exchange-2 reads having travelled under B's transposition
        radix8<DIR>(B);
    } else {
#pragma unroll
        for (int c = 0; c < 8; c++) *reinterpret_cast<c64*>(wr[c]) = B[c];
        sched_fence();
        // pass 3
        radix8<DIR>(A);
        sched_fence();
#pragma unroll
        for (int b = 0; b < 8; b++) B[b] = *reinterpret_cast<const c64*>(buf + 1024 * b + rd2);
        radix8<DIR>(B);
    }
    sched_fence(); // the image's next writer stays behind these reads
}

// ---- the LDS stores SPREAD through the arithmetic ------------------------------------------------------------------------
// tools/microbench/fft_pair_bench.hip (r04): eight waves per CU running transform pairs in lockstep need 7.9 k cycles per pair,
// the butterflies alone 4.7 k and the LDS traffic alone 4.2 k — the two hardly overlap, because each exchange leaves the wave as
// a burst of eight `ds_write_b128` (13 cycles of the CU's store path each, all eight waves bursting at once) and the other
// transform's table reads queue behind it.  Here the eight stores of one transform are issued two at a time between the
// three butterfly stages and the twiddle products of the OTHER transform (7.4 k cycles per pair in the same probe; that
// variant without shared twiddles lives beside the probe, tools/microbench/fft_pair1s.hpp; the library ships fft512_pair1ts).
// radix8 is cut into its three stages for that; the operations and their order per value are those of `radix8`: same words.
template <int DIR> __device__ __forceinline__ void radix8_stage1(const c64 (&v)[8], c64 (&s)[4], c64 (&t)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) { s[i] = cadd(v[i], v[i + 4]); t[i] = csub(v[i], v[i + 4]); }
}
template <int DIR> __device__ __forceinline__ void radix8_stage2(const c64 (&s)[4], const c64 (&t)[4], c64 (&u)[8])
{
    c64 t1w, t3w;
    if (DIR > 0) {
        double p1 = t[1].re + t[1].im, m1 = t[1].im - t[1].re;
        t1w.re = p1 * kSqrtHalf; t1w.im = m1 * kSqrtHalf;
        double p3 = t[3].re + t[3].im, m3 = t[3].im - t[3].re;
        t3w.re = m3 * kSqrtHalf; t3w.im = -(p3 * kSqrtHalf);
    } else {
        double p1 = t[1].re + t[1].im, m1 = t[1].re - t[1].im;
        t1w.re = m1 * kSqrtHalf; t1w.im = p1 * kSqrtHalf;
        double p3 = t[3].re + t[3].im, m3 = t[3].re - t[3].im;
        t3w.re = -(p3 * kSqrtHalf); t3w.im = m3 * kSqrtHalf;
    }
    u[0] = cadd(s[0], s[2]); u[1] = cadd(s[1], s[3]); u[2] = csub(s[0], s[2]); u[3] = csub(s[1], s[3]);
    if (DIR > 0) {
        u[4] = {t[0].re + t[2].im, t[0].im - t[2].re};
        u[5] = {t[0].re - t[2].im, t[0].im + t[2].re};
    } else {
        u[4] = {t[0].re - t[2].im, t[0].im + t[2].re};
        u[5] = {t[0].re + t[2].im, t[0].im - t[2].re};
    }
    u[6] = cadd(t1w, t3w); u[7] = csub(t1w, t3w);
}
template <int DIR> __device__ __forceinline__ void radix8_stage3(c64 (&v)[8], const c64 (&u)[8])
{
    v[0] = cadd(u[0], u[1]);
    v[4] = csub(u[0], u[1]);
    if (DIR > 0) {
        v[2] = {u[2].re + u[3].im, u[2].im - u[3].re};
        v[6] = {u[2].re - u[3].im, u[2].im + u[3].re};
    } else {
        v[2] = {u[2].re - u[3].im, u[2].im + u[3].re};
        v[6] = {u[2].re + u[3].im, u[2].im - u[3].re};
    }
    v[1] = cadd(u[4], u[6]);
    v[5] = csub(u[4], u[6]);
    if (DIR > 0) {
        v[3] = {u[5].re + u[7].im, u[5].im - u[7].re};
        v[7] = {u[5].re - u[7].im, u[5].im + u[7].re};
    } else {
        v[3] = {u[5].re - u[7].im, u[5].im + u[7].re};
        v[7] = {u[5].re + u[7].im, u[5].im - u[7].re};
    }
}
// ---- fft512_pair1 with the pass twiddles requested EARLY and SHARED by the two transforms ---------------------------------
// The ISA of fft512_pair1 (r04, `tools/isa_build.sh`) shows what hipcc makes of `X[k] = cmul_tw(X[k], tab[...])` when registers
// are tight: the seven twiddles of a pass are fetched just in time, one or two at a time, each `ds_read_b128` followed by an
// `s_waitcnt lgkmcnt(1)` four instructions later — about twenty exposed LDS round trips per pair that only the partner wave
// can cover — and each transform fetches its own copy of the same seven entries (lane-indexed T1, hi3-indexed T2: the same
// for A and B).  Here the seven entries of a pass are requested once, ahead of the butterflies they follow (they land under
// ~50 f64 instructions), and multiply both transforms.  28 registers, live from the request to the second transform's
// products: there is room for them wherever the frequency-domain product is not live (polynomial 0's forward pair, the
// inverse pair), because one of the two transforms is always parked in LDS while the other is in its butterflies.
template <int DIR, int XP = 2, class MID = no_hook>
__device__ __forceinline__ void fft512_pair1t(c64 (&A)[8], c64 (&B)[8], char* buf, const c64* tab, int lane, MID mid = MID())
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
    c64 tw[7];
    // pass 1: T1 for both transforms, requested ahead of A's butterflies
#pragma unroll
    for (int k = 0; k < 7; k++) tw[k] = tab[kT1Off + k * 64 + lane];
    compiler_fence();
    radix8<DIR>(A);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) A[k1] = cmul_tw<DIR>(A[k1], tw[k1 - 1]);
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++) *reinterpret_cast<c64*>(wr[k1]) = A[k1];
    sched_fence();
    radix8<DIR>(B);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) B[k1] = cmul_tw<DIR>(B[k1], tw[k1 - 1]);
    sched_fence();
#pragma unroll
    for (int a = 0; a < 8; a++) A[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd1);
    sched_fence();
#pragma unroll
    for (int k1 = 0; k1 < 8; k1++) *reinterpret_cast<c64*>(wr[k1]) = B[k1];
    sched_fence();
    // pass 2: T2 for both transforms, requested ahead of A's butterflies (behind B's stores in the queue)
#pragma unroll
    for (int c = 0; c < 7; c++) tw[c] = tab[kT2Off + c * 8 + hi3];
    compiler_fence();
    radix8<DIR>(A);
#pragma unroll
    for (int c = 1; c < 8; c++) A[c] = cmul_tw<DIR>(A[c], tw[c - 1]);
    sched_fence();
    mid();
#pragma unroll
    for (int a = 0; a < 8; a++) B[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd1);
    sched_fence();
    if constexpr (XA) {
        lane_transpose_hi3(A);
        radix8<DIR>(A); // pass 3 of A
    } else {
#pragma unroll
        for (int c = 0; c < 8; c++) *reinterpret_cast<c64*>(wr[c]) = A[c];
    }
    sched_fence();
    radix8<DIR>(B);
#pragma unroll
    for (int c = 1; c < 8; c++) B[c] = cmul_tw<DIR>(B[c], tw[c - 1]);
    sched_fence();
    if constexpr (!XA) {
#pragma unroll
        for (int b = 0; b < 8; b++) A[b] = *reinterpret_cast<const c64*>(buf + 1024 * b + rd2);
        sched_fence();
    }
    lane_transpose_hi3(B);
    if constexpr (!XA) radix8<DIR>(A); // pass 3 of A, its exchange-2 reads having travelled under B's transposition
    radix8<DIR>(B);
    sched_fence(); // the image's next writer stays behind these reads
}

// fft512_pair1ts below: fft512_pair1t with the stores of one transform issued two at a time between the butterfly stages of the
// other, measured after the shared twiddles had removed the exposed table reads (profiles/r04_experiments_blind_rotate.md; the
// reads of an exchange issued right behind its own stores, alone or on top of `…t`, lost there: 7 969 against 7 877 and 7 866
// against 6 638 cycles per pair, 42.45 against 40.25 ms per 4096).
// radix8_twr_spread2: radix8_twr_spread with the stores packed into the three butterfly stages (3 + 3 + 2) and `after()` — the reads of the
// transform just stored — issued behind the last store, ahead of the seven twiddle products: the butterfly temporaries are
// dead there and the stored transform's registers are free, so the reads cost no registers and have the products to land under
template <int DIR, class OP, class AFTER>
__device__ __forceinline__ void radix8_twr_spread2(c64 (&X)[8], const c64 (&tw)[7], OP op, AFTER after)
{
    {
        c64 s[4], t[4], u[8];
        radix8_stage1<DIR>(X, s, t);
        sched_fence();
        op(0); op(1); op(2);
        sched_fence();
        radix8_stage2<DIR>(s, t, u);
        sched_fence();
        op(3); op(4); op(5);
        sched_fence();
        radix8_stage3<DIR>(X, u);
    }
    sched_fence();
    op(6); op(7);
    sched_fence();
    after();
    sched_fence();
#pragma unroll
    for (int k = 1; k < 8; k++) X[k] = cmul_tw<DIR>(X[k], tw[k - 1]);
    sched_fence();
}
template <int DIR, class OP>
__device__ __forceinline__ void radix8_twr_spread(c64 (&X)[8], const c64 (&tw)[7], OP op)
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
    for (int k = 1; k < 5; k++) X[k] = cmul_tw<DIR>(X[k], tw[k - 1]);
    sched_fence();
    op(6); op(7);
    sched_fence();
#pragma unroll
    for (int k = 5; k < 8; k++) X[k] = cmul_tw<DIR>(X[k], tw[k - 1]);
    sched_fence();
}
// XP = 0 tail of the pairs below: exchange 2 of B through the image as well, behind A's (A's exchange-2 reads are issued, a wave's
// DS instructions execute in order, so B's stores cannot overtake them): eight stores and eight reads on the LDS pipe instead of
// lane_transpose_hi3's 80 vector instructions — 16 v_permlane*_swap at 8.5 cycles of the SIMD each, 32 DPP moves at 4.5, 16 moves
// (tools/microbench/valu_rates.hip): ~480 of a pair's ~5 600 vector cycles.  B's reads travel under A's last radix-8.
template <int DIR, class ST, class LD>
__device__ __forceinline__ void pair_tail_through_image(c64 (&A)[8], c64 (&B)[8], ST store, LD load, uint32_t rd2)
{
#pragma unroll
    for (int k = 0; k < 8; k++) store(B, k);
    sched_fence();
    load(B, rd2);
    sched_fence();
    radix8<DIR>(A);
    sched_fence();
    radix8<DIR>(B);
}
template <int DIR, int XP = 2, class MID = no_hook>
__device__ __forceinline__ void fft512_pair1ts(c64 (&A)[8], c64 (&B)[8], char* buf, const c64* tab, int lane, MID mid = MID())
{
    static_assert(XP == 2 || XP == 0, "exchange 2 of B in registers (2) or through the image behind A's (0)");
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const uint32_t rd1 = 16 * (8 * lo3 + (hi3 ^ lo3));
    const uint32_t rd2 = 16 * (8 * hi3 + (hi3 ^ lo3));
    const uint32_t wbase = 16 * (64 * hi3 + lo3);
    char* wr[8];
#pragma unroll
    for (int r = 0; r < 8; r++) wr[r] = buf + ((wbase ^ (16 * r)) + 128 * r);
    auto store = [&](c64 (&X)[8], int k) { *reinterpret_cast<c64*>(wr[k]) = X[k]; };
    auto load = [&](c64 (&X)[8], uint32_t rd) {
#pragma unroll
        for (int a = 0; a < 8; a++) X[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd);
    };
    c64 tw[7];
#pragma unroll
    for (int k = 0; k < 7; k++) tw[k] = tab[kT1Off + k * 64 + lane];
    compiler_fence();
    // pass 1 of A, then pass 1 of B with A's exchange-1 stores spread through it
    radix8<DIR>(A);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) A[k1] = cmul_tw<DIR>(A[k1], tw[k1 - 1]);
    sched_fence();
    radix8_twr_spread<DIR>(B, tw, [&](int k) { store(A, k); });
    load(A, rd1);
    sched_fence();
    // T2 for both transforms, pass 2 of A with B's exchange-1 stores
#pragma unroll
    for (int c = 0; c < 7; c++) tw[c] = tab[kT2Off + c * 8 + hi3];
    compiler_fence();
    radix8_twr_spread<DIR>(A, tw, [&](int k) { store(B, k); });
    mid();
    load(B, rd1);
    sched_fence();
    // pass 2 of B with A's exchange-2 stores
    radix8_twr_spread<DIR>(B, tw, [&](int k) { store(A, k); });
    load(A, rd2);
    sched_fence();
    if constexpr (XP == 2) {
        lane_transpose_hi3(B);
        radix8<DIR>(A);
        radix8<DIR>(B);
    } else {
        pair_tail_through_image<DIR>(A, B, store, load, rd2);
    }
    sched_fence();
}
// fft512_pair1ts with each exchange's reads issued inside the other transform's pass, right behind the last spread store
template <int DIR, int XP = 2, class MID = no_hook>
__device__ __forceinline__ void fft512_pair1ts2(c64 (&A)[8], c64 (&B)[8], char* buf, const c64* tab, int lane, MID mid = MID())
{
    static_assert(XP == 2 || XP == 0, "exchange 2 of B in registers (2) or through the image behind A's (0)");
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const uint32_t rd1 = 16 * (8 * lo3 + (hi3 ^ lo3));
    const uint32_t rd2 = 16 * (8 * hi3 + (hi3 ^ lo3));
    const uint32_t wbase = 16 * (64 * hi3 + lo3);
    char* wr[8];
#pragma unroll
    for (int r = 0; r < 8; r++) wr[r] = buf + ((wbase ^ (16 * r)) + 128 * r);
    auto store = [&](c64 (&X)[8], int k) { *reinterpret_cast<c64*>(wr[k]) = X[k]; };
    auto load = [&](c64 (&X)[8], uint32_t rd) {
#pragma unroll
        for (int a = 0; a < 8; a++) X[a] = *reinterpret_cast<const c64*>(buf + 1024 * a + rd);
    };
    c64 tw[7];
#pragma unroll
    for (int k = 0; k < 7; k++) tw[k] = tab[kT1Off + k * 64 + lane];
    compiler_fence();
    radix8<DIR>(A);
#pragma unroll
    for (int k1 = 1; k1 < 8; k1++) A[k1] = cmul_tw<DIR>(A[k1], tw[k1 - 1]);
    sched_fence();
    // pass 1 of B: A's exchange-1 stores in its butterflies, A's exchange-1 reads under its twiddle products
    radix8_twr_spread2<DIR>(B, tw, [&](int k) { store(A, k); }, [&]() { load(A, rd1); });
    // pass 2 of A: B's exchange-1 stores, then B's exchange-1 reads; T2 requested first
    c64 tw2[7];
#pragma unroll
    for (int c = 0; c < 7; c++) tw2[c] = tab[kT2Off + c * 8 + hi3];
    compiler_fence();
    radix8_twr_spread2<DIR>(A, tw2, [&](int k) { store(B, k); }, [&]() { load(B, rd1); });
    mid();
    // pass 2 of B: A's exchange-2 stores, then A's exchange-2 reads
    radix8_twr_spread2<DIR>(B, tw2, [&](int k) { store(A, k); }, [&]() { load(A, rd2); });
    if constexpr (XP == 2) {
        lane_transpose_hi3(B);
        radix8<DIR>(A);
        radix8<DIR>(B);
    } else {
        pair_tail_through_image<DIR>(A, B, store, load, rd2);
    }
    sched_fence();
}

// round half away from zero, then reduce mod 2^64 into the torus exactly as
// PolynomialFftRef::ifft does (entities/polynomial_fft.rs:82-99 -> simd/scalar.rs:26-35,
// 75-119 -> `x as i64` saturating, math/torus.rs:177-192).
__device__ __forceinline__ uint64_t f64_round_to_torus(double x)
{
    const double q = 18446744073709551616.0;      // 2^64
    const double q_div_2 = 9223372036854775808.0; // 2^63
    double v = __builtin_round(x);
    double m = __builtin_fma(-__builtin_trunc(v * (1.0 / q)), q, v);
    // branch-free form of `if m >= q/2 { m -= q } else if m <= -q/2 { m += q }`
    double adj = (m >= q_div_2) ? -q : ((m <= -q_div_2) ? q : 0.0);
    m += adj;
    // m is now in [-2^63, 2^63]; `as i64` saturates the single out-of-range value +2^63
    bool sat = m >= q_div_2;
    long long r = (long long)(sat ? 0.0 : m);
    r = sat ? 0x7FFFFFFFFFFFFFFFll : r;
    return (uint64_t)r;
}

// Fast form of f64_round_to_torus for an input that is already an integer (so round() is the identity): for an
// integer-valued v with 2^52 <= |v| < 2^116 the low 64 bits of v in two's complement are
// (mantissa << (exponent - 1075)), negated for v < 0 — nine 32-bit VALU instructions.  `sh_or` collects the shift
// amounts (the caller checks once per wave that every one is in [0, 64): that IS the magnitude
// test), `quirk_min` becomes 0 if some value hits the saturating-cast quirk (v < 0 and low 64 bits
// == 2^63, which `as i64` turns into 0x7FFF...F): the caller then redoes the wave's values with the
// literal sequence.  Same words as f64_round_to_torus whenever the two checks pass.
__device__ __forceinline__ uint64_t f64_bigint_to_torus_bits(double v, uint32_t& sh_or, uint32_t& quirk_min)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t hi = (uint32_t)(b >> 32), lo = (uint32_t)b;
    const uint32_t sh = ((hi >> 20) & 0x7FFu) - 1075u;
    sh_or |= sh;
    const uint64_t m = ((uint64_t)((hi & 0xFFFFFu) | 0x100000u) << 32) | lo;
    uint64_t r = m << (sh & 63u);
    const uint32_t s32 = (uint32_t)((int32_t)hi >> 31);
    const uint64_t s = ((uint64_t)s32 << 32) | s32;
    r = (r ^ s) - s;
    const uint32_t q = (uint32_t)r | ((uint32_t)(r >> 32) ^ 0x80000000u) | ~s32;
    quirk_min = q < quirk_min ? q : quirk_min;
    return r;
}

// r02's form of the fast path (mantissa extracted, shift amounts OR-ed, quirk by a running minimum): kept for cbs_trace_kernel,
// which is 5 % slower with the form below (4.38 against 4.58 ms per 4096; the blind rotation is 1 % faster with it)
__device__ __forceinline__ void torus_bits16_mantissa(const double (&tv)[16], uint64_t (&t)[16])
{
    uint32_t sh_or = 0, qmin = 0xFFFFFFFFu;
#pragma unroll
    for (int e = 0; e < 16; e++) t[e] = f64_bigint_to_torus_bits(tv[e], sh_or, qmin);
    if (!__all(sh_or < 64u && qmin != 0u)) {
#pragma unroll
        for (int e = 0; e < 16; e++) t[e] = f64_round_to_torus(tv[e]);
    }
}
// The conversion of the sixteen values of a wave with an integer fast path (r03: 42.8 -> 42.3 ms per 4096 against r02's mantissa-extracting form).  For an integer-valued v with
// 2^64 <= |v| < 2^116 the double's own bits shifted left by (exponent - 1075) mod 64 = (exponent + 13) & 63 ARE the low 64
// bits of |v|: the shift is at least 12, so sign, exponent field and the implicit one all leave the word.  Negated for
// v < 0.  Two checks per wave decide whether the sixteen values take this path: every exponent in [1087, 1138] (that IS the
// magnitude test; products of digits and torus words sit around 2^74..2^85), and no magnitude with the high word
// 0x80000000 — a superset of the saturating-cast quirk (v < 0 and |v| = 2^63 mod 2^64, which `as i64` turns into 0x7FFF...F;
// math/torus.rs:177-192), tested with one compare whose result goes to the scalar unit.  Otherwise the wave redoes its
// values with the literal sequence.  Same words as f64_round_to_torus in every case.
__device__ __forceinline__ void torus_bits16(const double (&tv)[16], uint64_t (&t)[16])
{
    uint32_t emin = 0xFFFFFFFFu, emax = 0u;
    uint64_t quirk = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint64_t b = (uint64_t)__double_as_longlong(tv[e]);
        const uint32_t hi = (uint32_t)(b >> 32);
        const uint32_t e11 = (hi >> 20) & 0x7FFu;
        emin = e11 < emin ? e11 : emin;
        emax = e11 > emax ? e11 : emax;
        const uint64_t r = b << ((e11 + 13u) & 63u);
        quirk |= __ballot((uint32_t)(r >> 32) == 0x80000000u);
        const uint32_t s32 = (uint32_t)((int32_t)hi >> 31);
        const uint64_t sg = ((uint64_t)s32 << 32) | s32;
        t[e] = (r ^ sg) - sg;
    }
    if (!__all(emin >= 1087u && emax <= 1138u) || quirk != 0) {
#pragma unroll
        for (int e = 0; e < 16; e++) t[e] = f64_round_to_torus(tv[e]);
    }
}
// inverse side of a transform: (z * 1/1024) * conj(twist), then round / mod 2^64 / saturating cast of the 16 values
// (polynomial_fft.rs:82-99), the twist factors read from the LDS image where they are used (all eight requested at once was
// within run-to-run: 40.11 / 42.78 against 40.11 / 42.76 ms per 4096, profiles/r04_experiments_blind_rotate.md)
template <bool MANTISSA_FORM = false>
__device__ __forceinline__ void untwist_to_torus_bits(const c64 (&V)[8], const c64* twist_lds, uint64_t (&t)[16])
{
    double tv[16];
#pragma unroll
    for (int n1 = 0; n1 < 8; n1++) {
        c64 xs = {V[n1].re * (1.0 / 1024.0), V[n1].im * (1.0 / 1024.0)};
        c64 u = cmul_nf_conj(xs, twist_lds[64 * n1]);
        tv[n1] = u.re;
        tv[8 + n1] = u.im;
    }
    if constexpr (MANTISSA_FORM) torus_bits16_mantissa(tv, t);
    else torus_bits16(tv, t);
}
// a + (uint64_t)b as ONE v_mad_u64_u32 (b * 1 + a; 4.9 cycles of a SIMD): hipcc widens b to a register pair (a move) and adds
// with v_lshl_add_u64, or emits a v_add_co / v_addc pair (9.8 cycles)
__device__ __forceinline__ uint64_t add_u32_to_u64(uint64_t a, uint32_t b)
{
    uint64_t out, carry;
    asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=&v"(out), "=s"(carry) : "v"(b), "v"(a));
    return out;
}

// NEGATED-ACCUMULATOR form of untwist_to_torus_bits + `acc += t` (the blind-rotation bodies): the caller keeps
// nacc = -acc (mod 2^64) and this does nacc -= t, i.e. nacc += (-t).  Same words as the plain form, fewer VALU cycles
// (tools/microbench/valu_rates.hip, profiles/r05_valu_rates.md: a v_sub_co / v_subb pair costs 9.8 cycles of a SIMD, the
// 64-bit add v_lshl_add_u64 4.8, a VOP2 32-bit operation 2.5, a VOP3 one 4.5):
//   * the untwist product is formed NEGATED for free ((-m1) - m2 and m3 - m4 swapped: source modifiers, exact), so the
//     integer of the negated value is what gets ADDED — no subtraction anywhere;
//   * two's complement of the shifted magnitude bits as (r + s) ^ s with s = the sign spread over 64 bits (a 64-bit shift,
//     a 64-bit add, two XORs) instead of (r ^ s) - s (…, a subtract pair);
//   * the exponent window [1087, 1138] is checked on (high word << 1) — the sign leaves, one VOP2 shift instead of a VOP3
//     bit-field extract — and the saturating-cast quirk by a running signed minimum of the results' high words (INT_MIN
//     <=> some magnitude has the high word 0x80000000; VOP2) instead of one 64-bit compare per value.
// The literal fall-back takes the original value (-tvn, exact) and is subtracted.
// The 1/1024 of the inverse transform is already in V: the blind-rotation kernels multiply with a bootstrap key whose device image
// carries it (`scale_bootstrap_key_kernel`); a power of two commutes with every rounding on the way, so the words are the same
// and 32 multiplications per polynomial are not executed.
// TWIST_AT_ONCE: the eight twist factors requested together ahead of the products (the latency shapes, one wave per SIMD: 3.572 ->
// 3.542 ms per 64, 6.695 -> 6.669 per 512; the four-per-workgroup shape is 0.1 % slower with it)
template <bool TWIST_AT_ONCE = false>
__device__ __forceinline__ void untwist_sub_from_negated(const c64 (&V)[8], const c64* twist_lds, uint64_t (&nacc)[16])
{
    double tvn[16];
    c64 twf[TWIST_AT_ONCE ? 8 : 1];
    if constexpr (TWIST_AT_ONCE) {
#pragma unroll
        for (int n1 = 0; n1 < 8; n1++) twf[n1] = twist_lds[64 * n1];
        compiler_fence();
    }
#pragma unroll
    for (int n1 = 0; n1 < 8; n1++) {
        const c64 xs = V[n1];
        const c64 tw = TWIST_AT_ONCE ? twf[TWIST_AT_ONCE ? n1 : 0] : twist_lds[64 * n1];
        // cmul_nf_conj negated: re = -(a.re b.re) - (a.im b.im), im = a.re b.im - a.im b.re
        tvn[n1] = -(xs.re * tw.re) - xs.im * tw.im;
        tvn[8 + n1] = xs.re * tw.im - xs.im * tw.re;
    }
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    int32_t qmin = 0x7FFFFFFF;
    uint64_t t[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint64_t b = (uint64_t)__double_as_longlong(tvn[e]);
        const uint32_t hi = (uint32_t)(b >> 32);
        const uint32_t k = hi << 1; // exponent field in bits 31..21, sign gone
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        const uint64_t r = b << (((hi >> 20) + 13u) & 63u);
        const int32_t rh = (int32_t)(uint32_t)(r >> 32);
        qmin = rh < qmin ? rh : qmin;
        const uint64_t sg = (uint64_t)((int64_t)b >> 63);
        t[e] = (r + sg) ^ sg;
    }
    if (__all(kmin >= (1087u << 21) && kmax < (1139u << 21) && qmin != (int32_t)0x80000000)) {
#pragma unroll
        for (int e = 0; e < 16; e++) nacc[e] += t[e];
    } else {
#pragma unroll
        for (int e = 0; e < 16; e++) nacc[e] -= f64_round_to_torus(-tvn[e]);
    }
}
// the same with the twist factors held in registers (the latency kernels)
__device__ __forceinline__ void untwist_to_torus_bits(const c64 (&V)[8], const c64 (&twist)[8], uint64_t (&t)[16])
{
    double tv[16];
#pragma unroll
    for (int n1 = 0; n1 < 8; n1++) {
        c64 xs = {V[n1].re * (1.0 / 1024.0), V[n1].im * (1.0 / 1024.0)};
        c64 u = cmul_nf_conj(xs, twist[n1]);
        tv[n1] = u.re;
        tv[8 + n1] = u.im;
    }
    torus_bits16(tv, t);
}

// ---- pieces shared by the latency-shape kernels (blind_rotate8 / cmux4) ----------

// RadixDecomposition of one torus word (math/radix.rs:81-113,157-162; simd/scalar.rs:52-71): round to
// the top L*LOGB bits (add the bit below), then L digits, least significant first, each reduced to
// [-B/2, B/2) with the carry going into the next; returned packed, LOGB bits per digit, two's
// complement inside each field.
template <int L, int LOGB>
__device__ __forceinline__ uint32_t gadget_digits_packed(uint64_t x)
{
    static_assert(L * LOGB <= 32, "packed digits need L*LOGB <= 32");
    constexpr int shift = 64 - L * LOGB;
    uint32_t s = (uint32_t)(x >> shift) + (uint32_t)((x >> (shift - 1)) & 1);
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < L; j++) {
        uint32_t d = s & ((1u << LOGB) - 1);
        s >>= LOGB;
        s += d >> (LOGB - 1);
        packed |= d << (j * LOGB);
    }
    return packed;
}

// complex sample of digit j: re from the packed word of coefficient c, im from that of c + N/2,
// sign-extended, converted to f64 and twisted (entities/polynomial.rs:257-274, scalar.rs:19-23)
// The two-digit case (L = 2, LOGB = 16) without the packed form: the rounded top word s = (x + 2^31) >> 32 itself is kept, and
//   digit 0 = sext16(s),   digit 1 = sext16((s >> 16) + bit15(s)) = (int)(s + 0x8000) >> 16
// (radix.rs:157-162: digit, shift, carry of digit >= B/2 into the next, digits as two's-complement small integers).
__device__ __forceinline__ c64 twisted_digit_top32(uint32_t s_re, uint32_t s_im, int j, c64 tw)
{
    const int dre = j == 0 ? (int)(int16_t)(s_re & 0xFFFFu) : (int)(s_re + 0x8000u) >> 16;
    const int dim = j == 0 ? (int)(int16_t)(s_im & 0xFFFFu) : (int)(s_im + 0x8000u) >> 16;
    return cmul_nf({(double)dre, (double)dim}, tw);
}

template <int LOGB>
__device__ __forceinline__ c64 twisted_digit(uint32_t packed_re, uint32_t packed_im, int j, c64 tw)
{
    const int sh = j * LOGB;
    int dre = ((int)(packed_re << (32 - LOGB - sh))) >> (32 - LOGB);
    int dim = ((int)(packed_im << (32 - LOGB - sh))) >> (32 - LOGB);
    return cmul_nf({(double)dre, (double)dim}, tw);
}

// ---- steps the two-waves-per-ciphertext kernels share (blind_rotate2p / cmux / cbs_trace / scheme_switch) ----
// Wave w of a pair owns the complex samples of parity w.  Parity is a template parameter wherever it selects registers: every
// choice is static, as in the bodies themselves (profiles/r12_shared_kernel_pieces.md: same code object with and without these).

// polynomial coefficient behind register e of the wave of parity w: c = half*1024 + 128*n1 + 2*lane + w, e = 8*half + n1
__device__ __forceinline__ int coef2(int e, int lane, int w) { return (e >> 3) * 1024 + (e & 7) * 128 + 2 * lane + w; }

// acc += k * x of the frequency-domain multiply-accumulate (complex_mad, AVX-512 order): four FMAs in this association
__device__ __forceinline__ void cmad(c64& acc, c64 k, c64 x)
{
    double re = __builtin_fma(k.re, x.re, acc.re);
    double im = __builtin_fma(k.re, x.im, acc.im);
    acc.re = __builtin_fma(-k.im, x.im, re);
    acc.im = __builtin_fma(k.im, x.re, im);
}

// The radix-2 stage across the two waves of a pair: wave 0 keeps registers 0..3 of a spectrum and hands over 4..7, wave 1 the
// other way round.  cross_put writes the half this wave does not keep into `image` (its own tile half or ring slot: 4 KiB
// per spectrum, value i of spectrum j at [(4j + i) * 64 + lane]); cross_take reads the partner's image into those registers.
template <int W> __device__ __forceinline__ void cross_put(char* image, int lane, const c64 (&x)[8])
{
#pragma unroll
    for (int i = 0; i < 4; i++) reinterpret_cast<c64*>(image)[i * 64 + lane] = x[W == 0 ? 4 + i : i];
}
template <int W> __device__ __forceinline__ void cross_put(char* image, int lane, const c64 (&x)[2][8])
{
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) reinterpret_cast<c64*>(image)[(j * 4 + i) * 64 + lane] = x[j][W == 0 ? 4 + i : i];
}
template <int W> __device__ __forceinline__ void cross_take(const char* image, int lane, c64 (&x)[8])
{
#pragma unroll
    for (int i = 0; i < 4; i++) x[W == 0 ? 4 + i : i] = reinterpret_cast<const c64*>(image)[i * 64 + lane];
}
template <int W> __device__ __forceinline__ void cross_take(const char* image, int lane, c64 (&x)[2][8])
{
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) x[j][W == 0 ? 4 + i : i] = reinterpret_cast<const c64*>(image)[(j * 4 + i) * 64 + lane];
}

// Ahead of the inverse transform pair: Ep = X[i] + X[i+4] (registers 0..3, kept by wave 0) and Op = (X[i] - X[i+4]) conj(W^k)
// (registers 4..7, kept by wave 1) of both product spectra; wc = this lane's cross twiddles, W1024^{lane + 64 (4w + i)} at wc[64 i]
__device__ __forceinline__ void inverse_split(const c64 (&prod)[2][8], const c64* wc, c64 (&WW)[2][8])
{
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const c64 wci = wc[64 * i];
            WW[q][i] = cadd(prod[q][i], prod[q][i + 4]);
            WW[q][4 + i] = cmul_tw<-1>(csub(prod[q][i], prod[q][i + 4]), wci);
        }
}

// Per-phase wall cycles of one wave, for the diagnostic build (-DSPF_STAMPS; s_memtime drains lgkmcnt: ~5 % overhead); empty
// otherwise.  mark(i) adds the time since the previous mark to slot i; flush writes the N sums to the wave's 16 words of
// `stamps` (null: nothing), where the host's stamp_report finds them.
template <int N> struct PhaseStamps {
    static_assert(N <= 16, "16 words per wave");
#ifdef SPF_STAMPS
    uint64_t acc[N], prev;
    __device__ __forceinline__ PhaseStamps() : acc{}, prev(__builtin_amdgcn_s_memtime()) {}
    __device__ __forceinline__ void mark(int i)
    {
        const uint64_t t = __builtin_amdgcn_s_memtime();
        acc[i] += t - prev;
        prev = t;
    }
    __device__ __forceinline__ void flush(uint64_t* stamps, size_t wave_index, int lane) const
    {
        if (stamps && lane == 0) {
#pragma unroll
            for (int i = 0; i < N; i++) stamps[wave_index * 16 + i] = acc[i];
        }
    }
#else
    __device__ __forceinline__ PhaseStamps() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush(uint64_t*, size_t, int) const {}
#endif
};

} // namespace spf
