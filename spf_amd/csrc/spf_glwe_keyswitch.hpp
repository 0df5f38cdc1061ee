// spf_glwe_keyswitch.hpp — GLWE keyswitch, one automorphism round and the homomorphic trace as entry points of their own:
//   keyswitch_glwe_to_glwe   (sunscreen_tfhe/src/ops/fft_ops.rs:457-495; integer twin ops/keyswitch/glwe_keyswitch.rs:26-55)
//       out = (0, .., 0, b) - sum_i <decomp(a_i), KSK_i>
//   one automorphism round   (polynomial_pow_k, ops/polynomial/mod.rs:62-84, then the keyswitch back: the loop body of
//                             ops/automorphisms/mod.rs:72-83)
//   trace                    (ops/automorphisms/mod.rs:53-85): x <- x + automorphism_round(x) for rounds 1 .. log2 N
// The circuit bootstrap reaches the trace only behind its own prologue (cbs_trace_kernel / generic_trace_kernel,
// spf_cbs_tail.hpp / spf_generic.hpp: un-rotate, X^-level, shr_round); these kernels take the GLWE as it is, under the context's
// automorphism key or a keyswitch key of the caller's (spf_load_glwe_keyswitch_key_std).  Same arithmetic in the same order as
// the two trace kernels, which is the oracle's: same words.
//   glwe_ks_kernel<6, 7, MODE>  N = 2048, k = 1, radix 6 levels x 7 bits: the schedule of cbs_trace_kernel
//   generic_glwe_ks_kernel      every other shape: one workgroup per GLWE over generic_glev_mad / generic_poly_ifft
//   glwe_ks_rows_kernel<6, 7, MODE>, generic_glwe_ks_rows_kernel   their twins for operands where they lie, through a pointer
//                               table (a level of a gate graph); the output must not overlap any operand there
// One launch per call, items on grid.x.  `out == in` exactly is allowed in every mode (each work unit reads the whole of its own
// item, and nothing else, before the first workgroup barrier, and stores to its own item only behind it).
#pragma once
#include "spf_cbs_tail.hpp"
#include "spf_generic.hpp"

#include <type_traits>

namespace spf {

enum GlweKsMode { GLWE_KS_TRACE = 0, GLWE_KS_AUTOMORPHISM = 1, GLWE_KS_KEYSWITCH = 2 };

struct GlweKsArgs {
    const uint64_t* in;  // B x 4096
    uint64_t* out;       // B x 4096 (may be `in` itself)
    const c64* key;      // trace: [11][L][2][1024], every round; otherwise the [L][2][1024] of the one keyswitch
    const c64* tables;
    uint32_t units;      // B
    uint32_t kk;         // GLWE_KS_AUTOMORPHISM: the power of the round, N / 2^(round-1) + 1
};

// The same launch over operands where they lie (a level of a gate graph, spf_graph.hpp): item u is read through in_rows[u], the
// output stays `units` consecutive GLWEs.  Aliasing contract of the rows form: the output rows of a launch are disjoint from
// EVERY operand row of that launch — trace and automorphism park into a unit's output row before other workgroups have
// necessarily read their inputs, so `out == in` of the in-place form has no counterpart here.  The same operand may stand in the
// table several times (read-only).
struct GlweKsRowsArgs {
    const uint64_t* const* in_rows; // [B] device pointers to GLWEs of 4096 words
    uint64_t* out;                  // B x 4096, disjoint from every row of in_rows
    const c64* key;
    const c64* tables;
    uint32_t units;
    uint32_t kk;
};

// The rows form with the parameter PER ITEM (spf_glwe_keyswitch_each_*, spf_glwe_automorphism_each_*): the keyswitch-key slot or
// the automorphism round belongs to the item, not to the launch.  The four units of a workgroup share one LDS key ring, so they
// share their key: the host orders the items by parameter and pads every parameter's run to whole workgroups (the segment plan,
// spf_each_plan.hpp) and hands the kernel
//   wg[w]     the key base and kk of workgroup w (workgroup-uniform: scalar loads)
//   unit[u]   the operand pointer of unit u = 4 w + slot and the output row it owns, or spf_each::kNoRow — a padding unit: a
//             duplicate of an item of its own workgroup that reads, takes part in every barrier and stores nothing
// Both tables cover gridDim.x whole workgroups: no unit index is clamped.  The results land in the caller's order (unit u of item i
// writes row i of `out`).  Aliasing contract: that of GlweKsRowsArgs.  Keyswitch and automorphism modes only (the trace has no
// parameter).
struct GlweKsEachUnit {
    const uint64_t* in;
    uint32_t out_row, reserved;
};
struct GlweKsEachWg {
    const c64* key;
    uint32_t kk, reserved;
};
struct GlweKsEachArgs {
    const GlweKsEachUnit* unit; // [gridDim.x * kWavesPerBlock]
    const GlweKsEachWg* wg;     // [gridDim.x]
    uint64_t* out;              // the rows named by unit[].out_row, disjoint from every operand row
    const c64* tables;
};
constexpr uint32_t kGlweKsNoRow = 0xFFFFFFFFu; // (= spf_each::kNoRow; the launcher asserts it)

// ---------------------------------------------------------------------------------------------------------------
// The body of cbs_trace_kernel (spf_cbs_tail.hpp, where the schedule is explained: three transform pairs for the six digits, one
// inverse pair, the key rows through a 64 KiB LDS ring filled by LDS-DMA one digit pair ahead, bare workgroup barriers) in three
// modes:
//   trace          rounds 1 .. 11, X -> X^kk gather, out = x + ks, key chunks 3 (round - 1) + m of `key`
//   automorphism   one round with the caller's kk, out = ks, key chunks 0 .. 2
//   keyswitch      one round without the gather (kk = 1 is the identity), out = ks, key chunks 0 .. 2
// In the single-round modes every item reads the same 192 KiB of key, which stay in L2; the ring is kept (what it is worth
// there: profiles/r32_glwe_keyswitch.md).  The trace and the automorphism round park the body half of the accumulator in the unit's
// own output rows, as cbs_trace_body does (left to hipcc, the automorphism round kept those 32 registers in scratch); the
// keyswitch, without the gather, holds everything in registers.  The first store to an item is
// behind the workgroup barrier that follows the loads of every unit of the workgroup, padding units included — a padding unit
// of a ragged last workgroup is a duplicate of the last item, lives in that item's workgroup and stores nothing.
// `Args` is GlweKsArgs or GlweKsRowsArgs: only the entry loads differ.  The rows form loads the item's pointer once per wave (the
// unit is wave-uniform: a scalar load) where the in-place form computes in + unit * 2N; park, padding units and the wait in front of
// the first barrier are the same.  GlweKsEachArgs (above): the unit's pointer and output row and the workgroup's key and kk come
// from the two tables, four scalar loads per wave; everything behind the entry is the rows form's.
template <int L, int LOGB, int W, int MODE, class Args>
__device__ __forceinline__ void glwe_ks_body(const Args& a, char* smem)
{
    constexpr bool kEach = std::is_same<Args, GlweKsEachArgs>::value;
    constexpr bool kRows = std::is_same<Args, GlweKsRowsArgs>::value || kEach;
    static_assert(!kEach || MODE != GLWE_KS_TRACE, "the trace has no parameter");
    static_assert(L == 6 && LOGB == 7, "three digit pairs; the state after the first pair fits 32 bits");
    constexpr int XP = 2;
    constexpr int NT = 512;
    constexpr bool kTrace = MODE == GLWE_KS_TRACE;
    constexpr bool kPark = MODE != GLWE_KS_KEYSWITCH; // (the keyswitch has no gather and fits the register file as it is)
    constexpr uint32_t kRounds = kTrace ? 11 : 1;
    c64* tab = reinterpret_cast<c64*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cslot = wv >> 1;
    constexpr int w = W;
    char* tile = smem + kTableBytes + cslot * kWaveBufBytes;
    char* mine = tile + w * 8192;
    char* theirs = tile + (w ^ 1) * 8192;
    char* ring = smem + kTableBytes + kWavesPerBlock * kWaveBufBytes;
    // rows form: the item's pointer first — wave-uniform index, ONE scalar load per wave (a padding unit takes the last item's, as
    // below).  The table is read through the constant address space (nothing writes it while the kernel runs): as a plain global
    // load hipcc made it scalar in the W = 0 body only, and a vector load of one address in all lanes in the other
    [[maybe_unused]] gu64_cptr row_in = nullptr;
    [[maybe_unused]] uint32_t each_row = 0;
    const c64* key_base;
    uint32_t kk_arg;
    if constexpr (kEach) {
        typedef const GlweKsEachUnit __attribute__((address_space(4))) * unit_ptr;
        typedef const GlweKsEachWg __attribute__((address_space(4))) * wg_ptr;
        const unit_ptr up = (unit_ptr)(uintptr_t)a.unit + (blockIdx.x * kWavesPerBlock + cslot);
        const wg_ptr wp = (wg_ptr)(uintptr_t)a.wg + blockIdx.x;
        row_in = global_view(up->in);
        each_row = up->out_row;
        key_base = wp->key;
        kk_arg = wp->kk;
    } else {
        if constexpr (kRows) {
            typedef const uint64_t* const __attribute__((address_space(4))) * table_ptr;
            const uint32_t u = blockIdx.x * kWavesPerBlock + cslot;
            row_in = global_view(((table_ptr)(uintptr_t)a.in_rows)[u < a.units ? u : a.units - 1]);
        }
        key_base = a.key;
        kk_arg = a.kk;
    }
    {
        const double2* src = reinterpret_cast<const double2*>(a.tables);
        double2* dst = reinterpret_cast<double2*>(smem);
        for (int i = tid; i < kTableEntries; i += NT) dst[i] = src[i];
    }
    bool owns_output;
    uint32_t unit;
    if constexpr (kEach) {
        owns_output = each_row != kGlweKsNoRow;
        unit = owns_output ? each_row : 0u; // (a padding unit's row is never addressed)
    } else {
        const uint32_t unit_raw = blockIdx.x * kWavesPerBlock + cslot;
        owns_output = unit_raw < a.units;
        unit = owns_output ? unit_raw : a.units - 1;
    }

    // key chunk c = 3 round + m: the 64 KiB [level L-2-2m | level L-1-2m] of that round, copied as it lies: the first digit of
    // the pair (j = 2m, level L-1-2m) is the ring's second half
    const uint32_t dma_voff = (uint32_t)tid * 16u;
    const uint32_t dma_dst = lds_address(ring) + wv * 1024;
    auto ring_dma = [&](uint32_t chunk) {
        const uint32_t rnd = chunk / 3, m = chunk % 3;
        const char* src = reinterpret_cast<const char*>(key_base) +
                          (size_t)__builtin_amdgcn_readfirstlane(rnd * L + (L - 2 - 2 * m)) * kBskSlotBytes;
#pragma unroll
        for (int k = 0; k < 2 * kBskSlotBytes / (NT * 16); k++)
            lds_dma_piece(src + k * NT * 16, dma_voff, dma_dst + k * NT * 16);
    };
    ring_dma(0);

    uint64_t accm[16], accb[16];
    if constexpr (kRows) {
        // (a pointer fetched from memory is generic to the compiler: the view pins it to global, loads that count on vmcnt alone)
        gu64_cptr g = row_in;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            accm[e] = g[coef2(e, lane, w)];
            accb[e] = g[kN + coef2(e, lane, w)];
        }
    } else {
        const uint64_t* g = a.in + (size_t)unit * 2 * kN;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            accm[e] = g[coef2(e, lane, w)];
            accb[e] = g[kN + coef2(e, lane, w)];
        }
    }
    // every word of every item of this workgroup is in registers: from here on a unit may store to its own item
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint32_t is_young = __builtin_amdgcn_readfirstlane(wv >= kWavesPerBlock ? 1u : 0u);
    uint32_t opaque_zero;
    asm volatile("s_mov_b32 %0, 0" : "=s"(opaque_zero));
    auto rendezvous = [&]() { // bare s_barrier; the never-repeating loop gives each phase its own basic block
        do {
            pair_barrier_w();
        } while (opaque_zero != 0);
    };

    uint64_t* stage_mine = reinterpret_cast<uint64_t*>(mine);
    const c64* twist = tab + kTWOff + w * 512 + lane;
    const c64* wc = tab + kWCOff + 256 * w + lane;
    uint32_t chunk = 0;
    constexpr uint32_t total_chunks = kRounds * 3;
    // trace and automorphism round: the body half of the accumulator waits out the round in the unit's own 32 KiB of the output, fully coalesced:
    // word (w * 16 + e) * 64 + lane (cbs_trace_body)
    // (addressed from the middle of the 8 KiB a wave parks: every one of the 16 rows is within the signed 13-bit immediate of
    // ONE base register pair)
    gu64_ptr park = global_view(a.out + (size_t)unit * 2 * kN) + (size_t)(w * 16 + 8) * 64 + lane;

#pragma unroll 1
    for (uint32_t it = 0; it < kRounds; it++) {
        // automorphism X -> X^kk (ops/polynomial/mod.rs:62-84): out[d] = +-in[c], c kk = d mod 2N <=> c' = d kk^-1 mod 2N,
        // c = c' mod N, sign = c' >= N.  kk^-1 is odd: every source lies in this wave's own staging region.
        const uint32_t kk = kTrace ? (uint32_t)(kN >> it) + 1 : kk_arg;
        uint32_t kinv = kk; // Newton iteration for the inverse of an odd number mod 2^12
        kinv *= 2 - kk * kinv; kinv *= 2 - kk * kinv; kinv *= 2 - kk * kinv; kinv *= 2 - kk * kinv;
        kinv &= 2 * kN - 1;
        const uint32_t cp0 = (uint32_t)(2 * lane + w) * kinv;
        uint32_t st[16];  // digit state of the mask coefficients once digits 0 and 1 are out (28 bits)
        uint32_t d01[16]; // digits 0 and 1, sign-extended 16-bit halves
#pragma unroll
        for (int p = 0; p < 2; p++) {
            auto take = [&](int e, uint64_t v) {
                if (p == 0) { // keyswitch decomposes the mask
                    uint64_t s64 = radix_round_state<L, LOGB>(v);
                    const int d0 = next_digit<LOGB>(s64);
                    const int d1 = next_digit<LOGB>(s64);
                    d01[e] = ((uint32_t)d0 & 0xFFFFu) | ((uint32_t)d1 << 16);
                    st[e] = (uint32_t)s64;
                } else if constexpr (kTrace) {
                    accb[e] += v; // x.b + trivial(b_k) ...
                } else {
                    accb[e] = v; // trivial(b_k) ...
                }
            };
            if constexpr (MODE == GLWE_KS_KEYSWITCH) {
#pragma unroll
                for (int e = 0; e < 16; e++) take(e, p == 0 ? accm[e] : accb[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 16; e++) stage_mine[(e >> 3) * 512 + (e & 7) * 64 + lane] = p == 0 ? accm[e] : accb[e];
                wave_lds_fence(); // own writes, own reads: in-order LDS needs no barrier
                uint64_t gin[16];
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uint32_t cp = cp0 + (uint32_t)((e >> 3) * 1024 + (e & 7) * 128) * kinv;
                    gin[e] = *reinterpret_cast<const uint64_t*>(mine + ((cp << 2) & 0x1FF8u));
                }
                compiler_fence();
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uint32_t cp = cp0 + (uint32_t)((e >> 3) * 1024 + (e & 7) * 128) * kinv;
                    const uint64_t sgn = (uint64_t)((int64_t)((uint64_t)cp << 52) >> 63); // bit 11 of c', spread
                    take(e, (gin[e] ^ sgn) - sgn);
                }
            }
            if constexpr (kPark) {
                if (p == 1 && owns_output) {
#pragma unroll
                    for (int e = 0; e < 16; e++) park[(e - 8) * 64] = accb[e];
                }
            }
            if constexpr (MODE != GLWE_KS_KEYSWITCH) wave_lds_fence(); // gathered: the region may be overwritten
        }

        c64 prod[2][8];
#pragma unroll
        for (int m = 0; m < 3; m++, chunk++) {
            c64 VV[2][8];
#pragma unroll
            for (int n1 = 0; n1 < 8; n1++) {
                int dre[2], dim[2];
                if (m == 0) {
                    dre[0] = (int)(int16_t)(d01[n1] & 0xFFFFu); dre[1] = (int)d01[n1] >> 16;
                    dim[0] = (int)(int16_t)(d01[8 + n1] & 0xFFFFu); dim[1] = (int)d01[8 + n1] >> 16;
                } else {
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) {
                        uint64_t sr = st[n1], si = st[8 + n1];
                        dre[jj] = next_digit<LOGB>(sr);
                        dim[jj] = next_digit<LOGB>(si);
                        st[n1] = (uint32_t)sr;
                        st[8 + n1] = (uint32_t)si;
                    }
                }
                const c64 tw = twist[64 * n1];
                VV[0][n1] = cmul_nf({(double)dre[0], (double)dim[0]}, tw);
                VV[1][n1] = cmul_nf({(double)dre[1], (double)dim[1]}, tw);
            }
            // the ring is free since the barrier behind the previous MADs: rows of this pair (those of a round's first pair
            // were requested ahead of the previous round's inverse transforms, or at entry)
            if (m == 0) young_prio<0>(is_young);
            if (m == 2) young_prio<1>(is_young);
            if (m > 0) ring_dma(chunk);
            SPF_TRACE_PAIR<+1, XP>(VV[0], VV[1], mine, tab, lane);
            // radix-2 stage across the two waves, both digits in one exchange
            cross_put<w>(mine, lane, VV);
            if (m == 2) young_prio<0>(is_young);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // my share of the key rows has landed
            __syncthreads();
            if constexpr (w == 0) {
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const c64 in = reinterpret_cast<const c64*>(theirs)[(j * 4 + i) * 64 + lane];
                        const c64 t = cmul_tw<+1>(in, wc[64 * i]);
                        const c64 Ei = VV[j][i];
                        VV[j][i] = cadd(Ei, t);
                        VV[j][i + 4] = csub(Ei, t);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const c64 Ei = reinterpret_cast<const c64*>(theirs)[(j * 4 + i) * 64 + lane];
                        const c64 t = cmul_tw<+1>(VV[j][4 + i], wc[64 * i]);
                        VV[j][i] = cadd(Ei, t);
                        VV[j][i + 4] = csub(Ei, t);
                    }
            }
            if constexpr (kPark) {
                if (m == 2) {
                    // the parked body half comes back under the last multiply-accumulate and the inverse cross exchange
#pragma unroll
                    for (int e = 0; e < 16; e++) accb[e] = park[(e - 8) * 64];
                }
            }
            // ... - sum_j <digit_j(a), glev row L-1-j>, digits in order, both output polynomials (fft_ops.rs:489-494)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const c64* row = reinterpret_cast<const c64*>(ring + (1 - j) * kBskSlotBytes) + 256 * w + lane;
                c64 kb[2][2];
                auto key2 = [&](int grp, c64 (&dst)[2]) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int r = (grp * 2 + i) & 7, q = grp >> 2;
                        dst[i] = row[q * kHalf + 64 * (r & 3) + 512 * (r >> 2)];
                    }
                };
                key2(0, kb[0]);
#pragma unroll
                for (int grp = 0; grp < 8; grp++) {
                    if (grp + 1 < 8) key2(grp + 1, kb[(grp + 1) % 2]);
                    compiler_fence();
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int r = (grp * 2 + i) & 7, q = grp >> 2;
                        const bool first = m == 0 && j == 0;
                        c64 acc = {first ? 0.0 : prod[q][r].re, first ? 0.0 : prod[q][r].im};
                        cmad(acc, kb[grp % 2][i], VV[j][r]);
                        prod[q][r] = acc;
                    }
                }
            }
            __syncthreads(); // every wave is done with the ring and with its partner's cross data
        }

        // ---- back to the torus, both output polynomials together
        c64 WW[2][8];
        inverse_split(prod, wc, WW);
        // the inverse cross exchange goes through the key ring, one barrier (cbs_trace_body): wave v writes slot v, reads slot
        // v^1 and then refills exactly that slot with its share of the next key chunk
        {
            c64* slot_mine = reinterpret_cast<c64*>(ring + wv * 8192);
            const c64* slot_theirs = reinterpret_cast<const c64*>(ring + (wv ^ 1) * 8192);
            if constexpr (w == 0) {
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int i = 0; i < 4; i++) slot_mine[(q * 4 + i) * 64 + lane] = WW[q][4 + i];
            } else {
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int i = 0; i < 4; i++) slot_mine[(q * 4 + i) * 64 + lane] = WW[q][i];
            }
            rendezvous();
            if constexpr (w == 0) {
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int i = 0; i < 4; i++) WW[q][4 + i] = slot_theirs[(q * 4 + i) * 64 + lane];
            } else {
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int i = 0; i < 4; i++) WW[q][i] = slot_theirs[(q * 4 + i) * 64 + lane];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slot's contents are in registers
            young_prio<1>(is_young);
        }
        if constexpr (kPark) {
            // the parked accumulator half has landed BEFORE the next key rows are requested: vmcnt counts in order
#pragma unroll
            for (int e = 0; e < 16; e++) asm volatile("" : "+v"(accb[e]));
        }
        if constexpr (kTrace) {
            if (chunk < total_chunks) { // rows of the next round's first digit pair, this wave's share = the slot it just read
                const uint32_t rnd = chunk / 3;
                const char* src = reinterpret_cast<const char*>(key_base) +
                                  (size_t)__builtin_amdgcn_readfirstlane(rnd * L + (L - 2)) * kBskSlotBytes + (wv ^ 1) * 8192;
                const uint32_t lane16 = (uint32_t)lane * 16u;
                const uint32_t dst = lds_address(ring) + (wv ^ 1) * 8192;
#pragma unroll
                for (int k = 0; k < 8; k++) lds_dma_piece(src + k * 1024, lane16, dst + k * 1024);
            }
        }
        SPF_TRACE_PAIR<-1, XP>(WW[0], WW[1], mine, tab, lane);
        {
            uint64_t t[16];
            untwist_to_torus_bits<true>(WW[0], twist, t);
#pragma unroll
            for (int e = 0; e < 16; e++) accm[e] = (kTrace ? accm[e] : (uint64_t)0) - t[e];
            untwist_to_torus_bits<true>(WW[1], twist, t);
#pragma unroll
            for (int e = 0; e < 16; e++) accb[e] -= t[e];
        }
    }
    if (!owns_output) return;
    // the item's index and the lane through a statement the compiler can neither fold nor move: the store addresses are worked
    // out here, not kept from the loads at entry on (hipcc kept the sixteen coefficient indices of the trace in scratch)
    uint32_t unit_v = unit;
    int lane_out = lane;
    asm volatile("" : "+v"(unit_v), "+v"(lane_out));
    const uint32_t unit_out = __builtin_amdgcn_readfirstlane(unit_v);
    uint64_t* out = a.out + (size_t)unit_out * 2 * kN;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        out[coef2(e, lane_out, w)] = accm[e];
        out[kN + coef2(e, lane_out, w)] = accb[e];
    }
}

template <int L, int LOGB, int MODE>
__global__ __launch_bounds__(512, 2) void glwe_ks_kernel(GlweKsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) glwe_ks_body<L, LOGB, 1, MODE>(a, smem);
    else glwe_ks_body<L, LOGB, 0, MODE>(a, smem);
}

// The rows form (GlweKsRowsArgs above): same grid, same LDS, same body
template <int L, int LOGB, int MODE>
__global__ __launch_bounds__(512, 2) void glwe_ks_rows_kernel(GlweKsRowsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) glwe_ks_body<L, LOGB, 1, MODE>(a, smem);
    else glwe_ks_body<L, LOGB, 0, MODE>(a, smem);
}

// The per-item form (GlweKsEachArgs above): grid = the plan's workgroups, same LDS, same body
template <int L, int LOGB, int MODE>
__global__ __launch_bounds__(512, 2) void glwe_ks_each_kernel(GlweKsEachArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) glwe_ks_body<L, LOGB, 1, MODE>(a, smem);
    else glwe_ks_body<L, LOGB, 0, MODE>(a, smem);
}

// ---------------------------------------------------------------------------------------------------------------
struct GenericGlweKsArgs {
    GenericShape g;
    const uint64_t* in;  // B x (k+1) N
    uint64_t* out;       // B x (k+1) N (may be `in` itself)
    const c64* key;      // trace: [log2 N][row<k][level<count][poly<k+1][N/2]; otherwise one [row<k][level<count][poly<k+1][N/2]
    uint32_t radix_log, count;
    uint32_t mode;       // GlweKsMode
    uint32_t kk;         // GLWE_KS_AUTOMORPHISM: the power of the round
};

// The three modes for any (N, k, radix) that fits generic_trace_lds_bytes, one workgroup per GLWE: the round of
// generic_trace_kernel (spf_generic.hpp) without the circuit bootstrap's prologue.  The workgroup holds the whole item in LDS
// before it stores a word of it.
__global__ __launch_bounds__(kGenericThreads) void generic_glwe_ks_kernel(GenericGlweKsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GenericShape& g = a.g;
    const uint32_t tid = threadIdx.x, N = g.N, h = N / 2, k = g.k, len = (k + 1) * N;
    c64* accf = reinterpret_cast<c64*>(smem);
    c64* buf = accf + (size_t)(k + 1) * h;
    uint64_t* state = reinterpret_cast<uint64_t*>(buf + h);
    c64* tmp = reinterpret_cast<c64*>(state + N);
    uint64_t* X = state + 2 * N;
    uint64_t* G = X + len;
    const uint64_t* in = a.in + (size_t)blockIdx.x * len;
    for (uint32_t i = tid; i < len; i += kGenericThreads) X[i] = in[i];
    __syncthreads();
    const bool trace = a.mode == GLWE_KS_TRACE;
    const uint32_t rounds = trace ? g.logN : 1;
    const size_t glev_len = (size_t)a.count * (k + 1) * h, ksk_len = (size_t)k * glev_len;
    for (uint32_t it = 0; it < rounds; it++) {
        const uint32_t kk = trace ? (N >> it) + 1 : a.mode == GLWE_KS_AUTOMORPHISM ? a.kk : 1;
        // polynomial_pow_k (ops/polynomial/mod.rs:62-84): p_k[(i kk) mod N] = +-p[i], minus when (i kk) / N is odd; kk = 1: a copy
        for (uint32_t i = tid; i < len; i += kGenericThreads) {
            const uint32_t p = i / N, c = i % N, prod = c * kk;
            const uint64_t v = X[i];
            G[p * N + (prod & (N - 1))] = ((prod >> g.logN) & 1) ? (uint64_t)0 - v : v;
        }
        for (uint32_t i = tid; i < (k + 1) * h; i += kGenericThreads) accf[i] = {0.0, 0.0};
        __syncthreads();
        const c64* ksk = a.key + (size_t)it * ksk_len;
        for (uint32_t r = 0; r < k; r++)
            generic_glev_mad(g, accf, buf, state, ksk + (size_t)r * glev_len, a.radix_log, a.count,
                             [&](uint32_t i) { return G[r * N + i]; });
        // trivial(b_k) - ks, on top of x in the trace
        for (uint32_t q = 0; q <= k; q++)
            generic_poly_ifft(g, accf + (size_t)q * h, buf, tmp, [&](uint32_t i, uint64_t t) {
                const uint64_t ks = (q == k ? G[k * N + i] : (uint64_t)0) - t;
                X[q * N + i] = trace ? X[q * N + i] + ks : ks;
            });
    }
    uint64_t* out = a.out + (size_t)blockIdx.x * len;
    for (uint32_t i = tid; i < len; i += kGenericThreads) out[i] = X[i];
}

// The rows form (a level of a gate graph): item b is in_rows[b] (a.in is not read), the output a.out's B consecutive GLWEs, disjoint
// from every operand row (the contract of GlweKsRowsArgs; this kernel stores only at its end, but the contract is one for both).
// A sibling, not a shared body: with the loop in a __forceinline__ function of both kernels hipcc gave generic_glwe_ks_kernel 156
// VGPRs (arguments by reference) or 128 (by value) where it has 124 as written above; only the entry load differs — keep the two
// in step.
__global__ __launch_bounds__(kGenericThreads) void generic_glwe_ks_rows_kernel(GenericGlweKsArgs a, const uint64_t* const* in_rows)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GenericShape& g = a.g;
    const uint32_t tid = threadIdx.x, N = g.N, h = N / 2, k = g.k, len = (k + 1) * N;
    c64* accf = reinterpret_cast<c64*>(smem);
    c64* buf = accf + (size_t)(k + 1) * h;
    uint64_t* state = reinterpret_cast<uint64_t*>(buf + h);
    c64* tmp = reinterpret_cast<c64*>(state + N);
    uint64_t* X = state + 2 * N;
    uint64_t* G = X + len;
    gu64_cptr in = global_view(in_rows[blockIdx.x]); // (a fetched pointer is generic to the compiler: pinned to global)
    for (uint32_t i = tid; i < len; i += kGenericThreads) X[i] = in[i];
    __syncthreads();
    const bool trace = a.mode == GLWE_KS_TRACE;
    const uint32_t rounds = trace ? g.logN : 1;
    const size_t glev_len = (size_t)a.count * (k + 1) * h, ksk_len = (size_t)k * glev_len;
    for (uint32_t it = 0; it < rounds; it++) {
        const uint32_t kk = trace ? (N >> it) + 1 : a.mode == GLWE_KS_AUTOMORPHISM ? a.kk : 1;
        // polynomial_pow_k (ops/polynomial/mod.rs:62-84): p_k[(i kk) mod N] = +-p[i], minus when (i kk) / N is odd; kk = 1: a copy
        for (uint32_t i = tid; i < len; i += kGenericThreads) {
            const uint32_t p = i / N, c = i % N, prod = c * kk;
            const uint64_t v = X[i];
            G[p * N + (prod & (N - 1))] = ((prod >> g.logN) & 1) ? (uint64_t)0 - v : v;
        }
        for (uint32_t i = tid; i < (k + 1) * h; i += kGenericThreads) accf[i] = {0.0, 0.0};
        __syncthreads();
        const c64* ksk = a.key + (size_t)it * ksk_len;
        for (uint32_t r = 0; r < k; r++)
            generic_glev_mad(g, accf, buf, state, ksk + (size_t)r * glev_len, a.radix_log, a.count,
                             [&](uint32_t i) { return G[r * N + i]; });
        // trivial(b_k) - ks, on top of x in the trace
        for (uint32_t q = 0; q <= k; q++)
            generic_poly_ifft(g, accf + (size_t)q * h, buf, tmp, [&](uint32_t i, uint64_t t) {
                const uint64_t ks = (q == k ? G[k * N + i] : (uint64_t)0) - t;
                X[q * N + i] = trace ? X[q * N + i] + ks : ks;
            });
    }
    uint64_t* out = a.out + (size_t)blockIdx.x * len;
    for (uint32_t i = tid; i < len; i += kGenericThreads) out[i] = X[i];
}

// The per-item form: item b is unit[b].in under the key and kk of wg[b] (one unit per workgroup: the segment plan of
// spf_each_plan.hpp at units_per_wg = 1, where both tables have one entry per item and no padding), its result row
// unit[b].out_row of a.out.  a.in, a.key and a.kk are not read; a.mode is GLWE_KS_KEYSWITCH or GLWE_KS_AUTOMORPHISM (one round).
// The third sibling of the two kernels above, for the reason given there — keep the three in step.
__global__ __launch_bounds__(kGenericThreads) void generic_glwe_ks_each_kernel(GenericGlweKsArgs a, const GlweKsEachUnit* units,
                                                                               const GlweKsEachWg* wgs)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GenericShape& g = a.g;
    const uint32_t tid = threadIdx.x, N = g.N, h = N / 2, k = g.k, len = (k + 1) * N;
    c64* accf = reinterpret_cast<c64*>(smem);
    c64* buf = accf + (size_t)(k + 1) * h;
    uint64_t* state = reinterpret_cast<uint64_t*>(buf + h);
    c64* tmp = reinterpret_cast<c64*>(state + N);
    uint64_t* X = state + 2 * N;
    uint64_t* G = X + len;
    const GlweKsEachUnit unit = units[blockIdx.x]; // workgroup-uniform: scalar loads
    const GlweKsEachWg wg = wgs[blockIdx.x];
    gu64_cptr in = global_view(unit.in);
    for (uint32_t i = tid; i < len; i += kGenericThreads) X[i] = in[i];
    __syncthreads();
    const size_t glev_len = (size_t)a.count * (k + 1) * h;
    {
        const uint32_t kk = a.mode == GLWE_KS_AUTOMORPHISM ? wg.kk : 1;
        // polynomial_pow_k (ops/polynomial/mod.rs:62-84): p_k[(i kk) mod N] = +-p[i], minus when (i kk) / N is odd; kk = 1: a copy
        for (uint32_t i = tid; i < len; i += kGenericThreads) {
            const uint32_t p = i / N, c = i % N, prod = c * kk;
            const uint64_t v = X[i];
            G[p * N + (prod & (N - 1))] = ((prod >> g.logN) & 1) ? (uint64_t)0 - v : v;
        }
        for (uint32_t i = tid; i < (k + 1) * h; i += kGenericThreads) accf[i] = {0.0, 0.0};
        __syncthreads();
        const c64* ksk = wg.key;
        for (uint32_t r = 0; r < k; r++)
            generic_glev_mad(g, accf, buf, state, ksk + (size_t)r * glev_len, a.radix_log, a.count,
                             [&](uint32_t i) { return G[r * N + i]; });
        // trivial(b_k) - ks
        for (uint32_t q = 0; q <= k; q++)
            generic_poly_ifft(g, accf + (size_t)q * h, buf, tmp, [&](uint32_t i, uint64_t t) {
                X[q * N + i] = (q == k ? G[k * N + i] : (uint64_t)0) - t;
            });
    }
    if (unit.out_row == kGlweKsNoRow) return;
    uint64_t* out = a.out + (size_t)unit.out_row * len;
    for (uint32_t i = tid; i < len; i += kGenericThreads) out[i] = X[i];
}

} // namespace spf
