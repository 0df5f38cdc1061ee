// spf_lwe_ring_pack.hpp — ring packing (Chen, Dai, Kim, Song: PackLWEs): p = 2^m LWE or GLWE ciphertexts into ONE GLWE under the
// context's automorphism key, p - 1 automorphism rounds in a tree of depth m and the first log2 N - m rounds of the trace behind it.
// A fixed composition of reference functions (include/spf_hip.h, "ring packing"):
//   leaf   c_j^(0) = polynomial_shr_round(embed(leaf j), log2 N)             (glwe_mod_switch_and_expand_pow_2's shift)
//   tree   c_r^(l) = (E + O) + round(E - O, L - l + 1), E = c_r^(l-1), O = X^(N/2^l) c_(r+cnt)^(l-1)     (mul_xn, add / sub, the
//          trace's loop body polynomial_pow_k + keyswitch_glwe_to_glwe, ops/automorphisms/mod.rs:72-83)
//   tail   x <- x + round(x, r), r = 1 .. L - m                               (ops/automorphisms/mod.rs:53-85, cut after L - m rounds)
// `embed` of an LWE of k N + 1 words is the GLWE whose sample_extract at index 0 (ops/ciphertext/glwe_ciphertext_ops.rs:31-76) is
// that LWE and whose body coefficients 1 .. N-1 are 0: a_i[0] = lwe[N i], a_i[c] = -lwe[N i + N - c], b[0] = lwe[k N].
// All additions wrap mod 2^64; the only floating point is the keyswitch, on exact input, in the order of the trace kernels: the
// words are the composition's.  Which launch reads and writes which rows: spf_lwe_ring_pack_plan.hpp.
//   ring_pack_kernel<6, 7, COMBINE>   N = 2048, k = 1, radix 6 levels x 7 bits: one tree level (COMBINE) or the tail, a sibling of
//                                     glwe_ks_body's trace mode — same schedule, same LDS key ring, same park — with two
//                                     operands at entry and a run-time count of rounds
//   generic_ring_pack_kernel          every other shape generic_glwe_ks_kernel takes: one workgroup per unit
//   ring_pack_leaf_kernel             p = 1 only: the leaf's embedding and shift, in front of the tail
// A sibling body, not new modes of glwe_ks_body: that body's instantiations (glwe_ks_kernel, glwe_ks_rows_kernel,
// glwe_ks_each_kernel) stay as the compiler made them.
#pragma once
#include "spf_glwe_keyswitch.hpp"

namespace spf {

// how a launch's operand rows are read (the values of spf_value_kind for the two leaf kinds)
enum RingPackSrc : uint32_t { RING_PACK_ROWS = 0, RING_PACK_LWE1 = 1, RING_PACK_GLWE1 = 2 };

__device__ __forceinline__ uint64_t ring_pack_shr_round(uint64_t x, uint32_t n) { return (x >> n) + ((x >> (n - 1)) & 1); }

// coefficient i of polynomial q of c^(0) of the leaf at `row` (RING_PACK_ROWS: of the GLWE at `row` as it is).  Every address is
// inside the row: an LWE's body is read for i = 0 only, its mask at N q + N - i in [N q + 1, N q + N - 1] for i > 0.
__device__ __forceinline__ uint64_t ring_pack_coef(gu64_cptr row, uint32_t src, uint32_t q, uint32_t i, uint32_t N, uint32_t k, uint32_t logN)
{
    if (src == RING_PACK_ROWS) return row[q * N + i];
    if (src == RING_PACK_GLWE1) return ring_pack_shr_round(row[q * N + i], logN);
    if (q == k) return i == 0 ? ring_pack_shr_round(row[k * N], logN) : (uint64_t)0;
    const uint64_t v = row[q * N + (i == 0 ? 0 : N - i)];
    return ring_pack_shr_round(i == 0 ? v : (uint64_t)0 - v, logN);
}

struct RingPackArgs {
    const uint64_t* src;  // COMBINE: 2 cnt operand rows per output (leaves, or the GLWEs of the level before); tail: `units` GLWEs
    uint64_t* out;        // `units` GLWEs of 4096 words, disjoint from every operand row of the launch
    const c64* key;       // COMBINE: the [L][2][1024] of the launch's round; tail: the automorphism key from round 1 on
    const c64* tables;
    uint32_t units;
    uint32_t cnt;         // COMBINE: nodes per output of this level (a power of two)
    uint32_t kk;          // COMBINE: the power of the round, 2^l + 1
    uint32_t x;           // COMBINE: the monomial on the odd operand, N / 2^l in 1 .. N/2
    uint32_t rounds;      // tail: rounds 1 .. rounds
    uint32_t src_kind;    // RingPackSrc (tail: RING_PACK_ROWS)
    uint32_t src_words;   // words from one operand row to the next: 4096, or 2049 for LWE leaves
};

// glwe_ks_body's trace mode (spf_glwe_keyswitch.hpp, where the schedule is explained) with
//   COMBINE   one round: S = E + X^x O stays in the accumulator, D = E - X^x O goes through the gather into the keyswitch:
//             out = S + keyswitch(D(X^kk)).  E is in registers before the first barrier; O is read while the staging region is
//             filled — the launch's result rows are disjoint from all its operand rows, so a late read sees what was there at launch
//   tail      rounds 1 .. a.rounds of the trace on a.src's item, out = x + sum of rounds; a.rounds >= 1
// The body half of the accumulator parks in the unit's own result row.  A padding unit of a ragged last workgroup is a duplicate of
// the last unit and stores nothing.
template <int L, int LOGB, int W, bool COMBINE>
__device__ __forceinline__ void ring_pack_body(const RingPackArgs& a, char* smem)
{
    static_assert(L == 6 && LOGB == 7, "three digit pairs; the state after the first pair fits 32 bits");
    constexpr int XP = 2;
    constexpr int NT = 512;
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
    const c64* key_base = a.key;
    {
        const double2* src = reinterpret_cast<const double2*>(a.tables);
        double2* dst = reinterpret_cast<double2*>(smem);
        for (int i = tid; i < kTableEntries; i += NT) dst[i] = src[i];
    }
    const uint32_t unit_raw = blockIdx.x * kWavesPerBlock + cslot;
    const bool owns_output = unit_raw < a.units;
    const uint32_t unit = owns_output ? unit_raw : a.units - 1;
    // operand rows (spf_lwe_ring_pack_plan.hpp): E = row (u / cnt) 2 cnt + u % cnt, O = cnt rows further; the tail's item is row u
    const uint32_t src_kind = COMBINE ? a.src_kind : (uint32_t)RING_PACK_ROWS;
    const size_t e_row = COMBINE ? (size_t)unit + (unit & ~(a.cnt - 1)) : (size_t)unit; // (cnt is a power of two)
    const gu64_cptr ge = global_view(a.src + e_row * a.src_words);
    [[maybe_unused]] const gu64_cptr go = global_view(a.src + (e_row + (COMBINE ? a.cnt : 0u)) * a.src_words);

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
#pragma unroll
    for (int e = 0; e < 16; e++) {
        accm[e] = ring_pack_coef(ge, src_kind, 0, (uint32_t)coef2(e, lane, w), kN, 1, 11);
        accb[e] = ring_pack_coef(ge, src_kind, 1, (uint32_t)coef2(e, lane, w), kN, 1, 11);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint32_t is_young = __builtin_amdgcn_readfirstlane(wv >= kWavesPerBlock ? 1u : 0u);
    uint32_t opaque_zero;
    asm volatile("s_mov_b32 %0, 0" : "=s"(opaque_zero));
    auto rendezvous = [&]() {
        do {
            pair_barrier_w();
        } while (opaque_zero != 0);
    };

    uint64_t* stage_mine = reinterpret_cast<uint64_t*>(mine);
    const c64* twist = tab + kTWOff + w * 512 + lane;
    const c64* wc = tab + kWCOff + 256 * w + lane;
    uint32_t chunk = 0;
    const uint32_t rounds = COMBINE ? 1u : a.rounds;
    const uint32_t total_chunks = rounds * 3;
    gu64_ptr park = global_view(a.out + (size_t)unit * 2 * kN) + (size_t)(w * 16 + 8) * 64 + lane;

#pragma unroll 1
    for (uint32_t it = 0; it < rounds; it++) {
        const uint32_t kk = COMBINE ? a.kk : (uint32_t)(kN >> it) + 1;
        uint32_t kinv = kk; // Newton iteration for the inverse of an odd number mod 2^12
        kinv *= 2 - kk * kinv; kinv *= 2 - kk * kinv; kinv *= 2 - kk * kinv; kinv *= 2 - kk * kinv;
        kinv &= 2 * kN - 1;
        const uint32_t cp0 = (uint32_t)(2 * lane + w) * kinv;
        uint32_t st[16];
        uint32_t d01[16];
#pragma unroll
        for (int p = 0; p < 2; p++) {
            auto take = [&](int e, uint64_t v) {
                if (p == 0) {
                    uint64_t s64 = radix_round_state<L, LOGB>(v);
                    const int d0 = next_digit<LOGB>(s64);
                    const int d1 = next_digit<LOGB>(s64);
                    d01[e] = ((uint32_t)d0 & 0xFFFFu) | ((uint32_t)d1 << 16);
                    st[e] = (uint32_t)s64;
                } else {
                    accb[e] += v; // (sum or x).b + trivial(b_k) ...
                }
            };
            if constexpr (COMBINE) {
                // X^x O (mul_xn): coefficient c is O[c - x] for c >= x and -O[c - x + N] below; the difference is staged, the
                // sum stays
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uint32_t c = (uint32_t)coef2(e, lane, w);
                    uint64_t o = ring_pack_coef(go, src_kind, (uint32_t)p, (c - a.x) & (uint32_t)(kN - 1), kN, 1, 11);
                    if (c < a.x) o = (uint64_t)0 - o;
                    const uint64_t ev = p == 0 ? accm[e] : accb[e];
                    stage_mine[(e >> 3) * 512 + (e & 7) * 64 + lane] = ev - o;
                    if (p == 0) accm[e] = ev + o;
                    else accb[e] = ev + o;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; e++) stage_mine[(e >> 3) * 512 + (e & 7) * 64 + lane] = p == 0 ? accm[e] : accb[e];
            }
            wave_lds_fence();
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
                const uint64_t sgn = (uint64_t)((int64_t)((uint64_t)cp << 52) >> 63);
                take(e, (gin[e] ^ sgn) - sgn);
            }
            if (p == 1 && owns_output) {
#pragma unroll
                for (int e = 0; e < 16; e++) park[(e - 8) * 64] = accb[e];
            }
            wave_lds_fence();
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
            if (m == 0) young_prio<0>(is_young);
            if (m == 2) young_prio<1>(is_young);
            if (m > 0) ring_dma(chunk);
            SPF_TRACE_PAIR<+1, XP>(VV[0], VV[1], mine, tab, lane);
            cross_put<w>(mine, lane, VV);
            if (m == 2) young_prio<0>(is_young);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
            if (m == 2) {
#pragma unroll
                for (int e = 0; e < 16; e++) accb[e] = park[(e - 8) * 64];
            }
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
            __syncthreads();
        }

        c64 WW[2][8];
        inverse_split(prod, wc, WW);
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
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            young_prio<1>(is_young);
        }
#pragma unroll
        for (int e = 0; e < 16; e++) asm volatile("" : "+v"(accb[e]));
        if constexpr (!COMBINE) {
            if (chunk < total_chunks) {
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
            for (int e = 0; e < 16; e++) accm[e] -= t[e];
            untwist_to_torus_bits<true>(WW[1], twist, t);
#pragma unroll
            for (int e = 0; e < 16; e++) accb[e] -= t[e];
        }
    }
    if (!owns_output) return;
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

template <int L, int LOGB, bool COMBINE>
__global__ __launch_bounds__(512, 2) void ring_pack_kernel(RingPackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) ring_pack_body<L, LOGB, 1, COMBINE>(a, smem);
    else ring_pack_body<L, LOGB, 0, COMBINE>(a, smem);
}

// ---------------------------------------------------------------------------------------------------------------
struct GenericRingPackArgs {
    GenericShape g;
    const uint64_t* src; // as RingPackArgs
    uint64_t* out;       // `units` GLWEs of (k+1) N words, one per workgroup
    const c64* key;      // combine: the keyswitch key of the launch's round; tail: the automorphism key from round 1 on
    uint32_t radix_log, count;
    uint32_t combine;    // 1: one tree level; 0: the tail
    uint32_t cnt, kk, x, rounds, src_kind, src_words;
};

// generic_glwe_ks_kernel's trace mode (spf_glwe_keyswitch.hpp) with the two-operand entry of a tree level and a run-time count of
// rounds; a sibling for the reason given there.  The workgroup holds the whole item in LDS and stores at its end only.
__global__ __launch_bounds__(kGenericThreads) void generic_ring_pack_kernel(GenericRingPackArgs a)
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
    const uint32_t u = blockIdx.x;
    const bool combine = a.combine != 0;
    const size_t e_row = combine ? (size_t)u + (u & ~(a.cnt - 1)) : (size_t)u; // (u / cnt) 2 cnt + u % cnt, cnt a power of two
    const gu64_cptr ge = global_view(a.src + e_row * a.src_words);
    if (combine) {
        // S = E + X^x O into X; D = E - X^x O straight through polynomial_pow_k into G
        const gu64_cptr go = global_view(a.src + (e_row + a.cnt) * a.src_words);
        for (uint32_t i = tid; i < len; i += kGenericThreads) {
            const uint32_t p = i / N, c = i % N, prod = c * a.kk;
            const uint64_t ev = ring_pack_coef(ge, a.src_kind, p, c, N, k, g.logN);
            uint64_t o = ring_pack_coef(go, a.src_kind, p, (c - a.x) & (N - 1), N, k, g.logN);
            if (c < a.x) o = (uint64_t)0 - o;
            X[i] = ev + o;
            const uint64_t d = ev - o;
            G[p * N + (prod & (N - 1))] = ((prod >> g.logN) & 1) ? (uint64_t)0 - d : d;
        }
    } else {
        for (uint32_t i = tid; i < len; i += kGenericThreads) X[i] = ge[i];
    }
    __syncthreads();
    const uint32_t rounds = combine ? 1 : a.rounds;
    const size_t glev_len = (size_t)a.count * (k + 1) * h, ksk_len = (size_t)k * glev_len;
    for (uint32_t it = 0; it < rounds; it++) {
        if (!combine) {
            const uint32_t kk = (N >> it) + 1;
            for (uint32_t i = tid; i < len; i += kGenericThreads) {
                const uint32_t p = i / N, c = i % N, prod = c * kk;
                const uint64_t v = X[i];
                G[p * N + (prod & (N - 1))] = ((prod >> g.logN) & 1) ? (uint64_t)0 - v : v;
            }
        }
        for (uint32_t i = tid; i < (k + 1) * h; i += kGenericThreads) accf[i] = {0.0, 0.0};
        __syncthreads();
        const c64* ksk = a.key + (size_t)it * ksk_len;
        for (uint32_t r = 0; r < k; r++)
            generic_glev_mad(g, accf, buf, state, ksk + (size_t)r * glev_len, a.radix_log, a.count,
                             [&](uint32_t i) { return G[r * N + i]; });
        for (uint32_t q = 0; q <= k; q++)
            generic_poly_ifft(g, accf + (size_t)q * h, buf, tmp, [&](uint32_t i, uint64_t t) {
                const uint64_t ks = (q == k ? G[k * N + i] : (uint64_t)0) - t;
                X[q * N + i] = X[q * N + i] + ks;
            });
    }
    uint64_t* out = a.out + (size_t)u * len;
    for (uint32_t i = tid; i < len; i += kGenericThreads) out[i] = X[i];
}

// p = 1: c^(0) of `units` leaves, one GLWE of (k+1) N words each, for the tail that follows
__global__ __launch_bounds__(256) void ring_pack_leaf_kernel(const uint64_t* leaves, uint64_t* out, uint32_t units, uint32_t src_kind,
                                                             uint32_t src_words, uint32_t N, uint32_t k, uint32_t logN)
{
    const uint32_t len = (k + 1) * N, u = blockIdx.x; // one workgroup per leaf
    if (u >= units) return;
    const gu64_cptr row = global_view(leaves + (size_t)u * src_words);
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x)
        out[(size_t)u * len + i] = ring_pack_coef(row, src_kind, i / N, i % N, N, k, logN);
}

} // namespace spf
