// spf_lwe_ring_pack_plan.hpp — the launch plan of spf_lwe_ring_pack_* (kernels: spf_lwe_ring_pack.hpp): which launches a call makes,
// over which rows, in how much scratch.  No HIP in this header: tests/cpp/lwe_ring_pack_plan.cpp builds it with the system compiler
// and checks it by brute force.
//
// The operation (include/spf_hip.h, "ring packing"): p = 2^m leaves per output, L = log2 N.
//   leaf     c_j^(0) = shr_round(embed(leaf j), L)
//   tree     level l = 1 .. m, cnt = p / 2^l nodes per output: c_r^(l) = (E + O) + round(E - O, L - l + 1) with E = c_r^(l-1),
//            O = X^(N / 2^l) c_(r+cnt)^(l-1)
//   tail     x = c_0^(m); x <- x + round(x, r) for r = 1 .. L - m
// One launch per tree level over the nodes of every output of the slice, one launch for the tail: m + 1 launches, m when p = N (no
// tail).  Level 1 reads the leaves where they lie (the kernels fuse the embedding and the shift into their entry load).  p = 1 has
// no tree level for the leaf to be fused into: a conversion launch in front of the tail, 2 launches.
//
// Rows.  Unit u of a level stands for node r = u % cnt of output b = u / cnt of the slice.  The level's operands are 2 cnt
// consecutive rows per output (the results of the level before it, or the output's p leaves): E is row b * 2 cnt + r, O row
// b * 2 cnt + r + cnt; the result is row u.  The results of level l lie in area A of the scratch (l odd) or in area B behind it
// (l even): a level reads one area and writes the other, so every result row of a launch is disjoint from every operand row of
// that launch (the rows contract of GlweKsRowsArgs: the hand-written kernel parks into its result row while other workgroups
// still read).  The last launch of a slice writes row b of the caller's output.
//   area A   nb * p / 2 rows when level 1 writes scratch (p < N or m > 1), one row per output when p = 1
//   area B   nb * p / 4 rows when level 2 writes scratch
// A call whose scratch would exceed the cap runs in slices over B, each with the whole scratch to itself (the stream orders them).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace spf_ring_pack {

constexpr size_t kDefaultScratchBytes = (size_t)1 << 30;
constexpr size_t kMaxUnitsPerLaunch = (size_t)1 << 30; // grid.x stays below 2^31 at one unit per workgroup

enum Kind : uint32_t { LEAF = 0, COMBINE = 1, TAIL = 2 };
enum Space : uint32_t { LEAVES = 0, SCRATCH = 1, OUT = 2 };

// where a launch reads or writes: rows (leaves: ciphertexts of the caller's leaf kind; otherwise GLWEs) counted from the start of
// the caller's leaves, of the scratch, or of the caller's output
struct Rows {
    Space space;
    size_t row0;
};

struct Launch {
    Kind kind;
    uint32_t units;  // LEAF, TAIL: the outputs of the slice; COMBINE: nb * cnt
    uint32_t cnt;    // COMBINE: nodes per output of this level (1 otherwise)
    uint32_t round;  // COMBINE: the automorphism round L - l + 1 (exponent t = 2^l + 1); TAIL: the first round, 1
    uint32_t rounds; // rounds run: COMBINE 1, TAIL L - m, LEAF 0
    uint32_t x;      // COMBINE: the monomial on O, N / 2^l
    Rows src, dst;
};

struct Slice {
    size_t at, nb; // outputs [at, at + nb) of the call
    std::vector<Launch> launches;
};

inline uint32_t log2u(size_t v)
{
    uint32_t l = 0;
    while (((size_t)1 << (l + 1)) <= v) l++;
    return l;
}

inline bool valid_p(size_t p, size_t N) { return p >= 1 && p <= N && (p & (p - 1)) == 0; }

// launches per slice: the rule of the header
inline uint32_t launches_per_slice(size_t p, size_t N) { return p == 1 ? 2u : log2u(p) + (p == N ? 0u : 1u); }

// scratch rows (GLWEs) one output needs
inline size_t area_a_rows(size_t p, size_t N) { return p == 1 ? 1 : (p == 2 && N == 2) ? 0 : p / 2; }
inline size_t area_b_rows(size_t p, size_t N) { return p < 4 ? 0 : (p == 4 && N == 4) ? 0 : p / 4; }
inline size_t rows_per_output(size_t p, size_t N) { return area_a_rows(p, N) + area_b_rows(p, N); }

// the scratch, in words, of ONE slice of nb outputs (spf_lwe_ring_pack_scratch_words; spf_lwe_ring_pack_enqueue is one slice)
inline size_t scratch_words(size_t nb, size_t p, size_t N, size_t k) { return nb * rows_per_output(p, N) * (k + 1) * N; }

// outputs per slice under a cap in bytes: as many as fit, at least one (a cap below one output's worth is raised to it)
inline size_t slice_outputs(size_t B, size_t p, size_t N, size_t k, size_t cap_bytes)
{
    const size_t one = scratch_words(1, p, N, k) * 8;
    size_t nb = one == 0 ? B : cap_bytes / one;
    const size_t by_grid = kMaxUnitsPerLaunch / (p > 1 ? p / 2 : 1);
    if (nb > by_grid) nb = by_grid;
    if (nb > B) nb = B;
    return nb < 1 ? 1 : nb;
}

// the cap of a call: SPF_LWE_RING_PACK_SCRATCH_BYTES (a testing knob, read at every call) or kDefaultScratchBytes
inline size_t scratch_cap_bytes()
{
    if (const char* e = std::getenv("SPF_LWE_RING_PACK_SCRATCH_BYTES")) {
        char* end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end != e && v > 0) return (size_t)v;
    }
    return kDefaultScratchBytes;
}

// the launches of one slice of nb outputs that begins at output `at` of the call
inline Slice plan_slice(size_t at, size_t nb, size_t p, size_t N)
{
    Slice s{at, nb, {}};
    const uint32_t L = log2u(N), m = log2u(p);
    const size_t a_rows = nb * area_a_rows(p, N); // area B begins behind area A
    if (p == 1) {
        s.launches.push_back({LEAF, (uint32_t)nb, 1, 0, 0, 0, {LEAVES, at}, {SCRATCH, 0}});
        s.launches.push_back({TAIL, (uint32_t)nb, 1, 1, L, 0, {SCRATCH, 0}, {OUT, at}});
        return s;
    }
    Rows prev{LEAVES, at * p};
    for (uint32_t l = 1; l <= m; l++) {
        const size_t cnt = p >> l;
        const bool last = l == m && p == N;
        const Rows dst = last ? Rows{OUT, at} : Rows{SCRATCH, (l & 1) ? 0 : a_rows};
        s.launches.push_back({COMBINE, (uint32_t)(nb * cnt), (uint32_t)cnt, L - l + 1, 1, (uint32_t)(N >> l), prev, dst});
        prev = dst;
    }
    if (p != N) s.launches.push_back({TAIL, (uint32_t)nb, 1, 1, L - m, 0, prev, {OUT, at}});
    return s;
}

// The slice loop of the host-pointer form: the slices of a call of B outputs under the cap, in the order they are enqueued.
inline std::vector<Slice> plan(size_t B, size_t p, size_t N, size_t k, size_t cap_bytes)
{
    std::vector<Slice> out;
    if (B == 0) return out;
    const size_t per = slice_outputs(B, p, N, k, cap_bytes);
    size_t done = 0;
    while (done < B) {
        const size_t nb = B - done < per ? B - done : per;
        out.push_back(plan_slice(done, nb, p, N));
        done = done + nb;
    }
    return out;
}

// ---- what the kernels work out per unit (the same expressions stand in spf_lwe_ring_pack.hpp) ---------------------------------

// operand rows of unit u of a COMBINE launch, counted from src.row0, and its result row, counted from dst.row0
inline size_t even_row(const Launch& l, size_t u) { return (u / l.cnt) * 2 * l.cnt + u % l.cnt; }
inline size_t odd_row(const Launch& l, size_t u) { return even_row(l, u) + l.cnt; }
inline size_t result_row(const Launch&, size_t u) { return u; }

// The hand-written kernel runs four units per workgroup: a ragged last workgroup is padded the way the each-plan pads its runs —
// slot s of the grid stands for unit min(s, units - 1), and a slot past the units stores nothing.
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
inline size_t padded_slots(size_t units, size_t per_wg) { return (units + per_wg - 1) / per_wg * per_wg; }
inline size_t slot_unit(size_t slot, size_t units) { return slot < units ? slot : units - 1; }
inline uint32_t slot_result(size_t slot, size_t units) { return slot < units ? (uint32_t)slot : kNoRow; }

} // namespace spf_ring_pack
