// The launch plan of ring packing (spf_amd/csrc/spf_lwe_ring_pack_plan.hpp) by brute force, on the CPU: a stand-alone program built
// from the HIP-free header alone (tests/test_lwe_ring_pack_plan.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer).
// For every N in {2, 4, 16, 64, 2048}, every p <= min(N, 64), k in {1, 3}, B <= 9 and caps from one output's worth upward it
// replays the launches on a model of the memory — every row of the leaves, the scratch and the output carries what it holds —
// and checks
//   operands     every operand row is a leaf, or a row written by an earlier launch of the same slice and not overwritten since,
//                and it holds exactly the node the definition puts there
//   disjoint     no result row of a launch is an operand row of that launch; no two units share a result row
//   scratch      every scratch row lies within the cap and within what scratch_words reports for the slice
//   outputs      row b of the output is written exactly once, by the last launch of its slice
//   parameters   rounds and X amounts equal the definition
//   launches     the launch count per slice equals the rule
//   padding      a padding slot of a ragged workgroup duplicates a unit of its own workgroup and stores nothing
#include "../../spf_amd/csrc/spf_lwe_ring_pack_plan.hpp"

#include <cstdio>
#include <map>
#include <set>
#include <string>

using namespace spf_ring_pack;

static long g_failed = 0, g_checked = 0;
#define CHECK(cond, ...)                                                                                                             \
    do {                                                                                                                             \
        g_checked++;                                                                                                                 \
        if (!(cond)) {                                                                                                               \
            if (g_failed++ < 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                            \
    } while (0)

// what a row holds: node r of level l of output b (level 0: the leaf), written by launch `by` of slice `slice`
struct Holds {
    int level = -2; // -2: never written, -1: the traced result
    size_t b = 0, r = 0, slice = 0;
    int by = -1;
    bool operator==(const Holds& o) const { return level == o.level && b == o.b && r == o.r; }
};

static void one_call(size_t B, size_t p, size_t N, size_t k, size_t cap)
{
    const uint32_t L = log2u(N), m = log2u(p);
    const size_t gw = (k + 1) * N;
    const std::vector<Slice> slices = plan(B, p, N, k, cap);
    const size_t per = slice_outputs(B, p, N, k, cap);
    CHECK(scratch_words(per, p, N, k) * 8 <= cap || per == 1, "B %zu p %zu N %zu cap %zu: %zu outputs per slice", B, p, N, cap, per);
    std::map<size_t, int> out_written;
    size_t next = 0;
    for (size_t si = 0; si < slices.size(); si++) {
        const Slice& s = slices[si];
        CHECK(s.at == next && s.nb >= 1 && s.nb <= per, "slice %zu at %zu nb %zu", si, s.at, s.nb);
        next = s.at + s.nb;
        CHECK(s.launches.size() == launches_per_slice(p, N), "p %zu N %zu: %zu launches", p, N, s.launches.size());
        CHECK(s.launches.size() == (p == 1 ? 2u : m + (p == N ? 0u : 1u)), "the rule, p %zu N %zu", p, N);
        const size_t rows = scratch_words(s.nb, p, N, k) / gw;
        CHECK(scratch_words(s.nb, p, N, k) % gw == 0, "whole rows");
        CHECK(rows * gw * 8 <= cap || s.nb == 1, "scratch %zu rows over the cap %zu", rows, cap);
        std::map<size_t, Holds> scratch; // fresh per slice: a slice may not count on what another left
        uint32_t level = 0;
        for (size_t li = 0; li < s.launches.size(); li++) {
            const Launch& l = s.launches[li];
            const bool last = li + 1 == s.launches.size();
            std::set<size_t> read_scratch, wrote_scratch, wrote_out;
            CHECK((l.dst.space == OUT) == last, "only the last launch writes the output (launch %zu)", li);
            CHECK(l.dst.space != LEAVES && l.src.space != OUT, "spaces");
            auto fetch = [&](size_t row, Holds want) {
                if (l.src.space == LEAVES) {
                    CHECK(want.level == 0 && row == want.b * p + want.r && row < B * p, "leaf row %zu", row);
                    return;
                }
                CHECK(row < rows, "operand row %zu outside the %zu scratch rows", row, rows);
                read_scratch.insert(row);
                const Holds h = scratch.count(row) ? scratch[row] : Holds{};
                CHECK(h == want && h.slice == si && h.by < (int)li, "scratch row %zu holds level %d b %zu r %zu, wanted level %d b %zu r %zu",
                      row, h.level, h.b, h.r, want.level, want.b, want.r);
            };
            auto store = [&](size_t row, Holds h) {
                h.slice = si;
                h.by = (int)li;
                if (l.dst.space == OUT) {
                    CHECK(row == h.b && row < B, "output row %zu for output %zu", row, h.b);
                    CHECK(wrote_out.insert(row).second, "output row %zu twice in a launch", row);
                    out_written[row]++;
                } else {
                    CHECK(row < rows, "result row %zu outside the %zu scratch rows", row, rows);
                    CHECK(wrote_scratch.insert(row).second, "scratch row %zu twice in a launch", row);
                }
            };
            std::map<size_t, Holds> pending;
            if (l.kind == LEAF) {
                CHECK(p == 1 && li == 0 && l.units == s.nb && l.src.space == LEAVES, "leaf launch");
                for (size_t u = 0; u < l.units; u++) {
                    fetch(l.src.row0 + u, Holds{0, s.at + u, 0});
                    store(l.dst.row0 + u, Holds{0, s.at + u, 0});
                    pending[l.dst.row0 + u] = Holds{0, s.at + u, 0, si, (int)li};
                }
            } else if (l.kind == COMBINE) {
                level++;
                const size_t cnt = p >> level;
                CHECK(l.cnt == cnt && l.units == s.nb * cnt, "level %u: cnt %u units %u", level, l.cnt, l.units);
                CHECK(l.round == L - level + 1 && l.rounds == 1, "level %u: round %u", level, l.round);
                CHECK((N >> (l.round - 1)) + 1 == ((size_t)1 << level) + 1, "level %u: t", level);
                CHECK(l.x == N >> level, "level %u: X^%u", level, l.x);
                CHECK((l.src.space == LEAVES) == (level == 1), "level %u reads the leaves", level);
                for (size_t u = 0; u < l.units; u++) {
                    const size_t b = s.at + u / cnt, r = u % cnt;
                    fetch(l.src.row0 + even_row(l, u), Holds{(int)level - 1, b, r});
                    fetch(l.src.row0 + odd_row(l, u), Holds{(int)level - 1, b, r + cnt});
                    store(l.dst.row0 + result_row(l, u), Holds{(int)level, b, r});
                    pending[l.dst.row0 + result_row(l, u)] = Holds{(int)level, b, r, si, (int)li};
                }
            } else {
                CHECK(last && l.units == s.nb && l.round == 1 && l.rounds == L - m && l.rounds >= 1, "tail: rounds %u", l.rounds);
                CHECK(level == m, "the tail follows level m");
                for (size_t u = 0; u < l.units; u++) {
                    fetch(l.src.row0 + u, Holds{(int)m, s.at + u, 0});
                    store(l.dst.row0 + u, Holds{-1, s.at + u, 0});
                }
            }
            for (size_t row : wrote_scratch) CHECK(!read_scratch.count(row), "launch %zu reads and writes scratch row %zu", li, row);
            if (l.dst.space == SCRATCH)
                for (auto& kv : pending) scratch[kv.first] = kv.second;
            else if (l.kind == COMBINE)
                CHECK(level == m && p == N, "a tree level writes the output only when p = N");
            // the hand-written kernel's padding
            for (size_t per_wg : {(size_t)1, (size_t)2, (size_t)4}) {
                const size_t slots = padded_slots(l.units, per_wg);
                CHECK(slots % per_wg == 0 && slots >= l.units && slots < l.units + per_wg, "slots");
                for (size_t sl = 0; sl < slots; sl++) {
                    const size_t u = slot_unit(sl, l.units);
                    CHECK(u < l.units && u / per_wg == sl / per_wg, "slot %zu stands for unit %zu of another workgroup", sl, u);
                    CHECK((slot_result(sl, l.units) == kNoRow) == (sl >= l.units), "slot %zu stores", sl);
                    if (sl < l.units) CHECK(u == sl && slot_result(sl, l.units) == sl, "slot %zu", sl);
                }
            }
        }
    }
    CHECK(next == B, "the slices cover %zu of %zu outputs", next, B);
    for (size_t b = 0; b < B; b++) CHECK(out_written[b] == 1, "output %zu written %d times", b, out_written[b]);
}

int main()
{
    long calls = 0;
    for (size_t N : {(size_t)2, (size_t)4, (size_t)16, (size_t)64, (size_t)2048})
        for (size_t k : {(size_t)1, (size_t)3})
            for (size_t p = 1; p <= N && p <= 64; p *= 2)
                for (size_t B = 0; B <= 9; B++) {
                    const size_t one = scratch_words(1, p, N, k) * 8;
                    // caps: one output's worth, every multiple up to the whole call and one beyond, odd byte counts between, the default
                    std::set<size_t> caps{one, one + 1, 2 * one - 1, 2 * one, 3 * one, 3 * one + 7, 4 * one, 8 * one, 9 * one, 10 * one,
                                          kDefaultScratchBytes};
                    for (size_t cap : caps) {
                        if (cap < one || cap == 0) continue;
                        one_call(B, p, N, k, cap);
                        calls++;
                    }
                }
    // the numbers of the header and of the GPU tests
    CHECK(launches_per_slice(32, 2048) == 6 && launches_per_slice(2048, 2048) == 11 && launches_per_slice(1, 2048) == 2, "launch rule");
    CHECK(rows_per_output(8, 2048) == 6 && rows_per_output(1, 16) == 1 && rows_per_output(2, 2) == 0 && rows_per_output(4, 4) == 2 &&
              rows_per_output(2, 16) == 1 && rows_per_output(4, 16) == 3,
          "scratch rows");
    {
        // N = 16, (B, p) = (7, 8) with a cap of three outputs' worth: slices of 3, 3 and 1
        const std::vector<Slice> s = plan(7, 8, 16, 1, 3 * scratch_words(1, 8, 16, 1) * 8);
        CHECK(s.size() == 3 && s[0].nb == 3 && s[1].nb == 3 && s[2].nb == 1 && s[2].at == 6, "the three-slice case");
    }
    CHECK(plan(0, 8, 16, 1, kDefaultScratchBytes).empty(), "B = 0");
    CHECK(!valid_p(0, 16) && !valid_p(3, 16) && !valid_p(32, 16) && valid_p(16, 16) && valid_p(1, 16), "valid_p");
    std::printf("calls: %ld planned and replayed\n", calls);
    std::printf("checks: %ld\n", g_checked);
    if (g_failed) {
        std::printf("FAILED: %ld checks\n", g_failed);
        return 1;
    }
    std::printf("lwe_ring_pack_plan ok\n");
    return 0;
}
