// spf_arena_plan.hpp — where the groups of a gate graph write: arena rows reused once their value is dead.
//
// The executor (spf_graph.hpp) runs a graph as one stream of launches in group order, groups ordered by level.  A group writes
// one contiguous block of equal rows, one row per member; every row is read by launches of later levels only.  So a row is
// free for any group of a level strictly above the level of its last reader (`death`): the stream orders the writer after
// every reader, and no launch is handed a row it reads as its output.  Nothing else is needed — no events, no second stream.
// The reference gets the same effect by dropping a task's output when its last dependent has run
// (circuit_processor/mod.rs:130-253).
//
// Allocation is contiguous first-fit over a coalescing free list ordered by offset.  Blocks start on kAlign bytes; rows go
// back one by one as they die (a block dies row by row: freeing whole blocks only leaves half of the saving unused).  The
// work is one ordered-map operation per row plus one walk over the free list per group, and the layout depends on nothing but
// the group list.  With every death at kNever nothing is ever released and the layout is the plain one: block after block,
// which is what spf_graph.hpp's plan() lays out today.
//
// Free of HIP (as spf_wake.hpp): tests/cpp/arena_plan.cpp drives it on the CPU.  The executor does not include it yet: plan()
// still gives every node a row for the life of the graph (profiles/r20_graph_memory.md).
#pragma once

#include <cstddef>
#include <cstdint>
#include <iterator>
#include <map>
#include <utility>
#include <vector>

namespace spf_arena {

constexpr uint32_t kNever = 0xffffffffu; // death of a row that lives to the end of the run (an output)
constexpr size_t kAlign = 256;           // every block starts on a multiple of this

struct Group {
    uint32_t level;        // groups come in non-decreasing level order
    size_t row_bytes;      // > 0
    size_t rows;           // > 0
    const uint32_t* death; // [rows] level of the row's last reader (>= level is expected; less counts as `level`), or kNever
    size_t offset;         // out: the block is [offset, offset + rows * row_bytes), row i at offset + i * row_bytes
};

inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// Lays the groups out above `base` (the region of inputs and constants, never reused) and returns the arena's size.
inline size_t plan(size_t base, Group* groups, size_t n)
{
    std::map<size_t, size_t> free_; // offset -> length, disjoint, no two adjacent
    auto release = [&](size_t off, size_t len) {
        if (!len) return;
        auto next = free_.lower_bound(off);
        if (next != free_.begin()) {
            auto prev = std::prev(next);
            if (prev->first + prev->second == off) {
                off = prev->first;
                len += prev->second;
                free_.erase(prev);
            }
        }
        if (next != free_.end() && off + len == next->first) {
            len += next->second;
            free_.erase(next);
        }
        free_[off] = len;
    };
    // rows waiting for their death level to pass, in the order they were allocated
    std::map<uint32_t, std::vector<std::pair<size_t, size_t>>> dying;
    size_t top = base;
    for (size_t gi = 0; gi < n; gi++) {
        Group& g = groups[gi];
        while (!dying.empty() && dying.begin()->first < g.level) {
            for (const auto& r : dying.begin()->second) release(r.first, r.second);
            dying.erase(dying.begin());
        }
        const size_t need = g.rows * g.row_bytes;
        size_t at = 0;
        bool found = false;
        for (auto it = free_.begin(); it != free_.end(); ++it) {
            const size_t s = it->first, e = s + it->second, a = align_up(s);
            if (a < e && e - a >= need) {
                free_.erase(it);
                release(s, a - s);
                release(a + need, e - (a + need));
                at = a;
                found = true;
                break;
            }
        }
        if (!found) {
            // grow the arena — from the start of the free range that touches its end, where there is one
            size_t s = top;
            if (!free_.empty()) {
                auto last = std::prev(free_.end());
                if (last->first + last->second == top) {
                    s = last->first;
                    free_.erase(last);
                }
            }
            at = align_up(s);
            release(s, at - s);
            top = at + need;
        }
        g.offset = at;
        // rows of one death next to each other go back as one range
        for (size_t i = 0; i < g.rows;) {
            const uint32_t d = g.death[i];
            size_t j = i + 1;
            while (j < g.rows && g.death[j] == d) j++;
            if (d != kNever) dying[d < g.level ? g.level : d].emplace_back(at + i * g.row_bytes, (j - i) * g.row_bytes);
            i = j;
        }
    }
    return align_up(top);
}

} // namespace spf_arena
