// spf_each_plan.hpp — the segment plan of a launch whose parameter is per item (spf_glwe_keyswitch_each_* and
// spf_glwe_automorphism_each_*, spf_glwe_keyswitch.hpp), free of HIP: tests/cpp/each_plan.cpp checks it on the CPU by brute force.
//
// The hand-written GLWE keyswitch kernel runs `units_per_wg` work units per workgroup over ONE key ring in LDS, so the units of a
// workgroup must share their key.  From B items with a parameter each (the keyswitch-key slot, the automorphism round) the plan
// makes, for a workgroup size of 1, 2 or 4 (the generic kernel: 1):
//   * the runs: the items ordered by parameter (parameters ascending, the items of one parameter in the caller's order — the
//     plan is a function of its input, not of a hash order), every run padded to whole workgroups;
//   * wg_param[w]: the parameter of workgroup w (the launcher turns it into the key base and kk);
//   * unit_item[u], unit_out[u]: the item unit u reads and the output row it writes.  The results land in the caller's order:
//     unit_out[u] == unit_item[u] for the unit that owns item i, kNoRow for a padding unit — the kernel's "duplicate of an item of
//     the same workgroup, stores nothing" (it reads, takes part in every barrier, and keeps its hands off the output);
//   * item_unit[i]: the unit that owns item i, the output permutation (a bijection of the items onto the owning units).
// The workgroup count is the sum over the runs of ceil(run / units_per_wg).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace spf_each {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;

struct Plan {
    uint32_t units_per_wg = 1;
    std::vector<uint64_t> wg_param;  // [workgroups]
    std::vector<uint32_t> unit_item; // [workgroups * units_per_wg]
    std::vector<uint32_t> unit_out;  // [workgroups * units_per_wg], kNoRow: a padding unit
    std::vector<uint32_t> item_unit; // [B]
    size_t workgroups() const { return wg_param.size(); }
    size_t units() const { return unit_item.size(); }
};

// items: indices into `params` (a launch takes the items of one radix shape; all of them: 0 .. B - 1), each at most once
inline Plan plan(const uint64_t* params, const std::vector<uint32_t>& items, size_t B, uint32_t units_per_wg)
{
    Plan p;
    p.units_per_wg = units_per_wg;
    p.item_unit.assign(B, kNoRow);
    std::vector<uint32_t> order(items);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return params[a] < params[b]; });
    for (size_t at = 0; at < order.size();) {
        size_t end = at;
        while (end < order.size() && params[order[end]] == params[order[at]]) end++;
        for (size_t w = at; w < end; w += units_per_wg) {
            p.wg_param.push_back(params[order[at]]);
            const size_t last = std::min(w + units_per_wg, end) - 1; // the padding units of a ragged workgroup repeat its last item
            for (size_t u = w; u < w + units_per_wg; u++) {
                const bool owns = u <= last;
                const uint32_t item = order[owns ? u : last];
                if (owns) p.item_unit[item] = (uint32_t)p.unit_item.size();
                p.unit_item.push_back(item);
                p.unit_out.push_back(owns ? item : kNoRow);
            }
        }
        at = end;
    }
    return p;
}

inline Plan plan(const uint64_t* params, size_t B, uint32_t units_per_wg)
{
    std::vector<uint32_t> all(B);
    std::iota(all.begin(), all.end(), 0u);
    return plan(params, all, B, units_per_wg);
}

} // namespace spf_each
