// The segment plan of the per-item-parameter launches (spf_amd/csrc/spf_each_plan.hpp) on the CPU: a stand-alone program built
// from the HIP-free header alone (g++, AddressSanitizer + UndefinedBehaviorSanitizer; tests/test_each_plan.py).  For units per
// workgroup 1, 2 and 4 it plans every assignment of up to 5 parameters to up to 7 items, seeded random cases of up to 20 items, and
// the named corner cases, and checks each plan by brute force against the four statements of check().
#include "../../spf_amd/csrc/spf_each_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

static int g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            g_failed++;                                    \
            return false;                                  \
        }                                                  \
    } while (0)

static bool check(const std::vector<uint64_t>& params, const std::vector<uint32_t>& items, uint32_t upw)
{
    const size_t B = params.size();
    const spf_each::Plan p = spf_each::plan(params.data(), items, B, upw);
    // the workgroup count is the sum over runs of ceil(run / units per workgroup)
    std::map<uint64_t, size_t> run;
    for (uint32_t i : items) run[params[i]]++;
    size_t want_wgs = 0;
    for (const auto& r : run) want_wgs += (r.second + upw - 1) / upw;
    CHECK(p.units_per_wg == upw && p.workgroups() == want_wgs, "workgroups %zu, want %zu", p.workgroups(), want_wgs);
    CHECK(p.units() == want_wgs * upw && p.unit_out.size() == p.units() && p.item_unit.size() == B, "table sizes");
    // every item owns exactly one unit and one distinct output row; the permutation is a bijection
    std::vector<int> owners(B, 0);
    std::set<uint32_t> rows;
    for (size_t u = 0; u < p.units(); u++) {
        CHECK(p.unit_item[u] < B, "unit %zu reads item %u of %zu", u, p.unit_item[u], B);
        if (p.unit_out[u] == spf_each::kNoRow) continue;
        CHECK(p.unit_out[u] == p.unit_item[u], "unit %zu writes row %u of item %u", u, p.unit_out[u], p.unit_item[u]);
        owners[p.unit_item[u]]++;
        rows.insert(p.unit_out[u]);
    }
    std::set<uint32_t> in_launch(items.begin(), items.end());
    for (size_t i = 0; i < B; i++) {
        const bool mine = in_launch.count((uint32_t)i) != 0;
        CHECK(owners[i] == (mine ? 1 : 0), "item %zu is owned by %d units", i, owners[i]);
        if (!mine) {
            CHECK(p.item_unit[i] == spf_each::kNoRow, "item %zu of another launch has a unit", i);
            continue;
        }
        const uint32_t u = p.item_unit[i];
        CHECK(u < p.units() && p.unit_item[u] == i && p.unit_out[u] == i, "item %zu: the permutation points at unit %u", i, u);
    }
    CHECK(rows.size() == items.size(), "%zu distinct rows for %zu items", rows.size(), items.size());
    for (size_t w = 0; w < p.workgroups(); w++) {
        std::set<uint32_t> owned;
        for (uint32_t s = 0; s < upw; s++) {
            const size_t u = w * upw + s;
            // all units of a workgroup carry one parameter
            CHECK(params[p.unit_item[u]] == p.wg_param[w], "unit %zu: parameter %llu in a workgroup of %llu", u,
                  (unsigned long long)params[p.unit_item[u]], (unsigned long long)p.wg_param[w]);
            if (p.unit_out[u] != spf_each::kNoRow) owned.insert(p.unit_item[u]);
        }
        CHECK(!owned.empty(), "workgroup %zu owns nothing", w);
        // a padding unit duplicates an item of its own workgroup and owns no output
        for (uint32_t s = 0; s < upw; s++) {
            const size_t u = w * upw + s;
            if (p.unit_out[u] == spf_each::kNoRow) CHECK(owned.count(p.unit_item[u]) == 1, "padding unit %zu reads item %u of another workgroup", u, p.unit_item[u]);
        }
    }
    // parameters ascending over the workgroups: a run is never split around another
    for (size_t w = 1; w < p.workgroups(); w++) CHECK(p.wg_param[w - 1] <= p.wg_param[w], "runs out of order at workgroup %zu", w);
    return true;
}

static bool check_all(const std::vector<uint64_t>& params, uint32_t upw)
{
    std::vector<uint32_t> all(params.size());
    for (size_t i = 0; i < all.size(); i++) all[i] = (uint32_t)i;
    return check(params, all, upw);
}

static void named(const char* name, const std::vector<uint64_t>& params)
{
    bool ok = true;
    for (uint32_t upw : {1u, 2u, 4u}) ok = check_all(params, upw) && ok;
    std::printf("%s: %zu items %s\n", name, params.size(), ok ? "ok" : "FAILED");
}

int main()
{
    named("no item", {});
    named("one item", {3});
    named("all items equal", std::vector<uint64_t>(13, 7));
    named("all items distinct", {9, 4, 11, 0, 15, 2, 8, 1, 14, 3, 5});
    named("one run of exactly a workgroup", {6, 6, 6, 6});
    named("a run of exactly a workgroup between two ragged ones", {1, 6, 2, 6, 1, 6, 2, 6, 2, 1, 1, 1, 1});
    named("runs of 1, 3 and 5, interleaved", {5, 9, 2, 9, 5, 9, 5, 9, 9});
    named("parameters at the top of 64 bits", {~(uint64_t)0, 0, ~(uint64_t)0, (uint64_t)1 << 63, 0});

    // every assignment of up to 5 parameters to up to 7 items
    size_t exhaustive = 0;
    bool ok = true;
    for (size_t B = 1; B <= 7; B++) {
        size_t total = 1;
        for (size_t i = 0; i < B; i++) total *= 5;
        std::vector<uint64_t> params(B);
        for (size_t code = 0; code < total; code++) {
            size_t c = code;
            for (size_t i = 0; i < B; i++, c /= 5) params[i] = 10 * (c % 5);
            for (uint32_t upw : {1u, 2u, 4u}) ok = check_all(params, upw) && ok;
            exhaustive++;
        }
    }
    std::printf("exhaustive: %zu assignments %s\n", exhaustive, ok ? "ok" : "FAILED");

    // seeded random cases of up to 20 items, 1 .. 5 distinct parameters; half of them plan a subset (a launch per radix shape)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    size_t random_cases = 0;
    ok = true;
    for (int it = 0; it < 4000; it++) {
        const size_t B = 1 + rnd() % 20, distinct = 1 + rnd() % 5;
        std::vector<uint64_t> params(B);
        for (auto& v : params) v = rnd() % distinct;
        std::vector<uint32_t> items;
        const bool subset = it & 1;
        for (size_t i = 0; i < B; i++)
            if (!subset || rnd() % 3) items.push_back((uint32_t)i);
        for (uint32_t upw : {1u, 2u, 4u}) ok = check(params, items, upw) && ok;
        random_cases++;
    }
    std::printf("random: %zu cases %s\n", random_cases, ok ? "ok" : "FAILED");

    if (g_failed) {
        std::printf("each_plan FAILED: %d checks\n", g_failed);
        return 1;
    }
    std::printf("each_plan ok\n");
    return 0;
}
