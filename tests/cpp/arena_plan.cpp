// arena_plan.cpp — the arena planner of the gate graphs (spf_amd/csrc/spf_arena_plan.hpp) on the CPU.
//
// Built from the HIP-free header alone with g++ -fsanitize=address,undefined and run directly (tests/test_arena_plan.py).
//   arena_plan                      seeded random group lists
//   arena_plan FILE MAX_NUM MAX_DEN  a circuit's groups as a file of numbers (format below); the arena may be at most
//                                    MAX_NUM / MAX_DEN of the circuit's values_bytes
// Checked on every list: no two rows whose lifetimes overlap share a byte; every group is one contiguous 256-aligned block
// above the input region; peak live bytes <= arena <= the layout without reuse; a second run gives the same layout; with every
// death at kNever the layout is block after block.
//
// File format (unsigned decimal numbers, white space between them):
//   base n_groups   then per group   level row_bytes rows death[0] ... death[rows-1]     (death 4294967295 = never)
#include "../../spf_amd/csrc/spf_arena_plan.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

struct List {
    size_t base = 0;
    std::vector<uint32_t> level;
    std::vector<size_t> row_bytes, rows;
    std::vector<std::vector<uint32_t>> death;
    size_t groups() const { return level.size(); }
};

struct Row { size_t off, len; uint32_t born, dies; }; // alive on levels born ..= dies

int g_failed = 0;
void fail(const std::string& what, const char* msg, size_t a = 0, size_t b = 0)
{
    g_failed++;
    std::printf("FAILED %s: %s (%zu, %zu)\n", what.c_str(), msg, a, b);
}

std::vector<size_t> run(const List& l, size_t* arena)
{
    std::vector<spf_arena::Group> g(l.groups());
    for (size_t i = 0; i < g.size(); i++) g[i] = spf_arena::Group{l.level[i], l.row_bytes[i], l.rows[i], l.death[i].data(), (size_t)-1};
    *arena = spf_arena::plan(l.base, g.data(), g.size());
    std::vector<size_t> off(g.size());
    for (size_t i = 0; i < g.size(); i++) off[i] = g[i].offset;
    return off;
}

std::vector<Row> rows_of(const List& l, const std::vector<size_t>& off)
{
    std::vector<Row> r;
    for (size_t i = 0; i < l.groups(); i++)
        for (size_t j = 0; j < l.rows[i]; j++) {
            const uint32_t d = l.death[i][j];
            r.push_back(Row{off[i] + j * l.row_bytes[i], l.row_bytes[i], l.level[i], d == spf_arena::kNever ? d : std::max(d, l.level[i])});
        }
    return r;
}

// most bytes alive at one level (on top of the input region): what no layout can go below
size_t peak_live(const List& l, const std::vector<Row>& rows)
{
    uint32_t top = 0;
    for (uint32_t lv : l.level) top = std::max(top, lv);
    std::vector<int64_t> delta(top + 2, 0);
    for (const Row& r : rows) {
        delta[r.born] += (int64_t)r.len;
        delta[std::min<uint64_t>((uint64_t)r.dies + 1, top + 1)] -= (int64_t)r.len;
    }
    int64_t live = 0, peak = 0;
    for (uint32_t lv = 0; lv <= top; lv++) {
        live += delta[lv];
        peak = std::max(peak, live);
    }
    return l.base + (size_t)peak;
}

// all pairs (exact, quadratic)
void check_pairs(const std::string& what, const std::vector<Row>& rows)
{
    for (size_t a = 0; a < rows.size(); a++)
        for (size_t b = a + 1; b < rows.size(); b++) {
            const Row &x = rows[a], &y = rows[b];
            const bool bytes = x.off < y.off + y.len && y.off < x.off + x.len;
            const bool time = !(y.born > x.dies) && !(x.born > y.dies);
            if (bytes && time) return fail(what, "two rows alive at the same level share a byte", a, b);
        }
}

// the same property for lists too long for all pairs: level by level, the live rows in an offset-ordered map
void check_sweep(const std::string& what, std::vector<Row> rows)
{
    std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.born < y.born; });
    std::multimap<uint32_t, size_t> dying; // dies -> offset
    std::map<size_t, size_t> live;         // offset -> len
    for (size_t i = 0; i < rows.size(); i++) {
        const Row& r = rows[i];
        while (!dying.empty() && dying.begin()->first < r.born) {
            live.erase(dying.begin()->second);
            dying.erase(dying.begin());
        }
        auto next = live.lower_bound(r.off);
        if (next != live.end() && next->first < r.off + r.len) return fail(what, "a row is written over a live one", i, next->first);
        if (next != live.begin()) {
            auto prev = std::prev(next);
            if (prev->first + prev->second > r.off) return fail(what, "a row is written over a live one", i, prev->first);
        }
        live[r.off] = r.len;
        dying.emplace(r.dies, r.off);
    }
}

size_t check(const std::string& what, const List& l, bool pairs)
{
    size_t arena = 0, arena2 = 0;
    const std::vector<size_t> off = run(l, &arena);
    if (off != run(l, &arena2) || arena != arena2) fail(what, "two runs give different layouts");
    size_t plain = l.base, need_end = l.base;
    for (size_t i = 0; i < l.groups(); i++) {
        if (off[i] % spf_arena::kAlign) fail(what, "a group is not 256-aligned", i, off[i]);
        if (off[i] < l.base) fail(what, "a group lies in the input region", i, off[i]);
        need_end = std::max(need_end, off[i] + l.rows[i] * l.row_bytes[i]);
        plain = spf_arena::align_up(plain + l.rows[i] * l.row_bytes[i]);
    }
    if (arena < need_end) fail(what, "a group ends beyond the arena", arena, need_end);
    const std::vector<Row> rows = rows_of(l, off);
    if (pairs) check_pairs(what, rows);
    check_sweep(what, rows);
    const size_t peak = peak_live(l, rows);
    if (arena < peak) fail(what, "the arena is smaller than the peak of live bytes", arena, peak);
    if (arena > plain) fail(what, "the arena is larger than the layout without reuse", arena, plain);
    // nothing dies: block after block, exactly the layout without reuse
    List forever = l;
    for (auto& d : forever.death) std::fill(d.begin(), d.end(), spf_arena::kNever);
    size_t arena3 = 0, at = l.base;
    const std::vector<size_t> off3 = run(forever, &arena3);
    for (size_t i = 0; i < l.groups(); i++) {
        if (off3[i] != at) { fail(what, "without deaths a group is not right behind the one before", i, off3[i]); break; }
        at = spf_arena::align_up(at + l.rows[i] * l.row_bytes[i]);
    }
    if (arena3 != plain) fail(what, "without deaths the arena is not the plain sum", arena3, plain);
    return arena;
}

uint64_t g_state;
uint64_t rnd() // splitmix64
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the five value sizes at DEFAULT_128 (LWE0, LWE1, GLWE1, GGSW1, GLEV1) and at a small generic set, where rows are shorter than
// the alignment
const size_t kSizes[2][5] = {{5104, 16392, 32768, 262144, 131072}, {136, 264, 256, 4096, 1024}};

List random_list(uint64_t seed)
{
    g_state = seed;
    List l;
    const size_t n = 1 + rnd() % 400;
    const size_t* sizes = kSizes[rnd() % 2];
    l.base = (rnd() % 64) * 256;
    const int mode = (int)(rnd() % 4); // how long values live: 0 next level only, 1 short, 2 mixed with "never", 3 anything
    uint32_t level = 1;
    for (size_t i = 0; i < n; i++) {
        if (i && rnd() % 3) level++; // (several groups share a level)
        size_t rows = 1 + rnd() % 8;
        if (rnd() % 24 == 0) rows = 40 + rnd() % 60; // wider than every free range so far, most of the time
        l.level.push_back(level);
        l.row_bytes.push_back(sizes[rnd() % 5]);
        l.rows.push_back(rows);
        std::vector<uint32_t> d(rows);
        for (auto& x : d) {
            const uint64_t r = rnd();
            if (mode == 0) x = level + 1;
            else if (mode == 1) x = level + (uint32_t)(r % 4);
            else if (mode == 2) x = r % 8 == 0 ? spf_arena::kNever : level + 1 + (uint32_t)((r >> 8) % 3);
            else x = r % 16 == 0 ? spf_arena::kNever : r % 16 == 1 ? 0 /* never read: dies where it is made */ : level + (uint32_t)((r >> 8) % 600);
        }
        l.death.push_back(d);
    }
    return l;
}

bool read_list(const char* path, List* l)
{
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    unsigned long long base = 0, n = 0;
    bool ok = std::fscanf(f, "%llu %llu", &base, &n) == 2;
    l->base = (size_t)base;
    for (unsigned long long i = 0; ok && i < n; i++) {
        unsigned long long lv = 0, rb = 0, rows = 0;
        ok = std::fscanf(f, "%llu %llu %llu", &lv, &rb, &rows) == 3 && rb > 0 && rows > 0;
        if (!ok) break;
        std::vector<uint32_t> d((size_t)rows);
        for (auto& x : d) {
            unsigned long long v = 0;
            ok = ok && std::fscanf(f, "%llu", &v) == 1;
            x = (uint32_t)v;
        }
        l->level.push_back((uint32_t)lv);
        l->row_bytes.push_back((size_t)rb);
        l->rows.push_back((size_t)rows);
        l->death.push_back(std::move(d));
    }
    std::fclose(f);
    return ok;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc == 4) {
        List l;
        if (!read_list(argv[1], &l)) {
            std::printf("FAILED %s: cannot read the group list\n", argv[1]);
            return 1;
        }
        size_t rows = 0, values = l.base;
        for (size_t i = 0; i < l.groups(); i++) {
            rows += l.rows[i];
            values += l.rows[i] * l.row_bytes[i];
        }
        const size_t arena = check(argv[1], l, rows <= 6000);
        const size_t peak = peak_live(l, rows_of(l, std::vector<size_t>(l.groups(), 0)));
        const unsigned long long num = std::strtoull(argv[2], nullptr, 10), den = std::strtoull(argv[3], nullptr, 10);
        std::printf("circuit: %zu groups, %zu rows, values_bytes %zu, peak live %zu, arena %zu (%.4f of values_bytes, bound %llu/%llu)\n",
                    l.groups(), rows, values, peak, arena, (double)arena / (double)values, num, den);
        if ((unsigned __int128)arena * den > (unsigned __int128)values * num) fail(argv[1], "the arena is above the bound", arena, values);
        if (g_failed) return 1;
        std::printf("arena_plan ok\n");
        return 0;
    }
    if (argc != 1) {
        std::printf("usage: arena_plan [FILE MAX_NUM MAX_DEN]\n");
        return 2;
    }
    size_t lists = 0, groups = 0, wide = 0;
    double saved = 0;
    for (uint64_t seed = 1; seed <= 300; seed++) {
        const List l = random_list(0xA7E4A000ull + seed);
        const size_t arena = check("seed " + std::to_string(seed), l, true);
        size_t plain = l.base;
        for (size_t i = 0; i < l.groups(); i++) {
            plain = spf_arena::align_up(plain + l.rows[i] * l.row_bytes[i]);
            wide += l.rows[i] >= 40;
        }
        saved += 1.0 - (double)arena / (double)plain;
        lists++;
        groups += l.groups();
    }
    // a hand-made case: a chain, every value read by the next level only, needs two rows however long it is
    {
        List l;
        l.base = 512;
        for (uint32_t lv = 1; lv <= 40; lv++) {
            l.level.push_back(lv);
            l.row_bytes.push_back(32768);
            l.rows.push_back(1);
            l.death.push_back({lv == 40 ? spf_arena::kNever : lv + 1});
        }
        const size_t arena = check("chain", l, true);
        if (arena != 512 + 2 * 32768) fail("chain", "a chain of 40 does not fit two rows", arena, 512 + 2 * 32768);
    }
    std::printf("random: %zu lists, %zu groups (%zu wide), mean saving %.3f, %d failed\n", lists, groups, wide, saved / (double)lists, g_failed);
    if (g_failed) return 1;
    std::printf("arena_plan ok\n");
    return 0;
}
