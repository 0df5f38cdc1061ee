// Every destroy order of the ABI's handles on real objects after real work (include/spf_hip.h, "Lifetimes": a child keeps its parent
// alive, the destroy functions may be called in any order) — test infrastructure.  One scenario per process, named by argv[1]; links
// libspf_hip.so; built and run by tests/test_gpu_lifetimes.py.
//
// The work is a chain of CMUX gates (no key needed; DEFAULT_128 with lwe_dimension 12, the tuned kernels) on random words and random
// selector spectra, through a gate graph, through a pool by host pointer and by handle, through a group's jobs and a group pool.  What
// is compared, word for word, is the chain run through the child that survived its parent's destroy against spf_cmux_batch on a
// context nobody touches: the kernels must run from memory that is still there.  Parity of these operations with the oracle is held
// elsewhere.  spf_live_objects is how a lost reference shows: the counts must be zero when everything has been destroyed.
#include "spf_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const std::string& what)
{
    std::printf("%-88s %s\n", what.c_str(), ok ? "ok" : "MISMATCH");
    std::fflush(stdout);
    if (!ok) failures++;
}
#define MUST(expr)                                                                                  \
    do {                                                                                            \
        const spf_status st_ = (expr);                                                              \
        if (st_ != SPF_OK) {                                                                        \
            std::printf("%s:%d: %s returned %d\n", __FILE__, __LINE__, #expr, st_);                 \
            std::exit(3);                                                                           \
        }                                                                                           \
    } while (0)

uint64_t state = 0x11FE;
uint64_t next_word() // splitmix64
{
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

spf_params P;
size_t GW = 0, SW = 0; // words of a GLWE, doubles of a GGSW
spf_ctx* REF = nullptr; // the untouched context every expectation comes from
constexpr size_t DEPTH = 3;

// the operands of one chain: x_0 = a, x_{i+1} = cmux(sel_i, x_i, b_i); the buffers keep their addresses, fresh() gives them new contents
struct Chain {
    std::vector<double> sel;
    std::vector<uint64_t> a, b, out;
    Chain() : sel(DEPTH * SW), a(GW), b(DEPTH * GW), out(GW) { fresh(); }
    void fresh()
    {
        for (auto& x : sel) x = (double)(int64_t)next_word() * 0.03125; // magnitudes up to 2^58
        for (auto& x : a) x = next_word();
        for (auto& x : b) x = next_word();
        std::fill(out.begin(), out.end(), 0);
    }
    const double* s(size_t i) const { return sel.data() + i * SW; }
    const uint64_t* hi(size_t i) const { return b.data() + i * GW; }
    // the expectation: spf_cmux_batch on the untouched context, from `start` (a, or the words of a value) over steps [first, DEPTH)
    std::vector<uint64_t> expected(const uint64_t* start = nullptr, size_t first = 0) const
    {
        std::vector<uint64_t> x(start ? start : a.data(), (start ? start : a.data()) + GW), y(GW);
        for (size_t i = first; i < DEPTH; i++) {
            MUST(spf_cmux_batch(REF, 1, s(i), x.data(), hi(i), y.data()));
            x.swap(y);
        }
        return x;
    }
    bool out_is_expected() const { return out == expected(); }
};

// the chain as nodes of `g`: inputs read from the chain's buffers at every run, the last gate written to chain.out
void add_chain(spf_graph* g, Chain& c)
{
    uint32_t x = 0;
    MUST(spf_graph_add_input(g, SPF_VAL_GLWE1, c.a.data(), &x));
    for (size_t i = 0; i < DEPTH; i++) {
        uint32_t in[3] = {0, x, 0};
        MUST(spf_graph_add_input(g, SPF_VAL_GGSW1, c.s(i), &in[0]));
        MUST(spf_graph_add_input(g, SPF_VAL_GLWE1, c.hi(i), &in[2]));
        MUST(spf_graph_add_op(g, SPF_OP_CMUX, in, 3, 0, &x));
    }
    MUST(spf_graph_add_output(g, x, c.out.data()));
}
bool graph_runs(spf_graph* g, Chain& c)
{
    c.fresh();
    MUST(spf_graph_run(g));
    return c.out_is_expected();
}
// the chain through the pool's host-pointer submits, one gate at a time
bool pool_runs_host(spf_pool* p, Chain& c)
{
    c.fresh();
    std::vector<uint64_t> x = c.a, y(GW);
    for (size_t i = 0; i < DEPTH; i++) {
        uint64_t t = 0;
        MUST(spf_pool_submit_cmux(p, c.s(i), x.data(), c.hi(i), y.data(), &t));
        MUST(spf_pool_wait(p, t));
        x.swap(y);
    }
    c.out = x;
    return c.out_is_expected();
}
// the chain by handle, starting at `start` (a value of member `member` whose words are `start_words`): every gate pushed on the
// still-pending result of the one before, one wait at the end
bool pool_runs_values(spf_pool* p, int member, const spf_value* start, const std::vector<uint64_t>& start_words, Chain& c)
{
    c.fresh();
    std::vector<spf_value*> held;
    const spf_value* x = start;
    for (size_t i = 0; i < DEPTH; i++) {
        spf_value *sel = nullptr, *hi = nullptr, *next = nullptr;
        MUST(spf_value_upload(p, member, SPF_VAL_GGSW1, c.s(i), &sel));
        MUST(spf_value_upload(p, member, SPF_VAL_GLWE1, c.hi(i), &hi));
        MUST(spf_pool_submit_cmux_v(p, sel, x, hi, &next, nullptr));
        held.insert(held.end(), {sel, hi, next});
        x = next;
    }
    MUST(spf_value_wait(x));
    MUST(spf_value_download(x, c.out.data()));
    for (spf_value* v : held) spf_value_release(v);
    return c.out == c.expected(start_words.data());
}
bool value_holds(const spf_value* v, const std::vector<uint64_t>& words)
{
    std::vector<uint64_t> got(GW);
    MUST(spf_value_download(v, got.data()));
    return got == words;
}
spf_value* upload_glwe(spf_pool* p, int member, std::vector<uint64_t>& words)
{
    words.resize(GW);
    for (auto& x : words) x = next_word();
    spf_value* v = nullptr;
    MUST(spf_value_upload(p, member, SPF_VAL_GLWE1, words.data(), &v));
    return v;
}

// the live counts: the reference context and nothing else / nothing at all
bool live_is(uint64_t contexts)
{
    spf_live_counts n;
    MUST(spf_live_objects(&n));
    const bool ok = n.contexts == contexts && !n.groups && !n.graphs && !n.pools && !n.values;
    if (!ok)
        std::printf("live: %llu contexts, %llu groups, %llu graphs, %llu pools, %llu values\n", (unsigned long long)n.contexts,
                    (unsigned long long)n.groups, (unsigned long long)n.graphs, (unsigned long long)n.pools, (unsigned long long)n.values);
    return ok;
}

spf_group* group_of_two()
{
    const int ids[2] = {0, 0};
    spf_group* g = nullptr;
    MUST(spf_group_create(&P, ids, 2, &g));
    return g;
}

void ctx_graph()
{
    spf_ctx* c = nullptr;
    MUST(spf_create(&P, 0, &c));
    spf_graph* g = nullptr;
    MUST(spf_graph_create(c, &g));
    Chain ch;
    add_chain(g, ch);
    expect(graph_runs(g, ch), "the graph runs while its context is there");
    spf_destroy(c);
    expect(graph_runs(g, ch), "spf_destroy(context): the graph runs again on new inputs, word-equal");
    expect(graph_runs(g, ch), "  ... and once more");
    spf_graph_destroy(g);
    expect(live_is(1), "spf_graph_destroy: nothing is left");
}

void ctx_pool_value()
{
    spf_ctx* c = nullptr;
    MUST(spf_create(&P, 0, &c));
    spf_pool* p = nullptr;
    MUST(spf_pool_create(c, 64, 100, &p));
    Chain ch;
    expect(pool_runs_host(p, ch), "host-pointer submits and waits while the context is there");
    std::vector<uint64_t> words;
    spf_value* v = upload_glwe(p, 0, words);
    spf_destroy(c);
    expect(pool_runs_values(p, 0, v, words, ch), "spf_destroy(context): a chain pushed by handle on the value, word-equal");
    expect(pool_runs_host(p, ch), "  ... and host-pointer submits");
    spf_pool_destroy(p);
    expect(value_holds(v, words), "spf_pool_destroy: the value still downloads its words");
    spf_value_release(v);
    expect(live_is(1), "spf_value_release: nothing is left");
}

void permutations()
{
    enum { CTX = 0, GRAPH, POOL, VALUE };
    static const char* const names[4] = {"context", "graph", "pool", "value"};
    int order[4] = {0, 1, 2, 3};
    int n_orders = 0;
    do {
        spf_ctx* c = nullptr;
        MUST(spf_create(&P, 0, &c));
        spf_graph* g = nullptr;
        MUST(spf_graph_create(c, &g));
        Chain cg, cp;
        add_chain(g, cg);
        bool ok = graph_runs(g, cg); // a graph that has run
        spf_pool* p = nullptr;
        MUST(spf_pool_create(c, 64, 100, &p));
        ok = pool_runs_host(p, cp) && ok; // a pool that has run a batch
        std::vector<uint64_t> words;
        spf_value* v = upload_glwe(p, 0, words);
        bool alive[4] = {true, true, true, true};
        std::string line = "destroy";
        for (int k = 0; k < 4; k++) {
            switch (order[k]) {
            case CTX: spf_destroy(c); break;
            case GRAPH: spf_graph_destroy(g); break;
            case POOL: spf_pool_destroy(p); break;
            default: spf_value_release(v); break;
            }
            alive[order[k]] = false;
            line += std::string(k ? ", " : " ") + names[order[k]];
            // whatever is still alive works
            if (alive[CTX]) {
                std::vector<uint64_t> got(GW);
                MUST(spf_cmux_batch(c, 1, cp.s(0), cp.a.data(), cp.hi(0), got.data()));
                std::vector<uint64_t> want(GW);
                MUST(spf_cmux_batch(REF, 1, cp.s(0), cp.a.data(), cp.hi(0), want.data()));
                ok = got == want && ok;
            }
            if (alive[GRAPH]) ok = graph_runs(g, cg) && ok;
            if (alive[POOL]) ok = pool_runs_host(p, cp) && ok;
            if (alive[POOL] && alive[VALUE]) ok = pool_runs_values(p, 0, v, words, cp) && ok;
            if (alive[VALUE]) ok = value_holds(v, words) && ok;
        }
        ok = live_is(1) && ok;
        expect(ok, line + ": the survivors work after every step, nothing is left");
        n_orders++;
    } while (std::next_permutation(order, order + 4));
    expect(n_orders == 24, "24 orders");
}

void group_jobs()
{
    static const int orders[3][4] = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}};
    for (int round = 0; round < 3; round++) {
        spf_group* grp = group_of_two();
        spf_graph* jobs[4];
        std::vector<Chain> ch(4);
        for (int j = 0; j < 4; j++) {
            MUST(spf_group_graph_create(grp, &jobs[j]));
            add_chain(jobs[j], ch[(size_t)j]);
        }
        MUST(spf_group_run_graphs(grp, jobs, 4)); // (merged graphs exist from here on)
        bool ok = true, both = false;
        int member[4];
        for (int j = 0; j < 4; j++) {
            ok = ch[(size_t)j].out_is_expected() && ok;
            member[j] = spf_graph_member(jobs[j]);
            both = both || member[j] != member[0];
        }
        expect(ok && both, "round " + std::to_string(round) + ": four jobs over both members, word-equal");
        spf_group_destroy(grp);
        ok = true;
        for (int j = 0; j < 4; j++) {
            uint32_t nodes = 0, levels = 0, launches = 0;
            ok = spf_graph_member(jobs[j]) == member[j] && spf_graph_stats(jobs[j], &nodes, &levels, &launches) == SPF_OK &&
                 nodes == 1 + 3 * DEPTH && levels > 0 && ok;
        }
        expect(ok, "  spf_group_destroy: spf_graph_member and spf_graph_stats still answer for the jobs");
        if (round == 0) expect(graph_runs(jobs[1], ch[1]), "  ... and a job still runs, word-equal");
        for (int k = 0; k < 4; k++) spf_graph_destroy(jobs[orders[round][k]]);
        expect(live_is(1), "  the jobs destroyed in order " + std::to_string(orders[round][0]) + std::to_string(orders[round][1]) +
                               std::to_string(orders[round][2]) + std::to_string(orders[round][3]) + ": nothing is left");
    }
}

void group_pool()
{
    spf_group* grp = group_of_two();
    spf_pool* p = nullptr;
    MUST(spf_pool_create_group(grp, 64, 100, &p));
    std::vector<uint64_t> words[2];
    spf_value* v[2] = {upload_glwe(p, 0, words[0]), upload_glwe(p, 1, words[1])};
    Chain ch;
    expect(pool_runs_values(p, 0, v[0], words[0], ch) && pool_runs_values(p, 1, v[1], words[1], ch), "by handle on both members while the group is there");
    spf_group_destroy(grp);
    expect(pool_runs_values(p, 0, v[0], words[0], ch), "spf_group_destroy: submit and wait on member 0, word-equal");
    expect(pool_runs_values(p, 1, v[1], words[1], ch), "  ... on member 1");
    expect(pool_runs_host(p, ch), "  ... and by host pointer (the calling thread is dealt to a member)");
    spf_pool_destroy(p);
    expect(value_holds(v[0], words[0]) && value_holds(v[1], words[1]), "spf_pool_destroy: the values still download their words");
    spf_value_release(v[0]);
    spf_value_release(v[1]);
    expect(live_is(1), "the values released: nothing is left");
}

void borrowed_member()
{
    spf_group* grp = group_of_two();
    spf_ctx* c = spf_group_ctx(grp, 1);
    expect(c != nullptr, "spf_group_ctx(group, 1)");
    spf_pool* p = nullptr;
    MUST(spf_pool_create(c, 64, 100, &p));
    spf_graph* g = nullptr;
    MUST(spf_graph_create(c, &g));
    Chain cg, cp;
    add_chain(g, cg);
    expect(graph_runs(g, cg) && pool_runs_host(p, cp), "a pool and a graph on the borrowed context while the group is there");
    spf_group_destroy(grp);
    expect(graph_runs(g, cg), "spf_group_destroy: the graph still runs, word-equal");
    expect(pool_runs_host(p, cp), "  ... and the pool");
    spf_graph_destroy(g);
    expect(pool_runs_host(p, cp), "spf_graph_destroy: the pool still runs");
    spf_pool_destroy(p);
    expect(live_is(1), "spf_pool_destroy: nothing is left");
}

void stale_value()
{
    spf_ctx* c = nullptr;
    MUST(spf_create(&P, 0, &c));
    std::vector<double> sel(SW);
    for (auto& x : sel) x = (double)(int64_t)next_word() * 0.03125;
    int same_address = 0;
    for (int round = 0; round < 8; round++) {
        spf_pool* a = nullptr;
        MUST(spf_pool_create(c, 64, 100, &a));
        std::vector<uint64_t> words;
        spf_value* v = upload_glwe(a, 0, words);
        spf_pool_destroy(a);
        spf_pool* b = nullptr;
        MUST(spf_pool_create(c, 64, 100, &b));
        same_address += (void*)b == (void*)a; // (the case the address comparison got wrong)
        spf_value *out = nullptr, *ggsw = nullptr;
        uint64_t t = 0;
        bool ok = spf_pool_submit_not_v(b, v, &out, &t) == SPF_ERR_INVALID_ARGUMENT && out == nullptr;
        const spf_value* two[2] = {v, v};
        ok = spf_pool_submit_op_v(b, SPF_OP_GLWE_ADD, two, 2, 0, &out, &t) == SPF_ERR_INVALID_ARGUMENT && out == nullptr && ok;
        MUST(spf_value_upload(b, 0, SPF_VAL_GGSW1, sel.data(), &ggsw));
        const spf_value* shift[1] = {ggsw};
        ok = spf_pool_submit_blind_rotation_v(b, v, shift, 1, 0, &out, &t) == SPF_ERR_INVALID_ARGUMENT && out == nullptr && ok;
        std::vector<uint64_t> other;
        spf_value* mine = upload_glwe(b, 0, other);
        ok = spf_pool_submit_cmux_v(b, ggsw, v, mine, &out, &t) == SPF_ERR_INVALID_ARGUMENT && out == nullptr && ok;
        ok = spf_pool_submit_not_v(b, mine, &out, &t) == SPF_OK && spf_pool_wait(b, t) == SPF_OK && ok; // (its own value is taken)
        if (out) spf_value_release(out);
        spf_value_release(ggsw);
        spf_value_release(mine);
        expect(ok, "round " + std::to_string(round) + ": the value of a destroyed pool is refused by the next pool" + ((void*)b == (void*)a ? " (same address)" : ""));
        expect(value_holds(v, words), "  ... and still downloads its words");
        spf_value_release(v);
        spf_pool_destroy(b);
    }
    std::printf("pools B at the address of their pool A: %d of 8\n", same_address);
    spf_destroy(c);
    expect(live_is(1), "everything destroyed: nothing is left");
}

} // namespace

int main(int argc, char** argv)
{
    const std::string which = argc > 1 ? argv[1] : "";
    spf_default_params(&P);
    P.lwe_dimension = 12; // no bootstrap runs here; every other parameter is DEFAULT_128
    GW = spf_ciphertext_words(&P, SPF_VAL_GLWE1);
    SW = 2 * (size_t)(P.glwe_size + 1) * P.cbs_radix_count * (P.glwe_size + 1) * (P.polynomial_degree / 2);
    MUST(spf_create(&P, 0, &REF));
    if (which == "ctx-graph") ctx_graph();
    else if (which == "ctx-pool-value") ctx_pool_value();
    else if (which == "permutations") permutations();
    else if (which == "group-jobs") group_jobs();
    else if (which == "group-pool") group_pool();
    else if (which == "borrowed-member") borrowed_member();
    else if (which == "stale-value") stale_value();
    else {
        std::printf("usage: lifetimes_gpu ctx-graph | ctx-pool-value | permutations | group-jobs | group-pool | borrowed-member | stale-value\n");
        return 2;
    }
    spf_destroy(REF);
    expect(live_is(0), "the reference context destroyed: every live count is zero");
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
