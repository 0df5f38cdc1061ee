// glwe_keyswitch_graph_plan.cpp — the GLWE keyswitch, automorphism and trace nodes (spf_graph_add_glwe_keyswitch / _automorphism /
// _trace: kinds 70, 71, 72) in the planner of the gate graphs (spf_amd/csrc/spf_graph_plan.hpp), on the CPU.
//
// Built from the HIP-free header alone with g++ -fsanitize=address,undefined and run directly
// (tests/test_glwe_keyswitch_graph_plan.py).  Hand-made graphs and small seeded random ones mix the new kinds with inputs, XOR
// (GlweAdd), pack, unpack and polynomial linear layers.  By brute force from the nodes' own fields:
//   * every new node is in exactly one group, and a group is uniform in (level, kind, parameter): its key is (level, op, 0, 0, 0,
//     slot or round or 0), two groups never share a key;
//   * a group reads its operands in place exactly when they lie consecutively in member order, else its pointer row is their
//     offsets in that order; nothing is staged for it;
//   * the output rows of a group are consecutive, 256-aligned, and share no byte with any operand row of the group (what the rows
//     kernels' parking needs);
//   * Plan::has_glwe_ks says whether the graph holds such a node;
//   * a graph without the kinds plans the same with new nodes stacked on top of it: every group, offset and table entry of the
//     graph below is where it was.
#include "../../spf_amd/csrc/spf_graph_plan.hpp"

#include <cstdio>
#include <string>

namespace P = spf_graph_plan;

namespace {

int g_failed = 0;
bool expect(bool ok, const std::string& what, size_t a = 0, size_t b = 0)
{
    if (!ok && g_failed++ < 40) std::printf("FAILED %s (%zu, %zu)\n", what.c_str(), a, b);
    return ok;
}

// value sizes: {LWE0, LWE1, GLWE1, GGSW1, GLEV1}.  With a GLWE of 256 bytes (N = 16, k = 1) inputs lie one behind the other; with
// 128 (half the alignment) every input is padded, so two inputs are never consecutive
P::Sizes sizes(size_t glwe_bytes)
{
    P::Sizes s{};
    s.bytes[SPF_VAL_LWE0] = 88;
    s.bytes[SPF_VAL_LWE1] = glwe_bytes / 2 + 8;
    s.bytes[SPF_VAL_GLWE1] = glwe_bytes;
    s.bytes[SPF_VAL_GGSW1] = 8 * glwe_bytes;
    s.bytes[SPF_VAL_GLEV1] = 4 * glwe_bytes;
    s.cbs_radix_count = 4;
    s.pufks_stage = false;
    return s;
}

using V = std::vector<uint32_t>;

struct Builder {
    P::Graph g;
    uint32_t input(int kind = SPF_VAL_GLWE1)
    {
        P::Node n{};
        n.op = -1; n.kind = kind;
        return g.add(n);
    }
    uint32_t xor_(uint32_t a, uint32_t b)
    {
        P::Node n{};
        n.op = SPF_OP_GLWE_ADD; n.kind = SPF_VAL_GLWE1; n.n_in = 2; n.in[0] = a; n.in[1] = b;
        return g.add(n);
    }
    uint32_t pack(const V& ids)
    {
        P::Node n{};
        n.op = P::kNodePack; n.kind = SPF_VAL_GLWE1;
        return g.add_listed(n, ids.data(), ids.size());
    }
    V unpack(uint32_t glwe, size_t width)
    {
        P::Node n{};
        n.op = P::kNodeUnpack; n.kind = SPF_VAL_LWE1; n.n_in = 1; n.in[0] = glwe; n.count = (uint32_t)width;
        return range(g.add_numbered(n, width), width);
    }
    V poly_layer(uint32_t slot, const V& ids, size_t M)
    {
        P::Node n{};
        n.op = P::kNodeGlwePolyLinear; n.kind = SPF_VAL_GLWE1; n.lin_slot = slot; n.lin_rows = (uint32_t)M;
        return range(g.add_listed(n, ids.data(), ids.size(), M), M);
    }
    // what spf_graph_add_glwe_keyswitch / _automorphism / _trace record
    uint32_t ks(int32_t op, uint32_t param, uint32_t glwe)
    {
        P::Node n{};
        n.op = op; n.kind = SPF_VAL_GLWE1; n.n_in = 1; n.in[0] = glwe; n.param = param;
        return g.add(n);
    }
    uint32_t keyswitch(uint32_t slot, uint32_t glwe) { return ks(P::kNodeGlweKeyswitch, slot, glwe); }
    uint32_t automorphism(uint32_t round, uint32_t glwe) { return ks(P::kNodeGlweAutomorphism, round, glwe); }
    uint32_t trace(uint32_t glwe) { return ks(P::kNodeGlweTrace, 0, glwe); }
    static V range(uint32_t first, size_t n)
    {
        V r(n);
        for (size_t i = 0; i < n; i++) r[i] = first + (uint32_t)i;
        return r;
    }
};

struct Want { int32_t op; uint64_t param; size_t members; bool in_place; };

// every group of the new kinds against the nodes, by brute force; then, when `want` is given, against it in key order.
// Returns the number of such groups
size_t check(const std::string& name, P::Graph g, const P::Sizes& sz, const std::vector<Want>* want, bool print = true)
{
    const int failed_before = g_failed;
    const P::Plan p = P::plan(g, sz);
    const size_t gw = sz.of(SPF_VAL_GLWE1);
    bool any = false;
    for (const auto& n : g.nodes) any = any || P::is_glwe_ks_node(n.op);
    expect(p.has_glwe_ks == any, name + ": has_glwe_ks does not say whether the graph holds a GLWE keyswitch, automorphism or trace node");
    std::vector<int> seen(g.nodes.size(), 0);
    std::vector<const P::Group*> mine;
    for (const auto& gr : p.groups) {
        if (!P::is_glwe_ks_node(gr.key.op)) {
            for (uint32_t id : gr.members) expect(!P::is_glwe_ks_node(g.nodes[id].op), name + ": a new node in a foreign group", id);
            continue;
        }
        mine.push_back(&gr);
        const size_t B = gr.members.size();
        const P::Node& head = g.nodes[gr.members[0]];
        expect(gr.key.level == head.level && gr.key.op == head.op && gr.key.kind == 0 && gr.key.slot == 0 && gr.key.rows == 0 && gr.key.n == head.param,
               name + ": the key is not (level, op, 0, 0, 0, parameter) of the first member", gr.members[0]);
        expect(gr.out_off % P::kAlign == 0, name + ": the block of a group is not 256-aligned", gr.out_off);
        std::vector<size_t> offs;
        for (size_t i = 0; i < B; i++) {
            const uint32_t id = gr.members[i];
            const P::Node& n = g.nodes[id];
            seen[id]++;
            expect(i == 0 || gr.members[i - 1] < id, name + ": the members are not in node order", id);
            expect(n.op == gr.key.op && n.level == gr.key.level && n.param == gr.key.n && n.kind == SPF_VAL_GLWE1 && n.n_in == 1,
                   name + ": a member does not have its group's (level, kind, parameter)", id);
            expect(n.off == gr.out_off + i * gw, name + ": the outputs are not consecutive GLWEs in member order", id);
            const uint32_t in = n.in[0];
            expect(in < id && g.nodes[in].kind == SPF_VAL_GLWE1 && g.nodes[in].level < gr.key.level, name + ": an operand is no earlier GLWE of a lower level", id);
            offs.push_back(g.nodes[in].off);
        }
        bool consecutive = true;
        for (size_t i = 1; i < B; i++) consecutive = consecutive && offs[i] == offs[0] + i * gw;
        expect(gr.contiguous[0] == consecutive, name + ": in place is not 'the operands lie consecutively'", gr.members[0], consecutive);
        if (gr.contiguous[0]) {
            expect(gr.first_off[0] == offs[0], name + ": first_off is not the first operand's offset", gr.first_off[0], offs[0]);
        } else if (expect(gr.ptr_index[0] + B <= p.table.size(), name + ": the pointer row ends beyond the table")) {
            for (size_t i = 0; i < B; i++)
                if (!expect(p.table[gr.ptr_index[0] + i] == offs[i], name + ": the pointer row is not the operand offsets in order", i)) break;
        }
        // the output block [out_off, out_off + B gw) shares no byte with any operand row
        for (size_t i = 0; i < B; i++)
            expect(offs[i] + gw <= gr.out_off || gr.out_off + B * gw <= offs[i], name + ": an operand row overlaps the group's output rows", gr.members[i], offs[i]);
        expect(gr.out_off + B * gw <= p.arena_bytes, name + ": the outputs end beyond the arena", gr.out_off);
        for (int s = 1; s < 3; s++)
            expect(!gr.contiguous[s] && !gr.first_off[s] && !gr.ptr_index[s], name + ": a slot the group does not have is described", (size_t)s);
        expect(!gr.one_lut, name + ": one_lut on a new group");
    }
    for (size_t id = 0; id < g.nodes.size(); id++)
        expect(seen[id] == (P::is_glwe_ks_node(g.nodes[id].op) ? 1 : 0), name + ": a new node is not in exactly one group", id);
    for (size_t i = 1; i < mine.size(); i++) expect(mine[i - 1]->key < mine[i]->key, name + ": two groups share a key or stand out of order", i);
    if (want && expect(mine.size() == want->size(), name + ": the number of new groups", mine.size(), want->size()))
        for (size_t i = 0; i < want->size(); i++) {
            const P::Group& gr = *mine[i];
            expect(gr.key.op == (*want)[i].op && gr.key.n == (*want)[i].param, name + ": (op, parameter) of group", i);
            expect(gr.members.size() == (*want)[i].members, name + ": members of group", i, gr.members.size());
            expect(gr.contiguous[0] == (*want)[i].in_place, name + ": in place or through the table, group", i);
        }
    if (print) std::printf("%s: %zu groups%s\n", name.c_str(), mine.size(), g_failed == failed_before ? " ok" : " FAILED");
    return mine.size();
}

void check(const char* name, const P::Graph& g, const P::Sizes& sz, const std::vector<Want>& want) { check(name, g, sz, &want); }

constexpr int32_t KS = P::kNodeGlweKeyswitch, AU = P::kNodeGlweAutomorphism, TR = P::kNodeGlweTrace;

Builder base()
{
    Builder b;
    for (int i = 0; i < 6; i++) b.input();
    return b;
}

void hand_made()
{
    {   // the consecutive results of one XOR group, in its order: in place, one group per mode
        Builder b = base();
        const V x = {b.xor_(0, 1), b.xor_(2, 3), b.xor_(4, 5)};
        for (uint32_t n : x) b.keyswitch(3, n);
        for (uint32_t n : x) b.automorphism(2, n);
        for (uint32_t n : x) b.trace(n);
        check("in place: an XOR group under the three modes", b.g, sizes(256), {{KS, 3, 3, true}, {AU, 2, 3, true}, {TR, 0, 3, true}});
        check("in place: the same at 3072-byte GLWEs", b.g, sizes(3072), {{KS, 3, 3, true}, {AU, 2, 3, true}, {TR, 0, 3, true}});
    }
    {   // the same results the other way round: through the table
        Builder b = base();
        const V x = {b.xor_(0, 1), b.xor_(2, 3), b.xor_(4, 5)};
        b.trace(x[2]); b.trace(x[1]); b.trace(x[0]);
        check("table: an XOR group the other way round", b.g, sizes(256), {{TR, 0, 3, false}});
    }
    {   // inputs: consecutive when a GLWE fills its alignment, padded apart when it does not; one lone operand is in place
        Builder b = base();
        b.keyswitch(0, 1); b.keyswitch(0, 2); b.keyswitch(0, 3);
        check("in place: inputs of 256 bytes", b.g, sizes(256), {{KS, 0, 3, true}});
        check("table: inputs of 128 bytes are padded apart", b.g, sizes(128), {{KS, 0, 3, false}});
        Builder one = base();
        one.automorphism(11, 4);
        check("in place: one lone operand", one.g, sizes(128), {{AU, 11, 1, true}});
    }
    {   // one operand twice, and a gap: through the table
        Builder b = base();
        b.trace(2); b.trace(2); b.trace(4);
        check("table: a duplicated operand", b.g, sizes(256), {{TR, 0, 3, false}});
    }
    {   // two slots and two rounds on one level are two groups each; the same parameter on another level is another group
        Builder b = base();
        const uint32_t x = b.xor_(0, 1);
        b.keyswitch(1, 0); b.keyswitch(2, 1); b.keyswitch(1, 2); b.keyswitch(2, 3);       // level 1: slots 1 and 2, operands 0, 2 | 1, 3
        b.automorphism(1, 4); b.automorphism(7, 5);                                      // level 1: rounds 1 and 7
        b.keyswitch(1, x);                                                              // level 2
        check("grouping: two slots, two rounds, another level", b.g, sizes(256),
              {{KS, 1, 2, false}, {KS, 2, 2, false}, {AU, 1, 1, true}, {AU, 7, 1, true}, {KS, 1, 1, true}});
    }
    {   // chains: a node of each kind reads the one before; the rows of a group read by an unpack, a pack and a polynomial layer
        Builder b = base();
        const uint32_t l = b.poly_layer(5, {3, 0}, 2)[1];     // level 1
        const uint32_t p = b.pack({1, 2});                    // level 1
        const uint32_t k1 = b.keyswitch(15, l);               // level 2
        const uint32_t k2 = b.keyswitch(15, p);               // level 2: with k1 one group; a layer's row and a pack's: scattered
        const uint32_t t = b.trace(k1);                       // level 3
        const uint32_t a = b.automorphism(4, t);              // level 4
        const uint32_t k3 = b.keyswitch(0, a);                // level 5
        b.unpack(k3, 3);
        b.pack({k2, t, a});
        b.poly_layer(6, {a, k1}, 1);
        check("chains: every kind reads the one before", b.g, sizes(256),
              {{KS, 15, 2, false}, {TR, 0, 1, true}, {AU, 4, 1, true}, {KS, 0, 1, true}});
    }
    {   // no new node
        Builder b = base();
        const uint32_t x = b.xor_(0, 1);
        b.unpack(x, 4);
        b.pack({x, 2});
        b.poly_layer(0, {x, 3}, 2);
        check("no new node", b.g, sizes(256), std::vector<Want>{});
    }
}

struct Rng {
    uint64_t s;
    uint32_t next(uint32_t n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((s >> 33) % n);
    }
};

// a random graph of GLWE nodes: inputs, XOR, pack, polynomial layers and — with `with_new` — the three new kinds
Builder random_graph(Rng& r, bool with_new, size_t steps)
{
    Builder b;
    const uint32_t inputs = 2 + r.next(5);
    for (uint32_t i = 0; i < inputs; i++) b.input();
    auto any = [&] { return r.next((uint32_t)b.g.nodes.size()); }; // (every node of these graphs is a GLWE)
    for (size_t s = 0; s < steps; s++) {
        const uint32_t what = r.next(with_new ? 7 : 3);
        if (what == 0) b.xor_(any(), any());
        else if (what == 1) b.pack({any(), any(), any()});
        else if (what == 2) b.poly_layer(r.next(3), {any(), any()}, 1 + r.next(2));
        else if (what <= 4) b.keyswitch(r.next(2), any());
        else if (what == 5) b.automorphism(1 + r.next(2), any());
        else b.trace(any());
    }
    return b;
}

void random_graphs()
{
    size_t groups = 0, in_place = 0, graphs = 0;
    for (uint64_t seed = 1; seed <= 120; seed++) {
        Rng r{seed * 0x9E3779B97F4A7C15ull};
        Builder b = random_graph(r, true, 4 + r.next(28));
        for (size_t glwe : {(size_t)256, (size_t)128, (size_t)3072}) {
            const std::string name = "random " + std::to_string(seed) + " / " + std::to_string(glwe);
            groups += check(name, b.g, sizes(glwe), nullptr, false);
        }
        const P::Plan p = [&] { P::Graph g = b.g; return P::plan(g, sizes(256)); }();
        for (const auto& gr : p.groups) in_place += P::is_glwe_ks_node(gr.key.op) && gr.contiguous[0] && gr.members.size() > 1;
        graphs++;
    }
    // (the generator must reach both forms, or the checks above prove less than they say)
    expect(groups > 300 && in_place > 0, "random graphs: too few groups, or no in-place group of more than one member", groups, in_place);
    std::printf("random graphs: %zu graphs%s\n", graphs, g_failed ? " FAILED" : " ok");
}

bool same_group(const P::Group& a, const P::Group& b)
{
    bool ok = a.key == b.key && a.members == b.members && a.out_off == b.out_off && a.one_lut == b.one_lut;
    for (int s = 0; s < 3; s++) ok = ok && a.contiguous[s] == b.contiguous[s] && a.first_off[s] == b.first_off[s] && a.ptr_index[s] == b.ptr_index[s];
    return ok;
}

// a graph without the kinds, and the same graph with new nodes stacked on top of its highest level: the plan below is unchanged
void unchanged_below()
{
    size_t stacked = 0;
    for (uint64_t seed = 1; seed <= 60; seed++) {
        Rng r{seed * 0xD1B54A32D192ED03ull};
        Builder b = random_graph(r, false, 3 + r.next(20));
        P::Graph g0 = b.g;
        const P::Plan p0 = P::plan(g0, sizes(256));
        const std::string name = "unchanged below " + std::to_string(seed);
        expect(!p0.has_glwe_ks, name + ": has_glwe_ks on a graph without the kinds");
        for (const auto& gr : p0.groups) expect(!P::is_glwe_ks_node(gr.key.op), name + ": a new group in a graph without the kinds");
        V top;
        for (uint32_t id = 0; id < g0.nodes.size(); id++)
            if (g0.nodes[id].level == p0.n_levels) top.push_back(id);
        if (p0.n_levels == 0 || top.empty()) continue;
        // new nodes over the top level, then over each other: every one of them lies above the graph below
        uint32_t last = b.trace(top[r.next((uint32_t)top.size())]);
        for (uint32_t i = 0, n = 1 + r.next(6); i < n; i++) {
            const uint32_t src = r.next(2) ? last : top[r.next((uint32_t)top.size())];
            const uint32_t what = r.next(3);
            last = what == 0 ? b.keyswitch(r.next(3), src) : what == 1 ? b.automorphism(1 + r.next(3), src) : b.trace(src);
        }
        P::Graph g1 = b.g;
        const P::Plan p1 = P::plan(g1, sizes(256));
        bool ok = p1.has_glwe_ks && p1.inputs_bytes == p0.inputs_bytes && p1.stage_bytes == p0.stage_bytes && p1.groups.size() > p0.groups.size() &&
                  p1.table.size() >= p0.table.size() && p1.arena_bytes > p0.arena_bytes;
        for (size_t i = 0; ok && i < p0.groups.size(); i++) ok = same_group(p0.groups[i], p1.groups[i]);
        for (size_t i = p0.groups.size(); ok && i < p1.groups.size(); i++) ok = P::is_glwe_ks_node(p1.groups[i].key.op) && p1.groups[i].out_off >= p0.arena_bytes;
        for (size_t i = 0; ok && i < p0.table.size(); i++) ok = p0.table[i] == p1.table[i];
        for (size_t id = 0; ok && id < g0.nodes.size(); id++) ok = g0.nodes[id].off == g1.nodes[id].off && g0.nodes[id].level == g1.nodes[id].level;
        expect(ok, name + ": the plan of the graph below moved when new nodes were stacked on it");
        check(name, b.g, sizes(256), nullptr, false);
        stacked++;
    }
    expect(stacked >= 30, "unchanged below: too few graphs had a node on their top level", stacked);
    std::printf("unchanged below: %zu graphs%s\n", stacked, g_failed ? " FAILED" : " ok");
}

// Graph::append carries the nodes: operands shifted, parameters kept, and two graphs' nodes of one (level, mode, parameter) are one group
void append()
{
    Builder a = base();
    a.keyswitch(2, 1);
    a.trace(0);
    Builder b = base();
    const uint32_t k = b.keyswitch(2, 5);
    b.automorphism(3, k);
    P::Graph m = a.g;
    const size_t before = m.nodes.size();
    const uint32_t base_id = m.append(b.g);
    bool ok = base_id == before && m.nodes.size() == before + b.g.nodes.size();
    for (size_t id = 0; ok && id < b.g.nodes.size(); id++) {
        const P::Node &n = m.nodes[before + id], &o = b.g.nodes[id];
        ok = n.op == o.op && n.param == o.param && n.n_in == o.n_in;
        for (uint32_t i = 0; ok && i < n.n_in; i++) ok = n.in[i] == o.in[i] + base_id;
    }
    expect(ok, "append: the second graph's nodes are not shifted behind the first's");
    check("append: two graphs' keyswitches of one slot are one group", m, sizes(256), {{KS, 2, 2, false}, {TR, 0, 1, true}, {AU, 3, 1, true}});
    std::printf("append shifts the operands%s\n", ok ? " ok" : " FAILED");
}

} // namespace

int main()
{
    static_assert(P::kNodeGlweKeyswitch == 70 && P::kNodeGlweAutomorphism == 71 && P::kNodeGlweTrace == 72,
                  "the node kinds' numbers are part of the recorded format");
    hand_made();
    random_graphs();
    unchanged_below();
    append();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("glwe_keyswitch_graph_plan ok\n");
    return 0;
}
