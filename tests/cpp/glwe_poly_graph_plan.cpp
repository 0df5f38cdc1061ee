// glwe_poly_graph_plan.cpp — the polynomial linear nodes (spf_graph_add_glwe_poly_linear) in the planner of the gate graphs
// (spf_amd/csrc/spf_graph_plan.hpp), on the CPU.
//
// Built from the HIP-free header alone with g++ -fsanitize=address,undefined and run directly (tests/test_glwe_poly_graph_plan.py).
// Hand-made graphs mix the new kind with inputs, XOR (GlweAdd), pack, unpack and LWE layers.  For every group of the new kind, by
// brute force from the nodes' own fields: the key is (level, 69, GLWE1, slot, M, K); the members are whole layers, layer-major;
// the operand GLWEs of all layers, in list order, are read in place exactly when they lie consecutively, else the group's pointer
// row equals their offsets in that order; the outputs are [layers][M] consecutive GLWEs; nothing is staged for the group; and
// Plan::has_glwe_poly says whether the graph holds such a node.  Each graph also states what it expects: how many such groups, how
// many layers each, in place or not.  Graph::append shifts the lists.
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

// value sizes: {LWE0, LWE1, GLWE1, GGSW1, GLEV1}.  With a GLWE of 256 bytes (N = 16, k = 1) or 3072 (N = 128, k = 2) inputs lie one
// behind the other; with 128 (half the alignment) every input is padded, so two inputs are never consecutive
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

struct Builder {
    P::Graph g;
    uint32_t input(int kind)
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
    uint32_t pack(const std::vector<uint32_t>& ids)
    {
        P::Node n{};
        n.op = P::kNodePack; n.kind = SPF_VAL_GLWE1;
        return g.add_listed(n, ids.data(), ids.size());
    }
    std::vector<uint32_t> unpack(uint32_t glwe, size_t width)
    {
        P::Node n{};
        n.op = P::kNodeUnpack; n.kind = SPF_VAL_LWE1; n.n_in = 1; n.in[0] = glwe; n.count = (uint32_t)width;
        return range(g.add_numbered(n, width), width);
    }
    std::vector<uint32_t> lwe_layer(uint32_t slot, const std::vector<uint32_t>& ids, size_t M)
    {
        P::Node n{};
        n.op = P::kNodeLweLinear; n.kind = g.nodes[ids[0]].kind; n.lin_slot = slot; n.lin_rows = (uint32_t)M;
        return range(g.add_listed(n, ids.data(), ids.size(), M), M);
    }
    std::vector<uint32_t> poly_layer(uint32_t slot, const std::vector<uint32_t>& ids, size_t M)
    {
        P::Node n{};
        n.op = P::kNodeGlwePolyLinear; n.kind = SPF_VAL_GLWE1; n.lin_slot = slot; n.lin_rows = (uint32_t)M;
        return range(g.add_listed(n, ids.data(), ids.size(), M), M);
    }
    static std::vector<uint32_t> range(uint32_t first, size_t n)
    {
        std::vector<uint32_t> r(n);
        for (size_t i = 0; i < n; i++) r[i] = first + (uint32_t)i;
        return r;
    }
};

struct Want { uint32_t slot; size_t M, K, layers; bool in_place; };

// every group of the new kind against the nodes, by brute force; then against `want`, in key order
void check(const char* name, P::Graph g, const P::Sizes& sz, const std::vector<Want>& want)
{
    const int failed_before = g_failed;
    const P::Plan p = P::plan(g, sz);
    const size_t gw = sz.of(SPF_VAL_GLWE1);
    bool any = false;
    for (const auto& n : g.nodes) any = any || n.op == P::kNodeGlwePolyLinear;
    expect(p.has_glwe_poly == any, std::string(name) + ": has_glwe_poly does not say whether the graph holds a polynomial linear node");
    std::vector<int> seen(g.nodes.size(), 0);
    std::vector<const P::Group*> poly;
    size_t staged_elsewhere = 0;
    for (const auto& gr : p.groups) {
        if (gr.key.op != P::kNodeGlwePolyLinear) {
            for (uint32_t id : gr.members) expect(g.nodes[id].op != P::kNodeGlwePolyLinear, std::string(name) + ": a polynomial linear node in a foreign group", id);
            // (what the other kinds of these graphs gather: scattered unpack sources and scattered rows of the table operations)
            if (gr.key.op == P::kNodeUnpack && !gr.contiguous[0]) staged_elsewhere = std::max(staged_elsewhere, gr.members.size() / (size_t)gr.key.n * gw);
            if (gr.key.op == SPF_OP_GLWE_ADD)
                for (int s = 0; s < 2; s++)
                    if (!gr.contiguous[s]) staged_elsewhere = std::max(staged_elsewhere, gr.members.size() * gw);
            continue;
        }
        poly.push_back(&gr);
        const size_t M = gr.key.rows, K = (size_t)gr.key.n;
        const P::Node& head = g.nodes[gr.members[0]];
        // the key
        expect(gr.key.level == head.level && gr.key.kind == SPF_VAL_GLWE1 && gr.key.slot == head.lin_slot && M == head.lin_rows && K == head.count,
               std::string(name) + ": the key is not (level, GLWE1, slot, M, K) of the first member", gr.members[0]);
        if (!expect(M > 0 && gr.members.size() % M == 0, std::string(name) + ": a group is no whole number of layers", gr.members.size(), M)) continue;
        const size_t layers = gr.members.size() / M;
        // layer-major members, every member with the group's parameters; the operand offsets in list order
        std::vector<size_t> offs;
        for (size_t l = 0; l < layers; l++) {
            const P::Node& first = g.nodes[gr.members[l * M]];
            for (size_t m = 0; m < M; m++) {
                const uint32_t id = gr.members[l * M + m];
                const P::Node& n = g.nodes[id];
                seen[id]++;
                expect(id == gr.members[l * M] + m && n.param == m, std::string(name) + ": a layer's rows are not successive members", l, m);
                expect(n.op == P::kNodeGlwePolyLinear && n.kind == SPF_VAL_GLWE1 && n.level == gr.key.level && n.lin_slot == gr.key.slot &&
                           n.lin_rows == M && n.count == K && n.list_at == first.list_at && n.n_in == 0,
                       std::string(name) + ": a member does not have its group's key or its layer's list", id);
                expect(n.off == gr.out_off + (l * M + m) * gw, std::string(name) + ": the outputs are not [layers][M] consecutive GLWEs", l, m);
            }
            for (size_t k = 0; k < K; k++) {
                const uint32_t in = g.operand(first, k);
                expect(in < gr.members[l * M] && g.nodes[in].kind == SPF_VAL_GLWE1 && g.nodes[in].level < gr.key.level,
                       std::string(name) + ": an operand is no earlier GLWE of a lower level", l, k);
                offs.push_back(g.nodes[in].off);
            }
        }
        expect(gr.out_off % P::kAlign == 0, std::string(name) + ": the block of a group is not 256-aligned", gr.out_off);
        bool consecutive = true;
        for (size_t i = 1; i < offs.size(); i++) consecutive = consecutive && offs[i] == offs[0] + i * gw;
        expect(gr.contiguous[0] == consecutive, std::string(name) + ": in place is not 'the layers * K rows are consecutive'", gr.members[0], consecutive);
        if (gr.contiguous[0]) {
            expect(gr.first_off[0] == offs[0], std::string(name) + ": first_off is not the first operand's offset", gr.first_off[0], offs[0]);
        } else if (expect(gr.ptr_index[0] + offs.size() <= p.table.size(), std::string(name) + ": the pointer row ends beyond the table")) {
            for (size_t i = 0; i < offs.size(); i++)
                if (!expect(p.table[gr.ptr_index[0] + i] == offs[i], std::string(name) + ": the pointer row is not the operand offsets in order", i)) break;
        }
        for (int s = 1; s < 3; s++)
            expect(!gr.contiguous[s] && !gr.first_off[s] && !gr.ptr_index[s], std::string(name) + ": a slot the group does not have is described", (size_t)s);
        expect(!gr.one_lut, std::string(name) + ": one_lut on a polynomial linear group");
    }
    for (size_t id = 0; id < g.nodes.size(); id++)
        expect(seen[id] == (g.nodes[id].op == P::kNodeGlwePolyLinear ? 1 : 0), std::string(name) + ": a polynomial linear node is not in exactly one group", id);
    expect(p.stage_bytes == staged_elsewhere, std::string(name) + ": the stage buffers are sized by something else than the other kinds", p.stage_bytes, staged_elsewhere);
    // the groups of one level with different (slot, M, K) are different groups, in key order
    for (size_t i = 1; i < poly.size(); i++) expect(poly[i - 1]->key < poly[i]->key, std::string(name) + ": two groups share a key or stand out of order", i);
    if (expect(poly.size() == want.size(), std::string(name) + ": the number of polynomial linear groups", poly.size(), want.size()))
        for (size_t i = 0; i < want.size(); i++) {
            const P::Group& gr = *poly[i];
            expect(gr.key.slot == want[i].slot && gr.key.rows == want[i].M && gr.key.n == want[i].K, std::string(name) + ": (slot, M, K) of group", i);
            expect(gr.members.size() == want[i].layers * want[i].M, std::string(name) + ": layers of group", i, gr.members.size());
            expect(gr.contiguous[0] == want[i].in_place, std::string(name) + ": in place or through the table, group", i);
        }
    std::printf("%s: %zu groups%s\n", name, poly.size(), g_failed == failed_before ? " ok" : " FAILED");
}

using V = std::vector<uint32_t>;

// six GLWE inputs and the XORs (0,1) (2,3) (4,5): one level-1 group of three consecutive GLWEs
Builder base()
{
    Builder b;
    for (int i = 0; i < 6; i++) b.input(SPF_VAL_GLWE1);
    return b;
}

void in_place_graphs()
{
    {   // the results of one XOR group, then of the layer itself, then its rows read by an unpack, a pack and an LWE layer
        Builder b = base();
        const V x = {b.xor_(0, 1), b.xor_(2, 3), b.xor_(4, 5)};
        const V a = b.poly_layer(1, x, 2);          // level 2, in place
        const V c = b.poly_layer(2, a, 3);          // level 3: reads a previous layer's rows in place
        const V bits = b.unpack(c[1], 5);           // level 4
        b.lwe_layer(3, {bits[4], bits[0]}, 2);      // level 5
        b.pack({c[2], a[0], x[1]});                 // level 4
        check("in place: an XOR group, a previous layer", b.g, sizes(256), {{1, 2, 3, 1, true}, {2, 3, 2, 1, true}});
        check("in place: the same at 3072-byte GLWEs", b.g, sizes(3072), {{1, 2, 3, 1, true}, {2, 3, 2, 1, true}});
    }
    {   // the results of one pack group
        Builder b = base();
        const V p = {b.pack({0, 1}), b.pack({2, 3}), b.pack({5, 4})};
        b.poly_layer(0, p, 1);
        check("in place: a pack group", b.g, sizes(256), {{0, 1, 3, 1, true}});
    }
    {   // two layers of one key whose lists follow each other: one group, in place; the other way round: through the table
        Builder b = base();
        const V x = {b.xor_(0, 1), b.xor_(2, 3), b.xor_(4, 5), b.xor_(0, 5)};
        b.poly_layer(7, {x[0], x[1]}, 2);
        b.poly_layer(7, {x[2], x[3]}, 2);
        check("in place: two layers, lists one behind the other", b.g, sizes(256), {{7, 2, 2, 2, true}});
        Builder r = base();
        const V y = {r.xor_(0, 1), r.xor_(2, 3), r.xor_(4, 5), r.xor_(0, 5)};
        r.poly_layer(7, {y[2], y[3]}, 2);
        r.poly_layer(7, {y[0], y[1]}, 2);
        check("table: two layers, lists the other way round", r.g, sizes(256), {{7, 2, 2, 2, false}});
    }
    {   // inputs: consecutive when a GLWE fills its alignment, padded apart when it does not
        Builder b = base();
        b.poly_layer(63, {1, 2, 3}, 4096);
        check("in place: inputs of 256 bytes, slot 63, M = 4096", b.g, sizes(256), {{63, 4096, 3, 1, true}});
        check("table: inputs of 128 bytes are padded apart", b.g, sizes(128), {{63, 4096, 3, 1, false}});
    }
    {   // one lone row is consecutive by definition; two lone rows out of order are not
        Builder b = base();
        b.poly_layer(4, {3}, 5);
        check("in place: one lone row", b.g, sizes(128), {{4, 5, 1, 1, true}});
        b.poly_layer(4, {2}, 5);
        check("table: two lone rows out of order", b.g, sizes(256), {{4, 5, 1, 2, false}});
    }
}

void scattered_graphs()
{
    // operands out of order from the inputs and from two levels, one repeated inside a list, one shared by two layers; further calls
    // on the same level with another slot, another M and another K
    Builder b = base();
    const V x = {b.xor_(0, 1), b.xor_(2, 3), b.xor_(4, 5)};      // level 1
    const uint32_t y = b.xor_(x[0], x[2]);                       // level 2
    b.poly_layer(1, {y, 4, x[1], x[1]}, 3);                      // level 3
    b.poly_layer(1, {x[2], y, 0, 5}, 3);                         // level 3, the same key: one group of two layers
    b.poly_layer(2, {y, 4, x[1], x[1]}, 3);                      // another slot
    b.poly_layer(1, {y, 4, x[1], x[1]}, 2);                      // another M
    b.poly_layer(1, {y, 4, x[1]}, 3);                            // another K
    b.poly_layer(1, {x[0], x[1], x[2], 0}, 3);                   // level 2: the same (slot, M, K) on another level
    // key order: level, then slot, M, K
    check("scattered: two layers of a key, three foreign keys, another level", b.g, sizes(256),
          {{1, 3, 4, 1, false}, {1, 2, 4, 1, false}, {1, 3, 3, 1, false}, {1, 3, 4, 2, false}, {2, 3, 4, 1, false}});
    check("scattered: the same at 3072-byte GLWEs", b.g, sizes(3072),
          {{1, 3, 4, 1, false}, {1, 2, 4, 1, false}, {1, 3, 3, 1, false}, {1, 3, 4, 2, false}, {2, 3, 4, 1, false}});
    // a scattered unpack source next to the layers: its stage size is its own
    Builder u = base();
    const V l = u.poly_layer(9, {5, 0}, 2);
    u.unpack(l[1], 3);
    u.unpack(l[0], 3);
    check("scattered: two unpacks of a layer's rows, out of order", u.g, sizes(256), {{9, 2, 2, 1, false}});
}

void none()
{
    Builder b = base();
    const uint32_t x = b.xor_(0, 1);
    const V bits = b.unpack(x, 4);
    b.lwe_layer(0, bits, 2);
    b.pack({x, 2});
    check("no polynomial linear node", b.g, sizes(256), {});
}

void append()
{
    Builder a = base();
    const V x = {a.xor_(0, 1), a.xor_(2, 3), a.xor_(4, 5)};
    a.poly_layer(1, x, 2);
    a.pack({x[0], 3});
    Builder b = base();
    const uint32_t y = b.xor_(5, 0);
    b.pack({y, 1, 2});
    const V l = b.poly_layer(1, {y, 4, y}, 2);
    b.poly_layer(6, {l[1], l[0]}, 1);
    P::Graph m = a.g;
    const size_t before = m.nodes.size(), listed = m.listed_operands();
    const uint32_t base_id = m.append(b.g);
    bool ok = base_id == before && m.nodes.size() == before + b.g.nodes.size() && m.listed_operands() == listed + b.g.listed_operands();
    for (size_t id = 0; ok && id < before; id++) { // the first graph's nodes keep their operands
        const P::Node &n = m.nodes[id], &o = a.g.nodes[id];
        ok = n.op == o.op && n.list_at == o.list_at && n.count == o.count;
        for (size_t i = 0; ok && i < (size_t)n.n_in + (n.n_in ? 0 : n.count); i++) ok = m.operand(n, i) == a.g.operand(o, i);
    }
    for (size_t id = 0; ok && id < b.g.nodes.size(); id++) { // the second graph's are shifted, lists included
        const P::Node &n = m.nodes[before + id], &o = b.g.nodes[id];
        ok = n.op == o.op && n.param == o.param && n.count == o.count && n.lin_slot == o.lin_slot && n.lin_rows == o.lin_rows && n.n_in == o.n_in;
        if (ok && n.op == P::kNodeGlwePolyLinear) ok = n.list_at == o.list_at + listed;
        for (size_t i = 0; ok && i < (size_t)n.n_in + (n.n_in ? 0 : n.count); i++) ok = m.operand(n, i) == b.g.operand(o, i) + base_id;
    }
    expect(ok, "append: the second graph's nodes and lists are not shifted behind the first's");
    // level 2: the first graph's in-place layer and the second's scattered one share (slot 1, M 2, K 3): one group, through the table
    check("append: two graphs' layers of one key are one group", m, sizes(256), {{1, 2, 3, 2, false}, {6, 1, 2, 1, false}});
    std::printf("append shifts the lists%s\n", ok ? " ok" : " FAILED");
}

} // namespace

int main()
{
    static_assert(P::kNodeGlwePolyLinear == 69, "the node kind's number is part of the recorded format");
    in_place_graphs();
    scattered_graphs();
    none();
    append();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("glwe_poly_graph_plan ok\n");
    return 0;
}
