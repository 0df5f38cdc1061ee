// graph_plan.cpp — the planner of the gate graphs (spf_amd/csrc/spf_graph_plan.hpp) on the CPU.
//
// Built from the HIP-free header alone with g++ -fsanitize=address,undefined and run directly (tests/test_graph_plan.py).
//   graph_plan FILE                   a recorded circuit as a file of numbers (format below): built through the header, planned,
//                                     every invariant of the plan checked by brute force, the plan printed
//   graph_plan --append FILE_A FILE_B the same for graph A with graph B appended (Graph::append), under A's sizes
// Checked: every operand's level is below its node's; a group's members share its key and stand in node order, the groups in key
// order; blocks are 256-aligned and disjoint and a node's offset is its row in its group's block; a slot marked in place has
// operands that are consecutive from first_off, any other slot a pointer row equal to its operands' offsets (member order;
// layer-major for linear and polynomial linear, int-major for unpack, one per member for the GLWE keyswitch, automorphism and trace
// nodes); the pointer rows tile the table; the CMUX units are the members' units,
// non-decreasing in selector, ties in member order; the stage size is the largest gathered slot; planning twice gives one plan.
//
// File format (decimal numbers, white space between them):
//   sizes  bytes(LWE0) bytes(LWE1) bytes(GLWE1) bytes(GGSW1) bytes(GLEV1)  cbs_radix_count  pufks_stage
//   nodes  n      then per node    op kind param  unpack_width  linear_slot linear_rows  k  operand[0] ... operand[k-1]
// (op: a spf_graph_op, 64 .. 72, -1 input, -2 constant; the nodes of one unpack, linear or polynomial linear call each have their
// line; a polynomial linear node (69) gives its slot and rows as a linear node does, the nodes 70 .. 72 their slot / round / 0 as param)
//
// The plan as printed (what the test compares and digests):
//   levels n l..    offsets n o..    per group: "group level op kind slot rows n | members out_off | (contiguous first_off
//   ptr_index) x 3 | one_lut" (first_off where in place, ptr_index where not, else 0) and "members id.."    table n t..
//   (18446744073709551615: null)    sizes inputs_bytes arena_bytes stage_bytes n_levels
#include "../../spf_amd/csrc/spf_graph_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace P = spf_graph_plan;

namespace {

int g_failed = 0;
void fail(const char* msg, size_t a = 0, size_t b = 0)
{
    if (g_failed++ < 20) std::printf("FAILED %s (%zu, %zu)\n", msg, a, b);
}

bool read_circuit(const char* path, P::Graph* g, P::Sizes* sz)
{
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    unsigned long long b[5], radix = 0, stage = 0, nn = 0;
    bool ok = std::fscanf(f, " sizes %llu %llu %llu %llu %llu %llu %llu nodes %llu", &b[0], &b[1], &b[2], &b[3], &b[4], &radix, &stage, &nn) == 8;
    for (int k = 0; k < 5; k++) sz->bytes[k] = (size_t)b[k];
    sz->cbs_radix_count = (size_t)radix;
    sz->pufks_stage = stage != 0;
    const size_t base = g->nodes.size();
    for (unsigned long long i = 0; ok && i < nn; i++) {
        long long op = 0, kind = 0;
        unsigned long long param = 0, width = 0, slot = 0, rows = 0, k = 0;
        ok = std::fscanf(f, "%lld %lld %llu %llu %llu %llu %llu", &op, &kind, &param, &width, &slot, &rows, &k) == 7;
        std::vector<uint32_t> ids((size_t)k);
        for (auto& x : ids) {
            unsigned long long v = 0;
            ok = ok && std::fscanf(f, "%llu", &v) == 1 && v < i;
            x = (uint32_t)(base + v);
        }
        if (!ok) break;
        if (base + i < g->nodes.size()) { // a further node of an unpack or linear call
            const P::Node& have = g->nodes[base + i];
            ok = have.op == op && have.param == param && have.kind == kind;
            continue;
        }
        P::Node n{};
        n.op = (int32_t)op; n.kind = (int32_t)kind; n.param = param;
        if (op == P::kNodeUnpack) {
            ok = param == 0 && k == 1 && width > 0;
            n.n_in = 1; n.in[0] = ids[0]; n.count = (uint32_t)width;
            if (ok) g->add_numbered(n, (size_t)width);
        } else if (op == P::kNodeLweLinear || op == P::kNodeGlwePolyLinear) {
            ok = param == 0 && k > 0 && rows > 0 && (op == P::kNodeLweLinear || kind == SPF_VAL_GLWE1);
            n.lin_slot = (uint32_t)slot; n.lin_rows = (uint32_t)rows;
            if (ok) g->add_listed(n, ids.data(), ids.size(), (size_t)rows);
        } else if (op == P::kNodePack || op == P::kNodePufks) {
            ok = k > 0;
            if (ok) g->add_listed(n, ids.data(), ids.size());
        } else if (op == P::kNodeGlweKeyswitch || op == P::kNodeGlweAutomorphism || op == P::kNodeGlweTrace) {
            ok = k == 1 && kind == SPF_VAL_GLWE1 && (op != P::kNodeGlweTrace || param == 0);
            n.n_in = 1; n.in[0] = ids[0];
            if (ok) g->add(n);
        } else {
            ok = k <= 3 && (op < 0 ? k == 0 : op == P::kNodeRotCmux ? k == 2 : spf_ops::pool_op_of((int)op) != spf_ops::kNone && (int)k == P::op_row((int)op).arity);
            n.n_in = (uint32_t)k;
            for (size_t j = 0; j < ids.size() && j < 3; j++) n.in[j] = ids[j];
            if (ok) g->add(n);
        }
    }
    std::fclose(f);
    return ok && g->nodes.size() == base + nn;
}

std::string dump(const P::Graph& g, const P::Plan& p)
{
    std::string s = "levels " + std::to_string(g.nodes.size());
    for (const auto& n : g.nodes) s += " " + std::to_string(n.level);
    s += "\noffsets " + std::to_string(g.nodes.size());
    for (const auto& n : g.nodes) s += " " + std::to_string(n.off);
    s += "\n";
    for (const auto& gr : p.groups) {
        const P::GroupKey& k = gr.key;
        s += "group " + std::to_string(k.level) + " " + std::to_string(k.op) + " " + std::to_string(k.kind) + " " + std::to_string(k.slot) + " " +
             std::to_string(k.rows) + " " + std::to_string(k.n) + " | " + std::to_string(gr.members.size()) + " " + std::to_string(gr.out_off) + " |";
        for (int sl = 0; sl < 3; sl++)
            s += " " + std::to_string((int)gr.contiguous[sl]) + " " + std::to_string(gr.contiguous[sl] ? gr.first_off[sl] : (size_t)0) + " " +
                 std::to_string(gr.contiguous[sl] ? (size_t)0 : gr.ptr_index[sl]);
        s += " | " + std::to_string((int)gr.one_lut) + "\nmembers";
        for (uint32_t id : gr.members) s += " " + std::to_string(id);
        s += "\n";
    }
    s += "table " + std::to_string(p.table.size());
    for (size_t t : p.table) s += " " + std::to_string(t);
    s += "\nsizes " + std::to_string(p.inputs_bytes) + " " + std::to_string(p.arena_bytes) + " " + std::to_string(p.stage_bytes) + " " +
         std::to_string(p.n_levels) + "\n";
    return s;
}

// the key of a node, from its fields (written out here, not taken from the header)
P::GroupKey expected_key(const P::Graph& g, const P::Node& n)
{
    P::GroupKey k{n.level, n.op, 0, 0, 0, n.param};
    switch (n.op) {
    case P::kNodeUnpack:
    case P::kNodePack: k.n = n.count; break;
    case P::kNodePufks: k.kind = (uint8_t)g.nodes[g.operand(n, 0)].kind; k.n = n.count; break;
    case P::kNodeLweLinear: k.kind = (uint8_t)n.kind; k.slot = (uint8_t)n.lin_slot; k.rows = (uint16_t)n.lin_rows; k.n = n.count; break;
    case P::kNodeGlwePolyLinear: k.kind = (uint8_t)SPF_VAL_GLWE1; k.slot = (uint8_t)n.lin_slot; k.rows = (uint16_t)n.lin_rows; k.n = n.count; break;
    case P::kNodeGlweKeyswitch: // the slot
    case P::kNodeGlweAutomorphism: k.n = n.param; break; // the round
    case P::kNodeGlweTrace: k.n = 0; break;
    default: break;
    }
    return k;
}

struct Slot { std::vector<size_t> offs; size_t row_bytes; bool staged; };

// the operand rows of slot `s` of a group in the order its launch reads them; false: the group has no such slot
bool slot_of(const P::Graph& g, const P::Sizes& sz, const P::Group& gr, int s, Slot* out)
{
    const int32_t op = gr.key.op;
    out->offs.clear();
    auto all_of = [&](const P::Node& n) { g.for_operands(n, [&](uint32_t in) { out->offs.push_back(g.nodes[in].off); }); };
    if (op == P::kNodePufks || op == P::kNodePack) {
        if (s) return false;
        for (uint32_t id : gr.members) all_of(g.nodes[id]);
        out->row_bytes = op == P::kNodePack ? sz.of(SPF_VAL_GLWE1) : sz.of(gr.key.kind);
        out->staged = op == P::kNodePufks && sz.pufks_stage;
        return true;
    }
    if (op == P::kNodeGlweKeyswitch || op == P::kNodeGlweAutomorphism || op == P::kNodeGlweTrace) { // one GLWE per member
        if (s) return false;
        for (uint32_t id : gr.members) {
            if (g.nodes[id].n_in != 1) fail("a node of the GLWE keyswitch family has not one operand", id);
            out->offs.push_back(g.nodes[g.nodes[id].in[0]].off);
        }
        out->row_bytes = sz.of(SPF_VAL_GLWE1);
        out->staged = false;
        return true;
    }
    if (op == P::kNodeLweLinear || op == P::kNodeGlwePolyLinear) { // layer-major: the list of every M-th member
        if (s) return false;
        if (gr.members.size() % gr.key.rows) fail("a linear group is no whole number of layers", gr.members.size(), gr.key.rows);
        for (size_t i = 0; i < gr.members.size(); i += gr.key.rows) {
            for (size_t m = 0; m < gr.key.rows && i + m < gr.members.size(); m++)
                if (gr.members[i + m] != gr.members[i] + m || g.nodes[gr.members[i + m]].param != m) fail("a layer's rows are not successive members", i, m);
            all_of(g.nodes[gr.members[i]]);
        }
        out->row_bytes = op == P::kNodeGlwePolyLinear ? sz.of(SPF_VAL_GLWE1) : sz.of(gr.key.kind);
        out->staged = false;
        return true;
    }
    if (op == P::kNodeUnpack) { // int-major: the source of every width-th member
        if (s) return false;
        const size_t w = (size_t)gr.key.n;
        if (gr.members.size() % w) fail("an unpack group is no whole number of integers", gr.members.size(), w);
        for (size_t i = 0; i < gr.members.size(); i += w) {
            for (size_t b = 0; b < w && i + b < gr.members.size(); b++)
                if (gr.members[i + b] != gr.members[i] + b || g.nodes[gr.members[i + b]].param != b) fail("an integer's bits are not successive members", i, b);
            out->offs.push_back(g.nodes[g.nodes[gr.members[i]].in[0]].off);
        }
        out->row_bytes = sz.of(SPF_VAL_GLWE1);
        out->staged = true;
        return true;
    }
    if (op == P::kNodeRotCmux || P::op_row(op).cmux_family) return false;
    const spf_ops::OpRow& info = P::op_row(op);
    if (s >= info.arity) return false;
    for (uint32_t id : gr.members) out->offs.push_back(g.nodes[g.nodes[id].in[s]].off);
    out->row_bytes = sz.of(info.in_kind[s]);
    out->staged = true;
    return true;
}

void check(const P::Graph& g, const P::Sizes& sz, const P::Plan& p)
{
    const size_t nn = g.nodes.size();
    // ---- levels
    uint32_t top = 0;
    for (size_t id = 0; id < nn; id++) {
        const P::Node& n = g.nodes[id];
        if (n.op < 0 && n.level != 0) fail("an input or constant is not on level 0", id);
        g.for_operands(n, [&](uint32_t in) {
            if (in >= id) fail("an operand does not precede its user", id, in);
            else if (g.nodes[in].level >= n.level) fail("an operand's level is not below its node's", id, in);
        });
        top = std::max(top, n.level);
    }
    if (top != p.n_levels) fail("n_levels is not the highest level", top, p.n_levels);
    // ---- groups
    std::vector<int> in_group(nn, 0);
    for (size_t gi = 0; gi < p.groups.size(); gi++) {
        const P::Group& gr = p.groups[gi];
        if (gr.members.empty()) { fail("an empty group", gi); continue; }
        if (gi && !(p.groups[gi - 1].key < gr.key)) fail("the groups are not in key order", gi);
        for (size_t i = 0; i < gr.members.size(); i++) {
            const uint32_t id = gr.members[i];
            if (id >= nn || g.nodes[id].op < 0) { fail("a member is no operation node", gi, i); continue; }
            in_group[id]++;
            if (!(expected_key(g, g.nodes[id]) == gr.key)) fail("a member does not have its group's key", gi, id);
            if (i && gr.members[i - 1] >= id) fail("members are not in node order", gi, i);
        }
    }
    for (size_t id = 0; id < nn; id++)
        if (in_group[id] != (g.nodes[id].op >= 0 ? 1 : 0)) fail("a node is not in exactly one group", id, (size_t)in_group[id]);
    // ---- blocks: inputs and constants, then the groups; all pairs by a sweep over the sorted starts
    std::vector<std::pair<size_t, size_t>> blocks; // (start, end)
    for (size_t id = 0; id < nn; id++)
        if (g.nodes[id].op < 0) {
            const size_t o = g.nodes[id].off, e = o + sz.of(g.nodes[id].kind);
            if (o % P::kAlign) fail("an input is not 256-aligned", id, o);
            if (e > p.inputs_bytes) fail("an input ends beyond the input region", id, e);
            blocks.emplace_back(o, e);
        }
    if (p.inputs_bytes % P::kAlign) fail("the input region is not 256-aligned", p.inputs_bytes);
    for (size_t gi = 0; gi < p.groups.size(); gi++) {
        const P::Group& gr = p.groups[gi];
        if (gr.members.empty()) continue;
        const size_t rb = sz.of(g.nodes[gr.members[0]].kind);
        if (gr.out_off % P::kAlign) fail("a group's block is not 256-aligned", gi, gr.out_off);
        if (gr.out_off < p.inputs_bytes) fail("a group's block lies in the input region", gi, gr.out_off);
        if (gr.out_off + gr.members.size() * rb > p.arena_bytes) fail("a group's block ends beyond the arena", gi);
        for (size_t i = 0; i < gr.members.size(); i++) {
            if (sz.of(g.nodes[gr.members[i]].kind) != rb) fail("the rows of a group differ in size", gi, i);
            if (g.nodes[gr.members[i]].off != gr.out_off + i * rb) fail("a node's offset is not its row in its group's block", gi, i);
        }
        blocks.emplace_back(gr.out_off, gr.out_off + gr.members.size() * rb);
    }
    std::sort(blocks.begin(), blocks.end());
    for (size_t i = 1; i < blocks.size(); i++)
        if (blocks[i].first < blocks[i - 1].second) fail("two blocks share a byte", blocks[i - 1].first, blocks[i].first);
    if (p.arena_bytes % P::kAlign) fail("the arena is not 256-aligned", p.arena_bytes);
    // ---- operand access, the table, the stage size
    size_t table_at = 0, stage = 0;
    bool any_pufks = false, any_linear = false, any_poly = false, any_glwe_ks = false;
    for (size_t gi = 0; gi < p.groups.size(); gi++) {
        const P::Group& gr = p.groups[gi];
        if (gr.members.empty()) continue;
        const int32_t op = gr.key.op;
        any_pufks = any_pufks || op == P::kNodePufks;
        any_linear = any_linear || op == P::kNodeLweLinear;
        any_poly = any_poly || op == P::kNodeGlwePolyLinear;
        any_glwe_ks = any_glwe_ks || op == P::kNodeGlweKeyswitch || op == P::kNodeGlweAutomorphism || op == P::kNodeGlweTrace;
        const bool rot = op == P::kNodeRotCmux;
        if (rot || (op < P::kNodeUnpack && P::op_row(op).cmux_family)) {
            // the members' units in member order
            const size_t per = op == SPF_OP_GLEV_CMUX ? sz.cbs_radix_count : 1, gw = sz.of(SPF_VAL_GLWE1);
            std::vector<P::Unit> want;
            for (uint32_t id : gr.members) {
                const P::Node& n = g.nodes[id];
                for (size_t j = 0; j < per; j++) {
                    const size_t sel = g.nodes[n.in[0]].off;
                    if (rot) want.push_back(P::Unit{{sel, g.nodes[n.in[1]].off, P::kNull, n.off}});
                    else if (op == SPF_OP_MULTIPLY_GGSW_GLWE) want.push_back(P::Unit{{sel, P::kNull, g.nodes[n.in[1]].off, n.off}});
                    else want.push_back(P::Unit{{sel, g.nodes[n.in[1]].off + j * gw, g.nodes[n.in[2]].off + j * gw, n.off + j * gw}});
                }
            }
            if (gr.contiguous[0] || gr.ptr_index[0] != table_at) fail("a CMUX group's units do not start where the table stood", gi, gr.ptr_index[0]);
            if (table_at + 4 * want.size() > p.table.size()) { fail("a CMUX group's units end beyond the table", gi); return; }
            // a permutation, non-decreasing in selector, ties in member order: the units of one selector, in table order, are
            // the wanted units of that selector in member order
            std::map<size_t, std::vector<size_t>> by_sel;
            for (size_t u = 0; u < want.size(); u++) by_sel[want[u].p[0]].push_back(u);
            std::map<size_t, size_t> taken;
            for (size_t u = 0; u < want.size(); u++) {
                const size_t* t = &p.table[table_at + 4 * u];
                if (u && t[0] < t[-4]) fail("units are not in selector order", gi, u);
                auto it = by_sel.find(t[0]);
                size_t& k = taken[t[0]];
                if (it == by_sel.end() || k >= it->second.size()) { fail("a unit that is none of the members'", gi, u); continue; }
                const P::Unit& w = want[it->second[k++]];
                if (!std::equal(t, t + 4, w.p)) fail("a unit is not the next of its selector in member order", gi, u);
            }
            table_at += 4 * want.size();
            continue;
        }
        bool in_place[3] = {false, false, false};
        Slot sl;
        for (int s = 0; s < 3; s++) {
            if (!slot_of(g, sz, gr, s, &sl)) {
                if (gr.contiguous[s] || gr.first_off[s] || gr.ptr_index[s]) fail("a slot the group does not have is described", gi, (size_t)s);
                continue;
            }
            in_place[s] = gr.contiguous[s];
            const bool lut_slot = gr.one_lut && op < P::kNodeUnpack && s == P::op_row(op).arity - 1; // every row is the one table
            if (gr.contiguous[s]) {
                for (size_t i = 0; i < sl.offs.size(); i++)
                    if (sl.offs[i] != gr.first_off[s] + (lut_slot ? 0 : i * sl.row_bytes)) { fail("a slot marked in place is not consecutive from first_off", gi, i); break; }
            } else {
                if (gr.ptr_index[s] != table_at) fail("a pointer row does not start where the table stood", gi, (size_t)s);
                if (table_at + sl.offs.size() > p.table.size()) { fail("a pointer row ends beyond the table", gi); return; }
                for (size_t i = 0; i < sl.offs.size(); i++)
                    if (p.table[table_at + i] != sl.offs[i]) { fail("a pointer row is not its operands' offsets in member order", gi, i); break; }
                table_at += sl.offs.size();
                if (sl.staged) stage = std::max(stage, sl.offs.size() * sl.row_bytes);
                // the planner may not scatter what lies consecutively — but for the bivariate rule, and a pack, which always reads through the table
                bool consecutive = true;
                for (size_t i = 1; i < sl.offs.size(); i++) consecutive = consecutive && sl.offs[i] == sl.offs[0] + i * sl.row_bytes;
                if (consecutive && op != P::kNodePack && op != SPF_OP_PBS_BIVARIATE) fail("consecutive operands are read through a pointer row", gi, (size_t)s);
            }
        }
        if (gr.one_lut) {
            if (op != SPF_OP_PBS_UNIVARIATE && op != SPF_OP_PBS_BIVARIATE) fail("one_lut on a group that has no table", gi);
            else if (!gr.contiguous[P::op_row(op).arity - 1]) fail("one table for the group, but not read in place", gi);
        }
        if (op == SPF_OP_PBS_UNIVARIATE || op == SPF_OP_PBS_BIVARIATE) {
            const int s = P::op_row(op).arity - 1;
            bool one = true;
            for (uint32_t id : gr.members) one = one && g.nodes[id].in[s] == g.nodes[gr.members[0]].in[s];
            if (one != gr.one_lut) fail("one_lut does not say whether the members share their table", gi);
        }
        if (op == SPF_OP_PBS_BIVARIATE && in_place[0] != in_place[1]) fail("one bivariate input in place, the other not", gi);
    }
    if (table_at != p.table.size()) fail("the pointer rows do not tile the table", table_at, p.table.size());
    if (stage != p.stage_bytes) fail("the stage size is not the largest gathered slot", stage, p.stage_bytes);
    if (any_pufks != p.has_pufks || any_linear != p.has_linear) fail("has_pufks / has_linear do not say what the graph holds");
    if (any_poly != p.has_glwe_poly || any_glwe_ks != p.has_glwe_ks) fail("has_glwe_poly / has_glwe_ks do not say what the graph holds");
}

} // namespace

int main(int argc, char** argv)
{
    const bool append = argc == 4 && std::string(argv[1]) == "--append";
    if (argc != 2 && !append) {
        std::printf("usage: graph_plan FILE | graph_plan --append FILE_A FILE_B\n");
        return 2;
    }
    P::Graph g;
    P::Sizes sz{}, sz_b{};
    if (!read_circuit(argv[append ? 2 : 1], &g, &sz)) {
        std::printf("FAILED cannot read the circuit %s\n", argv[append ? 2 : 1]);
        return 1;
    }
    if (append) {
        P::Graph b;
        if (!read_circuit(argv[3], &b, &sz_b)) {
            std::printf("FAILED cannot read the circuit %s\n", argv[3]);
            return 1;
        }
        const size_t before = g.nodes.size(), listed = g.listed_operands();
        if (g.append(b) != before || g.nodes.size() != before + b.nodes.size() || g.listed_operands() != listed + b.listed_operands())
            fail("append does not put the second graph behind the first");
    }
    const P::Plan p = P::plan(g, sz);
    check(g, sz, p);
    const std::string first = dump(g, p);
    P::Graph again = g; // (with the levels and offsets of the first plan in its nodes, as a graph that is planned a second time has)
    const P::Plan p2 = P::plan(again, sz);
    if (dump(again, p2) != first) fail("planning twice gives two plans");
    std::fputs(first.c_str(), stdout);
    if (g_failed) return 1;
    std::printf("graph_plan ok\n");
    return 0;
}
