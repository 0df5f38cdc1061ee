// glwe_keyswitch_ops.cpp — the GLWE keyswitch, one automorphism round and the homomorphic trace as rows of the operation table
// (spf_amd/csrc/spf_ops.hpp: OP_GLWE_KEYSWITCH / OP_GLWE_AUTOMORPHISM / OP_GLWE_TRACE, SPF_OP_GLWE_* = 12 / 13 / 14) and behind the
// generic door of the gate graphs (spf_graph_plan::op_node, what spf_graph_add_op records), on the CPU.
//
// Built from the two HIP-free headers alone with g++ -fsanitize=address,undefined and run directly
// (tests/test_glwe_keyswitch_ops_host.py).  It checks
//   * the three rows: numbers, arity, kinds, flags, parameter rules; pool_op_of for 12 / 13 / 14 and back; shape() == glwe_ks_shape;
//   * op_param on a generic shape with N = 16: slot 15 accepted and 16 refused, rounds 1 and 4 accepted and 0 and 5 refused, each
//     refusal with its number in the text; the trace's parameter forced to 0; and on N = 2048: round 11 accepted, 12 refused;
//   * the rows around them where they were: the existing twelve spf_graph_op values name the rows they named;
//   * a graph described through the generic door plans, field by field, as the same graph described through the three named
//     constructors' recorded nodes — on the scattered layout and the reload chain of tests/glwe_keyswitch_graph_cases.py, at
//     every batch size the GPU tests use, at GLWE sizes that lie consecutively and that are padded apart.
#include "../../spf_amd/csrc/spf_graph_plan.hpp"

#include <cstdio>
#include <cstring>
#include <string>

namespace P = spf_graph_plan;
namespace T = spf_ops;

namespace {

int g_failed = 0;
bool expect(bool ok, const std::string& what, size_t a = 0, size_t b = 0)
{
    if (!ok && g_failed++ < 40) std::printf("FAILED %s (%zu, %zu)\n", what.c_str(), a, b);
    return ok;
}

spf_params params(uint32_t N, uint32_t k)
{
    spf_params p;
    std::memset(&p, 0, sizeof p);
    p.polynomial_degree = N;
    p.glwe_size = k;
    p.lwe_dimension = 10;
    p.cbs_radix_count = 2;
    return p;
}

void rows()
{
    static_assert(T::OP_GLWE_KEYSWITCH == 14 && T::OP_GLWE_AUTOMORPHISM == 15 && T::OP_GLWE_TRACE == 16 && T::N_OPS == 17,
                  "the pool's numbers of the three operations (lanes, trace lines)");
    static_assert(SPF_OP_GLWE_KEYSWITCH == 12 && SPF_OP_GLWE_AUTOMORPHISM == 13 && SPF_OP_GLWE_TRACE == 14, "the public numbers");
    static_assert(SPF_OP_SAMPLE_EXTRACT == 0 && SPF_OP_MUL_XN == 9 && SPF_OP_PBS_UNIVARIATE == 10 && SPF_OP_PBS_BIVARIATE == 11,
                  "the existing twelve values do not move");
    const struct { int op, graph_op; T::ParamRule rule; } want[3] = {
        {T::OP_GLWE_KEYSWITCH, SPF_OP_GLWE_KEYSWITCH, T::PARAM_GLWE_KSK_SLOT},
        {T::OP_GLWE_AUTOMORPHISM, SPF_OP_GLWE_AUTOMORPHISM, T::PARAM_ROUND_1_TO_LOG_N},
        {T::OP_GLWE_TRACE, SPF_OP_GLWE_TRACE, T::PARAM_NONE}};
    for (const auto& w : want) {
        const T::OpRow& r = T::row(w.op);
        const std::string name = "row " + std::to_string(w.op);
        expect(r.op == w.op && r.graph_op == w.graph_op, name + ": its own number or its spf_graph_op");
        expect(r.arity == 1 && r.in_kind[0] == SPF_VAL_GLWE1 && r.in_kind[1] == T::kNone && r.in_kind[2] == T::kNone && r.out_kind == SPF_VAL_GLWE1,
               name + ": one GLWE1 in, one GLWE1 out");
        expect(!r.cmux_family && !T::cmux_family(w.op), name + ": not of the CMUX family");
        expect(r.rows_in_place && T::rows_in_place(w.op), name + ": rows_in_place");
        expect(r.param == w.rule, name + ": the parameter rule");
        expect(T::pool_op_of(w.graph_op) == w.op, name + ": pool_op_of of its spf_graph_op");
        expect(T::row(T::pool_op_of(w.graph_op)).graph_op == w.graph_op, name + ": and back");
    }
    // microseconds: the keyswitch and the round; the trace as measured (profiles/r34_glwe_keyswitch_pool.md)
    expect(!T::heavy(T::OP_GLWE_KEYSWITCH) && !T::heavy(T::OP_GLWE_AUTOMORPHISM) && !T::heavy(T::OP_GLWE_TRACE), "heavy on one of the three rows");
    for (int op = 0; op < T::OP_GLWE_KEYSWITCH; op++) expect(!T::rows_in_place(op), "rows_in_place on an older row", (size_t)op);
    expect(T::pool_op_of(15) == T::kNone && T::pool_op_of(-1) == T::kNone && T::pool_op_of(70) == T::kNone, "pool_op_of of a value that is no spf_graph_op");
    // the twelve that were there answer as before
    const int before[12] = {T::OP_SAMPLE_EXTRACT, T::OP_KEYSWITCH, T::OP_NOT, T::OP_GLWE_ADD, T::OP_CMUX, T::OP_GLEV_CMUX, T::OP_MULTIPLY_GGSW_GLWE,
                            T::OP_CBS, T::OP_SCHEME_SWITCH, T::OP_MUL_XN, T::OP_PBS_UNIVARIATE, T::OP_PBS_BIVARIATE};
    for (int g = 0; g < 12; g++) expect(T::pool_op_of(g) == before[g], "an existing spf_graph_op names another row", (size_t)g);
    for (const auto& prm : {params(16, 1), params(2048, 1), params(256, 3)})
        for (const auto& w : want) {
            const BatchShape a = T::shape(prm, w.op), b = glwe_ks_shape(prm);
            expect(a.n_in == b.n_in && a.n_in == 1 && a.in_words[0] == b.in_words[0] && a.in_words[1] == b.in_words[1] && a.in_words[2] == b.in_words[2] &&
                       a.out_words == b.out_words && a.max_batch == b.max_batch && a.out_words == (size_t)(prm.glwe_size + 1) * prm.polynomial_degree,
                   "shape() of a row is not glwe_ks_shape", (size_t)w.op, prm.polynomial_degree);
        }
    std::printf("rows%s\n", g_failed ? " FAILED" : " ok");
}

// op_param's verdict on (op, param): -1 refused, else the parameter it leaves; `text`: the refusal's words
long long rule(const spf_params& p, int op, uint64_t param, std::string* text = nullptr)
{
    const char* why = nullptr;
    const spf_status st = T::op_param(p, op, &param, &why);
    if (st == SPF_OK) return (long long)param;
    expect(st == SPF_ERR_INVALID_ARGUMENT && why, "a refusal is not SPF_ERR_INVALID_ARGUMENT with a text");
    if (text) *text = why ? why : "";
    return -1;
}

void parameters()
{
    const int failed_before = g_failed;
    const spf_params small = params(16, 1), tuned = params(2048, 1);
    std::string text;
    expect(T::log2_degree(small) == 4 && T::log2_degree(tuned) == 11, "log2_degree");
    expect(rule(small, T::OP_GLWE_KEYSWITCH, 0) == 0 && rule(small, T::OP_GLWE_KEYSWITCH, 15) == 15, "slots 0 and 15 are accepted");
    expect(rule(small, T::OP_GLWE_KEYSWITCH, 16, &text) == -1 && text == "slot 16 >= SPF_GLWE_KSK_SLOTS = 16", "slot 16 is refused, with its number: " + text);
    expect(rule(small, T::OP_GLWE_KEYSWITCH, (uint64_t)1 << 32, &text) == -1 && text.find("4294967296") != std::string::npos,
           "a slot beyond 32 bits is refused as it stands, not truncated: " + text);
    expect(rule(small, T::OP_GLWE_AUTOMORPHISM, 1) == 1 && rule(small, T::OP_GLWE_AUTOMORPHISM, 4) == 4, "rounds 1 and 4 = log2 N are accepted");
    expect(rule(small, T::OP_GLWE_AUTOMORPHISM, 0, &text) == -1 && text == "round 0 outside 1 .. log2 N = 4", "round 0 is refused, with its number: " + text);
    expect(rule(small, T::OP_GLWE_AUTOMORPHISM, 5, &text) == -1 && text == "round 5 outside 1 .. log2 N = 4", "round 5 is refused, with its number: " + text);
    expect(rule(tuned, T::OP_GLWE_AUTOMORPHISM, 11) == 11 && rule(tuned, T::OP_GLWE_AUTOMORPHISM, 12, &text) == -1 && text == "round 12 outside 1 .. log2 N = 11",
           "N = 2048: round 11 accepted, 12 refused: " + text);
    expect(rule(small, T::OP_GLWE_TRACE, 0) == 0 && rule(small, T::OP_GLWE_TRACE, 99) == 0 && rule(small, T::OP_GLWE_TRACE, ~(uint64_t)0) == 0,
           "the trace's parameter is forced to 0");
    // the rules that were there
    expect(rule(small, T::OP_SAMPLE_EXTRACT, 15) == 15 && rule(small, T::OP_SAMPLE_EXTRACT, 16) == -1 && rule(small, T::OP_MUL_XN, 35) == 3 &&
               rule(small, T::OP_NOT, 7) == 0 && rule(small, T::OP_PBS_BIVARIATE, 63) == 63 && rule(small, T::OP_PBS_BIVARIATE, 64) == -1,
           "an older parameter rule changed");
    std::printf("parameters%s\n", g_failed == failed_before ? " ok" : " FAILED");
}

// ---- the generic door against the named constructors

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

enum Mode { KS = 0, AU = 1, TR = 2 };

struct Builder {
    P::Graph g;
    bool door; // the three operations through op_node (spf_graph_add_op), or as the named constructors have always recorded them
    spf_params prm = params(16, 1);
    explicit Builder(bool through_the_door) : door(through_the_door) {}
    uint32_t input(int kind = SPF_VAL_GLWE1)
    {
        P::Node n{};
        n.op = -1; n.kind = kind;
        return g.add(n);
    }
    // a row of the table as spf_graph_add_op records it (both builders: these nodes are not what is compared)
    uint32_t op(spf_graph_op o, std::initializer_list<uint32_t> in, uint64_t param = 0)
    {
        const int pop = T::pool_op_of(o);
        const char* why = nullptr;
        expect(pop != T::kNone && T::op_param(prm, pop, &param, &why) == SPF_OK && in.size() == (size_t)T::row(pop).arity, "the builder's own operation");
        return g.add(P::op_node(pop, in.begin(), param));
    }
    uint32_t poly_row(uint32_t slot, uint32_t glwe)
    {
        P::Node n{};
        n.op = P::kNodeGlwePolyLinear; n.kind = SPF_VAL_GLWE1; n.lin_slot = slot; n.lin_rows = 1;
        return g.add_listed(n, &glwe, 1, 1);
    }
    uint32_t ks(Mode mode, uint32_t param, uint32_t glwe)
    {
        if (door) return op(mode == KS ? SPF_OP_GLWE_KEYSWITCH : mode == AU ? SPF_OP_GLWE_AUTOMORPHISM : SPF_OP_GLWE_TRACE, {glwe}, param);
        P::Node n{}; // the recorded format of spf_graph_add_glwe_keyswitch / _automorphism / _trace: kinds 70 / 71 / 72
        n.op = 70 + (int)mode; n.kind = SPF_VAL_GLWE1; n.n_in = 1; n.in[0] = glwe; n.param = mode == TR ? 0 : param;
        return g.add(n);
    }
};

// `Scattered` of tests/glwe_keyswitch_graph_cases.py: GLWE | LWE1 | GLWE | GGSW | GLWE | LWE1 | GLWE | GLWE; a CMUX, a polynomial
// linear row and two XORs on level 1; B nodes over the inputs [4, 0, 4, 2, 1][:B] and B over [poly row, CMUX, CMUX, XOR, XOR'][:B]
P::Graph scattered(bool door, Mode mode, uint32_t param, size_t B)
{
    Builder b(door);
    uint32_t ins[5], sel = 0;
    for (int i = 0; i < 5; i++) {
        ins[i] = b.input();
        if (i == 0 || i == 2) b.input(SPF_VAL_LWE1);
        if (i == 1) sel = b.input(SPF_VAL_GGSW1);
    }
    const uint32_t cm = b.op(SPF_OP_CMUX, {sel, ins[0], ins[1]});
    const uint32_t pl = b.poly_row(34, ins[2]);
    const uint32_t x1 = b.op(SPF_OP_GLWE_ADD, {ins[3], ins[4]});
    const uint32_t x2 = b.op(SPF_OP_GLWE_ADD, {ins[0], ins[4]});
    const uint32_t picks[5] = {4, 0, 4, 2, 1}, level1[5] = {pl, cm, cm, x1, x2};
    for (size_t i = 0; i < B; i++) b.ks(mode, param, ins[picks[i]]);
    for (size_t i = 0; i < B; i++) b.ks(mode, param, level1[i]);
    return b.g;
}

// `reload_rounds`: keyswitch nodes over scattered inputs feeding keyswitch nodes in place; and the three modes chained
P::Graph chain(bool door)
{
    Builder b(door);
    const uint32_t ins[3] = {b.input(), b.input(), b.input()};
    uint32_t a[3];
    const int order[3] = {2, 0, 1};
    for (int i = 0; i < 3; i++) a[i] = b.ks(KS, 7, ins[order[i]]);
    for (int i = 0; i < 3; i++) b.ks(KS, 7, a[i]);
    const uint32_t t = b.ks(TR, 99, a[1]); // (a trace's parameter is forced to 0 by either door)
    b.ks(AU, 4, t);
    b.ks(AU, 1, ins[0]);
    b.ks(KS, 15, t);
    return b.g;
}

bool same_node(const P::Node& a, const P::Node& b)
{
    return a.op == b.op && a.kind == b.kind && a.param == b.param && a.n_in == b.n_in && a.in[0] == b.in[0] && a.in[1] == b.in[1] && a.in[2] == b.in[2] &&
           a.count == b.count && a.list_at == b.list_at && a.lin_slot == b.lin_slot && a.lin_rows == b.lin_rows && a.level == b.level && a.off == b.off &&
           a.host == b.host;
}

size_t compare(const std::string& name, P::Graph by_door, P::Graph by_name, const P::Sizes& sz)
{
    const int failed_before = g_failed;
    const P::Plan p = P::plan(by_door, sz), q = P::plan(by_name, sz);
    expect(by_door.nodes.size() == by_name.nodes.size(), name + ": the number of nodes", by_door.nodes.size(), by_name.nodes.size());
    for (size_t i = 0; i < by_door.nodes.size() && i < by_name.nodes.size(); i++)
        expect(same_node(by_door.nodes[i], by_name.nodes[i]), name + ": a node differs after planning", i);
    expect(p.inputs_bytes == q.inputs_bytes && p.arena_bytes == q.arena_bytes && p.stage_bytes == q.stage_bytes && p.n_levels == q.n_levels,
           name + ": inputs_bytes, arena_bytes, stage_bytes or n_levels", p.arena_bytes, q.arena_bytes);
    expect(p.has_pufks == q.has_pufks && p.has_linear == q.has_linear && p.has_glwe_poly == q.has_glwe_poly && p.has_glwe_ks == q.has_glwe_ks,
           name + ": a has_ flag");
    expect(p.table == q.table, name + ": the pointer table", p.table.size(), q.table.size());
    size_t mine = 0;
    if (expect(p.groups.size() == q.groups.size(), name + ": the number of groups", p.groups.size(), q.groups.size()))
        for (size_t i = 0; i < p.groups.size(); i++) {
            const P::Group &a = p.groups[i], &b = q.groups[i];
            bool ok = a.key == b.key && a.members == b.members && a.out_off == b.out_off && a.one_lut == b.one_lut;
            for (int s = 0; s < 3; s++) ok = ok && a.contiguous[s] == b.contiguous[s] && a.first_off[s] == b.first_off[s] && a.ptr_index[s] == b.ptr_index[s];
            expect(ok, name + ": a group differs", i);
            mine += P::is_glwe_ks_node(a.key.op) ? 1 : 0;
        }
    for (const auto& n : by_door.nodes) expect(n.op < SPF_OP_GLWE_KEYSWITCH || n.op > SPF_OP_GLWE_TRACE, name + ": the door recorded a spf_graph_op value, not the node kind");
    std::printf("%s: %zu groups of the three kinds%s\n", name.c_str(), mine, g_failed == failed_before ? " ok" : " FAILED");
    return mine;
}

void doors()
{
    static_assert(P::kNodeGlweKeyswitch == 70 && P::kNodeGlweAutomorphism == 71 && P::kNodeGlweTrace == 72, "the recorded node kinds");
    expect(P::node_op_of(T::OP_GLWE_KEYSWITCH) == 70 && P::node_op_of(T::OP_GLWE_AUTOMORPHISM) == 71 && P::node_op_of(T::OP_GLWE_TRACE) == 72,
           "node_op_of of the three operations");
    for (int op = 0; op < T::OP_GLWE_KEYSWITCH; op++)
        if (T::row(op).graph_op != T::kNone) expect(P::node_op_of(op) == T::row(op).graph_op, "node_op_of of an older row is not its spf_graph_op", (size_t)op);
    const struct { Mode mode; uint32_t param; const char* name; } modes[3] = {{KS, 3, "keyswitch"}, {AU, 2, "automorphism"}, {TR, 0, "trace"}};
    size_t groups = 0;
    for (const auto& m : modes)
        for (size_t B : {(size_t)1, (size_t)3, (size_t)4, (size_t)5})
            for (size_t glwe : {(size_t)256, (size_t)128, (size_t)32768}) {
                const std::string name = std::string("scattered ") + m.name + " B=" + std::to_string(B) + " glwe=" + std::to_string(glwe);
                groups += compare(name, scattered(true, m.mode, m.param, B), scattered(false, m.mode, m.param, B), sizes(glwe));
            }
    expect(groups == 3 * 4 * 3 * 2, "scattered: two groups of the kind per graph", groups);
    for (size_t glwe : {(size_t)256, (size_t)128})
        expect(compare("chain glwe=" + std::to_string(glwe), chain(true), chain(false), sizes(glwe)) == 6, "chain: six groups");
    // the comparison bites: another slot is another plan
    {
        P::Graph a = scattered(true, KS, 3, 3), b = scattered(false, KS, 4, 3);
        const P::Plan p = P::plan(a, sizes(256)), q = P::plan(b, sizes(256));
        bool same = p.groups.size() == q.groups.size();
        for (size_t i = 0; same && i < p.groups.size(); i++) same = p.groups[i].key == q.groups[i].key;
        expect(!same, "two graphs with different slots compare equal: the comparison proves nothing");
    }
}

} // namespace

int main()
{
    rows();
    parameters();
    doors();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("glwe_keyswitch_ops ok\n");
    return 0;
}
