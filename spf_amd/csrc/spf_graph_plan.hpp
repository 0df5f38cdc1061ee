// spf_graph_plan.hpp — what the executor of gate graphs (spf_graph.hpp) decides before it touches a device: the graph's host-side
// data, and the plan of a run.
//
//   * kNodeRows: one row per node constructor that is no row of the operation table (spf_ops.hpp) — where its operands are kept,
//     what its group key is made of, how a group reads its operands, what it needs at run time.  Graph, key_of and plan_access
//     know a constructor kind through its row only.
//   * Graph: the node list and the operand lists of the nodes whose operands do not fit a node (pack, public functional keyswitch,
//     linear map).  Where operand ids are kept is known here only: for_operands / operand read them, add / add_numbered /
//     add_listed write them, append shifts them.
//   * plan(): the level of every node, the groups (one launch each) and their order, every arena offset, per group and operand
//     slot whether the rows are read in place or through a pointer row, the order of the CMUX units, the size of the stage
//     buffers — as offsets into an arena that does not exist yet.  It takes the five value sizes, cbs_radix_count and whether the
//     rows of a public functional keyswitch are gathered as plain numbers; spf_graph.hpp allocates, adds the arena's base to the
//     table and copies it up.
//
// Free of HIP (as spf_arena_plan.hpp, spf_glwe_poly_plan.hpp and spf_wake.hpp): tests/cpp/graph_plan.cpp drives it on the CPU
// under the sanitizers and checks every invariant below by brute force (tests/test_graph_plan.py).
#pragma once

#include "spf_ops.hpp"

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

namespace spf_graph_plan {

// the node constructors that are no spf_graph_op (spf_graph_add_unpack / spf_graph_add_pack / spf_graph_add_blind_rotation /
// spf_graph_add_public_functional_keyswitch / spf_graph_add_lwe_linear / spf_graph_add_glwe_poly_linear /
// spf_graph_add_glwe_keyswitch / spf_graph_add_glwe_automorphism / spf_graph_add_glwe_trace)
enum : int32_t {
    kNodeUnpack = 64, kNodePack = 65, kNodeRotCmux = 66, kNodePufks = 67, kNodeLweLinear = 68, kNodeGlwePolyLinear = 69,
    kNodeGlweKeyswitch = 70, kNodeGlweAutomorphism = 71, kNodeGlweTrace = 72
};
// the three nodes of spf_glwe_keyswitch.hpp: one GLWE1 operand in Node::in[0], one GLWE1 result; Node::param is the keyswitch-key
// slot, the round, or 0
inline bool is_glwe_ks_node(int32_t op) { return op >= kNodeGlweKeyswitch && op <= kNodeGlweTrace; }

// What a kind's groups need at run time besides their operands.  It may be loaded, and loaded again, after the graph is built, so
// it is looked at when the graph runs (spf_graph.hpp: one check per resource, in this order), and Plan::has(resource) says
// whether any group needs it.
enum Resource : uint8_t { kNoResource, kPufksKey, kLweSlot, kPolySlot, kGlweKsKeys, kResources };

// A node kind as the planner sees it: where its operands are, what its group key is made of, and how a group reads its operands.
// A group of a rows kind reads *records* of operand rows, one behind the other: every `step`-th member starts a record (its
// operands, in order), the rows are of one size, and they are read in place where they lie consecutively, else through one
// pointer row of the table.
struct NodeRow {
    int32_t op;
    bool listed;                                               // the operands are in the graph's side list, not in Node::in
    enum : uint8_t { kNoKind, kOperandKind, kNodeKind } kind;  // GroupKey::kind: 0, the first operand's kind, or the node's own
    bool slot_rows;                                            // GroupKey::slot and ::rows are Node::lin_slot and ::lin_rows (else 0)
    bool n_is_count;                                           // GroupKey::n is Node::count (else Node::param)
    enum : uint8_t { kTableOp, kUnits, kRows } access;         // an operation of spf_ops.hpp / CMUX units / records of rows
    enum : uint8_t { kEvery, kEveryRows, kEveryN } step;       // rows: a record starts at every member / key.rows-th / key.n-th
    bool glwe_rows;                                            // rows: they are GLWE1s (else of key.kind)
    bool in_place;                                             // rows: consecutive rows are read where they lie
    enum : uint8_t { kNoStage, kStage, kStagePufks } stage;    // rows: scattered rows are gathered into the stage buffer: never,
                                                               // always, or when Sizes::pufks_stage says so
    Resource needs;
};
constexpr NodeRow kNodeRows[] = {
    // {op, listed, kind, slot_rows, n_is_count, access, step, glwe_rows, in_place, stage, needs}
    // one source GLWE per integer (every width-th member; the bit nodes of a call share Node::in[0]): gathered unless consecutive
    {kNodeUnpack, false, NodeRow::kNoKind, false, true, NodeRow::kRows, NodeRow::kEveryN, true, true, NodeRow::kStage, kNoResource},
    // the rows of every pack, where they lie: never in place — glwe_pack_rows_kernel, the one kernel there is for it, reads its rows
    // through the table wherever they are, so consecutive rows go the same way and nothing is gathered
    {kNodePack, true, NodeRow::kNoKind, false, true, NodeRow::kRows, NodeRow::kEvery, true, false, NodeRow::kNoStage, kNoResource},
    // units {selector, accumulator, unused (the high operand is a rotated read of the accumulator), out}; key.n is the rotation
    {kNodeRotCmux, false, NodeRow::kNoKind, false, false, NodeRow::kUnits, NodeRow::kEvery, true, false, NodeRow::kNoStage, kNoResource},
    // the lwe_count rows of every output, output-major: in place when they lie consecutively; else read through the table by the
    // pre-pass of the hand-written radices, or gathered for generic_pufks_kernel
    {kNodePufks, true, NodeRow::kOperandKind, false, true, NodeRow::kRows, NodeRow::kEvery, false, true, NodeRow::kStagePufks, kPufksKey},
    // the K rows of every layer, layer-major (the M nodes of a call share one list): in place when all of them lie consecutively
    // (the batch dispatcher, matrix cores included), else read through the table by lwe_linear_rows_kernel
    {kNodeLweLinear, true, NodeRow::kNodeKind, true, true, NodeRow::kRows, NodeRow::kEveryRows, false, true, NodeRow::kNoStage, kLweSlot},
    // the K GLWEs of every layer, the same way (the node's kind is SPF_VAL_GLWE1): the batch kernels in place, else the rows kernels
    {kNodeGlwePolyLinear, true, NodeRow::kNodeKind, true, true, NodeRow::kRows, NodeRow::kEveryRows, true, true, NodeRow::kNoStage, kPolySlot},
    // one GLWE per member (Node::in[0]): the batch kernels in place, else the rows kernels, which park into the group's output rows
    // while other workgroups still read: those rows are this group's own fresh block (lay_out), its operands rows of earlier
    // levels — disjoint.  key.n is the slot, the round, or 0: the operation is the mode
    {kNodeGlweKeyswitch, false, NodeRow::kNoKind, false, false, NodeRow::kRows, NodeRow::kEvery, true, true, NodeRow::kNoStage, kGlweKsKeys},
    {kNodeGlweAutomorphism, false, NodeRow::kNoKind, false, false, NodeRow::kRows, NodeRow::kEvery, true, true, NodeRow::kNoStage, kGlweKsKeys},
    {kNodeGlweTrace, false, NodeRow::kNoKind, false, false, NodeRow::kRows, NodeRow::kEvery, true, true, NodeRow::kNoStage, kGlweKsKeys},
};
constexpr size_t kNodeRowCount = sizeof kNodeRows / sizeof kNodeRows[0];
// every node that is no constructor's — an operation of the table (spf_ops.hpp), an input, a constant: operands in Node::in, keyed
// by its parameter
constexpr NodeRow kTableOpRow = {-1, false, NodeRow::kNoKind, false, false, NodeRow::kTableOp, NodeRow::kEvery, false, false, NodeRow::kNoStage, kNoResource};
constexpr bool node_rows_in_order(size_t i = 0) { return i == kNodeRowCount || (kNodeRows[i].op == kNodeUnpack + (int32_t)i && node_rows_in_order(i + 1)); }
static_assert(kNodeRowCount == kNodeGlweTrace - kNodeUnpack + 1 && node_rows_in_order(), "one row per constructor kind, in the order of the enum");
inline const NodeRow& node_row(int32_t op) { return op >= kNodeUnpack && op <= kNodeGlweTrace ? kNodeRows[op - kNodeUnpack] : kTableOpRow; }

constexpr size_t kAlign = 256;        // inputs, constants and every group's block start on a multiple of this
constexpr size_t kNull = (size_t)-1;  // a table entry that is no arena offset but a null pointer
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Node {
    int32_t op;        // spf_graph_op, one of the kNode constructors, or -1 input, -2 trivial constant
    int32_t kind;      // spf_value_kind of the value the node produces
    uint64_t param;    // SampleExtract index / MulXN amount / trivial bit / bit index of an unpack node / rotation of a rotate-CMUX node /
                       // row index m of a linear node / keyswitch-key slot of a GLWE keyswitch node / round of an automorphism node
    uint32_t in[3];    // (rotate-CMUX nodes: {selector, accumulator})
    uint32_t n_in;
    uint32_t count;    // unpack nodes: the bit nodes of their call (the integer's width); nodes with an operand list: its length
    uint32_t list_at;  // ... where their list starts (n_in = 0)
    uint32_t lin_slot, lin_rows; // linear and polynomial linear nodes: the weight slot and M (the M nodes of one call share one operand list)
    uint32_t level;
    size_t off;        // byte offset of the value in the arena
    const void* host;  // inputs: caller's buffer, read at every run
};

// The node of an operation of the table (spf_ops.hpp) over `inputs[0 .. arity)`, as spf_graph_add_op records it and as the named
// constructors of the three GLWE keyswitch operations do: Node::op is the row's spf_graph_op — except for those three, whose
// nodes keep the kinds 70 / 71 / 72 of their constructors (the planner groups, places and keys them by that kind: the recorded
// plans do not move).  `pool_op` is a row with a spf_graph_op; the parameter has been through spf_ops::op_param.
inline int32_t node_op_of(int pool_op)
{
    return pool_op == spf_ops::OP_GLWE_KEYSWITCH      ? (int32_t)kNodeGlweKeyswitch
           : pool_op == spf_ops::OP_GLWE_AUTOMORPHISM ? (int32_t)kNodeGlweAutomorphism
           : pool_op == spf_ops::OP_GLWE_TRACE        ? (int32_t)kNodeGlweTrace
                                                      : (int32_t)spf_ops::row(pool_op).graph_op;
}
inline Node op_node(int pool_op, const uint32_t* inputs, uint64_t param)
{
    const spf_ops::OpRow& r = spf_ops::row(pool_op);
    Node n{};
    n.op = node_op_of(pool_op); n.kind = r.out_kind; n.n_in = (uint32_t)r.arity; n.param = param;
    for (int i = 0; i < r.arity; i++) n.in[i] = inputs[i];
    return n;
}

struct Graph {
    std::vector<Node> nodes; // in topological order: operands precede their users

    // f(operand id) for every operand of a node
    template <class F> void for_operands(const Node& n, F f) const
    {
        for (uint32_t i = 0; i < n.n_in; i++) f(n.in[i]);
        if (has_list(n.op))
            for (uint32_t i = 0; i < n.count; i++) f(lists[n.list_at + i]);
    }
    uint32_t operand(const Node& n, size_t i) const { return has_list(n.op) ? lists[n.list_at + i] : n.in[i]; }
    size_t listed_operands() const { return lists.size(); } // (of all nodes together)

    // The three ways a node comes to be; each returns the id of its first node and adds all of its nodes or none (what does not
    // fit is thrown, as std::vector throws it).  One node, operands in n.in:
    uint32_t add(const Node& n)
    {
        nodes.push_back(n);
        return (uint32_t)nodes.size() - 1;
    }
    // `copies` nodes like n, param = 0 .. copies - 1 (the bit nodes of one unpack call)
    uint32_t add_numbered(Node n, size_t copies)
    {
        const uint32_t first = (uint32_t)nodes.size();
        nodes.reserve(nodes.size() + copies);
        for (size_t i = 0; i < copies; i++) {
            n.param = i;
            nodes.push_back(n);
        }
        return first;
    }
    // `copies` numbered nodes over ONE operand list ids[0 .. count)
    uint32_t add_listed(Node n, const uint32_t* ids, size_t count, size_t copies = 1)
    {
        n.n_in = 0;
        n.count = (uint32_t)count;
        n.list_at = (uint32_t)lists.size();
        nodes.reserve(nodes.size() + copies);
        lists.insert(lists.end(), ids, ids + count);
        return add_numbered(n, copies);
    }
    // `other` behind this graph's nodes, every operand id and list position of it shifted; returns the shift of its node ids
    uint32_t append(const Graph& other)
    {
        const uint32_t base = (uint32_t)nodes.size(), list_base = (uint32_t)lists.size();
        nodes.reserve(nodes.size() + other.nodes.size());
        lists.reserve(lists.size() + other.lists.size());
        for (Node n : other.nodes) {
            for (uint32_t i = 0; i < n.n_in; i++) n.in[i] += base;
            if (has_list(n.op)) n.list_at += list_base;
            nodes.push_back(n);
        }
        for (uint32_t in : other.lists) lists.push_back(in + base);
        return base;
    }

private:
    static bool has_list(int32_t op) { return node_row(op).listed; }
    std::vector<uint32_t> lists; // the operand lists of the kinds whose row says `listed`
};

// What the planner needs to know of the parameter set and the context
struct Sizes {
    size_t bytes[SPF_VAL_GLEV1 + 1]; // of one value of each spf_value_kind
    size_t cbs_radix_count;          // GLWEs of a GLEV: a GlevCMux node is that many CMUX units
    bool pufks_stage;                // scattered rows of a public functional keyswitch are gathered (generic_pufks_kernel): they need room
    size_t of(int kind) const { return bytes[kind]; }
};
inline Sizes sizes_of(const spf_params& p, bool pufks_stage)
{
    Sizes s{};
    for (int k = SPF_VAL_LWE0; k <= SPF_VAL_GLEV1; k++) s.bytes[k] = value_bytes(p, k);
    s.cbs_radix_count = p.cbs_radix_count;
    s.pufks_stage = pufks_stage;
    return s;
}

// What the nodes of one launch have in common.  Groups run, and lie in the arena, in the order of their keys: by level, then
// operation, then — public functional keyswitch: (operand kind, lwe_count); linear map and polynomial linear map: (operand kind,
// slot, M, K); unpack and pack: the width; every other operation: its parameter (GLWE keyswitch: the slot, automorphism: the round,
// trace: 0 — the operation is the mode).
struct GroupKey {
    uint32_t level;
    int32_t op;
    uint8_t kind;  // public functional keyswitch and linear groups: spf_value_kind of the operands; else 0
    uint8_t slot;  // linear groups: the weight slot; else 0
    uint16_t rows; // linear groups: M; else 0
    uint64_t n;    // unpack and pack groups: the width; public functional keyswitch groups: lwe_count; linear groups: K; else the parameter
    bool operator<(const GroupKey& o) const
    {
        return std::tie(level, op, kind, slot, rows, n) < std::tie(o.level, o.op, o.kind, o.slot, o.rows, o.n);
    }
    bool operator==(const GroupKey& o) const
    {
        return std::tie(level, op, kind, slot, rows, n) == std::tie(o.level, o.op, o.kind, o.slot, o.rows, o.n);
    }
};
static_assert(SPF_LWE_LINEAR_SLOTS - 1 <= 0xff, "a weight slot does not fit GroupKey::slot");
static_assert(SPF_GRAPH_LWE_LINEAR_MAX_ROWS <= 0xffff, "the rows of a linear node do not fit GroupKey::rows");
static_assert(SPF_GLWE_POLY_SLOTS - 1 <= 0xff, "a polynomial weight slot does not fit GroupKey::slot");
static_assert(SPF_GLWE_POLY_MAX_ROWS <= 0xffff, "the rows of a polynomial linear node do not fit GroupKey::rows");
static_assert(SPF_VAL_GLEV1 <= 0xff, "a value kind does not fit GroupKey::kind");

struct Group {
    GroupKey key;
    std::vector<uint32_t> members; // in node order; their results are consecutive rows from out_off
    size_t out_off = 0;
    // per operand slot: offset of the first operand when the members' operands are contiguous
    // in member order, else index of the slot's pointer row in the table
    bool contiguous[3] = {false, false, false};
    size_t first_off[3] = {0, 0, 0};
    size_t ptr_index[3] = {0, 0, 0};
    bool one_lut = false; // the bootstraps by table: every member names the same table node (read in place, lut_stride = 0)
};

struct Plan {
    std::vector<Group> groups;
    std::vector<size_t> table; // the pointer table as arena offsets (kNull: a null pointer)
    size_t inputs_bytes = 0, arena_bytes = 0, stage_bytes = 0;
    uint32_t n_levels = 0;
    bool has_pufks = false;  // public functional keyswitch nodes: any
    bool has_linear = false; // linear nodes: any (their weight slots are checked at every run)
    bool has_glwe_poly = false; // polynomial linear nodes: any (likewise)
    bool has_glwe_ks = false;   // GLWE keyswitch, automorphism or trace nodes: any (their keys are checked at every run)
    // the flag of a resource (not kNoResource): set by plan_access for every group whose kind needs it
    bool& has(Resource r) { return r == kPufksKey ? has_pufks : r == kLweSlot ? has_linear : r == kPolySlot ? has_glwe_poly : has_glwe_ks; }
    bool has(Resource r) const { return r != kNoResource && const_cast<Plan*>(this)->has(r); }
};

// the table row (spf_ops.hpp) of a node's operation: a spf_graph_op that spf_graph_add_op has accepted
inline const spf_ops::OpRow& op_row(int graph_op) { return spf_ops::row(spf_ops::pool_op_of(graph_op)); }
// CMUX units of one node
inline size_t units_per_node(int32_t op, size_t cbs_radix_count) { return op == SPF_OP_GLEV_CMUX ? cbs_radix_count : 1; }

// Node::level of every node; returns the number of levels
inline uint32_t assign_levels(Graph& g)
{
    uint32_t max_level = 0;
    for (auto& n : g.nodes) {
        uint32_t lv = 0;
        g.for_operands(n, [&](uint32_t in) { lv = std::max(lv, g.nodes[in].level); });
        n.level = n.op < 0 ? 0 : lv + 1;
        max_level = std::max(max_level, n.level);
    }
    // A circuit bootstrap launch costs as much as ~150 CMUX levels whatever its width (up to one ciphertext per CU),
    // and conversions in the middle of a circuit become ready one by one (the 128 partial-product bits of a 32 x 32
    // multiplication at 32 different depths): batch them.  Within the slack that does not lengthen the graph
    // (latest level = min over consumers of their latest level - 1), bootstraps are moved to common levels —
    // repeatedly take the bootstrap that must run soonest and run every bootstrap that is ready by then with it —
    // and the SampleExtract / KeyswitchL1toL0 nodes feeding them follow.  (Nodes are in topological order: operands
    // precede their users.)
    const size_t nn = g.nodes.size();
    std::vector<uint32_t> alap(nn, max_level);
    for (size_t id = nn; id-- > 0;) {
        const auto& n = g.nodes[id];
        if (n.op < 0) continue;
        g.for_operands(n, [&](uint32_t in) {
            if (g.nodes[in].op >= 0) alap[in] = std::min(alap[in], alap[id] - 1);
        });
    }
    // (the bootstraps by table cost the same blind rotation: each of the three kinds is batched among its own)
    std::vector<uint32_t> fixed(nn, 0);
    std::vector<bool> done(nn, false);
    for (const int32_t kind : {(int32_t)SPF_OP_CIRCUIT_BOOTSTRAP, (int32_t)SPF_OP_PBS_UNIVARIATE, (int32_t)SPF_OP_PBS_BIVARIATE}) {
        std::vector<uint32_t> cbs;
        for (uint32_t id = 0; id < nn; id++)
            if (g.nodes[id].op == kind) cbs.push_back(id);
        std::sort(cbs.begin(), cbs.end(), [&](uint32_t a, uint32_t b) { return alap[a] != alap[b] ? alap[a] < alap[b] : a < b; });
        for (uint32_t lead : cbs) {
            if (done[lead]) continue;
            const uint32_t t = alap[lead];
            for (uint32_t id : cbs)
                if (!done[id] && g.nodes[id].level <= t) { done[id] = true; fixed[id] = t; }
        }
    }
    // forward again with the chosen bootstrap levels as lower bounds (t <= latest level: depth unchanged)
    for (size_t id = 0; id < nn; id++) {
        auto& n = g.nodes[id];
        if (n.op < 0) continue;
        uint32_t lv = 0;
        g.for_operands(n, [&](uint32_t in) { lv = std::max(lv, g.nodes[in].level); });
        n.level = std::max(lv + 1, fixed[id]);
    }
    // pull the conversion chain's head (SampleExtract -> KeyswitchL1toL0) up against its bootstrap
    std::vector<uint32_t> min_user(nn, 0xffffffffu);
    for (size_t id = nn; id-- > 0;) {
        auto& n = g.nodes[id];
        if (n.op < 0) continue;
        if ((n.op == SPF_OP_KEYSWITCH_L1_TO_L0 || n.op == SPF_OP_SAMPLE_EXTRACT) && min_user[id] != 0xffffffffu)
            n.level = std::max(n.level, min_user[id] - 1);
        g.for_operands(n, [&](uint32_t in) { min_user[in] = std::min(min_user[in], n.level); });
    }
    return max_level;
}

// the key of a node that has its level
inline GroupKey key_of(const Graph& g, const Node& n)
{
    const NodeRow& r = node_row(n.op);
    return GroupKey{n.level, n.op,
                    (uint8_t)(r.kind == NodeRow::kOperandKind ? g.nodes[g.operand(n, 0)].kind : r.kind == NodeRow::kNodeKind ? n.kind : 0),
                    (uint8_t)(r.slot_rows ? n.lin_slot : 0), (uint16_t)(r.slot_rows ? n.lin_rows : 0), r.n_is_count ? n.count : n.param};
}

// One group per key, members in node order, groups in key order.  Unpack and pack nodes group by their width: the bit
// nodes of one spf_graph_add_unpack call have consecutive ids and one level (their source's + 1; nothing below moves
// them), so a group's members are whole integers, int-major.  Linear nodes group by (operand kind, slot, M, K): the M nodes of
// one spf_graph_add_lwe_linear call have consecutive ids, one operand list and so one level, and nothing above moves them (they
// are no bootstrap and no head of a conversion chain), so a group's members are whole layers, layer-major.  Polynomial linear nodes
// (spf_graph_add_glwe_poly_linear) likewise, by (slot, M, K)
inline std::vector<Group> make_groups(const Graph& g)
{
    std::map<GroupKey, std::vector<uint32_t>> by_key;
    for (uint32_t id = 0; id < g.nodes.size(); id++)
        if (g.nodes[id].op >= 0) by_key[key_of(g, g.nodes[id])].push_back(id);
    std::vector<Group> groups;
    groups.reserve(by_key.size());
    for (auto& kv : by_key) {
        groups.emplace_back();
        groups.back().key = kv.first;
        groups.back().members = std::move(kv.second);
    }
    return groups;
}

// Node::off of every node and Group::out_off: inputs and constants first, packed, so one copy brings them up; then one block
// per group, its members' results consecutive rows
inline void lay_out(Graph& g, const Sizes& sz, Plan& p)
{
    size_t off = 0;
    for (auto& n : g.nodes)
        if (n.op < 0) {
            n.off = off;
            off = align_up(off + sz.of(n.kind), kAlign);
        }
    p.inputs_bytes = off;
    for (auto& gr : p.groups) {
        const size_t ob = sz.of(g.nodes[gr.members[0]].kind);
        gr.out_off = off;
        for (size_t i = 0; i < gr.members.size(); i++) g.nodes[gr.members[i]].off = off + i * ob;
        off = align_up(off + gr.members.size() * ob, kAlign);
    }
    p.arena_bytes = off;
}

// do rows of row_bytes at these offsets lie one behind the other?
inline bool consecutive(const std::vector<size_t>& offs, size_t row_bytes)
{
    for (size_t i = 1; i < offs.size(); i++)
        if (offs[i] != offs[0] + i * row_bytes) return false;
    return true;
}

// Operand slot s of a group reads the rows at `offs`: in place from the first one, or through a new pointer row of the table —
// and, where the launch gathers them first (`staged`), the stage buffers have room for them
inline void read_rows(Plan& p, Group& gr, int s, const std::vector<size_t>& offs, size_t row_bytes, bool in_place, bool staged)
{
    gr.contiguous[s] = in_place;
    if (in_place) {
        gr.first_off[s] = offs[0];
        return;
    }
    gr.ptr_index[s] = p.table.size();
    p.table.insert(p.table.end(), offs.begin(), offs.end());
    if (staged) p.stage_bytes = std::max(p.stage_bytes, offs.size() * row_bytes);
}

// A group of the CMUX family reads its units {selector, low, high, out} through the table.
// Units that select on the same GGSW go next to each other: a level of a mux_circuits block tests ONE
// variable (MuxCircuit::from(&[Bdd]), lib.rs:358-445), so a wide level is a handful of selectors with
// dozens of gates each, and neighbouring workgroups then hit the same 256 KiB in L2 (the streaming kernel
// does 17.3 M gates/s on four units per selector against 12.9 M/s on distinct ones).  Order inside a
// level is free: every unit carries its own output pointer.
struct Unit { size_t p[4]; };
inline void read_units(Plan& p, Group& gr, std::vector<Unit>& units)
{
    gr.ptr_index[0] = p.table.size();
    std::stable_sort(units.begin(), units.end(), [](const Unit& x, const Unit& y) { return x.p[0] < y.p[0]; });
    for (const Unit& u : units) p.table.insert(p.table.end(), u.p, u.p + 4);
}

// operand access per group (after lay_out: needs the offsets)
inline void plan_access(const Graph& g, const Sizes& sz, Plan& p)
{
    const auto off_of = [&](uint32_t id) { return g.nodes[id].off; };
    for (auto& gr : p.groups) {
        const int32_t op = gr.key.op;
        const size_t B = gr.members.size();
        const NodeRow& kind = node_row(op);
        if (kind.needs != kNoResource) p.has(kind.needs) = true;
        if (kind.access == NodeRow::kRows) {
            // the records: the operands of every `step`-th member, one behind the other
            const size_t step = kind.step == NodeRow::kEveryN ? (size_t)gr.key.n : kind.step == NodeRow::kEveryRows ? gr.key.rows : 1;
            std::vector<size_t> offs;
            for (size_t i = 0; i < B; i += step) g.for_operands(g.nodes[gr.members[i]], [&](uint32_t in) { offs.push_back(off_of(in)); });
            const size_t row_bytes = sz.of(kind.glwe_rows ? (int)SPF_VAL_GLWE1 : (int)gr.key.kind);
            read_rows(p, gr, 0, offs, row_bytes, kind.in_place && consecutive(offs, row_bytes),
                      kind.stage == NodeRow::kStage || (kind.stage == NodeRow::kStagePufks && sz.pufks_stage));
        } else if (kind.access == NodeRow::kUnits || op_row(op).cmux_family) {
            // units: a rotate-CMUX node is one (its row), a node of the CMUX family one per GLWE pair, {selector, low (a), high (b), out}
            const bool rot = kind.access == NodeRow::kUnits;
            const size_t per = rot ? 1 : units_per_node(op, sz.cbs_radix_count), gw = sz.of(SPF_VAL_GLWE1);
            std::vector<Unit> units;
            units.reserve(B * per);
            for (uint32_t id : gr.members) {
                const Node& n = g.nodes[id];
                for (size_t j = 0; j < per; j++) {
                    if (rot)
                        units.push_back(Unit{{off_of(n.in[0]), off_of(n.in[1]), kNull, n.off}});
                    else if (op == SPF_OP_MULTIPLY_GGSW_GLWE) // (low: the zero ciphertext)
                        units.push_back(Unit{{off_of(n.in[0]), kNull, off_of(n.in[1]), n.off + j * gw}});
                    else
                        units.push_back(Unit{{off_of(n.in[0]), off_of(n.in[1]) + j * gw, off_of(n.in[2]) + j * gw, n.off + j * gw}});
                }
            }
            read_units(p, gr, units);
        } else {
            // an operation of the table over rows: every slot in place or gathered
            const spf_ops::OpRow& info = op_row(op);
            std::vector<size_t> offs[3];
            bool in_place[3] = {false, false, false};
            for (int s = 0; s < info.arity; s++) {
                for (uint32_t id : gr.members) offs[s].push_back(off_of(g.nodes[id].in[s]));
                in_place[s] = consecutive(offs[s], sz.of(info.in_kind[s]));
            }
            if (op == SPF_OP_PBS_UNIVARIATE || op == SPF_OP_PBS_BIVARIATE) { // one table node for the whole group: read in place with lut_stride = 0 (B = 1 included)
                const int s = info.arity - 1;
                gr.one_lut = true;
                for (size_t i = 1; i < B && gr.one_lut; i++) gr.one_lut = g.nodes[gr.members[i]].in[s] == g.nodes[gr.members[0]].in[s];
                if (gr.one_lut) in_place[s] = true;
            }
            // bivariate inputs: one of them scattered -> both are read through their pointer rows by lwe_pack_rows_kernel, which
            // writes the packed rows into the stage buffer
            if (op == SPF_OP_PBS_BIVARIATE && !(in_place[0] && in_place[1])) in_place[0] = in_place[1] = false;
            for (int s = 0; s < info.arity; s++) read_rows(p, gr, s, offs[s], sz.of(info.in_kind[s]), in_place[s], true);
        }
    }
}

// Levels, groups, arena layout, pointer table: writes Node::level and Node::off, returns the rest
inline Plan plan(Graph& g, const Sizes& sz)
{
    Plan p;
    p.n_levels = assign_levels(g);
    p.groups = make_groups(g);
    lay_out(g, sz, p);
    plan_access(g, sz, p);
    return p;
}

} // namespace spf_graph_plan
