// spf_graph.hpp — level-batching executor for gate graphs.
//
// The reference runs an `FheCircuit` (parasol_runtime/src/fhe_circuit.rs:34-126: a DAG of `FheOp`
// nodes) by spawning one rayon task per node as its operands become ready
// (circuit_processor/mod.rs:130-253) and calling `Evaluation` with ONE ciphertext per task
// (`exec_op`, :255-560).  On a GPU the same DAG is executed by topological level: all nodes of one
// level, one kind and one parameter are a *group* and become one batched launch, every intermediate value stays in HBM, and the
// whole graph is enqueued on one HIP stream without a host round trip — inputs go up in one copy, outputs
// come back at the end.
//
// Operands of a group live wherever their producers wrote them, and a group reads each operand slot in one of two ways.  *In
// place*: the rows lie consecutively in member order (the common KeyswitchL1toL0 -> CircuitBootstrap chain, the results of one
// group feeding the next), and the batch entry point takes the first row's address.  *Through a pointer row* of the graph's
// table: the CMUX family always (`CmuxArgs::ptrs`; a 256 KiB GGSW per gate is not worth copying); a kind that has a rows kernel
// reads the table itself; the small operands of the others are packed into a stage buffer by `gather_rows_kernel` first.
//
// A node is a row of the operation table (spf_ops.hpp: the `FheOp`s and the bootstraps by a caller's table) or comes from one of
// the nine node constructors, which are no `FheOp` in the reference and no spf_graph_op here: each stands for a composition that
// would cost more levels and launches, because a level is batched by parameter.  What the planner knows of a constructor kind
// is its row in spf_graph_plan.hpp's kNodeRows; what the executor knows is its launcher below (kNodeLaunchers, indexed like the
// rows) and, where its groups need something that is loaded into the context, the check of that resource (kResourceChecks).  A
// resource is read when the graph runs: it may be loaded, and loaded again, after the graph is built.  Each kind's particulars
// — what it computes, its reference, its kernels — stand at its launcher and at its constructor.
//
// The bootstraps by a caller's table (SPF_OP_PBS_UNIVARIATE / SPF_OP_PBS_BIVARIATE: `programmable_bootstrap_univariate` / `_bivariate`,
// programmable_bootstrapping.rs:291, 575-621) are rows of the operation table whose LAST operand is the table, a GLWE1 node.  A group
// whose members all name one table node launches with lut_stride = 0 and copies nothing; otherwise the tables are gathered like any
// operand.  Bivariate inputs that do not lie consecutively are packed straight from where they lie (lwe_pack_rows_kernel: one launch
// where two gathers and lwe_pack_kernel were three).  The slack rule (spf_graph_plan.hpp) batches each of the two kinds as it batches the circuit
// bootstraps.
//
// What is decided before a device is touched — levels, groups and their order, arena offsets, in place or through a pointer row,
// the order of the CMUX units, the size of the stage buffers — is spf_graph_plan.hpp's, free of HIP and checked on the CPU; here
// are the handle, the node constructors with their checks, the device memory of a plan and the launches.
//
// Included at the end of spf_hip.hip: uses its `fail` / HIPCHK helpers and the `_dev` entry points.
#pragma once

#include "spf_graph_plan.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

// host memory the copy engines can reach directly (hipHostMalloc): a copy to or from pageable memory is staged by the runtime
// through its own pinned bounce buffer, synchronously, ~20 us per call — 33 of them were 0.68 of a 32-bit addition's 5.5 ms
struct spf_pinned_buf {
    uint8_t* p = nullptr;
    size_t n = 0;
    bool pinned = false;
    uint8_t* data() const { return p; }
    bool resize(size_t bytes)
    {
        if (p) { if (pinned) (void)hipHostFree(p); else std::free(p); }
        p = nullptr;
        n = 0;
        if (!bytes) return true;
        pinned = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) == hipSuccess;
        if (!pinned) { // (no pinned memory left for a very large graph: pageable still works, the copies are just staged by the runtime)
            (void)hipGetLastError();
            p = static_cast<uint8_t*>(std::malloc(bytes));
            if (!p) return false;
        }
        std::memset(p, 0, bytes);
        n = bytes;
        return true;
    }
    void free_buf() { (void)resize(0); }
};

// the nodes (spf_graph_plan::Graph) and, once planned, their plan (spf_graph_plan::Plan) with its device memory
struct spf_graph : spf_graph_plan::Graph, spf_graph_plan::Plan {
    spf_live::Tick<spf_live::GRAPH> live;
    spf_ctx* ctx = nullptr;
    spf_params prm{};
    struct spf_group* grp = nullptr; // a graph of a device group (spf_group_graph_create): placed on a member when it is run
    int member = -1;                 // ... the member its most recent run took place on
    std::vector<std::pair<uint32_t, void*>> outputs;
    bool planned = false;
    spf_pinned_buf h_inputs;
    // outputs leave in ONE device-to-host copy: gathered on the device (one gather_rows launch per value size) into d_out_stage,
    // copied into pinned h_out_stage, handed to the callers' buffers from there
    struct OutClass { size_t words = 0, count = 0, ptr_index = 0, stage_off = 0; std::vector<size_t> which; };
    std::vector<OutClass> out_classes;
    spf_pinned_buf h_out_stage;
    char* d_out_stage = nullptr;
    void** d_out_ptrs = nullptr;
    size_t out_bytes = 0, outputs_planned = (size_t)-1;
    void release_outputs()
    {
        if (d_out_stage) (void)hipFree(d_out_stage);
        if (d_out_ptrs) (void)hipFree(d_out_ptrs);
        d_out_stage = nullptr;
        d_out_ptrs = nullptr;
        h_out_stage.free_buf();
        out_classes.clear();
        outputs_planned = (size_t)-1;
    }
    bool pufks_stage = false; // planned with room to gather the rows of the public functional keyswitch nodes
    char* d_arena = nullptr;
    char* d_stage[2] = {nullptr, nullptr};
    void** d_ptrs = nullptr; // the plan's table, the arena's base added
    uint32_t n_launches = 0;
    // hipGraph of the planned launch sequence (everything between the input copy and the output copies; opt-in,
    // SPF_GRAPH_CAPTURE=1): captured on the second run after planning (the first one sizes the context's scratch buffers),
    // replayed afterwards; dropped when the graph is re-planned or a captured scratch buffer moved
    hipGraphExec_t exec = nullptr;
    uint64_t exec_epoch = 0;
    uint64_t exec_res_epoch[spf_graph_plan::kResources] = {}; // per resource: the context's count of its loads at the capture (kResourceEpochs)
    uint32_t runs_since_plan = 0, captured_launches = 0;

    void drop_exec()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
    void release()
    {
        drop_exec();
        release_outputs();
        runs_since_plan = 0;
        if (d_arena) (void)hipFree(d_arena);
        if (d_stage[0]) (void)hipFree(d_stage[0]);
        if (d_stage[1]) (void)hipFree(d_stage[1]);
        if (d_ptrs) (void)hipFree(d_ptrs);
        d_arena = d_stage[0] = d_stage[1] = nullptr;
        d_ptrs = nullptr;
        planned = false;
    }
};

namespace spf_graph_impl {

using namespace spf_graph_plan; // (the node kinds and their rows, op_row, align_up, units_per_node)

// The plan of spf_graph_plan.hpp and its device memory.  Called by the first run after the graph changed.
inline spf_status plan(spf_graph* g)
{
    spf_ctx* c = g->ctx;
    g->release();
    HIPCHK(c, hipSetDevice(c->device));
    g->pufks_stage = !pufks_tuned(c) || pufks_rows_gather(); // (also while no key is loaded: the key that comes may be of any radix)
    static_cast<Plan&>(*g) = spf_graph_plan::plan(*g, sizes_of(g->prm, g->pufks_stage));
    HIPCHK(c, hipMalloc((void**)&g->d_arena, std::max<size_t>(g->arena_bytes, 256)));
    if (g->stage_bytes) {
        HIPCHK(c, hipMalloc((void**)&g->d_stage[0], g->stage_bytes));
        HIPCHK(c, hipMalloc((void**)&g->d_stage[1], g->stage_bytes));
    }
    if (!g->table.empty()) {
        // offsets become addresses where they stand (a table of the four-multiplication graph is 16 MB: no second copy of it)
        static_assert(sizeof(size_t) == sizeof(void*), "the table is converted in place");
        for (size_t& t : g->table) t = t == kNull ? 0 : reinterpret_cast<size_t>(g->d_arena + t);
        HIPCHK(c, hipMalloc((void**)&g->d_ptrs, g->table.size() * sizeof(void*)));
        HIPCHK(c, hipMemcpy(g->d_ptrs, g->table.data(), g->table.size() * sizeof(void*), hipMemcpyHostToDevice));
        std::vector<size_t>().swap(g->table); // (it lives on the device from here)
    }
    if (getenv("SPF_GRAPH_WIDTHS")) { // diagnostic: CMUX-family launch widths (units) of the plan
        std::map<size_t, size_t> hist;
        for (auto& gr : g->groups)
            if (gr.key.op < kNodeUnpack && op_row(gr.key.op).cmux_family) hist[gr.members.size() * units_per_node(gr.key.op, g->prm.cbs_radix_count)]++;
        for (auto& kv : hist) fprintf(stderr, "[graph widths] %zu units x %zu launches\n", kv.first, kv.second);
    }
    if (!g->h_inputs.resize(g->inputs_bytes)) return fail(c, SPF_ERR_HIP, "graph: out of host memory for the inputs");
    g->planned = true;
    return SPF_OK;
}

// ---- the constructor kinds: one launcher each, indexed like spf_graph_plan::kNodeRows ----------------------------------------------

// A group of a constructor kind, resolved: its width, its output block, and operand slot 0 both ways — the first row in place
// (meaningful when gr.contiguous[0]) and the pointer row of the table (when not)
struct GroupLaunch {
    spf_graph* g; spf_ctx* c; hipStream_t s;
    const Group& gr;
    size_t B; uint64_t* out;
    const uint64_t* in; const uint64_t* const* rows;
    spf_status launched(spf_status st) const // the status of a kind's one launch, counted when it was made
    {
        if (st == SPF_OK) g->n_launches++;
        return st;
    }
};

// Packed integers enter and leave a graph as `PackedGenericInt::graph_input(..).unpack(..)` and `.pack(..).collect_output(..)` do in
// the reference's fluent layer (fluent/packed_dynamic_generic_int_graph_node.rs:24-60,
// fluent/dynamic_generic_int_graph_nodes.rs:139-200).  Composed from SampleExtract(i) / MulXN(i) / GlweAdd nodes, one 32-bit
// integer costs 32 + 31 launches and five more levels.  Unpack: the n_bits LWEs of all integers of a level in ONE
// glwe_unpack_l1_kernel launch, behind a gather of the source GLWEs where they do not lie consecutively
inline spf_status launch_unpack_group(const GroupLaunch& l)
{
    const size_t ints = l.B / l.gr.key.n;
    const uint64_t* src = l.in;
    if (!l.gr.contiguous[0]) {
        src = (const uint64_t*)l.g->d_stage[0];
        const spf_status st = l.launched(spf_gather_rows_dev(l.c, l.s, ints, value_bytes(l.g->prm, SPF_VAL_GLWE1) / 8, l.rows, (uint64_t*)l.g->d_stage[0]));
        if (st != SPF_OK) return st;
    }
    return l.launched(launch_glwe_unpack(l.c, l.s, ints, l.gr.key.n, src, l.out));
}

// ... pack: the rows of all packs of a level summed in ONE glwe_pack_rows_kernel launch that reads them where they lie — always
// through the table: the kernel has no other form
inline spf_status launch_pack_group(const GroupLaunch& l)
{
    return l.launched(launch_glwe_pack_rows(l.c, l.s, l.B, l.gr.key.n, l.rows, l.out));
}

// One bit of a blind rotation by an encrypted shift (`blind_rotation`, blind_rotation.rs:202-223): acc' = cmux(bit, acc, X^-r * acc),
// whose high operand is a rotated read of the low one — composed from MulXN(2N - r) + CMux nodes the same words cost two levels
// and two launches per bit.  All such nodes of one level and one rotation are ONE launch over the units of the table
// (launch_cmux_rot_scattered), each writing its own row
inline spf_status launch_rot_cmux_group(const GroupLaunch& l)
{
    return l.launched(launch_cmux_rot_scattered(l.c, l.s, l.B, (uint32_t)l.gr.key.n, (const void* const*)l.rows));
}

// The public functional keyswitch (`public_functional_keyswitch`, public_functional_keyswitch.rs:74-148, message j to coefficient
// j) packs lwe_count LWE nodes of one kind, from anywhere, into ONE GLWE1 node — what brings the LWEs out of a bootstrap or a
// sample extract back into a packed integer or into CMUX-land.  All such nodes of one level with one (lwe_count, kind) are one
// main launch: launch_pufks_rows (which counts its own launches), or the contiguous entry point where the rows lie consecutively
// (the hand-written radices: a pre-pass and the main kernel)
inline spf_status launch_pufks_group(const GroupLaunch& l)
{
    const size_t p = (size_t)l.gr.key.n;
    if (!l.gr.contiguous[0])
        return launch_pufks_rows(l.c, l.s, l.B, p, l.rows, l.g->pufks_stage ? (uint64_t*)l.g->d_stage[0] : nullptr, l.out, &l.g->n_launches);
    l.g->n_launches += pufks_tuned(l.c) ? 2 : 1;
    return spf_public_functional_keyswitch_enqueue(l.c, l.s, l.B, p, l.in, l.out);
}

// A plaintext linear map over LWE ciphertexts (spf_lwe_linear.hpp): the M rows of weight slot `slot` times K LWE nodes of one kind,
// from anywhere — what stands between two bootstraps by table (a layer, then its activation).  All layers of one level with one
// (slot, M, K, kind) are one group whose output is [layers][M][W]; operand rows that lie consecutively (the results of one
// bootstrap or keyswitch group, or of another layer) go to the batch dispatcher in place, matrix cores included (it says how
// many launches it took), anything else is ONE launch of lwe_linear_rows_kernel over a pointer row
inline spf_status launch_lwe_linear_group(const GroupLaunch& l)
{
    const size_t layers = l.B / l.gr.key.rows;
    const spf_value_kind kind = (spf_value_kind)l.gr.key.kind;
    if (l.gr.contiguous[0]) {
        const spf_status st = spf_lwe_linear_enqueue(l.c, l.s, l.gr.key.slot, kind, layers, l.in, l.out);
        l.g->n_launches += l.c->last_lin_launches;
        return st;
    }
    l.g->n_launches++;
    return launch_lwe_linear_rows(l.c, l.s, l.gr.key.slot, kind, layers, l.rows, l.out);
}

// A plaintext polynomial linear map over GLWE ciphertexts (spf_glwe_poly.hpp), the same way: the M rows of polynomial weight slot
// `slot` times K GLWE1 nodes from anywhere — a packed integer shifted and added to another one before it is unpacked, a lookup
// table that is a plaintext polynomial times an encrypted GLWE.  All layers of one level with one (slot, M, K) are one group
// whose output is [layers][M][(k+1) N]; operand GLWEs that lie consecutively go to the batch kernels in place, anything else is
// ONE launch of glwe_poly_lds_rows_kernel or glwe_poly_stream_rows_kernel over a pointer row
inline spf_status launch_glwe_poly_group(const GroupLaunch& l)
{
    const size_t layers = l.B / l.gr.key.rows;
    return l.launched(l.gr.contiguous[0] ? spf_glwe_poly_linear_enqueue(l.c, l.s, l.gr.key.slot, layers, l.in, l.out)
                                         : launch_glwe_poly_rows(l.c, l.s, l.gr.key.slot, layers, l.g->d_arena, l.rows, l.out));
}

// GlweKsMode (spf_glwe_keyswitch.hpp) of a GLWE keyswitch, automorphism or trace node
inline int glwe_ks_mode_of(int32_t op)
{
    return op == kNodeGlweKeyswitch ? GLWE_KS_KEYSWITCH : op == kNodeGlweAutomorphism ? GLWE_KS_AUTOMORPHISM : GLWE_KS_TRACE;
}

// The GLWE keyswitch, one automorphism round and the homomorphic trace (spf_glwe_keyswitch.hpp) over ONE GLWE1 node from anywhere —
// a packed integer that changes its key, a GLWE traced behind an X^-j polynomial map to isolate one coefficient.  All nodes of one
// level with one mode and one slot (or round; key.n) are one group and ONE launch: operands that lie consecutively go to
// glwe_ks_kernel / generic_glwe_ks_kernel in place, anything else to their rows twins over a pointer row.  The rows kernels park
// into the output while other workgroups still read, so the output block must overlap no operand: operands are rows of earlier
// levels (or inputs), and a group's output is a fresh block of its own level (spf_graph_plan::lay_out).  The automorphism key is
// the context's, rewritten in place by a load, so a captured graph is kept over its reload as with circuit bootstrap nodes
inline spf_status launch_glwe_ks_group(const GroupLaunch& l)
{
    const int mode = glwe_ks_mode_of(l.gr.key.op);
    return l.launched(l.gr.contiguous[0] ? glwe_ks_enqueue(l.c, l.s, mode, (uint32_t)l.gr.key.n, l.B, l.in, l.out)
                                         : launch_glwe_ks_rows(l.c, l.s, mode, (uint32_t)l.gr.key.n, l.B, l.rows, l.out));
}

using GroupLauncher = spf_status (*)(const GroupLaunch&);
constexpr GroupLauncher kNodeLaunchers[] = {launch_unpack_group,     launch_pack_group,      launch_rot_cmux_group,
                                            launch_pufks_group,      launch_lwe_linear_group, launch_glwe_poly_group,
                                            launch_glwe_ks_group,    launch_glwe_ks_group,   launch_glwe_ks_group};
static_assert(sizeof kNodeLaunchers / sizeof kNodeLaunchers[0] == kNodeRowCount, "one launcher per row of kNodeRows, in its order");

// ---- what the groups need at run time: one check per spf_graph_plan::Resource, against a group's key ---------------------------------

// the public functional keyswitch key comes with its own shape
inline spf_status check_pufks_key(spf_graph* g, const GroupKey& key)
{
    spf_ctx* c = g->ctx;
    if (!c->pufks_ready) return fail(c, SPF_ERR_NO_KEY, "graph: public functional keyswitch key not loaded");
    const size_t dim = value_bytes(g->prm, key.kind) / 8 - 1;
    if (c->pufks_n != dim)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "graph: the public functional keyswitch key's from_dimension " + std::to_string(c->pufks_n) +
                                                     " is not the dimension " + std::to_string(dim) + " of its " +
                                                     (key.kind == SPF_VAL_LWE0 ? "lwe0" : "lwe1") + " operands");
    return SPF_OK;
}

// the shape of a weight slot against the (M, K) its nodes were built for; `poly`: " polynomial" or ""
template <class Slot> inline spf_status check_weight_slot(spf_ctx* c, const Slot& l, const GroupKey& key, const std::string& poly)
{
    const size_t K = (size_t)key.n, M = key.rows;
    const std::string slot = std::to_string(key.slot);
    if (!l.ready) return fail(c, SPF_ERR_NO_KEY, "graph: no" + poly + " weights loaded in slot " + slot);
    if (l.M != M || l.K != K)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "graph: slot " + slot + " holds " + std::to_string(l.M) + " x " + std::to_string(l.K) + poly +
                                                     " weights, its" + poly + " linear nodes were built for " + std::to_string(M) + " x " +
                                                     std::to_string(K));
    return SPF_OK;
}
inline spf_status check_lwe_slot(spf_graph* g, const GroupKey& key) { return check_weight_slot(g->ctx, g->ctx->lin[key.slot], key, ""); }
inline spf_status check_poly_slot(spf_graph* g, const GroupKey& key) { return check_weight_slot(g->ctx, g->ctx->gpoly[key.slot], key, " polynomial"); }

// an empty keyswitch-key slot or a missing automorphism key is SPF_ERR_NO_KEY, a tr_radix no kernel serves SPF_ERR_UNSUPPORTED, with
// the texts of the batch entry points (glwe_ks_args)
inline spf_status check_glwe_ks_keys(spf_graph* g, const GroupKey& key)
{
    return glwe_ks_args(g->ctx, glwe_ks_mode_of(key.op), (uint32_t)key.n, 0, nullptr, nullptr);
}

using ResourceCheck = spf_status (*)(spf_graph*, const GroupKey&);
constexpr ResourceCheck kResourceChecks[kResources] = {nullptr, check_pufks_key, check_lwe_slot, check_poly_slot, check_glwe_ks_keys};
// the context's count of loads of a resource: a load frees the old image (a keyswitch-key slot may change its kernel too), so a
// captured graph that holds its pointers is dropped when the count has moved.  (None for the public functional keyswitch key)
constexpr uint64_t spf_ctx::* kResourceEpochs[kResources] = {nullptr, nullptr, &spf_ctx::lin_epoch, &spf_ctx::gpoly_epoch, &spf_ctx::gksk_epoch};

// resource `r` against every group that needs it, in group order
inline spf_status check_resource(spf_graph* g, Resource r)
{
    if (!g->has(r)) return SPF_OK;
    for (const auto& gr : g->groups)
        if (node_row(gr.key.op).needs == r) {
            const spf_status st = kResourceChecks[r](g, gr.key);
            if (st != SPF_OK) return st;
        }
    return SPF_OK;
}

// Everything a run puts on the stream between the input copy and the output copies: the GGSW constants
// (device to device) and one launch per group.  No allocation, no synchronisation: capturable.
inline spf_status enqueue(spf_graph* g, hipStream_t s)
{
    spf_ctx* c = g->ctx;
    for (const auto& n : g->nodes)
        if (n.op == -2 && n.kind == SPF_VAL_GGSW1) {
            const size_t sw = value_bytes(g->prm, SPF_VAL_GGSW1);
            HIPCHK(c, hipMemcpyAsync(g->d_arena + n.off, (const char*)c->d_ggsw_const + (size_t)(n.param & 1) * sw, sw,
                                     hipMemcpyDeviceToDevice, s));
        }
    g->n_launches = 0;
    // The public functional keyswitch key is checked here, before anything is enqueued — and so, unlike the resources run() checks,
    // not before the replay of a captured graph.  Kept where it was: checking it in run() would change what a replay answers.
    if (spf_status st = check_resource(g, kPufksKey)) return st;
    for (const auto& gr : g->groups) {
        const size_t B = gr.members.size();
        char* out = g->d_arena + gr.out_off;
        const NodeRow& kind = node_row(gr.key.op);
        if (kind.access != NodeRow::kTableOp) { // a constructor kind: the launcher of its row
            const spf_status st = kNodeLaunchers[&kind - kNodeRows](GroupLaunch{g, c, s, gr, B, (uint64_t*)out, (const uint64_t*)(g->d_arena + gr.first_off[0]),
                                                                                (const uint64_t* const*)(g->d_ptrs + gr.ptr_index[0])});
            if (st != SPF_OK) return st;
            continue;
        }
        const spf_ops::OpRow& info = op_row(gr.key.op);
        if (info.cmux_family) {
            spf_status st = spf_cmux_scattered_dev(c, s, B * units_per_node(gr.key.op, g->prm.cbs_radix_count), (const void* const*)(g->d_ptrs + gr.ptr_index[0]));
            if (st != SPF_OK) return st;
            g->n_launches++;
            continue;
        }
        const void* in[3] = {nullptr, nullptr, nullptr};
        // (stage buffers: the table of a bootstrap by table goes to the second one, its LWE rows — gathered, or packed from where
        // they lie — to the first)
        const bool pack_rows = gr.key.op == SPF_OP_PBS_BIVARIATE && !gr.contiguous[0];
        if (pack_rows) {
            spf_status st = launch_lwe_pack_rows(c, s, B, (const uint64_t* const*)(g->d_ptrs + gr.ptr_index[0]),
                                                 (const uint64_t* const*)(g->d_ptrs + gr.ptr_index[1]), (uint32_t)gr.key.n, (uint64_t*)g->d_stage[0]);
            if (st != SPF_OK) return st;
            g->n_launches++;
            const void* lut = g->d_arena + gr.first_off[2];
            if (!gr.contiguous[2]) {
                st = spf_gather_rows_dev(c, s, B, value_bytes(g->prm, SPF_VAL_GLWE1) / 8, (const uint64_t* const*)(g->d_ptrs + gr.ptr_index[2]),
                                         (uint64_t*)g->d_stage[1]);
                if (st != SPF_OK) return st;
                g->n_launches++;
                lut = g->d_stage[1];
            }
            st = spf_pbs_univariate_dev(c, s, B, (const uint64_t*)g->d_stage[0], (const uint64_t*)lut, gr.one_lut ? 0 : value_bytes(g->prm, SPF_VAL_GLWE1) / 8,
                                        (uint64_t*)out);
            if (st != SPF_OK) return st;
            g->n_launches++;
            continue;
        }
        for (int sl = 0; sl < info.arity; sl++) {
            char* stage_sl = g->d_stage[sl == info.arity - 1 && sl > 0 ? 1 : sl];
            if (gr.contiguous[sl]) {
                in[sl] = g->d_arena + gr.first_off[sl];
            } else {
                spf_status st = spf_gather_rows_dev(c, s, B, value_bytes(g->prm, info.in_kind[sl]) / 8,
                                                    (const uint64_t* const*)(g->d_ptrs + gr.ptr_index[sl]),
                                                    (uint64_t*)stage_sl);
                if (st != SPF_OK) return st;
                g->n_launches++;
                in[sl] = stage_sl;
            }
        }
        const spf_status st = spf_ops::launch_op(c, s, info.op, B, in, out, gr.key.n, nullptr, 0, nullptr, gr.one_lut);
        if (st != SPF_OK) return st;
        g->n_launches += gr.key.op == SPF_OP_PBS_BIVARIATE ? 2 : 1; // (contiguous bivariate inputs: lwe_pack_kernel, then the bootstrap)
    }
    return SPF_OK;
}

// Output staging (after plan(): needs the arena offsets): outputs grouped by value size, one pointer row per group
inline spf_status plan_outputs(spf_graph* g)
{
    spf_ctx* c = g->ctx;
    g->release_outputs();
    std::map<size_t, spf_graph::OutClass> by_words;
    for (size_t i = 0; i < g->outputs.size(); i++) {
        const auto& n = g->nodes[g->outputs[i].first];
        auto& oc = by_words[value_bytes(g->prm, n.kind) / 8];
        oc.words = value_bytes(g->prm, n.kind) / 8;
        oc.which.push_back(i);
    }
    std::vector<void*> table;
    size_t off = 0;
    for (auto& kv : by_words) {
        auto& oc = kv.second;
        oc.count = oc.which.size();
        oc.ptr_index = table.size();
        oc.stage_off = off;
        for (size_t i : oc.which) table.push_back(g->d_arena + g->nodes[g->outputs[i].first].off);
        off = align_up(off + oc.count * oc.words * 8, 256);
        g->out_classes.push_back(oc);
    }
    g->out_bytes = off;
    if (off) {
        HIPCHK(c, hipMalloc((void**)&g->d_out_stage, off));
        HIPCHK(c, hipMalloc((void**)&g->d_out_ptrs, table.size() * sizeof(void*)));
        HIPCHK(c, hipMemcpy(g->d_out_ptrs, table.data(), table.size() * sizeof(void*), hipMemcpyHostToDevice));
        if (!g->h_out_stage.resize(off)) return fail(c, SPF_ERR_HIP, "graph: out of host memory for the outputs");
    }
    g->outputs_planned = g->outputs.size();
    return SPF_OK;
}

inline spf_status run(spf_graph* g)
{
    spf_ctx* c = g->ctx;
    // one graph at a time per context: the _dev calls below share the context's scratch buffers and
    // stream, and a run must not interleave its launches with another run's
    std::lock_guard<std::recursive_mutex> whole(c->mu);
    // (planned under a key of a hand-written radix, run under one that goes to generic_pufks_kernel: that one gathers its rows)
    if (g->planned && g->has_pufks && !g->pufks_stage && (!pufks_tuned(c) || pufks_rows_gather())) g->planned = false;
    if (!g->planned) {
        spf_status st = plan(g);
        if (st != SPF_OK) return st;
    }
    // what the groups need, resource by resource, before anything is enqueued and before the replay of a captured graph as well
    // (the public functional keyswitch key: by enqueue)
    for (int r = kLweSlot; r < kResources; r++)
        if (spf_status st = check_resource(g, (Resource)r)) return st;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t k = g->prm.glwe_size, N = g->prm.polynomial_degree;
    // inputs: read the callers' buffers now (they may have changed since the last run)
    for (const auto& n : g->nodes) {
        if (n.op == -1) {
            std::memcpy(g->h_inputs.data() + n.off, n.host, value_bytes(g->prm, n.kind));
        } else if (n.op == -2 && n.kind == SPF_VAL_GLEV1) {
            // trivial_glev_l1_{zero,one} (crypto/encryption.rs:434-451 -> trivially_encrypt_glev_ciphertext,
            // ops/encryption/glev_encryption.rs:23-80): GLWE j = zero mask, body = bit * q / B^(j+1) at coefficient 0
            uint64_t* v = reinterpret_cast<uint64_t*>(g->h_inputs.data() + n.off);
            std::memset(v, 0, value_bytes(g->prm, n.kind));
            for (size_t j = 0; j < g->prm.cbs_radix_count; j++)
                v[j * (k + 1) * N + k * N] = (n.param & 1) << (64 - g->prm.cbs_radix_log * (j + 1));
        } else if (n.op == -2 && n.kind != SPF_VAL_GGSW1) {
            // trivial_lwe / trivial_glwe of a bit at one plaintext bit (crypto/encryption.rs:345-412):
            // zero mask, body (coefficient 0) = bit << 63
            uint64_t* v = reinterpret_cast<uint64_t*>(g->h_inputs.data() + n.off);
            std::memset(v, 0, value_bytes(g->prm, n.kind));
            const size_t body = n.kind == SPF_VAL_LWE0 ? g->prm.lwe_dimension : k * N;
            v[body] = (n.param & 1) << 63;
        }
    }
    if (g->inputs_bytes) HIPCHK(c, hipMemcpyAsync(g->d_arena, g->h_inputs.data(), g->inputs_bytes, hipMemcpyHostToDevice, s));
    bool has_ggsw_const = false;
    for (const auto& n : g->nodes) has_ggsw_const = has_ggsw_const || (n.op == -2 && n.kind == SPF_VAL_GGSW1);
    if (has_ggsw_const) { // built (and synchronised) outside any capture
        spf_status st = ensure_ggsw_constants(c);
        if (st != SPF_OK) return st;
    }
    // Off unless SPF_GRAPH_CAPTURE=1: measured on MI355X / ROCm 7.2 the replay is SLOWER than enqueueing the ~100
    // launches (32-bit addition 8.00 ms replayed vs 7.67 ms eager; 16 additions 24.8 vs 24.1 ms) — the launches
    // are already back to back on one stream and hipGraphLaunch adds more than it removes.  (r05 re-measured: 5.11 ms either way
    // for the addition, 42.6 against 43.0 ms for four 32 x 32 multiplications: still opt-in.)
    static const bool capture_on = [] { const char* e = getenv("SPF_GRAPH_CAPTURE"); return e && e[0] == '1'; }();
    g->runs_since_plan++;
    if (g->exec && g->exec_epoch != c->buf_epoch) g->drop_exec(); // a scratch buffer moved since the capture
    for (int r = 0; r < kResources; r++) // a resource of its groups was loaded again since the capture (not one of another graph's)
        if (g->exec && kResourceEpochs[r] && g->has((Resource)r) && g->exec_res_epoch[r] != c->*kResourceEpochs[r]) g->drop_exec();
    if (g->exec) {
        HIPCHK(c, hipGraphLaunch(g->exec, s));
        g->n_launches = g->captured_launches;
    } else {
        const bool capture = capture_on && !c->timing && g->runs_since_plan >= 2;
        const uint64_t epoch0 = c->buf_epoch;
        if (capture) HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        spf_status st = enqueue(g, s);
        if (capture) {
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamEndCapture(s, &graph);
            if (st == SPF_OK && e == hipSuccess && graph && epoch0 == c->buf_epoch &&
                hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                g->exec_epoch = c->buf_epoch;
                for (int r = 0; r < kResources; r++)
                    if (kResourceEpochs[r]) g->exec_res_epoch[r] = c->*kResourceEpochs[r];
                g->captured_launches = g->n_launches;
            } else {
                g->exec = nullptr;
            }
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            if (st != SPF_OK) return st;
            if (g->exec) HIPCHK(c, hipGraphLaunch(g->exec, s));
            else {                       // the capture did not take (a buffer grew, ...): run it plainly this time
                st = enqueue(g, s);
                if (st != SPF_OK) return st;
            }
        } else if (st != SPF_OK) return st;
    }
    if (g->outputs_planned != g->outputs.size()) {
        spf_status st = plan_outputs(g);
        if (st != SPF_OK) return st;
    }
    for (const auto& oc : g->out_classes) {
        spf_status st = spf_gather_rows_dev(c, s, oc.count, oc.words, (const uint64_t* const*)(g->d_out_ptrs + oc.ptr_index),
                                            (uint64_t*)(g->d_out_stage + oc.stage_off));
        if (st != SPF_OK) return st;
    }
    if (g->out_bytes) HIPCHK(c, hipMemcpyAsync(g->h_out_stage.data(), g->d_out_stage, g->out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (const auto& oc : g->out_classes)
        for (size_t i = 0; i < oc.count; i++)
            std::memcpy(g->outputs[oc.which[i]].second, g->h_out_stage.data() + oc.stage_off + i * oc.words * 8, oc.words * 8);
    return SPF_OK;
}

} // namespace spf_graph_impl

static spf_status group_run_graphs(struct spf_group* grp, spf_graph* const* graphs, size_t n); // spf_group.hpp
static void group_forget_graph(struct spf_group* grp, spf_graph* graph);
static void group_release(struct spf_group* grp);

spf_status spf_graph_create(spf_ctx* c, spf_graph** out)
{
    if (!c || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    spf_graph* g = new (std::nothrow) spf_graph();
    if (!g) return fail(c, SPF_ERR_HIP, "out of host memory");
    g->ctx = c;
    g->prm = c->prm;
    ctx_retain(c); // (the graph's device memory is the context's device's, its launches the context's stream's)
    *out = g;
    return SPF_OK;
}

void spf_graph_destroy(spf_graph* g)
{
    if (!g) return;
    spf_ctx* c = g->ctx;
    struct spf_group* grp = g->grp;
    if (grp) group_forget_graph(grp, g); // (a merged graph of the group may still read this job's buffers)
    (void)hipSetDevice(c->device);
    g->release();
    g->h_inputs.free_buf();
    delete g;
    ctx_release(c);
    if (grp) group_release(grp); // (a job holds its group: the last one out, after spf_group_destroy, takes the group down)
}

spf_status spf_graph_add_input(spf_graph* g, spf_value_kind kind, const void* host, uint32_t* node)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!host || !node || value_bytes(g->prm, kind) == 0) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph input: bad kind or null pointer");
    spf_graph_plan::Node n{};
    n.op = -1; n.kind = kind; n.host = host;
    *node = g->add(n);
    g->planned = false;
    return SPF_OK;
}

spf_status spf_graph_add_trivial(spf_graph* g, spf_value_kind kind, uint64_t bit, uint32_t* node)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!node || value_bytes(g->prm, kind) == 0 || bit > 1)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph constant: LWE0 / LWE1 / GLWE1 / GGSW1 / GLEV1 of bit 0 or 1");
    spf_graph_plan::Node n{};
    n.op = -2; n.kind = kind; n.param = bit;
    *node = g->add(n);
    g->planned = false;
    return SPF_OK;
}

static spf_status graph_add_glwe_ks(spf_graph* g, int32_t op, const char* what, uint32_t param, uint32_t glwe_node, uint32_t* node_out);

// Validation happens here, before anything runs, as the reference's graph-level `RuntimeError`s do
// (task.rs:26-31): wrong arity or operand type is an error of the call, not of the run.
spf_status spf_graph_add_op(spf_graph* g, spf_graph_op op, const uint32_t* inputs, size_t n_inputs, uint64_t param,
                            uint32_t* node)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    const int pop = spf_ops::pool_op_of(op);
    if (!node || pop == spf_ops::kNone) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph op: unknown operation");
    const spf_ops::OpRow& info = spf_ops::row(pop);
    const bool glwe_ks = pop == spf_ops::OP_GLWE_KEYSWITCH || pop == spf_ops::OP_GLWE_AUTOMORPHISM || pop == spf_ops::OP_GLWE_TRACE;
    // The values 12 .. 14 stand for three node constructors, and this door knows them in the constructors' own form only, over ONE
    // operand.  With any other count the call names no operation of this door: it is refused as it was while the values named
    // nothing, "unknown operation" (tests/test_gpu_pbs_graph.py holds value 12 over two operands to that text), and the text says
    // what the value takes.  The rows of the table that were there keep "wrong number of operands".
    if (glwe_ks && n_inputs != 1)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph op: unknown operation: value " + std::to_string((int)op) + " over " + std::to_string(n_inputs) +
                                                          " operands (the GLWE keyswitch, automorphism round and trace take one GLWE1)");
    if (n_inputs != (size_t)info.arity || (n_inputs && !inputs))
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph op: wrong number of operands");
    // GLWE keyswitch, automorphism round, trace: the node of their named constructors (the planner's kinds 70 / 71 / 72), built by
    // the builder they share; a parameter beyond 32 bits is refused as the table's rule refuses it, with its number
    if (glwe_ks) {
        const char* why = nullptr;
        if (spf_ops::op_param(g->prm, pop, &param, &why) != SPF_OK) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, std::string("graph op: ") + why);
        return pop == spf_ops::OP_GLWE_KEYSWITCH      ? graph_add_glwe_ks(g, spf_graph_plan::kNodeGlweKeyswitch, "op (GLWE keyswitch)", (uint32_t)param, inputs[0], node)
               : pop == spf_ops::OP_GLWE_AUTOMORPHISM ? graph_add_glwe_ks(g, spf_graph_plan::kNodeGlweAutomorphism, "op (GLWE automorphism)", (uint32_t)param, inputs[0], node)
                                                      : graph_add_glwe_ks(g, spf_graph_plan::kNodeGlweTrace, "op (GLWE trace)", 0, inputs[0], node);
    }
    for (int i = 0; i < info.arity; i++) {
        if (inputs[i] >= g->nodes.size()) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph op: operand is not a node of this graph");
        if (g->nodes[inputs[i]].kind != info.in_kind[i]) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph op: operand has the wrong ciphertext type");
    }
    const char* why = nullptr;
    if (spf_ops::op_param(g->prm, pop, &param, &why) != SPF_OK) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, std::string("graph op: ") + why);
    *node = g->add(spf_graph_plan::op_node(pop, inputs, param));
    g->planned = false;
    return SPF_OK;
}

// ---- the node constructors ---------------------------------------------------------------------------------------------------------
// What they share.  The operands ids[0 .. n) of a call: nodes of this graph and L1 GLWEs — or, with `lwe`, LWEs of one kind;
// `what` names the call in the texts
static spf_status check_operands(spf_graph* g, const char* what, const uint32_t* ids, size_t n, bool lwe = false)
{
    const auto refuse = [&](const char* why) { return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, std::string("graph ") + what + why); };
    for (size_t i = 0; i < n; i++) {
        if (ids[i] >= g->nodes.size()) return refuse(": operand is not a node of this graph");
        const int kind = g->nodes[ids[i]].kind;
        if (lwe ? kind != SPF_VAL_LWE0 && kind != SPF_VAL_LWE1 : kind != SPF_VAL_GLWE1) return refuse(lwe ? ": operand is not an LWE" : ": operand is not an L1 GLWE");
        if (kind != g->nodes[ids[0]].kind) return refuse(": lwe0 and lwe1 operands mixed");
    }
    return SPF_OK;
}

// ... and the insertion: `add` adds all of the call's nodes or none (what does not fit is thrown, as std::vector throws it) and
// returns the first one's id; the ids first .. first + n_out go to `out` once the nodes exist, and the graph is planned again
template <class F> static spf_status add_nodes(spf_graph* g, uint32_t* out, size_t n_out, F add)
{
    uint32_t first;
    try {
        first = add();
    } catch (const std::exception&) {
        return fail(g->ctx, SPF_ERR_HIP, "out of host memory");
    }
    for (size_t i = 0; i < n_out; i++) out[i] = first + (uint32_t)i;
    g->planned = false;
    return SPF_OK;
}

// `PackedDynamicGenericIntGraphNode::unpack` as a node constructor: n_bits LWE1 nodes, node i = sample_extract(glwe_node, i)
spf_status spf_graph_add_unpack(spf_graph* g, uint32_t glwe_node, size_t n_bits, uint32_t* nodes_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!nodes_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph unpack: null pointer");
    if (n_bits == 0 || n_bits > g->prm.polynomial_degree)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph unpack: n_bits must be in 1 ..= polynomial_degree");
    if (spf_status st = check_operands(g, "unpack", &glwe_node, 1)) return st;
    spf_graph_plan::Node n{};
    n.op = spf_graph_plan::kNodeUnpack; n.kind = SPF_VAL_LWE1; n.n_in = 1; n.in[0] = glwe_node; n.count = (uint32_t)n_bits;
    return add_nodes(g, nodes_out, n_bits, [&] { return g->add_numbered(n, n_bits); });
}

// `DynamicGenericIntGraphNodes::pack` as a node constructor: one GLWE1 node = sum over i of X^i * nodes[i]
spf_status spf_graph_add_pack(spf_graph* g, const uint32_t* nodes, size_t n_bits, uint32_t* node_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!nodes || !node_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph pack: null pointer");
    if (n_bits == 0 || n_bits > g->prm.polynomial_degree)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph pack: n_bits must be in 1 ..= polynomial_degree");
    if (spf_status st = check_operands(g, "pack", nodes, n_bits)) return st;
    spf_graph_plan::Node n{};
    n.op = spf_graph_plan::kNodePack; n.kind = SPF_VAL_GLWE1;
    return add_nodes(g, node_out, 1, [&] { return g->add_listed(n, nodes, n_bits); });
}

// `public_functional_keyswitch` (public_functional_keyswitch.rs:74-148) as a node constructor: one GLWE1 node whose coefficient j
// carries the message of lwe_nodes[j]; the operands in the side list, as a pack node's
spf_status spf_graph_add_public_functional_keyswitch(spf_graph* g, const uint32_t* lwe_nodes, size_t lwe_count, uint32_t* node_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!lwe_nodes || !node_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph public functional keyswitch: null pointer");
    if (lwe_count == 0 || lwe_count > g->prm.polynomial_degree)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph public functional keyswitch: lwe_count must be in 1 ..= polynomial_degree");
    if (spf_status st = check_operands(g, "public functional keyswitch", lwe_nodes, lwe_count, true)) return st;
    spf_graph_plan::Node n{};
    n.op = spf_graph_plan::kNodePufks; n.kind = SPF_VAL_GLWE1;
    return add_nodes(g, node_out, 1, [&] { return g->add_listed(n, lwe_nodes, lwe_count); });
}

// The linear map of weight slot `slot` (spf_lwe_linear.hpp) as a node constructor: M nodes of the operands' kind, node m = row m of
// the slot's matrix times lwe_nodes[0 .. K) (+ bias[m]); one operand list in the side list for all M.  The slot itself is looked at
// by spf_graph_run, not here
spf_status spf_graph_add_lwe_linear(spf_graph* g, uint32_t slot, const uint32_t* lwe_nodes, size_t K, size_t M, uint32_t* nodes_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!lwe_nodes || !nodes_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph linear map: null pointer");
    if (slot >= SPF_LWE_LINEAR_SLOTS)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph linear map: slot " + std::to_string(slot) + " >= SPF_LWE_LINEAR_SLOTS = " +
                                                          std::to_string(SPF_LWE_LINEAR_SLOTS));
    if (K == 0 || K > 0xffffffffu) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph linear map: K must be in 1 ..= 2^32 - 1");
    if (M == 0 || M > SPF_GRAPH_LWE_LINEAR_MAX_ROWS)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph linear map: M must be in 1 ..= SPF_GRAPH_LWE_LINEAR_MAX_ROWS = " +
                                                          std::to_string(SPF_GRAPH_LWE_LINEAR_MAX_ROWS));
    if (spf_status st = check_operands(g, "linear map", lwe_nodes, K, true)) return st;
    spf_graph_plan::Node n{};
    n.op = spf_graph_plan::kNodeLweLinear; n.kind = g->nodes[lwe_nodes[0]].kind;
    n.lin_slot = slot; n.lin_rows = (uint32_t)M;
    return add_nodes(g, nodes_out, M, [&] { return g->add_listed(n, lwe_nodes, K, M); });
}

// The polynomial linear map of polynomial weight slot `slot` (spf_glwe_poly.hpp) as a node constructor: M GLWE1 nodes, node m = row
// m of the slot's polynomial matrix times glwe_nodes[0 .. K) (+ bias[m] on the body); one operand list in the side list for all M.
// The slot itself is looked at by spf_graph_run, not here
spf_status spf_graph_add_glwe_poly_linear(spf_graph* g, uint32_t slot, const uint32_t* glwe_nodes, size_t K, size_t M, uint32_t* nodes_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!glwe_nodes || !nodes_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph polynomial linear map: null pointer");
    if (slot >= SPF_GLWE_POLY_SLOTS)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph polynomial linear map: slot " + std::to_string(slot) + " >= SPF_GLWE_POLY_SLOTS = " +
                                                          std::to_string(SPF_GLWE_POLY_SLOTS));
    if (K == 0 || K > 0xffffffffu) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph polynomial linear map: K must be in 1 ..= 2^32 - 1");
    if (M == 0 || M > SPF_GLWE_POLY_MAX_ROWS)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph polynomial linear map: M must be in 1 ..= SPF_GLWE_POLY_MAX_ROWS = " +
                                                          std::to_string(SPF_GLWE_POLY_MAX_ROWS));
    if (spf_status st = check_operands(g, "polynomial linear map", glwe_nodes, K)) return st;
    spf_graph_plan::Node n{};
    n.op = spf_graph_plan::kNodeGlwePolyLinear; n.kind = SPF_VAL_GLWE1;
    n.lin_slot = slot; n.lin_rows = (uint32_t)M;
    return add_nodes(g, nodes_out, M, [&] { return g->add_listed(n, glwe_nodes, K, M); });
}

// `keyswitch_glwe_to_glwe`, one round of the trace's loop and `trace` (spf_glwe_keyswitch.hpp) as node constructors: one GLWE1
// operand in Node::in[0], one GLWE1 node, Node::param = the keyswitch-key slot / the round / 0.  The keys are looked at by
// spf_graph_run, not here.  `what` names the call in the messages, which — unlike check_operands' — name the operand and the node
// count; nothing is written to *node_out before the node exists
static spf_status graph_add_glwe_ks(spf_graph* g, int32_t op, const char* what, uint32_t param, uint32_t glwe_node, uint32_t* node_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    const std::string w = std::string("graph ") + what;
    if (!node_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, w + ": null pointer");
    const int pop = op == spf_graph_plan::kNodeGlweKeyswitch ? spf_ops::OP_GLWE_KEYSWITCH
                    : op == spf_graph_plan::kNodeGlweAutomorphism ? spf_ops::OP_GLWE_AUTOMORPHISM : spf_ops::OP_GLWE_TRACE;
    uint64_t p64 = param;
    { // the slot / the round by the operation table's rule (spf_ops::op_param), which states it once for graphs and the pool
        const char* why = nullptr;
        if (spf_ops::op_param(g->prm, pop, &p64, &why) != SPF_OK) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, w + ": " + why);
    }
    if (glwe_node >= g->nodes.size())
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, w + ": operand " + std::to_string(glwe_node) + " is not a node of this graph (" +
                                                          std::to_string(g->nodes.size()) + " nodes)");
    if (g->nodes[glwe_node].kind != SPF_VAL_GLWE1)
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, w + ": operand " + std::to_string(glwe_node) + " is not an L1 GLWE (its kind is " +
                                                          std::to_string(g->nodes[glwe_node].kind) + ")");
    // (the node spf_graph_add_op records for the same operation)
    return add_nodes(g, node_out, 1, [&] { return g->add(spf_graph_plan::op_node(pop, &glwe_node, p64)); });
}

spf_status spf_graph_add_glwe_keyswitch(spf_graph* g, uint32_t slot, uint32_t glwe_node, uint32_t* node_out)
{
    return graph_add_glwe_ks(g, spf_graph_plan::kNodeGlweKeyswitch, "GLWE keyswitch", slot, glwe_node, node_out);
}
spf_status spf_graph_add_glwe_automorphism(spf_graph* g, uint32_t round, uint32_t glwe_node, uint32_t* node_out)
{
    return graph_add_glwe_ks(g, spf_graph_plan::kNodeGlweAutomorphism, "GLWE automorphism", round, glwe_node, node_out);
}
spf_status spf_graph_add_glwe_trace(spf_graph* g, uint32_t glwe_node, uint32_t* node_out)
{
    return graph_add_glwe_ks(g, spf_graph_plan::kNodeGlweTrace, "GLWE trace", 0, glwe_node, node_out);
}

// `blind_rotation` (blind_rotation.rs:202-223) as a node constructor: n_bits chained GLWE1 nodes,
// acc_{i+1} = cmux(shift_nodes[i], acc_i, X^-(2^(i + log_stride)) * acc_i), acc_0 = glwe_node; *node_out = the last one
spf_status spf_graph_add_blind_rotation(spf_graph* g, uint32_t glwe_node, const uint32_t* shift_nodes, size_t n_bits, size_t log_stride,
                                        uint32_t* node_out)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!shift_nodes || !node_out) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph blind rotation: null pointer");
    if (const char* why = blind_rotation_shape_error(g->prm, 1, n_bits, log_stride))
        return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, std::string("graph blind rotation: ") + why);
    if (spf_status st = check_operands(g, "blind rotation", &glwe_node, 1)) return st;
    for (size_t i = 0; i < n_bits; i++) {
        if (shift_nodes[i] >= g->nodes.size()) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph blind rotation: selector is not a node of this graph");
        if (g->nodes[shift_nodes[i]].kind != SPF_VAL_GGSW1) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph blind rotation: selector is not an L1 GGSW");
    }
    if (!g->ctx->generic && (g->prm.cbs_radix_log != 4 || g->prm.cbs_radix_count != 4))
        return fail(g->ctx, SPF_ERR_UNSUPPORTED, "cmux kernel is built for cbs_radix 4 x 4 bits");
    spf_graph_plan::Node n{};
    n.op = spf_graph_plan::kNodeRotCmux; n.kind = SPF_VAL_GLWE1; n.n_in = 2;
    return add_nodes(g, node_out, 1, [&] {
        g->nodes.reserve(g->nodes.size() + n_bits); // all of the chain's nodes or none
        uint32_t acc = glwe_node;
        for (size_t i = 0; i < n_bits; i++) {
            n.in[0] = shift_nodes[i]; n.in[1] = acc; n.param = (uint64_t)1 << (i + log_stride);
            acc = g->add(n);
        }
        return acc;
    });
}

spf_status spf_graph_add_output(spf_graph* g, uint32_t node, void* host)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (!host || node >= g->nodes.size()) return fail(g->ctx, SPF_ERR_INVALID_ARGUMENT, "graph output: bad node or null pointer");
    g->outputs.emplace_back(node, host);
    return SPF_OK;
}


spf_status spf_graph_run(spf_graph* g)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (g->grp) return group_run_graphs(g->grp, &g, 1); // a group's graph: placed and run by the group
    return spf_graph_impl::run(g);
}

spf_status spf_graph_stats(spf_graph* g, uint32_t* nodes, uint32_t* levels, uint32_t* launches)
{
    if (!g) return SPF_ERR_INVALID_ARGUMENT;
    if (nodes) *nodes = (uint32_t)g->nodes.size();
    if (levels) *levels = g->n_levels;
    if (launches) *launches = g->n_launches;
    return SPF_OK;
}
