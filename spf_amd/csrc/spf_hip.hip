// spf_hip.hip — host side of the C ABI declared in include/spf_hip.h.
//
// Owns the per-GPU context: device copies of the evaluation keys (reference layouts, 288 GB of
// HBM means every rank simply holds a full replica), the twiddle image, growable staging
// buffers for the host-pointer entry points, and hipEvent timing for bench.py.
// No exception leaves this file; every entry point returns spf_status.
#include "../../include/spf_hip.h"
#include "spf_kernels.hpp"
#include "spf_cbs_tail.hpp"
#include "spf_generic.hpp"
#include "spf_poly_fft.hpp"
#include "spf_pufks.hpp"
#include "spf_pfks.hpp"
#include "spf_lwe_linear.hpp"
#include "spf_glwe_poly.hpp"
#include "spf_glwe_keyswitch.hpp"
#include "spf_lwe_ring_pack.hpp"
#include "spf_lwe_ring_pack_plan.hpp"
#include "spf_each_plan.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

using namespace spf;

// HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and two streams that share a queue
// run their kernels one after the other: with the default, two bootstrap launches on two streams took 7.45 ms, with more queues
// 3.76 (tools/concurrency_probe.py; r06: sixteen staging sets, 24 queues — a 32-bit adder by handles 10.4 ms against 11.5 with 16).
// The pool keeps several batches resident on the GPU at once, each on its own stream, beside
// the streams of the context and of the caller — so the library asks for more queues, unless the environment already says
// otherwise.  The runtime reads the variable when it initialises (first HIP call of the process); this runs when the library is
// loaded.  A process that has initialised HIP before loading the library keeps its setting: export GPU_MAX_HW_QUEUES there.
__attribute__((constructor(101))) static void spf_ask_for_hw_queues() { (void)setenv("GPU_MAX_HW_QUEUES", "24", 0); }

namespace {

thread_local std::string g_create_error;

// (A three-ciphertexts-per-workgroup blind rotation for 2 x #CU < B <= 3 x #CU — r05, the 512 -> 513 step of the launch time,
// 6.95 -> 9.76 ms — was built, bit-equal and no faster than four per workgroup: 9.90-9.97 ms against 9.74-9.82, plain PBS 10.61
// against 10.28; profiles/r05_experiments_other_kernels.md, source in profiles/r09_experimental_sources/retired_knobs.patch.)
constexpr size_t kMaxGridRows = 32768; // rows per launch of the one-grid-row-per-ciphertext kernels

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct TimedLaunch {
    hipEvent_t start, stop;
};

// intermediates of the keyswitch (digits [Mpad][K], digit sums [Mpad]) and of the circuit bootstrap (lo-noise GLWE, GLEV): one set
// per stream of work that may run concurrently — the context's own for the entry points, one per staging set of a pool
struct Scratch {
    DevBuf ks_dig, ks_rowsum, cbs_glwe, cbs_glev;
};

// kernels whose launches spf_set_timing brackets with hipEvents on the launch stream (spf_last_kernel_ms)
enum TimedKernel { T_PBS = 0, T_KS, T_TRACE, T_SS, T_CMUX, T_PUFKS_PRE, T_LIN_PLANES, T_LIN, T_GLWE_POLY, T_GLWE_KS, T_RING_PACK, T_COUNT };
const char* const kTimedNames[T_COUNT] = {"pbs", "keyswitch", "trace", "scheme_switch", "cmux", "pufks_prepass", "lwe_linear_planes",
                                          "lwe_linear", "glwe_poly_linear", "glwe_keyswitch", "lwe_ring_pack"};

// one slot of plaintext weights for spf_lwe_linear_* (spf_lwe_linear.hpp): the int64 matrix as loaded, always; the int8 limbs of
// -w and their sums where the matrix-core path takes the matrix (U > 0)
struct LweLinearSlot {
    bool ready = false;
    size_t M = 0, K = 0, Mpad = 0, Kpad = 0;
    uint32_t U = 0, nseg = 0;
    long long* d_w = nullptr; // [M][K]
    uint64_t* d_bias = nullptr; // [M], or null
    int8_t* d_A = nullptr;    // [U][Mpad][Kpad]
    int* d_rs = nullptr;      // [nseg][U][Mpad]
};

// one slot of plaintext polynomial weights for spf_glwe_poly_linear_* (spf_glwe_poly.hpp): the image spf_glwe_poly::pack makes
struct GlwePolySlot {
    bool ready = false;
    bool constants_only = false;
    size_t M = 0, K = 0, terms = 0;
    uint32_t* d_offsets = nullptr;           // [M K + 1]
    spf_glwe_poly::Term* d_terms = nullptr;  // [terms], or null where there are none
    uint64_t* d_scalars = nullptr;           // [M][K], constants-only slots
    uint64_t* d_bias = nullptr;              // [M][N], or null
};

// one slot of spf_load_glwe_keyswitch_key_std (spf_glwe_keyswitch.hpp): the key's spectra [row<k][level<count][poly<k+1][N/2] and
// the radix that came with it
struct GlweKskSlot {
    bool ready = false;
    c64* d_key = nullptr;
    uint32_t radix_log = 0, radix_count = 0;
};

} // namespace

// Process-wide counts of the live handles (spf_live_objects).  Every handle struct has a Tick member: the counts move in the
// constructors and at the final frees and nowhere else — never on a submit, run or wait path.
namespace spf_live {
enum Kind { CTX = 0, GROUP, GRAPH, POOL, VALUE, KINDS };
inline std::atomic<uint64_t> g_count[KINDS];
template <Kind K> struct Tick {
    Tick() { g_count[K].fetch_add(1, std::memory_order_relaxed); }
    ~Tick() { g_count[K].fetch_sub(1, std::memory_order_relaxed); }
    Tick(const Tick&) = delete;
    Tick& operator=(const Tick&) = delete;
};
} // namespace spf_live

struct spf_ctx {
    spf_live::Tick<spf_live::CTX> live;
    std::atomic<int> refs{1}; // the caller's (spf_destroy drops it), one per graph and pool made on the context, a group's on its members
    spf_params prm{};
    int device = 0;
    std::recursive_mutex mu; // recursive: the host-pointer entry points hold it across the _dev calls they make
    std::string err;               // last error message; guarded by err_mu (read and written from any thread)
    mutable std::mutex err_mu;
    c64* d_tables = nullptr;
    c64* d_bsk = nullptr;        // the caller's spectra (what spf_key_blob hands out and a broadcast replicates)
    c64* d_bsk_scaled = nullptr; // the same times 2^-10: what the blind-rotation kernels read (finish_bootstrap_key)
    size_t bsk_bytes = 0;
    bool bsk_ready = false;
    uint64_t* d_ksk = nullptr;
    size_t ksk_bytes = 0;
    bool ksk_ready = false;
    uint64_t* d_cbs_lut = nullptr; // fill_multifunctional_cbs_decomposition_lut, constant per params
    DevBuf in, out, mid, aux;      // staging for the host-pointer entry points
    DevBuf packed;                  // the packed level-0 input of spf_pbs_bivariate_dev
    DevBuf unpack_l1, unpack_l0;    // the unpacked bits of spf_unpack_circuit_bootstrap_dev, before and after the keyswitch
    DevBuf brot_mid, brot_high;     // spf_blind_rotation_dev: the accumulator between steps; generic contexts: X^-r * accumulator
    int8_t* d_ksk_planes = nullptr; // key byte planes for the int8-MFMA keyswitch [Npad][K]
    size_t ks_npad = 0;
    Scratch scr;                    // intermediates of the entry points (keyswitch digits, circuit-bootstrap GLWE / GLEV)
    c64* d_ak = nullptr;            // automorphism key, FFT'd: [log2 N][l_tr][2][N/2]
    size_t ak_bytes = 0;
    bool ak_ready = false;
    c64* d_ssk = nullptr;           // scheme-switch key, FFT'd: [l_ss][2][N/2]
    size_t ssk_bytes = 0;
    bool ssk_ready = false;
    double* d_ggsw_const = nullptr; // l1ggsw_zero | l1ggsw_one (Evaluation::new, evaluation.rs:161-197), built on first use
    bool ggsw_const_ready = false;  // reset whenever a key of the circuit bootstrap changes
    int n_cu = 256;                // compute units of the device (picks the blind-rotation shape)
    hipStream_t stream = nullptr;  // stream of the host-pointer entry points
    uint64_t buf_epoch = 0;            // bumped whenever a scratch buffer is reallocated (captured gate graphs hold their addresses)
    const char* last_pbs_kernel = "";  // name of the blind-rotation kernel the last launch used
    const char* last_cmux_kernel = ""; // ... and of the CMUX kernel
    const char* last_ks_kernel = "";   // ... and of the LWE keyswitch
    hipStream_t copy_stream = nullptr; // device-to-host copies of finished slices, under the next slice's kernel
    std::vector<hipEvent_t> slice_ev;  // one "slice k is computed" event per slice in flight
    bool timing = false;
    std::vector<TimedLaunch> timed[T_COUNT];
    // any other parameter set (spf_generic.hpp): N a power of two in 16 .. 2048, any k and radix that fit the LDS.  One workgroup per ciphertext,
    // the oracle's transform for those sizes; every batch and device-pointer entry point is served (keyswitch in its VALU form);
    // gate graphs are not.
    bool generic = false;
    uint32_t log_n = 11;
    c64* d_gen_tables = nullptr; // [N/2] twist, then [N/4] transform twiddles
    // public functional keyswitch (spf_pufks.hpp): the key's spectra [n][count][k+1][N/2]; its shape comes with the key, not with
    // spf_params.  A tuned context whose key has another radix than the hand-written kernel's runs generic_pufks_kernel and keeps
    // the generic twist table (d_gen_tables, [N/2] only) for it.
    c64* d_pufks = nullptr;
    size_t pufks_bytes = 0;
    bool pufks_ready = false;
    uint32_t pufks_n = 0, pufks_log = 0, pufks_count = 0; // from_dimension, radix_log, radix_count (0: no shape yet)
    DevBuf pufks_dig;                                     // packed digits of pufks_digits_kernel, [outputs of a chunk][n][pstride]
    const char* last_pufks_kernel = "";
    // private functional keyswitch (spf_pfks.hpp): n_keys keys back to back, each [lwe_count][n+1][count][k+1][N] words, as loaded
    // (key blob 5); their byte planes for the matrix-core path (null where that path declines the key: the VALU kernel reads the
    // words).  The shape comes with the keys.
    uint64_t* d_pfks = nullptr;
    size_t pfks_bytes = 0;
    bool pfks_ready = false;
    uint32_t pfks_keys = 0, pfks_n = 0, pfks_p = 0, pfks_log = 0, pfks_count = 0; // n_keys, from_dimension, lwe_count, radix (0: no shape yet)
    int8_t* d_pfks_planes = nullptr;
    DevBuf pfks_dig, pfks_rowsum; // limbs [U][Mpad][Kpad] and limb sums [nseg][U][Mpad] of one launch
    DevBuf pfks_glwe, pfks_lwe;   // circuit bootstrap via PFKS: the lo-noise GLWEs and the extracted, rotated LWE rows
    const char* last_pfks_kernel = "";
    // plaintext linear maps over LWE ciphertexts (spf_lwe_linear.hpp): the weight slots and the byte planes of one launch
    LweLinearSlot lin[SPF_LWE_LINEAR_SLOTS];
    DevBuf lin_planes;
    const char* last_lin_kernel = "";
    uint64_t lin_epoch = 0;         // bumped by every spf_load_lwe_linear_weights (captured gate graphs hold a slot's pointers)
    uint32_t last_lin_launches = 0; // kernel launches the last spf_lwe_linear_enqueue made (spf_graph_stats)
    // plaintext polynomial linear maps over GLWE ciphertexts (spf_glwe_poly.hpp): the weight slots
    GlwePolySlot gpoly[SPF_GLWE_POLY_SLOTS];
    const char* last_gpoly_kernel = "";
    uint64_t gpoly_epoch = 0; // bumped by every spf_load_glwe_poly_weights (captured gate graphs hold a slot's pointers)
    // GLWE keyswitch, automorphism round and trace (spf_glwe_keyswitch.hpp): the keyswitch-key slots; whether the generic kernel
    // has what it needs on this context (always on a generic one; on a tuned one from the first key or radix that needs it)
    GlweKskSlot gksk[SPF_GLWE_KSK_SLOTS];
    bool glwe_ks_generic_ready = false;
    const char* last_glwe_ks_kernel = "";
    uint64_t gksk_epoch = 0; // bumped by every spf_load_glwe_keyswitch_key_std (captured gate graphs hold a slot's pointer and kernel)
    // ring packing (spf_lwe_ring_pack.hpp): the scratch of the host-pointer form, one slice's worth
    DevBuf ring_pack_scratch;
    const char* last_ring_pack_kernel = "";
    // the per-item entry points (spf_*_each_*): the pointer, parameter, workgroup and unit tables of ONE call, built on the host in
    // `each_host` (pinned), copied to `each_tab` on the call's stream; `each_ev` says when that copy has read the host image
    DevBuf each_tab;
    void* each_host = nullptr;
    size_t each_host_cap = 0;
    hipEvent_t each_ev = nullptr;
    bool each_ev_recorded = false;
};

namespace {

spf_status fail(spf_ctx* c, spf_status s, const std::string& msg)
{
    if (c) {
        std::lock_guard<std::mutex> g(c->err_mu);
        c->err = msg;
    } else {
        g_create_error = msg;
    }
    return s;
}

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(ctx, SPF_ERR_HIP,                                                         \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

// e^{+2 pi i num/den}: first-octant cosl/sinl, rounded once to double, mirrored by octant so
// conjugate / quarter-turn partners are exact.  (The build's definition of its twiddles.)
c64 root_of_unity(uint64_t num, uint64_t den)
{
    static const long double TWO_PI = 6.283185307179586476925286766559005768L;
    uint64_t j = num % den, eighth = den / 8, oct = j / eighth, r = j % eighth;
    uint64_t rr = (oct & 1) ? (eighth - r) : r;
    long double th = TWO_PI * (long double)rr / (long double)den;
    double c = (double)cosl(th), s = (double)sinl(th);
    if (rr == 0) { c = 1.0; s = 0.0; }
    switch (oct) {
    case 0: return {c, s};
    case 1: return {s, c};
    case 2: return {-s, c};
    case 3: return {-c, s};
    case 4: return {-c, -s};
    case 5: return {-s, -c};
    case 6: return {s, -c};
    default: return {c, -s};
    }
}

c64 conj(c64 a) { return {a.re, -a.im}; }

void build_tables(std::vector<c64>& t)
{
    t.resize(kTableEntries);
    for (int k1 = 1; k1 < 8; k1++)
        for (int lane = 0; lane < 64; lane++)
            t[kT1Off + (k1 - 1) * 64 + lane] = conj(root_of_unity((uint64_t)(lane * k1), 512));
    for (int c = 1; c < 8; c++)
        for (int b = 0; b < 8; b++) t[kT2Off + (c - 1) * 8 + b] = conj(root_of_unity((uint64_t)(b * c), 64));
    for (int k = 0; k < 512; k++) t[kWCOff + k] = conj(root_of_unity((uint64_t)k, 1024));
    // negacyclic twist e^{+2 pi i j / (2N)}, j = 2n' + par (math/fft/negacyclic/mod.rs:56-65)
    for (int par = 0; par < 2; par++)
        for (int n = 0; n < 512; n++) t[kTWOff + par * 512 + n] = root_of_unity((uint64_t)(2 * n + par), 4096);
}

uint32_t ceil_log2(uint32_t v)
{
    uint32_t l = 0;
    while ((1u << l) < v) l++;
    return l;
}

spf_status ensure(spf_ctx* c, DevBuf& b, size_t bytes)
{
    if (b.cap >= bytes) return SPF_OK;
    c->buf_epoch++;
    if (b.p) HIPCHK(c, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return SPF_OK;
}

} // namespace

#include "spf_ops.hpp" // ciphertext sizes, the operation table, the parameter rule: where an operation is declared
#include "spf_ops_launch.hpp" // ... and its dispatcher

namespace {

size_t ak_complex(const spf_params& p)
{
    uint32_t logn = 0;
    while ((1u << logn) < p.polynomial_degree) logn++;
    return (size_t)logn * p.glwe_size * p.tr_radix_count * (p.glwe_size + 1) * (p.polynomial_degree / 2);
}
size_t ssk_complex(const spf_params& p)
{
    return (size_t)(p.glwe_size * (p.glwe_size + 1) / 2) * p.ss_radix_count * (p.glwe_size + 1) * (p.polynomial_degree / 2);
}

spf_status get_events(spf_ctx* c, hipEvent_t* a, hipEvent_t* b)
{
    HIPCHK(c, hipEventCreate(a));
    HIPCHK(c, hipEventCreate(b));
    return SPF_OK;
}

// hipEvent bracket around the launches of one entry point, when timing is on
struct TimedScope {
    spf_ctx* c; hipStream_t s; int which; TimedLaunch tl{}; bool on = false;
    TimedScope(spf_ctx* c_, hipStream_t s_, int which_) : c(c_), s(s_), which(which_) {}
    spf_status begin()
    {
        if (!c->timing) return SPF_OK;
        spf_status st = get_events(c, &tl.start, &tl.stop);
        if (st != SPF_OK) return st;
        on = true;
        HIPCHK(c, hipEventRecord(tl.start, s));
        return SPF_OK;
    }
    spf_status end()
    {
        if (!on) return SPF_OK;
        on = false;
        hipError_t e = hipEventRecord(tl.stop, s);
        if (e != hipSuccess) {
            (void)hipEventDestroy(tl.start); (void)hipEventDestroy(tl.stop);
            return fail(c, SPF_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
        }
        c->timed[which].push_back(tl);
        return SPF_OK;
    }
    ~TimedScope() // a launch failed between begin() and end(): the pair goes back instead of leaking
    {
        if (on) { (void)hipEventDestroy(tl.start); (void)hipEventDestroy(tl.stop); }
    }
};

#ifdef SPF_STAMPS
// Diagnostic build (-DSPF_STAMPS): one launch with a zeroed stamp buffer — 16 words per wave, slot i = the cycles the wave spent in
// phase i (PhaseStamps, spf_device.hpp) — then one line per phase on stderr: the median over the waves, divided by `per` (the steps
// of a launch); with `share` the phase's part of the total, with `halves` the medians of the older (0-3) and of the younger (4-7)
// waves of the eight-wave workgroups as well.  The caller prints the heading; `name_fmt` is a line's prefix and name column,
// `total_fmt` the closing line.  `launch(stamps)` launches on `s` with the buffer and returns its status.
template <class LAUNCH>
static spf_status stamp_report(spf_ctx* c, hipStream_t s, size_t waves, const char* const* names, size_t n_names, double per,
                               bool share, bool halves, const char* name_fmt, const char* total_fmt, LAUNCH launch)
{
    uint64_t* d_st = nullptr;
    HIPCHK(c, hipMalloc(&d_st, waves * 16 * 8));
    HIPCHK(c, hipMemsetAsync(d_st, 0, waves * 16 * 8, s));
    spf_status st = launch(d_st);
    if (st != SPF_OK) return st;
    HIPCHK(c, hipStreamSynchronize(s));
    std::vector<uint64_t> h(waves * 16);
    HIPCHK(c, hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_st);
    auto median = [&](size_t i, int half) { // half 0 / 1: the older / younger waves of each workgroup, -1: all
        std::vector<uint64_t> v;
        for (size_t wv = 0; wv < waves; wv++)
            if (half < 0 || (int)(wv % 8) / 4 == half) v.push_back(h[wv * 16 + i]);
        std::sort(v.begin(), v.end());
        return (double)v[v.size() / 2] / per;
    };
    double total = 0;
    for (size_t i = 0; i < n_names; i++) total += median(i, -1);
    for (size_t i = 0; i < n_names; i++) {
        fprintf(stderr, name_fmt, names[i]);
        fprintf(stderr, " %8.0f", median(i, -1));
        if (share) fprintf(stderr, " %5.1f%%", 100.0 * median(i, -1) / total);
        if (halves) fprintf(stderr, " | %8.0f | %8.0f", median(i, 0), median(i, 1));
        fprintf(stderr, "\n");
    }
    fprintf(stderr, total_fmt, total);
    return SPF_OK;
}
// what the slots of each kernel hold (the stamps.mark(i) of its body)
static const char* const kStampNames2p[12] = {"stage+rendezvous", "gather+decomp+twist", "rendezvous(gathered) + key-row wait", "fwd transform pair",
    "cross write+key barrier", "cross read+combine", "MAD x2", "ring barrier", "inverse cross exchange",
    "inv transform pair", "untwist+convert+acc", "step head"};
static const char* const kStampNames8[12] = {"step head+stage", "barrier A (j=1: A+F)", "gather+decomp+post+F+twist", "fwd transform", "cross write+barrier B",
    "cross read+combine+publish", "barrier C", "MAD+inverse split+post", "barrier D", "inbox read", "inv transform", "untwist+convert+acc"};
static const char* const kStampNamesTrace[10] = {"round head: stage, gather, digits 0-1 (+park)", "digits + twist x3", "fwd transform pair x3",
    "cross write + key barrier x3", "cross read + combine + MAD x3", "ring barrier x3", "inverse cross exchange",
    "next rows requested", "inv transform pair", "untwist + convert + acc"};
static const char* const kStampNamesCmux4[9] = {"entry: pointers, loads issued, table copy", "barrier (table in place)", "twist tables to registers",
    "decompose + 2 x (transform pair, cross)", "key1 issue + spectra out + 2 barriers", "8-row accumulation chain",
    "inverse cross (3 barriers)", "inverse transform + untwist + store issue", "store drain"};
static const char* const kStampNamesCmux[16] = {"entry: operand words in, decomposition", "barrier (table in place)", "digit + twist x8",
    "hand-over (cross data consumed) x7", "forward transform x8", "cross write + hand-over x8", "cross read + combine x8",
    "wait for the round's selector rows x8", "MAD + next rows requested x8", "inverse cross exchange (3 hand-overs)",
    "inverse transform pair", "untwist + d0 + store issue", "entry: kernel arguments + pointer table", "entry: 64 operand loads issued",
    "(unused)", "(unused)"};
#endif

GenericShape generic_shape(const spf_ctx* c)
{
    GenericShape g{};
    g.N = c->prm.polynomial_degree; g.logN = c->log_n; g.k = c->prm.glwe_size;
    g.twist = c->d_gen_tables;
    g.w = g.N == (uint32_t)kN ? c->d_tables : c->d_gen_tables + g.N / 2; // N = 2048: DAG-I reads the tuned kernels' table image
    return g;
}

spf_status blind_rotate_args(spf_ctx* c, size_t B, uint32_t log_chi, uint32_t log_v)
{
    if (B > kBatchMax) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    // modulus switch needs log_modulus - log_v >= 1 and shifts below 64
    if (log_v >= c->log_n + 1 || log_chi >= 52) return fail(c, SPF_ERR_INVALID_ARGUMENT, "log_v / log_chi out of range");
    return SPF_OK;
}

spf_status launch_blind_rotate(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_lwe,
                               const uint64_t* d_lut, size_t lut_stride, uint32_t log_chi,
                               uint32_t log_v, uint64_t body_rotate, uint64_t* d_out,
                               size_t out_stride, bool extract, int per_wg_hint = 0)
{
    if (!c->bsk_ready) return fail(c, SPF_ERR_NO_KEY, "bootstrap key not loaded");
    if (B == 0) return SPF_OK;
    {
        spf_status st = blind_rotate_args(c, B, log_chi, log_v);
        if (st != SPF_OK) return st;
    }
    if (c->generic) {
        GenericPbsArgs ga{};
        ga.g = generic_shape(c);
        ga.lwe_in = d_lwe; ga.lut = d_lut; ga.lut_stride = lut_stride; ga.bsk = c->d_bsk; ga.out = d_out; ga.out_stride = out_stride;
        ga.n = c->prm.lwe_dimension; ga.B = (uint32_t)B; ga.radix_log = c->prm.pbs_radix_log; ga.count = c->prm.pbs_radix_count;
        ga.log_chi = log_chi; ga.log_v = log_v; ga.sample_extract = extract ? 1u : 0u; ga.body_rotate = body_rotate;
        c->last_pbs_kernel = "generic_pbs_kernel";
        TimedScope tsg(c, s, T_PBS);
        spf_status stg = tsg.begin();
        if (stg != SPF_OK) return stg;
        hipLaunchKernelGGL(generic_pbs_kernel, dim3((unsigned)B), dim3(kGenericThreads),
                           generic_lds_bytes(ga.g.N, ga.g.k, true), s, ga);
        HIPCHK(c, hipGetLastError());
        return tsg.end();
    }
    BlindRotateArgs a{};
    a.lwe_in = d_lwe; a.lut = d_lut; a.lut_stride = lut_stride; a.bsk = c->d_bsk_scaled;
    a.tables = c->d_tables; a.out = d_out; a.out_stride = out_stride;
    a.n = c->prm.lwe_dimension; a.B = (uint32_t)B; a.log_chi = log_chi; a.log_v = log_v;
    a.body_rotate = body_rotate; a.sample_extract = extract ? 1u : 0u;
    // Shape by batch size: at most one ciphertext per CU -> eight waves per ciphertext (blind_rotate8_kernel, latency);
    // up to two per CU -> the paired schedule with two ciphertexts per workgroup (blind_rotate2p2_kernel);
    // beyond -> four ciphertexts per workgroup, one workgroup per CU, two waves per SIMD (blind_rotate2p_kernel).
    // per_wg_hint (the pool): ciphertexts per workgroup the CALLER wants at least — a batch that shares the chip with other
    // batches in flight takes the shape of the whole population, so that the batches tile the CUs instead of each spreading thin.
    const size_t n_cu = (size_t)c->n_cu;
    const bool quad = B <= n_cu && per_wg_hint <= 1;
    const bool pair2 = !quad && B <= 2 * n_cu && per_wg_hint <= 2;
    const size_t per_wg = quad ? 1 : (pair2 ? 2 : 4);
    dim3 grid((unsigned)((B + per_wg - 1) / per_wg)), block(pair2 ? 256 : 512);
    // one launch of the shape's kernel (`stamps`: the diagnostic build's phase buffer, otherwise null)
    auto launch = [&](uint64_t* stamps) -> spf_status {
        a.stamps = stamps;
        TimedScope ts(c, s, T_PBS);
        spf_status st = ts.begin();
        if (st != SPF_OK) return st;
#define SPF_STR2(x) #x
#define SPF_STR(x) SPF_STR2(x)
#define SPF_LAUNCH(NAME, KERNEL, LDS) do { c->last_pbs_kernel = NAME; hipLaunchKernelGGL(KERNEL, grid, block, LDS, s, a); } while (0)
        // log_v >= 1 makes every rotation amount even: the kernels then skip the hand-overs around the rotation gather (",even")
        if (quad && log_v == 0) SPF_LAUNCH("blind_rotate8_kernel<2,16>", (blind_rotate8_kernel<2, 16, 1>), kBlindRotate8Lds);
        else if (quad) SPF_LAUNCH("blind_rotate8_kernel<2,16,even>", (blind_rotate8_kernel<2, 16, 0>), kBlindRotate8Lds);
        else if (pair2 && log_v == 0) SPF_LAUNCH("blind_rotate2p2_kernel<2,16," SPF_STR(SPF_BR2_OPT) ">", (blind_rotate2p2_kernel<2, 16, SPF_BR2_OPT, 1>), kBlindRotate2p2Lds);
        else if (pair2) SPF_LAUNCH("blind_rotate2p2_kernel<2,16," SPF_STR(SPF_BR2_OPT) ",even>", (blind_rotate2p2_kernel<2, 16, SPF_BR2_OPT, 0>), kBlindRotate2p2Lds);
        else if (log_v == 0) SPF_LAUNCH("blind_rotate2p_kernel<2,16," SPF_STR(SPF_BR_OPT_MIX) ">", (blind_rotate2p_kernel<2, 16, SPF_BR_OPT_MIX, 1>), kBlindRotate2pLds);
        else SPF_LAUNCH("blind_rotate2p_kernel<2,16," SPF_STR(SPF_BR_OPT) ",even>", (blind_rotate2p_kernel<2, 16, SPF_BR_OPT, 0>), kBlindRotate2pLds);
#undef SPF_LAUNCH
        HIPCHK(c, hipGetLastError());
        return ts.end();
    };
#ifdef SPF_STAMPS
    if (!pair2) { // every launch of the eight-wave workgroups reports, per CMUX step
        const size_t waves = (size_t)grid.x * 8;
        fprintf(stderr, "[stamps] per CMUX step, median over %zu waves (cycles, share | waves 0-3 | waves 4-7)\n", waves);
        return stamp_report(c, s, waves, quad ? kStampNames8 : kStampNames2p, 12, a.n, true, true, "[stamps] %-30s", "[stamps] total                      %8.0f\n", launch);
    }
#endif
    return launch(nullptr);
}

// the int8-MFMA formulation applies when digits fit int8, K is a multiple of the MFMA depth and
// the int32 accumulators cannot overflow
bool ks_mfma_ok(const spf_params& p)
{
    const uint64_t K = (uint64_t)p.glwe_size * p.polynomial_degree * p.ks_radix_count;
    return p.ks_radix_log <= 8 && K % 256 == 0 && K * ((uint64_t)1 << (p.ks_radix_log - 1)) * 128 < ((uint64_t)1 << 31);
}

// (re)build the byte-plane image of the keyswitch key; called whenever the key becomes ready
spf_status build_ks_planes(spf_ctx* c)
{
    if (c->generic || !ks_mfma_ok(c->prm)) return SPF_OK;
    const uint32_t n_in = c->prm.glwe_size * c->prm.polynomial_degree, w = c->prm.lwe_dimension + 1;
    const size_t K = (size_t)n_in * c->prm.ks_radix_count;
    const size_t npad = ((size_t)w * 8 + KSG_TILE - 1) / KSG_TILE * KSG_TILE;
    if (!c->d_ksk_planes) HIPCHK(c, hipMalloc((void**)&c->d_ksk_planes, npad * K));
    c->ks_npad = npad;
    HIPCHK(c, hipMemsetAsync(c->d_ksk_planes, 0, npad * K, c->stream));
    const size_t total = (size_t)n_in * c->prm.ks_radix_count * w;
    hipLaunchKernelGGL(ks_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->d_ksk,
                       c->d_ksk_planes, n_in, w, c->prm.ks_radix_count, K);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPF_OK;
}

spf_status launch_keyswitch(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_in,
                            uint64_t* d_out, Scratch* sc = nullptr)
{
    if (!sc) sc = &c->scr;
    if (!c->ksk_ready) return fail(c, SPF_ERR_NO_KEY, "keyswitch key not loaded");
    if (B == 0) return SPF_OK;
    if (B > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    KeyswitchArgs a{};
    a.in = d_in; a.ksk = c->d_ksk; a.out = d_out;
    a.n_in = c->prm.glwe_size * c->prm.polynomial_degree; a.n_out = c->prm.lwe_dimension;
    a.B = (uint32_t)B; a.radix_log = c->prm.ks_radix_log; a.count = c->prm.ks_radix_count;
    const bool mfma = c->d_ksk_planes != nullptr; // (null when the radix does not fit the int8 formulation: keyswitch_kernel)
    const size_t K = (size_t)a.n_in * a.count, mpad = (B + KSG_TILE - 1) / KSG_TILE * KSG_TILE;
    if (mfma) {
        spf_status st = ensure(c, sc->ks_dig, mpad * K);
        if (st != SPF_OK) return st;
        st = ensure(c, sc->ks_rowsum, mpad * sizeof(int));
        if (st != SPF_OK) return st;
    }
    TimedScope ts(c, s, T_KS);
    {
        spf_status st = ts.begin();
        if (st != SPF_OK) return st;
    }
    if (mfma) {
        HIPCHK(c, hipMemsetAsync(sc->ks_rowsum.p, 0, mpad * sizeof(int), s));
        hipLaunchKernelGGL(ks_digits_kernel, dim3((unsigned)B), dim3(256), 0, s, d_in, (int8_t*)sc->ks_dig.p,
                           (int*)sc->ks_rowsum.p, a.n_in, a.B, a.radix_log, a.count);
        KsGemmArgs g{};
        g.A = (const int8_t*)sc->ks_dig.p; g.Bt = c->d_ksk_planes; g.rowsum = (const int*)sc->ks_rowsum.p;
        g.in = d_in; g.out = d_out; g.B = a.B; g.n_in = a.n_in; g.n_out = a.n_out; g.K = (uint32_t)K;
        dim3 grid((unsigned)(c->ks_npad / KSG_TILE), (unsigned)(mpad / KSG_TILE));
        hipLaunchKernelGGL(ks_gemm_lds_kernel, grid, dim3(256), kKsLdsBytes, s, g); // operand tiles staged through LDS by LDS-DMA
        c->last_ks_kernel = "ks_gemm_lds_kernel";
    } else {
        // (the whole batch in one grid: grid.y = 65536 launches and computes on gfx950, tests/test_gpu_launch_slices.py; larger
        // values are not held by a test)
        dim3 grid((a.n_out + 1 + 255) / 256, (unsigned)((B + KS_CT - 1) / KS_CT)), block(256);
        hipLaunchKernelGGL(keyswitch_kernel, grid, block, 0, s, a);
        c->last_ks_kernel = "keyswitch_kernel";
    }
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

// the parameter sets of the generic kernels (spf_generic.hpp)
bool params_generic(const spf_params& p, std::string& why)
{
    const uint32_t N = p.polynomial_degree;
    if (N < 16 || N > 2048 || (N & (N - 1))) {
        why = "polynomial_degree must be a power of two in 16 .. 2048";
        return false;
    }
    if (p.glwe_size == 0 || p.glwe_size > 8) { why = "glwe_size must be in 1 .. 8"; return false; }
    auto radix_ok = [](uint32_t lg, uint32_t cnt) { return lg >= 1 && cnt >= 1 && lg * cnt < 64; };
    if (!radix_ok(p.pbs_radix_log, p.pbs_radix_count) || !radix_ok(p.cbs_radix_log, p.cbs_radix_count)) {
        why = "a radix decomposition needs 1 <= radix_log * count < 64";
        return false;
    }
    if (generic_trace_lds_bytes(N, p.glwe_size) > 160 * 1024) { why = "(k+1) polynomials of this degree do not fit the generic kernels' LDS"; return false; }
    if (!radix_ok(p.tr_radix_log, p.tr_radix_count) || !radix_ok(p.ss_radix_log, p.ss_radix_count)) {
        why = "a radix decomposition needs 1 <= radix_log * count < 64";
        return false;
    }
    if (p.lwe_dimension == 0 || p.lwe_dimension > 4096) { why = "lwe_dimension out of range"; return false; }
    if (p.ks_radix_log == 0 || p.ks_radix_log * p.ks_radix_count > 32) { why = "ks_radix must satisfy 0 < l*logB <= 32"; return false; }
    if (p.cbs_radix_count >= 8) { why = "cbs_radix.count must be in 1..7"; return false; }
    return true;
}

bool params_supported(const spf_params& p, std::string& why)
{
    if (p.polynomial_degree != kN) { why = "kernels are built for polynomial_degree 2048"; return false; }
    if (p.glwe_size != 1) { why = "kernels are built for glwe_size 1"; return false; }
    if (p.pbs_radix_log != 16 || p.pbs_radix_count != 2) { why = "blind rotation is built for pbs_radix 2 x 16 bits"; return false; }
    if (p.lwe_dimension == 0 || p.lwe_dimension > 4096) { why = "lwe_dimension out of range"; return false; }
    if (p.ks_radix_log == 0 || p.ks_radix_log * p.ks_radix_count > 32) { why = "ks_radix must satisfy 0 < l*logB <= 32"; return false; }
    if (p.cbs_radix_count == 0 || p.cbs_radix_count >= 8 || p.cbs_radix_log == 0) { why = "cbs_radix.count must be in 1..7"; return false; }
    return true;
}

// ---- staging of the host-pointer forms

// `bytes` from the caller's `host` into the context's buffer `buf` (a null `host`: an operand this call does not have)
struct HostIn {
    DevBuf& buf;
    const void* host;
    size_t bytes;
};

// The one way a host-pointer form reaches the device, after its arguments are checked: under c->mu (the staging buffers are
// shared: one caller at a time), stage `ins`, make c->out hold `out_bytes`, then `work` enqueues on c->stream.  Once anything is
// enqueued, no return before c->stream is idle: copies from the caller's buffers may still be in flight, and the caller is free
// to release those after an error.  The first failure's status and message stay in place.
template <class Work>
spf_status staged(spf_ctx* c, std::initializer_list<HostIn> ins, size_t out_bytes, Work&& work)
{
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    auto enqueue = [&]() -> spf_status {
        for (const HostIn& in : ins) {
            if (!in.host) continue;
            spf_status s = ensure(c, in.buf, in.bytes);
            if (s != SPF_OK) return s;
            HIPCHK(c, hipMemcpyAsync(in.buf.p, in.host, in.bytes, hipMemcpyHostToDevice, c->stream));
        }
        spf_status s = ensure(c, c->out, out_bytes);
        if (s != SPF_OK) return s;
        return work();
    };
    const spf_status st = enqueue();
    if (st != SPF_OK) (void)hipStreamSynchronize(c->stream);
    return st;
}

// staged(), then c->out to the caller's `host_out`
template <class Work>
spf_status host_call(spf_ctx* c, std::initializer_list<HostIn> ins, size_t out_bytes, void* host_out, Work&& work)
{
    return staged(c, ins, out_bytes, [&]() -> spf_status {
        spf_status s = work();
        if (s != SPF_OK) return s;
        HIPCHK(c, hipMemcpyAsync(host_out, c->out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SPF_OK;
    });
}

// an operand of host_batch(): the caller's rows and the staging buffer they go to
struct HostRows {
    DevBuf& buf;
    const void* host;
};
// the rows of one operand or of the result as host_batch() and group_batch() hand them to their lambda, whose parameter names
// the element type (uint64_t words, or the doubles of a spectrum)
struct Rows {
    void* p;
    template <class T> operator T*() const { return static_cast<T*>(p); }
};

// host_call() for B items of `sh`: operand k of `ins` is B * sh.in_words[k] words, the result B * sh.out_words; `enqueue` gets
// the device pointers of the operands, in the order of `ins`, then that of the result.  B = 0 is SPF_OK and touches nothing.
template <class Enqueue>
spf_status host_batch(spf_ctx* c, const BatchShape& sh, size_t B, std::initializer_list<HostRows> ins, void* host_out, Enqueue&& enqueue)
{
    if (B == 0) return SPF_OK;
    const HostRows* o = ins.begin();
    const auto in = [&](size_t k) { return k < ins.size() ? HostIn{o[k].buf, o[k].host, B * sh.in_words[k] * 8} : HostIn{c->in, nullptr, 0}; };
    return host_call(c, {in(0), in(1), in(2)}, B * sh.out_words * 8, host_out, [&]() -> spf_status {
        const Rows out{c->out.p};
        if constexpr (std::is_invocable_v<Enqueue, Rows, Rows>) return enqueue(Rows{o[0].buf.p}, out);
        else if constexpr (std::is_invocable_v<Enqueue, Rows, Rows, Rows>) return enqueue(Rows{o[0].buf.p}, Rows{o[1].buf.p}, out);
        else return enqueue(Rows{o[0].buf.p}, Rows{o[1].buf.p}, Rows{o[2].buf.p}, out);
    });
}

spf_status batch_limit(spf_ctx* c, const BatchShape& sh, size_t B)
{
    return B > sh.max_batch ? fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large") : SPF_OK;
}

bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// whether the result of B items of `sh` at `out` overlaps their operand k at `in`
bool batch_overlaps(const BatchShape& sh, size_t B, const void* out, const void* in, int k = 0)
{
    return ranges_overlap(out, B * sh.out_words * 8, in, B * sh.in_words[k] * 8);
}

} // namespace

extern "C" {

void spf_default_params(spf_params* o)
{
    if (!o) return;
    *o = spf_params{637, 2048, 1, 16, 2, 4, 4, 2, 6, 7, 6, 3, 15};
}

// the build's identity: version, target, the compile-time options of the blind rotation as built
#define SPF_VSTR2(x) #x
#define SPF_VSTR(x) SPF_VSTR2(x)
const char* spf_version(void)
{
    return "spf_hip 0.6 gfx950"
           " (blind rotation: BR_OPT=" SPF_VSTR(SPF_BR_OPT) " BR_OPT_MIX=" SPF_VSTR(SPF_BR_OPT_MIX) " BR2_OPT=" SPF_VSTR(SPF_BR2_OPT)
#ifdef SPF_STAMPS
           " STAMPS"
#endif
#ifdef SPF_POOL_TRACE
           " POOL_TRACE"
#endif
           "; int8-MFMA keyswitch; cbs_radix CMUX; values by handle)";
}

// The text is copied into storage of the calling thread, so the pointer stays valid while other
// threads keep using (and failing on) the same context.
const char* spf_last_error(const spf_ctx* ctx)
{
    thread_local std::string copy;
    if (!ctx) return g_create_error.c_str();
    std::lock_guard<std::mutex> g(ctx->err_mu);
    copy = ctx->err;
    return copy.c_str();
}

// ---- GLWE keyswitch, automorphism round, trace (spf_glwe_keyswitch.hpp): which kernel a radix gets and what it needs

// the hand-written kernel's shape: N = 2048, k = 1 (a tuned context) at 6 levels x 7 bits
static bool glwe_ks_tuned(const spf_ctx* c, uint32_t radix_log, uint32_t radix_count) { return !c->generic && radix_log == 7 && radix_count == 6; }

// why a radix is refused, with its numbers, or empty
static std::string glwe_ks_radix_error(uint32_t radix_log, uint32_t radix_count)
{
    const std::string r = "radix_log " + std::to_string(radix_log) + ", radix_count " + std::to_string(radix_count);
    if (radix_log == 0 || radix_count == 0) return r + ": a radix decomposition needs radix_log >= 1 and radix_count >= 1";
    if ((uint64_t)radix_log * radix_count > 64) return r + ": radix_log * radix_count = " + std::to_string((uint64_t)radix_log * radix_count) + " > 64";
    if ((uint64_t)radix_log * radix_count == 64)
        return r + ": radix_log * radix_count = 64; the kernels round to the top radix_log * radix_count bits by the bit below them and need at most 63";
    return "";
}

// what generic_glwe_ks_kernel needs on a tuned context: the generic twist table e^{+2 pi i j / (2N)} (shared with the public
// functional keyswitch) and the launch attribute.  Synchronous (a table copy): called from spf_create and from a key load only.
static spf_status glwe_ks_prepare_generic(spf_ctx* c)
{
    if (c->glwe_ks_generic_ready) return SPF_OK;
    const uint32_t N = c->prm.polynomial_degree, h = N / 2;
    if (generic_trace_lds_bytes(N, c->prm.glwe_size) > 160 * 1024)
        return fail(c, SPF_ERR_UNSUPPORTED, "(k+1) polynomials of this degree do not fit the generic kernels' LDS");
    if (!c->d_gen_tables) {
        std::vector<c64> gt(h);
        for (uint32_t j = 0; j < h; j++) gt[j] = root_of_unity(j, 2 * (uint64_t)N);
        HIPCHK(c, hipMalloc((void**)&c->d_gen_tables, gt.size() * sizeof(c64)));
        HIPCHK(c, hipMemcpy(c->d_gen_tables, gt.data(), gt.size() * sizeof(c64), hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_glwe_ks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)generic_trace_lds_bytes(N, c->prm.glwe_size)));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_glwe_ks_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)generic_trace_lds_bytes(N, c->prm.glwe_size)));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_glwe_ks_each_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)generic_trace_lds_bytes(N, c->prm.glwe_size)));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_ring_pack_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)generic_trace_lds_bytes(N, c->prm.glwe_size)));
    c->glwe_ks_generic_ready = true;
    return SPF_OK;
}

spf_status spf_create(const spf_params* params, int device_id, spf_ctx** out)
{
    if (!params || !out) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::string why, why_generic;
    const bool specialised = params_supported(*params, why);
    if (!specialised && !params_generic(*params, why_generic))
        return fail(nullptr, SPF_ERR_UNSUPPORTED, why_generic);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, SPF_ERR_HIP, "no HIP device visible: the HIP path is the only path, there is no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "device_id out of range");
    spf_ctx* c = new (std::nothrow) spf_ctx();
    if (!c) return fail(nullptr, SPF_ERR_HIP, "out of host memory");
    c->prm = *params;
    c->device = device_id;
    c->generic = !specialised;
    c->log_n = ceil_log2(params->polynomial_degree);
    auto bail = [&](spf_status s) { g_create_error = c->err; spf_destroy(c); return s; };
#define CK(expr)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            c->err = std::string(#expr) + ": " + hipGetErrorString(e_);                           \
            return bail(SPF_ERR_HIP);                                                             \
        }                                                                                         \
    } while (0)
    CK(hipSetDevice(device_id));
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    {
        int cu = 0;
        CK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device_id));
        if (cu > 0) c->n_cu = cu;
    }
    std::vector<c64> t;
    build_tables(t);
    CK(hipMalloc((void**)&c->d_tables, kTableBytes));
    CK(hipMemcpy(c->d_tables, t.data(), kTableBytes, hipMemcpyHostToDevice));
    // fill_multifunctional_cbs_decomposition_lut (circuit_bootstrapping.rs:430-482)
    {
        std::vector<uint64_t> lut(glwe_words(*params), 0);
        uint64_t levels[16] = {0};
        for (uint32_t i = 0; i < 16; i++) {
            uint32_t lvl = i + 1;
            if (lvl * params->cbs_radix_log + 1 < 64) {
                uint32_t bits = params->cbs_radix_log * lvl + 1;
                uint64_t minus_one = ((uint64_t)1 << bits) - 1;
                levels[i] = minus_one << (64 - bits);
            }
        }
        uint32_t v = 1u << ceil_log2(params->cbs_radix_count);
        uint64_t* b = lut.data() + (size_t)params->glwe_size * params->polynomial_degree;
        for (uint32_t i = 0; i < params->polynomial_degree; i++) {
            uint32_t fn = i % v;
            b[i] = fn < params->cbs_radix_count ? levels[fn] : 0;
        }
        CK(hipMalloc((void**)&c->d_cbs_lut, lut.size() * 8));
        CK(hipMemcpy(c->d_cbs_lut, lut.data(), lut.size() * 8, hipMemcpyHostToDevice));
    }
    if (c->generic) {
        // twist e^{+2 pi i j / (2N)} and transform twiddles e^{+2 pi i j / (N/2)}: the oracle's definitions for N != 2048
        const uint32_t N = params->polynomial_degree, h = N / 2;
        std::vector<c64> gt(h + h / 2);
        for (uint32_t j = 0; j < h; j++) gt[j] = root_of_unity(j, 2 * (uint64_t)N);
        for (uint32_t j = 0; j < h / 2; j++) gt[h + j] = root_of_unity(j, h);
        CK(hipMalloc((void**)&c->d_gen_tables, gt.size() * sizeof(c64)));
        CK(hipMemcpy(c->d_gen_tables, gt.data(), gt.size() * sizeof(c64), hipMemcpyHostToDevice));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_pbs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_lds_bytes(N, params->glwe_size, true)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_cmux_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_lds_bytes(N, params->glwe_size, false)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_cmux_rot_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_lds_bytes(N, params->glwe_size, false)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_trace_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_trace_lds_bytes(N, params->glwe_size)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_scheme_switch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_lds_bytes(N, params->glwe_size, false)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_glwe_ks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_trace_lds_bytes(N, params->glwe_size)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_glwe_ks_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_trace_lds_bytes(N, params->glwe_size)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_glwe_ks_each_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_trace_lds_bytes(N, params->glwe_size)));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_ring_pack_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)generic_trace_lds_bytes(N, params->glwe_size)));
        c->glwe_ks_generic_ready = true;
        *out = c;
        return SPF_OK;
    }
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ks_gemm_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                           kKsLdsBytes));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&blind_rotate2p_kernel<2, 16, SPF_BR_OPT_MIX, 1>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kBlindRotate2pLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&blind_rotate2p_kernel<2, 16, SPF_BR_OPT, 0>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kBlindRotate2pLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&blind_rotate2p2_kernel<2, 16, SPF_BR2_OPT, 1>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kBlindRotate2p2Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&blind_rotate2p2_kernel<2, 16, SPF_BR2_OPT, 0>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kBlindRotate2p2Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&blind_rotate8_kernel<2, 16, 1>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kBlindRotate8Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&blind_rotate8_kernel<2, 16, 0>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kBlindRotate8Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux_kernel<4, 4, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                           cmux_lds_bytes(2)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux_kernel<4, 4, 2>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(2)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux4_kernel<4, 4>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kCmux4Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux_kernel<4, 4, 2, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                           cmux_lds_bytes(2)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux_kernel<4, 4, 2, false, true>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(2)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux4_kernel<4, 4, true>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kCmux4Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux_rot_scattered_kernel<4, 4, 2>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(2)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cmux4_rot_scattered_kernel<4, 4>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kCmux4Lds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cbs_trace_kernel<6, 7>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&scheme_switch_kernel<15, 3>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_kernel<6, 7, GLWE_KS_TRACE>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_kernel<6, 7, GLWE_KS_AUTOMORPHISM>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_kernel<6, 7, GLWE_KS_KEYSWITCH>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_rows_kernel<6, 7, GLWE_KS_TRACE>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_rows_kernel<6, 7, GLWE_KS_AUTOMORPHISM>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_rows_kernel<6, 7, GLWE_KS_KEYSWITCH>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_each_kernel<6, 7, GLWE_KS_AUTOMORPHISM>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&glwe_ks_each_kernel<6, 7, GLWE_KS_KEYSWITCH>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ring_pack_kernel<6, 7, true>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ring_pack_kernel<6, 7, false>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, kTraceLds));
#undef CK
    // an automorphism key of another radix than the hand-written kernel's: spf_glwe_automorphism_* / spf_glwe_trace_* run the
    // generic kernel (the *_enqueue forms only enqueue: its table is made here)
    if (!glwe_ks_tuned(c, params->tr_radix_log, params->tr_radix_count) &&
        glwe_ks_radix_error(params->tr_radix_log, params->tr_radix_count).empty() && glwe_ks_prepare_generic(c) != SPF_OK)
        return bail(SPF_ERR_HIP);
    *out = c;
    return SPF_OK;
}

spf_status spf_live_objects(spf_live_counts* out)
{
    if (!out) return SPF_ERR_INVALID_ARGUMENT;
    auto n = [](spf_live::Kind k) { return spf_live::g_count[k].load(std::memory_order_relaxed); };
    out->contexts = n(spf_live::CTX);
    out->groups = n(spf_live::GROUP);
    out->graphs = n(spf_live::GRAPH);
    out->pools = n(spf_live::POOL);
    out->values = n(spf_live::VALUE);
    return SPF_OK;
}

// Lifetimes (include/spf_hip.h): a child keeps its parent alive.  A graph and a pool retain their context, a group its members'
// contexts; the streams and the device memory go with the last reference, whoever drops it.
static void ctx_retain(spf_ctx* c) { c->refs.fetch_add(1, std::memory_order_relaxed); }
static void ctx_release(spf_ctx* c)
{
    if (!c || c->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& v : c->timed)
        for (auto& t : v) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    for (void* p : {(void*)c->d_tables, (void*)c->d_bsk, (void*)c->d_bsk_scaled, (void*)c->d_ksk, (void*)c->d_cbs_lut,
                    c->in.p, c->out.p, c->mid.p, c->aux.p, c->packed.p, c->unpack_l1.p, c->unpack_l0.p, c->brot_mid.p, c->brot_high.p, (void*)c->d_ksk_planes,
                    c->scr.ks_dig.p, c->scr.ks_rowsum.p, (void*)c->d_ak, (void*)c->d_ssk, c->scr.cbs_glwe.p, c->scr.cbs_glev.p, (void*)c->d_gen_tables,
                    (void*)c->d_pufks, c->pufks_dig.p, (void*)c->d_pfks, (void*)c->d_pfks_planes, c->pfks_dig.p, c->pfks_rowsum.p, c->pfks_glwe.p,
                    c->pfks_lwe.p, c->lin_planes.p, c->each_tab.p, c->ring_pack_scratch.p})
        if (p) (void)hipFree(p);
    if (c->each_ev) { (void)hipEventSynchronize(c->each_ev); (void)hipEventDestroy(c->each_ev); }
    if (c->each_host) (void)hipHostFree(c->each_host);
    for (LweLinearSlot& l : c->lin)
        for (void* p : {(void*)l.d_w, (void*)l.d_bias, (void*)l.d_A, (void*)l.d_rs})
            if (p) (void)hipFree(p);
    for (GlwePolySlot& l : c->gpoly)
        for (void* p : {(void*)l.d_offsets, (void*)l.d_terms, (void*)l.d_scalars, (void*)l.d_bias})
            if (p) (void)hipFree(p);
    for (GlweKskSlot& l : c->gksk)
        if (l.d_key) (void)hipFree(l.d_key);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->d_ggsw_const) (void)hipFree(c->d_ggsw_const);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (hipEvent_t e : c->slice_ev) (void)hipEventDestroy(e);
    delete c;
}

void spf_destroy(spf_ctx* c) { ctx_release(c); }

// The blind-rotation kernels read a copy of the bootstrap key scaled by 2^-10 (the 1/N of the inverse transform travels with
// the key through the multiply-accumulate: exact, and 32 multiplications per polynomial and step are not executed).  Built
// whenever the caller's image is complete; a value no forward transform of a torus polynomial produces (NaN, non-zero magnitude
// outside [2^-900, 2^1000)), where scaling first could round differently from scaling last, makes the key unusable instead.
static spf_status finish_bootstrap_key(spf_ctx* c)
{
    if (c->generic) return SPF_OK; // (the generic kernels read the caller's spectra as they are)
    c->bsk_ready = false;
    const size_t n_complex = (size_t)c->prm.lwe_dimension * ggsw_fft_complex(c->prm, c->prm.pbs_radix_count);
    if (!c->d_bsk_scaled) HIPCHK(c, hipMalloc((void**)&c->d_bsk_scaled, n_complex * sizeof(c64)));
    spf_status st = ensure(c, c->aux, sizeof(unsigned int));
    if (st != SPF_OK) return st;
    unsigned int* d_bad = (unsigned int*)c->aux.p;
    HIPCHK(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(scale_bootstrap_key_kernel, dim3(4 * (unsigned)c->n_cu), dim3(256), 0, c->stream,
                       (const double*)c->d_bsk, (double*)c->d_bsk_scaled, 2 * n_complex, d_bad);
    HIPCHK(c, hipGetLastError());
    unsigned int bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad)
        return fail(c, SPF_ERR_INVALID_ARGUMENT,
                    "bootstrap key holds a value that is no forward transform of a torus polynomial (NaN, or a non-zero magnitude outside [2^-900, 2^1000))");
    return SPF_OK;
}

// ---- public functional keyswitch: the key's shape and what a context needs besides the key

static size_t pufks_complex(const spf_params& p, uint32_t n, uint32_t count)
{
    return (size_t)n * count * (p.glwe_size + 1) * (p.polynomial_degree / 2);
}

// the hand-written kernel's shapes: N = 2048, k = 1 (a tuned context) at 4 bits x 8 or 4 bits x 4
static bool pufks_tuned(const spf_ctx* c) { return !c->generic && c->pufks_log == 4 && (c->pufks_count == 8 || c->pufks_count == 4); }

// why (from_dimension, radix) is refused, or nullptr
static const char* pufks_key_shape_error(size_t from_dimension, uint32_t radix_log, uint32_t radix_count)
{
    if (from_dimension == 0) return "from_dimension must be at least 1";
    if (radix_log == 0 || radix_count == 0 || (uint64_t)radix_log * radix_count >= 64) return "a radix decomposition needs 1 <= radix_log * count < 64";
    if (from_dimension > 0x0fffffffu / radix_count) return "from_dimension * radix_count above 0x0fffffff";
    return nullptr;
}

// what the kernels of this key's shape need on this context besides the key: launch attributes, and on a tuned context that
// runs the generic kernel the generic twist table e^{+2 pi i j / (2N)}
static spf_status pufks_prepare(spf_ctx* c)
{
    if (pufks_tuned(c)) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&pufks_kernel<4, 8, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(2)));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&pufks_kernel<4, 8, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(4)));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&pufks_kernel<4, 4, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(2)));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&pufks_kernel<4, 4, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, cmux_lds_bytes(4)));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&pufks4_kernel<4, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, kPufks4Lds));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&pufks4_kernel<4, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, kPufks4Lds));
        return SPF_OK;
    }
    const uint32_t N = c->prm.polynomial_degree, h = N / 2;
    if (generic_lds_bytes(N, c->prm.glwe_size, false) > 160 * 1024)
        return fail(c, SPF_ERR_UNSUPPORTED, "(k+1) polynomials of this degree do not fit the generic kernels' LDS");
    if (!c->d_gen_tables) {
        std::vector<c64> gt(h);
        for (uint32_t j = 0; j < h; j++) gt[j] = root_of_unity(j, 2 * (uint64_t)N);
        HIPCHK(c, hipMalloc((void**)&c->d_gen_tables, gt.size() * sizeof(c64)));
        HIPCHK(c, hipMemcpy(c->d_gen_tables, gt.data(), gt.size() * sizeof(c64), hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&generic_pufks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)generic_lds_bytes(N, c->prm.glwe_size, false)));
    return SPF_OK;
}

// ---- private functional keyswitch: the keys' shape and what a context derives from them (spf_pfks.hpp)

constexpr size_t kPfksDigitCap = (size_t)1 << 30; // bytes of limb scratch one launch may use; larger batches go in several launches

static size_t pfks_row_words(const spf_ctx* c) { return (size_t)c->pfks_p * ((size_t)c->pfks_n + 1); }
static size_t pfks_K(const spf_ctx* c) { return pfks_row_words(c) * c->pfks_count; }
static size_t pfks_Kpad(const spf_ctx* c) { return (pfks_K(c) + 127) & ~(size_t)127; }

// why a key set of this shape is refused, or nullptr; *words receives n_keys * lwe_count * (n+1) * count * (k+1) * N
static const char* pfks_key_shape_error(const spf_params& p, size_t n_keys, size_t from_dimension, size_t lwe_count, uint32_t radix_log,
                                        uint32_t radix_count, size_t* words)
{
    if (n_keys == 0 || from_dimension == 0 || lwe_count == 0) return "n_keys, from_dimension and lwe_count must be at least 1";
    if (radix_log == 0 || radix_count == 0 || (uint64_t)radix_log * radix_count >= 64) return "a radix decomposition needs 1 <= radix_log * count < 64";
    const size_t W = glwe_words(p), lim = 0x7fffff00u;
    if (n_keys > 65535 || n_keys > lim / (8 * W)) return "n_keys * (k+1) * N above the index range";
    if (from_dimension >= lim || lwe_count > lim / (from_dimension + 1) || lwe_count * (from_dimension + 1) > lim / radix_count)
        return "lwe_count * (from_dimension + 1) * radix_count above 0x7fffff00";
    const size_t K = lwe_count * (from_dimension + 1) * radix_count;
    if (K > ((size_t)1 << 60) / (n_keys * W)) return "the key set is too large";
    *words = n_keys * K * W;
    return nullptr;
}

// the byte planes of the keys in the blob, where the matrix-core path takes them: radix_log <= 23 and a tile of 128 rows of limbs
// within the scratch cap.  Everything else is served from the words by pfks_valu_kernel.
static spf_status pfks_prepare(spf_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->d_pfks_planes) {
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, hipFree(c->d_pfks_planes));
        c->d_pfks_planes = nullptr;
    }
    const uint32_t U = pfks_limbs(c->pfks_log);
    const size_t K = pfks_K(c), Kpad = pfks_Kpad(c), W = glwe_words(c->prm);
    if (U == 0 || (size_t)PFKS_TILE * Kpad * U > kPfksDigitCap) return SPF_OK;
    const size_t npad = ((8 * (size_t)c->pfks_keys * W + 127) & ~(size_t)127) + PFKS_TILE; // a tile may start at any key's first plane row
    HIPCHK(c, hipMalloc((void**)&c->d_pfks_planes, npad * Kpad));
    HIPCHK(c, hipMemsetAsync(c->d_pfks_planes, 0, npad * Kpad, c->stream));
    hipLaunchKernelGGL(pfks_planes_kernel, dim3((unsigned)(Kpad / 32), (unsigned)((W + 31) / 32), c->pfks_keys), dim3(256), 0, c->stream,
                       c->d_pfks, c->d_pfks_planes, c->pfks_count, (uint32_t)W, (uint32_t)K, (uint32_t)Kpad);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPF_OK;
}

spf_status spf_key_blob(spf_ctx* c, int which, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr || !bytes) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (which == 0) {
        size_t need = (size_t)c->prm.lwe_dimension * ggsw_fft_complex(c->prm, c->prm.pbs_radix_count) * sizeof(c64);
        if (!c->d_bsk) { HIPCHK(c, hipMalloc((void**)&c->d_bsk, need)); c->bsk_bytes = need; }
        *dev_ptr = c->d_bsk; *bytes = c->bsk_bytes;
    } else if (which == 1) {
        size_t need = (size_t)c->prm.glwe_size * c->prm.polynomial_degree * c->prm.ks_radix_count * lwe0_words(c->prm) * 8;
        if (!c->d_ksk) { HIPCHK(c, hipMalloc((void**)&c->d_ksk, need)); c->ksk_bytes = need; }
        *dev_ptr = c->d_ksk; *bytes = c->ksk_bytes;
    } else if (which == 2) {
        size_t need = ak_complex(c->prm) * sizeof(c64);
        if (!c->d_ak) { HIPCHK(c, hipMalloc((void**)&c->d_ak, need)); c->ak_bytes = need; }
        *dev_ptr = c->d_ak; *bytes = c->ak_bytes;
    } else if (which == 3) {
        size_t need = ssk_complex(c->prm) * sizeof(c64);
        if (!c->d_ssk) { HIPCHK(c, hipMalloc((void**)&c->d_ssk, need)); c->ssk_bytes = need; }
        *dev_ptr = c->d_ssk; *bytes = c->ssk_bytes;
    } else if (which == 4) {
        // the shape of this key is not in spf_params: it is known once a load (here, or on member 0 of a group) has stated it
        if (!c->pufks_n) return fail(c, SPF_ERR_NO_KEY, "the public functional keyswitch key has no shape yet: load one first");
        size_t need = pufks_complex(c->prm, c->pufks_n, c->pufks_count) * sizeof(c64);
        if (c->d_pufks && c->pufks_bytes != need) { // another shape than the blob was made for
            c->pufks_ready = false;
            HIPCHK(c, hipDeviceSynchronize());
            HIPCHK(c, hipFree(c->d_pufks));
            c->d_pufks = nullptr; c->pufks_bytes = 0;
        }
        if (!c->d_pufks) { HIPCHK(c, hipMalloc((void**)&c->d_pufks, need)); c->pufks_bytes = need; }
        *dev_ptr = c->d_pufks; *bytes = c->pufks_bytes;
    } else if (which == 5) {
        // as for 4: the shape comes with a load
        if (!c->pfks_keys) return fail(c, SPF_ERR_NO_KEY, "the private functional keyswitch keys have no shape yet: load them first");
        size_t need = (size_t)c->pfks_keys * pfks_K(c) * glwe_words(c->prm) * 8;
        if (c->d_pfks && c->pfks_bytes != need) {
            c->pfks_ready = false;
            HIPCHK(c, hipDeviceSynchronize());
            HIPCHK(c, hipFree(c->d_pfks));
            c->d_pfks = nullptr; c->pfks_bytes = 0;
        }
        if (!c->d_pfks) { HIPCHK(c, hipMalloc((void**)&c->d_pfks, need)); c->pfks_bytes = need; }
        *dev_ptr = c->d_pfks; *bytes = c->pfks_bytes;
    } else {
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "which must be 0 (bootstrap), 1 (keyswitch), 2 (automorphism), 3 (scheme switch), "
                                                 "4 (public functional keyswitch) or 5 (private functional keyswitch)");
    }
    return SPF_OK;
}

spf_status spf_key_blob_commit(spf_ctx* c, int which)
{
    if (!c) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device)); // the byte planes are allocated and built on THIS context's GPU
    // Whatever filled the blob (a copy on the caller's stream, an RCCL broadcast on its own) must have landed before the derived
    // images are built from it on this context's stream, which is ordered with no other stream: once per key load.
    HIPCHK(c, hipDeviceSynchronize());
    if (which == 0 && c->d_bsk) {
        spf_status st = finish_bootstrap_key(c);
        if (st != SPF_OK) return st;
        c->bsk_ready = true, c->ggsw_const_ready = false;
    }
    else if (which == 1 && c->d_ksk) {
        spf_status st = build_ks_planes(c);
        if (st != SPF_OK) return st;
        c->ksk_ready = true;
    }
    else if (which == 2 && c->d_ak) c->ak_ready = true, c->ggsw_const_ready = false;
    else if (which == 3 && c->d_ssk) c->ssk_ready = true, c->ggsw_const_ready = false;
    else if (which == 4 && c->d_pufks) {
        spf_status st = pufks_prepare(c);
        if (st != SPF_OK) return st;
        c->pufks_ready = true;
    }
    else if (which == 5 && c->d_pfks) {
        c->pfks_ready = false;
        spf_status st = pfks_prepare(c);
        if (st != SPF_OK) return st;
        c->pfks_ready = true;
    }
    else return fail(c, SPF_ERR_INVALID_ARGUMENT, "blob not allocated");
    return SPF_OK;
}

spf_status spf_load_bootstrap_key(spf_ctx* c, const double* bsk_fft, size_t n_complex)
{
    if (!c || !bsk_fft) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    size_t want = (size_t)c->prm.lwe_dimension * ggsw_fft_complex(c->prm, c->prm.pbs_radix_count);
    if (n_complex != want)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "bootstrap key length " + std::to_string(n_complex) + " != " + std::to_string(want));
    void* p; size_t bytes;
    spf_status s = spf_key_blob(c, 0, &p, &bytes);
    if (s != SPF_OK) return s;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    c->bsk_ready = false;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(p, bsk_fft, bytes, hipMemcpyHostToDevice));
    {
        spf_status st = finish_bootstrap_key(c);
        if (st != SPF_OK) return st;
    }
    c->bsk_ready = true, c->ggsw_const_ready = false;
    return SPF_OK;
}

spf_status spf_load_keyswitch_key(spf_ctx* c, const uint64_t* ksk, size_t n_words)
{
    if (!c || !ksk) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    size_t want = (size_t)c->prm.glwe_size * c->prm.polynomial_degree * c->prm.ks_radix_count * lwe0_words(c->prm);
    if (n_words != want)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "keyswitch key length " + std::to_string(n_words) + " != " + std::to_string(want));
    void* p; size_t bytes;
    spf_status s = spf_key_blob(c, 1, &p, &bytes);
    if (s != SPF_OK) return s;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(p, ksk, bytes, hipMemcpyHostToDevice));
    spf_status st = build_ks_planes(c);
    if (st != SPF_OK) return st;
    c->ksk_ready = true;
    return SPF_OK;
}

// ---------------------------------------------------------------- device buffers for callers without a HIP binding
// (a Rust shim that chains the `_dev` entry points keeps its ciphertexts in HBM between calls; these four spare it a
// HIP binding of its own.  Plain hipMalloc / hipMemcpy on the context's device.)

spf_status spf_device_alloc(spf_ctx* c, size_t bytes, void** dev_ptr)
{
    if (!c || !dev_ptr) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    *dev_ptr = nullptr;
    if (bytes == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(dev_ptr, bytes));
    return SPF_OK;
}

spf_status spf_device_free(spf_ctx* c, void* dev_ptr)
{
    if (!c) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null context");
    if (!dev_ptr) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipFree(dev_ptr));
    return SPF_OK;
}

spf_status spf_device_upload(spf_ctx* c, void* dev_dst, const void* host_src, size_t bytes)
{
    if (!c || (bytes && (!dev_dst || !host_src))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return SPF_OK;
}

spf_status spf_device_download(spf_ctx* c, void* stream, void* host_dst, const void* dev_src, size_t bytes)
{
    if (!c || (bytes && (!host_dst || !dev_src))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream)); // what was enqueued on `stream` has written dev_src
    if (bytes) HIPCHK(c, hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return SPF_OK;
}

// ---------------------------------------------------------------- device-pointer forms

spf_status spf_keyswitch_lwe_l1_lwe_l0_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_in, uint64_t* d_out)
{
    if (!c || (B && (!d_in || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_keyswitch(c, (hipStream_t)stream, B, d_in, d_out);
}

spf_status spf_generalized_pbs_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_lwe, const uint64_t* d_lut,
                                   size_t lut_stride, uint32_t log_chi, uint32_t log_v, uint64_t body_rotate,
                                   uint64_t* d_out)
{
    if (!c || (B && (!d_lwe || !d_lut || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_blind_rotate(c, (hipStream_t)stream, B, d_lwe, d_lut, lut_stride, log_chi, log_v, body_rotate, d_out,
                               glwe_words(c->prm), false);
}

spf_status spf_pbs_univariate_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_lwe, const uint64_t* d_lut,
                                  size_t lut_stride, uint64_t* d_out)
{
    if (!c || (B && (!d_lwe || !d_lut || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_blind_rotate(c, (hipStream_t)stream, B, d_lwe, d_lut, lut_stride, 0, 0, 0, d_out, lwe1_words(c->prm), true);
}

// d_out = d_left * 2^plaintext_bits + d_right over B level-0 LWEs (lwe_pack_kernel; d_out may be d_left)
static spf_status launch_lwe_pack(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_left, const uint64_t* d_right,
                                  uint32_t plaintext_bits, uint64_t* d_out)
{
    const size_t words = B * lwe0_words(c->prm);
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 4 * (size_t)c->n_cu);
    hipLaunchKernelGGL(lwe_pack_kernel, dim3(blocks), dim3(256), 0, s, d_left, d_right, d_out, words, (uint64_t)1 << plaintext_bits);
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// the same with row b of either operand at d_left[b] / d_right[b] (device tables of device pointers; lwe_pack_rows_kernel).  At most
// one workgroup per CU: a level of a graph is a few hundred rows of a few KiB
static spf_status launch_lwe_pack_rows(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* const* d_left, const uint64_t* const* d_right,
                                       uint32_t plaintext_bits, uint64_t* d_out)
{
    const size_t words = lwe0_words(c->prm), items = B * ((words + 255) / 256);
    if (items == 0) return SPF_OK;
    const unsigned blocks = (unsigned)std::min<size_t>(items, (size_t)c->n_cu);
    hipLaunchKernelGGL(lwe_pack_rows_kernel, dim3(blocks), dim3(256), 0, s, d_left, d_right, d_out, B, (uint32_t)words,
                       (uint64_t)1 << plaintext_bits);
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// programmable_bootstrap_bivariate (programmable_bootstrapping.rs:575-621): pack into the context's buffer, then the
// univariate bootstrap of the packed input
spf_status spf_pbs_bivariate_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_left, const uint64_t* d_right,
                                 const uint64_t* d_lut, size_t lut_stride, uint32_t plaintext_bits, uint64_t* d_out)
{
    if (!c || (B && (!d_left || !d_right || !d_lut || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (plaintext_bits >= 64) return fail(c, SPF_ERR_INVALID_ARGUMENT, "plaintext_bits must be below 64");
    if (B == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->bsk_ready) return fail(c, SPF_ERR_NO_KEY, "bootstrap key not loaded");
    if (B > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    spf_status st = ensure(c, c->packed, B * lwe0_words(c->prm) * 8);
    if (st != SPF_OK) return st;
    uint64_t* d_packed = (uint64_t*)c->packed.p;
    st = launch_lwe_pack(c, (hipStream_t)stream, B, d_left, d_right, plaintext_bits, d_packed);
    if (st != SPF_OK) return st;
    return launch_blind_rotate(c, (hipStream_t)stream, B, d_packed, d_lut, lut_stride, 0, 0, 0, d_out, lwe1_words(c->prm), true);
}

spf_status spf_circuit_bootstrap_pbs_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_lwe, uint64_t* d_out)
{
    if (!c || (B && (!d_lwe || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    // hi_noise_lwe_to_lo_noise_glwe (circuit_bootstrapping.rs:387-427)
    return launch_blind_rotate(c, (hipStream_t)stream, B, d_lwe, c->d_cbs_lut, 0, 0, ceil_log2(c->prm.cbs_radix_count),
                               (uint64_t)1 << 62, d_out, glwe_words(c->prm), false);
}

// the circuit-bootstrap tail launches cbs_radix_count units per ciphertext
static spf_status tail_batch_args(spf_ctx* c, size_t B)
{
    return B > kBatchMaxRows ? fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large") : SPF_OK;
}

static spf_status tail_supported(spf_ctx* c)
{
    const spf_params& p = c->prm;
    if (c->generic) return SPF_OK; // (generic_trace_kernel / generic_scheme_switch_kernel take any radix)
    if (p.cbs_radix_log != 4 || p.cbs_radix_count != 4 || p.tr_radix_log != 7 || p.tr_radix_count != 6 ||
        p.ss_radix_log != 3 || p.ss_radix_count != 15)
        return fail(c, SPF_ERR_UNSUPPORTED, "circuit-bootstrap tail is built for cbs 4x4, tr 6x7, ss 15x3 bits");
    return SPF_OK;
}

static spf_status launch_trace(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_glwe, uint64_t* d_glev)
{
    if (!c->ak_ready) return fail(c, SPF_ERR_NO_KEY, "automorphism key not loaded");
    if (c->generic) {
        GenericTraceArgs ga{};
        ga.g = generic_shape(c);
        ga.glwe_in = d_glwe; ga.glev_out = d_glev; ga.ak = c->d_ak;
        ga.units = (uint32_t)(B * c->prm.cbs_radix_count); ga.cbs_count = c->prm.cbs_radix_count; ga.cbs_radix_log = c->prm.cbs_radix_log;
        ga.tr_radix_log = c->prm.tr_radix_log; ga.tr_count = c->prm.tr_radix_count;
        hipLaunchKernelGGL(generic_trace_kernel, dim3(ga.units), dim3(kGenericThreads), generic_trace_lds_bytes(ga.g.N, ga.g.k), s, ga);
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    TraceArgs a{};
    a.glwe_in = d_glwe; a.glev_out = d_glev; a.ak = c->d_ak; a.tables = c->d_tables;
    a.units = (uint32_t)(B * c->prm.cbs_radix_count); a.cbs_count = c->prm.cbs_radix_count;
    a.cbs_radix_log = c->prm.cbs_radix_log;
    dim3 grid((a.units + kWavesPerBlock - 1) / kWavesPerBlock), block(512);
    auto launch = [&](uint64_t* stamps) -> spf_status { // (`stamps`: the diagnostic build's phase buffer, otherwise null)
        a.stamps = stamps;
        TimedScope ts(c, s, T_TRACE);
        spf_status st = ts.begin();
        if (st != SPF_OK) return st;
        hipLaunchKernelGGL((cbs_trace_kernel<6, 7>), grid, block, kTraceLds, s, a);
        HIPCHK(c, hipGetLastError());
        return ts.end();
    };
#ifdef SPF_STAMPS
    static int reported_t = 0;
    if (reported_t < 1 && a.units >= 4096) { // the first large launch reports, per automorphism round
        reported_t++;
        const size_t waves = (size_t)grid.x * 8;
        fprintf(stderr, "[trace stamps] per automorphism round, median over %zu waves (cycles | waves 0-3 | waves 4-7)\n", waves);
        return stamp_report(c, s, waves, kStampNamesTrace, 10, 11.0, false, true, "[trace stamps] %-48s", "[trace stamps] total %.0f\n", launch);
    }
#endif
    return launch(nullptr);
}

static spf_status launch_scheme_switch(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_glev, double* d_ggsw)
{
    if (!c->ssk_ready) return fail(c, SPF_ERR_NO_KEY, "scheme-switch key not loaded");
    if (c->generic) {
        GenericSchemeSwitchArgs ga{};
        ga.g = generic_shape(c);
        ga.glev = d_glev; ga.ggsw_out = reinterpret_cast<c64*>(d_ggsw); ga.ssk = c->d_ssk;
        ga.units = (uint32_t)(B * c->prm.cbs_radix_count); ga.cbs_count = c->prm.cbs_radix_count;
        ga.ss_radix_log = c->prm.ss_radix_log; ga.ss_count = c->prm.ss_radix_count;
        hipLaunchKernelGGL(generic_scheme_switch_kernel, dim3(ga.units), dim3(kGenericThreads), generic_lds_bytes(ga.g.N, ga.g.k, false), s, ga);
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    SchemeSwitchArgs a{};
    a.glev = d_glev; a.ggsw_out = reinterpret_cast<c64*>(d_ggsw); a.ssk = c->d_ssk; a.tables = c->d_tables;
    a.units = (uint32_t)(B * c->prm.cbs_radix_count); a.cbs_count = c->prm.cbs_radix_count;
    dim3 grid((a.units + kWavesPerBlock - 1) / kWavesPerBlock), block(512);
    TimedScope ts(c, s, T_SS);
    spf_status st = ts.begin();
    if (st != SPF_OK) return st;
    hipLaunchKernelGGL((scheme_switch_kernel<15, 3>), grid, block, kTraceLds, s, a);
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

spf_status spf_mod_switch_trace_and_rotate_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe, uint64_t* d_glev)
{
    if (!c || (B && (!d_glwe || !d_glev))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    spf_status st = tail_batch_args(c, B);
    if (st != SPF_OK) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    st = tail_supported(c);
    if (st != SPF_OK) return st;
    return launch_trace(c, (hipStream_t)stream, B, d_glwe, d_glev);
}

spf_status spf_scheme_switch_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glev, double* d_ggsw)
{
    if (!c || (B && (!d_glev || !d_ggsw))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    spf_status st = tail_batch_args(c, B);
    if (st != SPF_OK) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    st = tail_supported(c);
    if (st != SPF_OK) return st;
    return launch_scheme_switch(c, (hipStream_t)stream, B, d_glev, d_ggsw);
}

// circuit_bootstrap_via_trace_and_scheme_switch (circuit_bootstrapping.rs:342-385) on `s`, intermediates in `sc`
static spf_status circuit_bootstrap_chain(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_lwe, double* d_ggsw, Scratch* sc,
                                          int per_wg_hint)
{
    spf_status st = tail_supported(c);
    if (st != SPF_OK) return st;
    st = ensure(c, sc->cbs_glwe, B * glwe_words(c->prm) * 8);
    if (st != SPF_OK) return st;
    st = ensure(c, sc->cbs_glev, B * c->prm.cbs_radix_count * glwe_words(c->prm) * 8);
    if (st != SPF_OK) return st;
    st = launch_blind_rotate(c, s, B, d_lwe, c->d_cbs_lut, 0, 0, ceil_log2(c->prm.cbs_radix_count), (uint64_t)1 << 62,
                             (uint64_t*)sc->cbs_glwe.p, glwe_words(c->prm), false, per_wg_hint);
    if (st != SPF_OK) return st;
    st = launch_trace(c, s, B, (const uint64_t*)sc->cbs_glwe.p, (uint64_t*)sc->cbs_glev.p);
    if (st != SPF_OK) return st;
    return launch_scheme_switch(c, s, B, (const uint64_t*)sc->cbs_glev.p, d_ggsw);
}

spf_status spf_circuit_bootstrap_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_lwe, double* d_ggsw)
{
    if (!c || (B && (!d_lwe || !d_ggsw))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    spf_status st = tail_batch_args(c, B);
    if (st != SPF_OK) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return circuit_bootstrap_chain(c, (hipStream_t)stream, B, d_lwe, d_ggsw, &c->scr, 0);
}

spf_status spf_sample_extract_l1_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe, size_t idx, uint64_t* d_out)
{
    if (!c || (B && (!d_glwe || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (idx >= c->prm.polynomial_degree) return fail(c, SPF_ERR_INVALID_ARGUMENT, "sample_extract index >= polynomial_degree");
    if (B == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->generic) {
        const uint32_t N = c->prm.polynomial_degree, k = c->prm.glwe_size;
        for (size_t at = 0; at < B; at += kMaxGridRows) {
            const size_t nb = std::min(B - at, kMaxGridRows);
            hipLaunchKernelGGL(generic_sample_extract_kernel, dim3((k * N + 1 + 255) / 256, (unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                               d_glwe + at * glwe_words(c->prm), d_out + at * lwe1_words(c->prm), (uint32_t)nb, N, k, (uint32_t)idx);
        }
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    // one grid row per ciphertext; grid.y is limited to 65535, larger batches go in slices
    for (size_t at = 0; at < B; at += kMaxGridRows) {
        const size_t nb = std::min(B - at, kMaxGridRows);
        dim3 grid((kN + 1 + 255) / 256, (unsigned)nb), block(256);
        hipLaunchKernelGGL(sample_extract_kernel, grid, block, 0, (hipStream_t)stream, d_glwe + at * 2 * kN,
                           d_out + at * (kN + 1), (uint32_t)nb, (uint32_t)idx);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

static spf_status glwe_linear_dev(spf_ctx* c, void* stream, size_t B, uint32_t op, const uint64_t* d_a,
                                  const uint64_t* d_b, uint32_t n, uint64_t* d_out)
{
    if (!c || (B && (!d_a || !d_out || (op == GLWE_XOR && !d_b)))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (c->generic) {
        const uint32_t N = c->prm.polynomial_degree, k = c->prm.glwe_size;
        for (size_t at = 0; at < B; at += kMaxGridRows) {
            const size_t nb = std::min(B - at, kMaxGridRows), off = at * glwe_words(c->prm);
            hipLaunchKernelGGL(generic_linear_kernel, dim3(((k + 1) * N + 255) / 256, (unsigned)nb), dim3(256), 0, s, d_a + off,
                               d_b ? d_b + off : nullptr, d_out + off, N, c->log_n, k, op == GLWE_NOT ? 0u : (op == GLWE_XOR ? 1u : 2u), n);
        }
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    for (size_t at = 0; at < B; at += kMaxGridRows) {
        const size_t nb = std::min(B - at, kMaxGridRows), off = at * 2 * kN;
        dim3 grid(2 * kN / 256, (unsigned)nb), block(256);
        const uint64_t* pa = d_a + off;
        const uint64_t* pb = d_b ? d_b + off : nullptr;
        if (op == GLWE_NOT) hipLaunchKernelGGL(glwe_linear_kernel<GLWE_NOT>, grid, block, 0, s, pa, pb, d_out + off, (uint32_t)nb, n);
        else if (op == GLWE_XOR) hipLaunchKernelGGL(glwe_linear_kernel<GLWE_XOR>, grid, block, 0, s, pa, pb, d_out + off, (uint32_t)nb, n);
        else hipLaunchKernelGGL(glwe_linear_kernel<GLWE_MUL_XN>, grid, block, 0, s, pa, pb, d_out + off, (uint32_t)nb, n);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

spf_status spf_glwe_not_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_in, uint64_t* d_out)
{
    return glwe_linear_dev(c, stream, B, GLWE_NOT, d_in, nullptr, 0, d_out);
}

spf_status spf_glwe_xor_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out)
{
    return glwe_linear_dev(c, stream, B, GLWE_XOR, d_a, d_b, 0, d_out);
}

spf_status spf_glwe_mul_xn_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_in, size_t n, uint64_t* d_out)
{
    return glwe_linear_dev(c, stream, B, GLWE_MUL_XN, d_in, nullptr, c ? (uint32_t)(n % (2 * (size_t)c->prm.polynomial_degree)) : 0u, d_out);
}

// ---- packed integers: B ciphertexts of n_bits bits, bit i of ciphertext b in row b * n_bits + i (int-major)

// why (B, n_bits) is refused, or nullptr: 0 < n_bits <= N (dynamic_generic_int_graph_nodes.rs:146-147), and B * n_bits rows
// within the batch limit of the circuit-bootstrap entry points
static const char* packed_shape_error(const spf_params& p, size_t B, size_t n_bits)
{
    if (n_bits == 0 || n_bits > p.polynomial_degree) return "n_bits must be in 1 ..= polynomial_degree";
    if (B > packed_shape(p, n_bits, SPF_VAL_GLWE1, SPF_VAL_GLWE1, true).max_batch) return "B * n_bits above 0x0fffffff";
    return nullptr;
}

static spf_status packed_args(spf_ctx* c, size_t B, size_t n_bits, const void* in, const void* out)
{
    if (!c || (B && (!in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (const char* why = packed_shape_error(c->prm, B, n_bits)) return fail(c, SPF_ERR_INVALID_ARGUMENT, why);
    return SPF_OK;
}

static spf_status launch_glwe_pack(spf_ctx* c, hipStream_t s, size_t B, size_t n_bits, const uint64_t* d_bits, uint64_t* d_out)
{
    const size_t pieces = (glwe_words(c->prm) + 255) / 256;
    const unsigned blocks = (unsigned)std::min<size_t>(B * pieces, 8 * (size_t)c->n_cu);
    hipLaunchKernelGGL(glwe_pack_bits_kernel, dim3(blocks), dim3(256), 0, s, d_bits, d_out, B, (uint32_t)n_bits, c->log_n,
                       c->prm.glwe_size);
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// the pack of rows that are not contiguous (a level of a gate graph, spf_graph.hpp): d_rows is a device table of B * n_bits
// device pointers, d_out B contiguous GLWEs that overlap none of the rows
static spf_status launch_glwe_pack_rows(spf_ctx* c, hipStream_t s, size_t B, size_t n_bits, const uint64_t* const* d_rows,
                                        uint64_t* d_out)
{
    const size_t pieces = (glwe_words(c->prm) + 255) / 256;
    const unsigned blocks = (unsigned)std::min<size_t>(B * pieces, 8 * (size_t)c->n_cu);
    hipLaunchKernelGGL(glwe_pack_rows_kernel, dim3(blocks), dim3(256), 0, s, d_rows, d_out, B, (uint32_t)n_bits, c->log_n,
                       c->prm.glwe_size);
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// Bits per workgroup: all of a ciphertext's when the batch alone fills the chip (each packed GLWE read once), fewer when it does
// not, down to one bit per workgroup (a lone integer is unpacked by n_bits workgroups side by side).
static spf_status launch_glwe_unpack(spf_ctx* c, hipStream_t s, size_t B, size_t n_bits, const uint64_t* d_glwe, uint64_t* d_lwe)
{
    const size_t rows = B * n_bits, target = 4 * (size_t)c->n_cu;
    const uint32_t chunk = (uint32_t)std::min(n_bits, (rows + target - 1) / target);
    const size_t items = B * ((n_bits + chunk - 1) / chunk);
    const unsigned blocks = (unsigned)std::min<size_t>(items, 8 * (size_t)c->n_cu);
    const size_t lds = (size_t)c->prm.glwe_size * c->prm.polynomial_degree * 8;
    hipLaunchKernelGGL(glwe_unpack_l1_kernel, dim3(blocks), dim3(256), lds, s, d_glwe, d_lwe, B, (uint32_t)n_bits, chunk, c->log_n,
                       c->prm.glwe_size);
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

spf_status spf_glwe_pack_dev(spf_ctx* c, void* stream, size_t B, size_t n_bits, const uint64_t* d_bits, uint64_t* d_out)
{
    spf_status st = packed_args(c, B, n_bits, d_bits, d_out);
    if (st != SPF_OK || B == 0) return st;
    if (batch_overlaps(packed_shape(c->prm, n_bits, SPF_VAL_GLWE1, SPF_VAL_GLWE1, true), B, d_out, d_bits))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "the packed output overlaps the bit GLWEs");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_glwe_pack(c, (hipStream_t)stream, B, n_bits, d_bits, d_out);
}

spf_status spf_glwe_unpack_l1_dev(spf_ctx* c, void* stream, size_t B, size_t n_bits, const uint64_t* d_glwe, uint64_t* d_lwe1)
{
    spf_status st = packed_args(c, B, n_bits, d_glwe, d_lwe1);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_glwe_unpack(c, (hipStream_t)stream, B, n_bits, d_glwe, d_lwe1);
}

// unpack, then FheOp::KeyswitchL1toL0 -> FheOp::CircuitBootstrap of every bit as spf_keyswitch_circuit_bootstrap_batch runs
// them (same kernels for the same B * n_bits rows); the L1 and L0 LWEs stay in buffers of the context
spf_status spf_unpack_circuit_bootstrap_dev(spf_ctx* c, void* stream, size_t B, size_t n_bits, const uint64_t* d_glwe,
                                            double* d_ggsw)
{
    spf_status st = packed_args(c, B, n_bits, d_glwe, d_ggsw);
    if (st != SPF_OK || B == 0) return st;
    const size_t rows = B * n_bits;
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    st = ensure(c, c->unpack_l1, rows * lwe1_words(c->prm) * 8);
    if (st == SPF_OK) st = ensure(c, c->unpack_l0, rows * lwe0_words(c->prm) * 8);
    if (st == SPF_OK) st = launch_glwe_unpack(c, s, B, n_bits, d_glwe, (uint64_t*)c->unpack_l1.p);
    if (st == SPF_OK) st = launch_keyswitch(c, s, rows, (const uint64_t*)c->unpack_l1.p, (uint64_t*)c->unpack_l0.p);
    if (st == SPF_OK) st = circuit_bootstrap_chain(c, s, rows, (const uint64_t*)c->unpack_l0.p, d_ggsw, &c->scr, 0);
    return st;
}

// At most one gate per CU: the four-waves-per-gate latency shape (a level of a gate graph); beyond
// that two gates per workgroup, the streaming shape.
static void launch_cmux_args(spf_ctx* c, hipStream_t s, const CmuxArgs& a)
{
    if (a.B <= (uint32_t)c->n_cu) {
        c->last_cmux_kernel = "cmux4_kernel<4,4>";
#ifdef SPF_STAMPS
        static int reported = 0;
        if (reported < 6 && a.B <= 256) { // the first few cmux4 launches report
            reported++;
            fprintf(stderr, "[cmux4 stamps] B=%u\n", a.B);
            (void)stamp_report(c, s, (size_t)a.B * 4, kStampNamesCmux4, 9, 1.0, false, false, "[cmux4 stamps] %-44s", "[cmux4 stamps] total %.0f cycles\n",
                               [&](uint64_t* stamps) {
                                   CmuxArgs b = a;
                                   b.stamps = stamps;
                                   hipLaunchKernelGGL((cmux4_kernel<4, 4>), dim3(a.B), dim3(256), kCmux4Lds, s, b);
                                   return SPF_OK;
                               });
            return;
        }
#endif
        hipLaunchKernelGGL((cmux4_kernel<4, 4>), dim3(a.B), dim3(256), kCmux4Lds, s, a);
    } else {
        // two gates per workgroup, two workgroups per CU: the same eight waves as one workgroup of four gates, but
        // the two halves drift apart, so one half's selector requests fly while the other computes, and a barrier
        // ties four waves instead of eight (0.329 -> 0.316 ms per 4096 gates against four gates per 512-thread workgroup)
#ifdef SPF_STAMPS
        static int reported_s = 0;
        if (reported_s < 2 && a.B >= 512) { // the first few streaming-shape launches report
            reported_s++;
            const size_t waves = (size_t)((a.B + 1) / 2) * 4;
            fprintf(stderr, "[cmux stamps] B=%u (cycles per gate, median over %zu waves)\n", a.B, waves);
            (void)stamp_report(c, s, waves, kStampNamesCmux, 16, 1.0, false, false, "[cmux stamps] %-52s", "[cmux stamps] total %.0f cycles\n",
                               [&](uint64_t* stamps) {
                                   CmuxArgs b = a;
                                   b.stamps = stamps;
                                   hipLaunchKernelGGL((cmux_kernel<4, 4, 2>), dim3((a.B + 1) / 2), dim3(256), cmux_lds_bytes(2), s, b);
                                   return SPF_OK;
                               });
            return;
        }
#endif
        // selectors of the launch (one per `per_ggsw` units, (k+1) l (k+1) N/2 complex each) that, with the operands, no
        // longer fit the Infinity Cache (256 MB on MI355X; measured cross-over between 768 and 1024 gates of 256 KiB):
        // streaming loads.  Gate graphs (ptrs) share selectors between gates and keep plain loads.
        const size_t sel_bytes = ggsw_fft_complex(c->prm, c->prm.cbs_radix_count) * sizeof(c64);
        const bool stream = !a.ptrs && (size_t)(a.B / (a.per_ggsw ? a.per_ggsw : 1)) * sel_bytes >= ((size_t)224 << 20);
        if (stream) {
            c->last_cmux_kernel = "cmux_kernel<4,4,2,stream>";
            hipLaunchKernelGGL((cmux_kernel<4, 4, 2, true>), dim3((a.B + 1) / 2), dim3(256), cmux_lds_bytes(2), s, a);
        } else {
            c->last_cmux_kernel = "cmux_kernel<4,4,2>";
            hipLaunchKernelGGL((cmux_kernel<4, 4, 2>), dim3((a.B + 1) / 2), dim3(256), cmux_lds_bytes(2), s, a);
        }
    }
}

static spf_status launch_cmux(spf_ctx* c, hipStream_t s, size_t units, uint32_t per_ggsw, const double* d_sel,
                              const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out)
{
    if (c->generic) {
        if (units == 0) return SPF_OK;
        if (units > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
        GenericCmuxArgs ga{};
        ga.g = generic_shape(c);
        ga.ggsw = reinterpret_cast<const c64*>(d_sel); ga.d0 = d_a ? d_a : d_b; ga.d1 = d_b; ga.out = d_out;
        ga.units = (uint32_t)units; ga.per_ggsw = per_ggsw; ga.d0_zero = d_a ? 0u : 1u;
        ga.radix_log = c->prm.cbs_radix_log; ga.count = c->prm.cbs_radix_count;
        c->last_cmux_kernel = "generic_cmux_kernel";
        hipLaunchKernelGGL(generic_cmux_kernel, dim3((unsigned)units), dim3(kGenericThreads), generic_lds_bytes(ga.g.N, ga.g.k, false), s, ga);
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    if (c->prm.cbs_radix_log != 4 || c->prm.cbs_radix_count != 4)
        return fail(c, SPF_ERR_UNSUPPORTED, "cmux kernel is built for cbs_radix 4 x 4 bits");
    if (units == 0) return SPF_OK;
    if (units > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    CmuxArgs a{};
    // cmux(c, d_0 = a, d_1 = b, b_fft = sel) (crypto/evaluation.rs:68-83); d_a == nullptr means the
    // zero ciphertext (multiply_glwe_ggsw)
    a.ggsw = reinterpret_cast<const c64*>(d_sel); a.d0 = d_a ? d_a : d_b; a.d1 = d_b; a.out = d_out;
    a.tables = c->d_tables; a.B = (uint32_t)units; a.per_ggsw = per_ggsw; a.d0_zero = d_a ? 0u : 1u;
    TimedScope ts(c, s, T_CMUX);
    spf_status st = ts.begin();
    if (st != SPF_OK) return st;
    launch_cmux_args(c, s, a);
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

spf_status spf_cmux_dev(spf_ctx* c, void* stream, size_t B, const double* d_sel, const uint64_t* d_a, const uint64_t* d_b,
                        uint64_t* d_out)
{
    if (!c || (B && (!d_sel || !d_a || !d_b || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_cmux(c, (hipStream_t)stream, B, 1, d_sel, d_a, d_b, d_out);
}

// cmux over operands that are not contiguous: d_ptrs is a device array of 4 pointers per unit
// {selector GGSW-FFT, a (null = the zero ciphertext), b, out}; same kernel, same results
spf_status spf_cmux_scattered_dev(spf_ctx* c, void* stream, size_t units, const void* const* d_ptrs)
{
    if (!c || (units && !d_ptrs)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->generic && (c->prm.cbs_radix_log != 4 || c->prm.cbs_radix_count != 4))
        return fail(c, SPF_ERR_UNSUPPORTED, "cmux kernel is built for cbs_radix 4 x 4 bits");
    if (units == 0) return SPF_OK;
    if (units > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->generic) {
        GenericCmuxArgs ga{};
        ga.g = generic_shape(c);
        ga.units = (uint32_t)units; ga.per_ggsw = 1; ga.ptrs = d_ptrs;
        ga.radix_log = c->prm.cbs_radix_log; ga.count = c->prm.cbs_radix_count;
        c->last_cmux_kernel = "generic_cmux_kernel";
        hipLaunchKernelGGL(generic_cmux_kernel, dim3((unsigned)units), dim3(kGenericThreads), generic_lds_bytes(ga.g.N, ga.g.k, false),
                           (hipStream_t)stream, ga);
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    CmuxArgs a{};
    a.tables = c->d_tables; a.B = (uint32_t)units; a.per_ggsw = 1; a.ptrs = d_ptrs;
    launch_cmux_args(c, (hipStream_t)stream, a);
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// dst row r = `words` u64 from d_src_ptrs[r]
spf_status spf_gather_rows_dev(spf_ctx* c, void* stream, size_t rows, size_t words, const uint64_t* const* d_src_ptrs,
                               uint64_t* d_dst)
{
    if (!c || (rows && (!d_src_ptrs || !d_dst))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (rows == 0 || words == 0) return SPF_OK;
    if (words > 0xffffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "gather rows too long");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    for (size_t at = 0; at < rows; at += kMaxGridRows) {
        const size_t nb = std::min(rows - at, kMaxGridRows);
        dim3 grid((unsigned)((words + 255) / 256), (unsigned)nb), block(256);
        hipLaunchKernelGGL(gather_rows_kernel, grid, block, 0, (hipStream_t)stream, d_src_ptrs + at, d_dst + at * words,
                           (uint32_t)nb, (uint32_t)words);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// KeylessEvaluation::glev_cmux (crypto/evaluation.rs:86-101) = glev_cmux (ops/fft_ops.rs:203-220):
// a cmux over each of the l_cbs GLWEs of two GLEVs with one selector
spf_status spf_glev_cmux_dev(spf_ctx* c, void* stream, size_t B, const double* d_sel, const uint64_t* d_a,
                             const uint64_t* d_b, uint64_t* d_out)
{
    if (!c || (B && (!d_sel || !d_a || !d_b || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_cmux(c, (hipStream_t)stream, B * c->prm.cbs_radix_count, c->prm.cbs_radix_count, d_sel, d_a, d_b, d_out);
}

// KeylessEvaluation::multiply_glwe_ggsw (crypto/evaluation.rs:104-123): out = IFFT(glwe [*] ggsw)
spf_status spf_multiply_glwe_ggsw_dev(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe, const double* d_ggsw,
                                      uint64_t* d_out)
{
    if (!c || (B && (!d_glwe || !d_ggsw || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_cmux(c, (hipStream_t)stream, B, 1, d_ggsw, nullptr, d_glwe, d_out);
}

// ---- blind rotation by an encrypted shift (`blind_rotation`, sunscreen_tfhe/src/ops/bootstrapping/blind_rotation.rs:202-223)

// One step on a tuned context: out = cmux(sel = selector `sel_stride` * u of d_sel, low = acc, high = X^-rot * acc), the high operand
// a rotated read of the low one (the ROT instantiations).  Shapes as launch_cmux_args picks them, one selector per unit.
static void launch_cmux_rot(spf_ctx* c, hipStream_t s, size_t B, const c64* d_sel, uint32_t sel_stride, uint32_t rot,
                            const uint64_t* d_acc, uint64_t* d_out)
{
    CmuxArgs a{};
    a.ggsw = d_sel; a.d0 = d_acc; a.out = d_out; a.tables = c->d_tables; a.B = (uint32_t)B; a.per_ggsw = 1;
    a.rot = rot; a.sel_stride = sel_stride;
    if (a.B <= (uint32_t)c->n_cu) {
        c->last_cmux_kernel = "cmux4_kernel<4,4,rot>";
        hipLaunchKernelGGL((cmux4_kernel<4, 4, true>), dim3(a.B), dim3(256), kCmux4Lds, s, a);
    } else if (B * ggsw_fft_complex(c->prm, c->prm.cbs_radix_count) * sizeof(c64) >= ((size_t)224 << 20)) {
        c->last_cmux_kernel = "cmux_kernel<4,4,2,stream,rot>";
        hipLaunchKernelGGL((cmux_kernel<4, 4, 2, true, true>), dim3((a.B + 1) / 2), dim3(256), cmux_lds_bytes(2), s, a);
    } else {
        c->last_cmux_kernel = "cmux_kernel<4,4,2,rot>";
        hipLaunchKernelGGL((cmux_kernel<4, 4, 2, false, true>), dim3((a.B + 1) / 2), dim3(256), cmux_lds_bytes(2), s, a);
    }
}

// The same step over SCATTERED operands (a level of spf_graph_add_blind_rotation nodes, a batch of the pool's rotate-CMUX kind):
// d_ptrs holds 4 pointers per unit {selector GGSW-FFT, accumulator, unused, out}, the layout of spf_cmux_scattered_dev; the high
// operand is X^-rot * accumulator, `rot` one value per launch.  Shapes as launch_cmux_args picks them for a pointer table: four
// waves per unit up to one unit per CU, two units per workgroup beyond; plain loads (selectors are shared between units).
// Generic contexts: generic_cmux_rot_kernel, the rotated read in the pointer-table path — no row of X^-rot * accumulator exists.
static spf_status launch_cmux_rot_scattered(spf_ctx* c, hipStream_t s, size_t units, uint32_t rot, const void* const* d_ptrs)
{
    if (!c || (units && !d_ptrs)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->generic && (c->prm.cbs_radix_log != 4 || c->prm.cbs_radix_count != 4))
        return fail(c, SPF_ERR_UNSUPPORTED, "cmux kernel is built for cbs_radix 4 x 4 bits");
    if (rot == 0 || rot >= c->prm.polynomial_degree) return fail(c, SPF_ERR_INVALID_ARGUMENT, "rotation must be in 1 .. polynomial_degree - 1");
    if (units == 0) return SPF_OK;
    if (units > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->generic) {
        GenericCmuxArgs ga{};
        ga.g = generic_shape(c);
        ga.units = (uint32_t)units; ga.per_ggsw = 1; ga.ptrs = d_ptrs; ga.rot = rot;
        ga.radix_log = c->prm.cbs_radix_log; ga.count = c->prm.cbs_radix_count;
        c->last_cmux_kernel = "generic_cmux_rot_kernel";
        hipLaunchKernelGGL(generic_cmux_rot_kernel, dim3((unsigned)units), dim3(kGenericThreads), generic_lds_bytes(ga.g.N, ga.g.k, false), s, ga);
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    CmuxArgs a{};
    a.tables = c->d_tables; a.B = (uint32_t)units; a.per_ggsw = 1; a.ptrs = d_ptrs; a.rot = rot;
    if (a.B <= (uint32_t)c->n_cu) {
        c->last_cmux_kernel = "cmux4_kernel<4,4,rot,scattered>";
        hipLaunchKernelGGL((cmux4_rot_scattered_kernel<4, 4>), dim3(a.B), dim3(256), kCmux4Lds, s, a);
    } else {
        c->last_cmux_kernel = "cmux_kernel<4,4,2,rot,scattered>";
        hipLaunchKernelGGL((cmux_rot_scattered_kernel<4, 4, 2>), dim3((a.B + 1) / 2), dim3(256), cmux_lds_bytes(2), s, a);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// why (B, n_bits, log_stride) is refused, or nullptr: every step's rotation 2^(i + log_stride) stays below N
static const char* blind_rotation_shape_error(const spf_params& p, size_t B, size_t n_bits, size_t log_stride)
{
    uint32_t log_n = 0;
    while ((1u << log_n) < p.polynomial_degree) log_n++;
    if (n_bits == 0) return "n_bits must be at least 1";
    if (n_bits > log_n || log_stride > log_n - n_bits) return "n_bits + log_stride above log2(polynomial_degree)";
    if (B > blind_rotation_shape(p, n_bits).max_batch) return "B * n_bits above 0x0fffffff";
    return nullptr;
}

static spf_status blind_rotation_args(spf_ctx* c, size_t B, size_t n_bits, size_t log_stride, const void* shift, const void* in,
                                      const void* out)
{
    if (!c || (B && (!shift || !in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (const char* why = blind_rotation_shape_error(c->prm, B, n_bits, log_stride)) return fail(c, SPF_ERR_INVALID_ARGUMENT, why);
    return SPF_OK;
}

// `blind_rotation` (blind_rotation.rs:202-223) with the shift as `BlindRotationShiftFft` (entities/blind_rotation_shift.rs): for
// bit i ascending, acc = cmux(shift[b][i], acc, X^-(2^(i + log_stride)) * acc) (`cmux`, fft_ops.rs:149-181;
// `rotate_glwe_negative_monomial_negacyclic`, blind_rotation.rs:107-116).  One launch per bit; the steps alternate between a buffer
// of the context and d_out so that the last one writes d_out.
spf_status spf_blind_rotation_dev(spf_ctx* c, void* stream, size_t B, size_t n_bits, size_t log_stride, const double* d_shift,
                                  const uint64_t* d_in, uint64_t* d_out)
{
    spf_status st = blind_rotation_args(c, B, n_bits, log_stride, d_shift, d_in, d_out);
    if (st != SPF_OK) return st;
    if (!c->generic && (c->prm.cbs_radix_log != 4 || c->prm.cbs_radix_count != 4))
        return fail(c, SPF_ERR_UNSUPPORTED, "cmux kernel is built for cbs_radix 4 x 4 bits");
    if (B == 0) return SPF_OK;
    const BatchShape sh = blind_rotation_shape(c->prm, n_bits);
    const size_t gw = sh.out_words, sel = ggsw_fft_complex(c->prm, c->prm.cbs_radix_count);
    if (batch_overlaps(sh, B, d_out, d_in, 1) || batch_overlaps(sh, B, d_out, d_shift, 0))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps an input");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (n_bits > 1) {
        st = ensure(c, c->brot_mid, B * gw * 8);
        if (st != SPF_OK) return st;
    }
    if (c->generic) {
        st = ensure(c, c->brot_high, B * gw * 8);
        if (st != SPF_OK) return st;
    }
    const c64* shift = reinterpret_cast<const c64*>(d_shift);
    const uint64_t* acc = d_in;
    for (size_t i = 0; i < n_bits; i++) {
        uint64_t* dst = ((n_bits - 1 - i) & 1) ? (uint64_t*)c->brot_mid.p : d_out;
        const uint32_t rot = 1u << (i + log_stride);
        if (c->generic) {
            // X^-rot = X^(2N - rot) into scratch, then the CMUX; an item's selectors are n_bits apart: one launch per item
            st = spf_glwe_mul_xn_dev(c, stream, B, acc, 2 * (size_t)c->prm.polynomial_degree - rot, (uint64_t*)c->brot_high.p);
            for (size_t b = 0; b < B && st == SPF_OK; b++)
                st = launch_cmux(c, s, 1, 1, d_shift + 2 * (b * n_bits + i) * sel, acc + b * gw, (const uint64_t*)c->brot_high.p + b * gw,
                                 dst + b * gw);
            if (st != SPF_OK) return st;
        } else {
            TimedScope ts(c, s, T_CMUX);
            st = ts.begin();
            if (st != SPF_OK) return st;
            launch_cmux_rot(c, s, B, shift + i * sel, (uint32_t)n_bits, rot, acc, dst);
            HIPCHK(c, hipGetLastError());
            st = ts.end();
            if (st != SPF_OK) return st;
        }
        acc = dst;
    }
    return SPF_OK;
}

// ---------------------------------------------------------------- host-pointer forms
//
// Each form checks every argument it can see, then reaches the device through host_batch() on its batch shape (spf_ops.hpp), or,
// where it has staging of its own, through staged() / host_call().

spf_status spf_keyswitch_lwe_l1_lwe_l0_batch(spf_ctx* c, size_t B, const uint64_t* in, uint64_t* out)
{
    if (!c || (B && (!in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_KEYSWITCH), B, {{c->in, in}}, out,
                      [&](const uint64_t* d_in, uint64_t* d_out) { return launch_keyswitch(c, c->stream, B, d_in, d_out); });
}

// Bootstrap a device-resident batch and bring the outputs to the caller's host buffer, in SLICES of one
// full round of the chip (4 ciphertexts x #CU): all slices are enqueued on the compute stream at once,
// each followed by an event; the copy stream waits for slice k's event and copies it out while slices
// k+1.. run.  The output is 32 KiB per ciphertext (134 MB per 4096): in one piece behind the kernel it
// added 10-15 % to a call, sliced only the last slice's copy is exposed.  (A pageable destination makes
// hipMemcpyAsync block the host until that copy is done — which is why every kernel is enqueued first.)
static spf_status bootstrap_sliced_to_host(spf_ctx* c, size_t B, const uint64_t* d_lwe, const uint64_t* d_lut,
                                           size_t lut_stride, uint32_t log_chi, uint32_t log_v, uint64_t rot, const BatchShape& sh,
                                           bool extract, uint64_t* host_out)
{
    const size_t lw = sh.in_words[0], ow = sh.out_words;
    const size_t round = 4 * (size_t)c->n_cu;
    const size_t slice = B > round ? round : B;
    const size_t n_slices = (B + slice - 1) / slice;
    while (c->slice_ev.size() < n_slices) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->slice_ev.push_back(e);
    }
    uint64_t* d_out = (uint64_t*)c->out.p;
    // Once something is enqueued, no return before both streams are idle: kernels may still be writing c->out and
    // copies may still be landing in the caller's buffer, which the caller is free to release after an error.
    auto enqueue = [&]() -> spf_status {
        for (size_t k = 0; k < n_slices; k++) {
            const size_t off = k * slice, n = std::min(slice, B - off);
            spf_status s = launch_blind_rotate(c, c->stream, n, d_lwe + off * lw, d_lut + off * lut_stride, lut_stride, log_chi,
                                               log_v, rot, d_out + off * ow, ow, extract);
            if (s != SPF_OK) return s;
            HIPCHK(c, hipEventRecord(c->slice_ev[k], c->stream));
        }
        for (size_t k = 0; k < n_slices; k++) {
            const size_t off = k * slice, n = std::min(slice, B - off);
            HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->slice_ev[k], 0));
            HIPCHK(c, hipMemcpyAsync(host_out + off * ow, d_out + off * ow, n * ow * 8, hipMemcpyDeviceToHost, c->copy_stream));
        }
        return SPF_OK;
    };
    const spf_status st = enqueue();
    const hipError_t e1 = hipStreamSynchronize(c->copy_stream), e2 = hipStreamSynchronize(c->stream);
    if (st != SPF_OK) return st; // the message of the first failure stays in place
    HIPCHK(c, e1);
    HIPCHK(c, e2);
    return SPF_OK;
}

// `rhs` (bivariate): the input bootstrapped is lwe * 2^shift_bits + rhs, packed in place in the staging buffer
static spf_status pbs_host(spf_ctx* c, size_t B, const uint64_t* lwe, const uint64_t* lut, size_t lut_stride,
                           uint32_t log_chi, uint32_t log_v, uint64_t rot, uint64_t* out, bool extract,
                           const uint64_t* rhs = nullptr, uint32_t shift_bits = 0)
{
    if (!c || (B && (!lwe || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    if (lut_stride && lut_stride < glwe_words(c->prm)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "lut_stride smaller than a GLWE");
    spf_status s = blind_rotate_args(c, B, log_chi, log_v);
    if (s != SPF_OK) return s;
    const BatchShape sh = pbs_shape(c->prm, extract);
    const size_t lw = B * sh.in_words[0] * 8;
    const size_t lut_words = lut_stride ? (B - 1) * lut_stride + glwe_words(c->prm) : glwe_words(c->prm);
    return staged(c, {{c->in, lwe, lw}, {c->mid, rhs, lw}, {c->aux, lut, lut_words * 8}}, B * sh.out_words * 8, [&]() -> spf_status {
        if (rhs) {
            spf_status st = launch_lwe_pack(c, c->stream, B, (const uint64_t*)c->in.p, (const uint64_t*)c->mid.p, shift_bits,
                                            (uint64_t*)c->in.p);
            if (st != SPF_OK) return st;
        }
        return bootstrap_sliced_to_host(c, B, (const uint64_t*)c->in.p, lut ? (const uint64_t*)c->aux.p : c->d_cbs_lut,
                                        lut ? lut_stride : 0, log_chi, log_v, rot, sh, extract, out);
    });
}

spf_status spf_generalized_pbs_batch(spf_ctx* c, size_t B, const uint64_t* lwe, const uint64_t* lut, size_t lut_stride,
                                     uint32_t log_chi, uint32_t log_v, uint64_t body_rotate, uint64_t* out)
{
    if (B && !lut) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null lut");
    return pbs_host(c, B, lwe, lut, lut_stride, log_chi, log_v, body_rotate, out, false);
}

spf_status spf_pbs_univariate_batch(spf_ctx* c, size_t B, const uint64_t* lwe, const uint64_t* lut, size_t lut_stride,
                                    uint64_t* out)
{
    if (B && !lut) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null lut");
    return pbs_host(c, B, lwe, lut, lut_stride, 0, 0, 0, out, true);
}

spf_status spf_pbs_bivariate_batch(spf_ctx* c, size_t B, const uint64_t* left, const uint64_t* right, const uint64_t* lut,
                                   size_t lut_stride, uint32_t plaintext_bits, uint64_t* out)
{
    if (B && (!right || !lut)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (plaintext_bits >= 64) return fail(c, SPF_ERR_INVALID_ARGUMENT, "plaintext_bits must be below 64");
    return pbs_host(c, B, left, lut, lut_stride, 0, 0, 0, out, true, right, plaintext_bits);
}

spf_status spf_circuit_bootstrap_pbs_batch(spf_ctx* c, size_t B, const uint64_t* lwe, uint64_t* out)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    return pbs_host(c, B, lwe, nullptr, 0, 0, ceil_log2(c->prm.cbs_radix_count), (uint64_t)1 << 62, out, false);
}

spf_status spf_sample_extract_l1_batch(spf_ctx* c, size_t B, const uint64_t* glwe, size_t idx, uint64_t* out)
{
    if (!c || (B && (!glwe || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (idx >= c->prm.polynomial_degree) return fail(c, SPF_ERR_INVALID_ARGUMENT, "sample_extract index >= polynomial_degree");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_SAMPLE_EXTRACT), B, {{c->in, glwe}}, out,
                      [&](const uint64_t* d_glwe, uint64_t* d_out) { return spf_sample_extract_l1_dev(c, c->stream, B, d_glwe, idx, d_out); });
}

spf_status spf_glwe_not_batch(spf_ctx* c, size_t B, const uint64_t* in, uint64_t* out)
{
    if (!c || (B && (!in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_NOT), B, {{c->in, in}}, out,
                      [&](const uint64_t* d_in, uint64_t* d_out) { return spf_glwe_not_dev(c, c->stream, B, d_in, d_out); });
}

spf_status spf_glwe_xor_batch(spf_ctx* c, size_t B, const uint64_t* a, const uint64_t* b, uint64_t* out)
{
    if (!c || (B && (!a || !b || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_GLWE_ADD), B, {{c->in, a}, {c->mid, b}}, out,
                      [&](const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out) { return spf_glwe_xor_dev(c, c->stream, B, d_a, d_b, d_out); });
}

spf_status spf_glwe_mul_xn_batch(spf_ctx* c, size_t B, const uint64_t* in, size_t n, uint64_t* out)
{
    if (!c || (B && (!in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_MUL_XN), B, {{c->in, in}}, out,
                      [&](const uint64_t* d_in, uint64_t* d_out) { return spf_glwe_mul_xn_dev(c, c->stream, B, d_in, n, d_out); });
}

spf_status spf_glwe_pack_batch(spf_ctx* c, size_t B, size_t n_bits, const uint64_t* bits, uint64_t* out)
{
    spf_status s = packed_args(c, B, n_bits, bits, out);
    if (s != SPF_OK) return s;
    return host_batch(c, packed_shape(c->prm, n_bits, SPF_VAL_GLWE1, SPF_VAL_GLWE1, true), B, {{c->in, bits}}, out,
                      [&](const uint64_t* d_bits, uint64_t* d_out) { return spf_glwe_pack_dev(c, c->stream, B, n_bits, d_bits, d_out); });
}

spf_status spf_glwe_unpack_l1_batch(spf_ctx* c, size_t B, size_t n_bits, const uint64_t* glwe, uint64_t* lwe1_out)
{
    spf_status s = packed_args(c, B, n_bits, glwe, lwe1_out);
    if (s != SPF_OK) return s;
    return host_batch(c, packed_shape(c->prm, n_bits, SPF_VAL_GLWE1, SPF_VAL_LWE1, false), B, {{c->in, glwe}}, lwe1_out,
                      [&](const uint64_t* d_glwe, uint64_t* d_out) { return spf_glwe_unpack_l1_dev(c, c->stream, B, n_bits, d_glwe, d_out); });
}

spf_status spf_cmux_batch(spf_ctx* c, size_t B, const double* sel, const uint64_t* a, const uint64_t* b, uint64_t* out)
{
    if (!c || (B && (!sel || !a || !b || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_CMUX), B,
                      {{c->aux, sel}, {c->in, a}, {c->mid, b}}, out, [&](const double* d_sel, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out) {
                          return spf_cmux_dev(c, c->stream, B, d_sel, d_a, d_b, d_out);
                      });
}

spf_status spf_blind_rotation_batch(spf_ctx* c, size_t B, size_t n_bits, size_t log_stride, const double* shift, const uint64_t* in,
                                    uint64_t* out)
{
    spf_status s = blind_rotation_args(c, B, n_bits, log_stride, shift, in, out);
    if (s != SPF_OK) return s;
    return host_batch(c, blind_rotation_shape(c->prm, n_bits), B, {{c->aux, shift}, {c->in, in}}, out,
                      [&](const double* d_shift, const uint64_t* d_in, uint64_t* d_out) {
                          return spf_blind_rotation_dev(c, c->stream, B, n_bits, log_stride, d_shift, d_in, d_out);
                      });
}

spf_status spf_glev_cmux_batch(spf_ctx* c, size_t B, const double* sel, const uint64_t* a, const uint64_t* b, uint64_t* out)
{
    if (!c || (B && (!sel || !a || !b || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_GLEV_CMUX), B,
                      {{c->aux, sel}, {c->in, a}, {c->mid, b}}, out, [&](const double* d_sel, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out) {
                          return spf_glev_cmux_dev(c, c->stream, B, d_sel, d_a, d_b, d_out);
                      });
}

spf_status spf_multiply_glwe_ggsw_batch(spf_ctx* c, size_t B, const uint64_t* glwe, const double* ggsw, uint64_t* out)
{
    if (!c || (B && (!glwe || !ggsw || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return host_batch(c, spf_ops::shape(c->prm, spf_ops::OP_MULTIPLY_GGSW_GLWE), B, {{c->aux, ggsw}, {c->in, glwe}}, out,
                      [&](const double* d_ggsw, const uint64_t* d_glwe, uint64_t* d_out) {
                          return spf_multiply_glwe_ggsw_dev(c, c->stream, B, d_glwe, d_ggsw, d_out);
                      });
}

static spf_status load_fft_key(spf_ctx* c, int which, const double* src, size_t n_complex, size_t want, bool* ready)
{
    if (!c || !src) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (n_complex != want)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "key length " + std::to_string(n_complex) + " != " + std::to_string(want));
    void* p; size_t bytes;
    spf_status s = spf_key_blob(c, which, &p, &bytes);
    if (s != SPF_OK) return s;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *ready = true;
    c->ggsw_const_ready = false;
    return SPF_OK;
}

spf_status spf_load_automorphism_key(spf_ctx* c, const double* ak_fft, size_t n_complex)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    return load_fft_key(c, 2, ak_fft, n_complex, ak_complex(c->prm), &c->ak_ready);
}

spf_status spf_load_scheme_switch_key(spf_ctx* c, const double* ssk_fft, size_t n_complex)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    return load_fft_key(c, 3, ssk_fft, n_complex, ssk_complex(c->prm), &c->ssk_ready);
}

// ---------------------------------------------------------------- standard (integer) form -> transform domain on the device
// `PolynomialRef::fft` (entities/polynomial.rs:257-274) of n_polys polynomials (spf_poly_fft.hpp).  d_out == d_in is allowed.

static spf_status launch_poly_fft(spf_ctx* c, hipStream_t s, size_t n_polys, const uint64_t* d_in, c64* d_out)
{
    if (n_polys == 0) return SPF_OK;
    if (c->prm.polynomial_degree == (uint32_t)kN) { // (whatever the radix: the transform does not depend on it)
        static_assert(kPolyFftLds <= 64 * 1024, "within the default dynamic LDS limit");
        PolyFftArgs a{d_in, d_out, c->d_tables, (uint32_t)n_polys};
        // two workgroups fit a CU's LDS; a wave walks the batch with the grid's stride, so the table image is copied once per slot
        const size_t groups = (n_polys + kPolyFftWaves - 1) / kPolyFftWaves;
        const unsigned grid = (unsigned)std::min(groups, 2 * (size_t)c->n_cu);
        hipLaunchKernelGGL(poly_fft2048_kernel, dim3(grid), dim3(64 * kPolyFftWaves), kPolyFftLds, s, a);
    } else {
        GenericPolyFftArgs a{generic_shape(c), d_in, d_out};
        hipLaunchKernelGGL(generic_poly_fft_kernel, dim3((unsigned)n_polys), dim3(kGenericThreads),
                           generic_poly_fft_lds_bytes(a.g.N), s, a);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

spf_status spf_poly_fft_dev(spf_ctx* c, void* stream, size_t n_polys, const uint64_t* d_in, double* d_out)
{
    if (!c || (n_polys && (!d_in || !d_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (n_polys == 0) return SPF_OK;
    if (n_polys > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    {
        // the same memory (in place) or disjoint memory: a partial overlap would let one polynomial's bins land on another's words
        const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out, bytes = (uintptr_t)n_polys * c->prm.polynomial_degree * 8;
        if (a != b && a < b + bytes && b < a + bytes)
            return fail(c, SPF_ERR_INVALID_ARGUMENT, "spf_poly_fft_dev: d_out must be d_in itself or must not overlap it");
    }
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_poly_fft(c, (hipStream_t)stream, n_polys, d_in, reinterpret_cast<c64*>(d_out));
}

spf_status spf_poly_fft_batch(spf_ctx* c, size_t n_polys, const uint64_t* in, double* out)
{
    if (!c || (n_polys && (!in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const BatchShape sh = poly_fft_shape(c->prm);
    if (spf_status s = batch_limit(c, sh, n_polys)) return s;
    return host_batch(c, sh, n_polys, {{c->in, in}}, out,
                      [&](const uint64_t* d_in, double* d_out) { return spf_poly_fft_dev(c, c->stream, n_polys, d_in, d_out); });
}

// A key in standard form: the words go into the key blob as they are (same bytes as its spectra) and are transformed there;
// then exactly what the float loader does behind its copy.  The key is not ready from the first touched byte until the end.
static spf_status load_std_key(spf_ctx* c, int which, const char* name, const uint64_t* words, size_t n_words, size_t want_complex)
{
    if (!c || !words) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (n_words / 2 != want_complex || (n_words & 1))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string(name) + " key length " + std::to_string(n_words) + " words != " +
                                                     std::to_string(2 * want_complex));
    void* p; size_t bytes;
    spf_status s = spf_key_blob(c, which, &p, &bytes);
    if (s != SPF_OK) return s;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    bool& ready = which == 0 ? c->bsk_ready : (which == 2 ? c->ak_ready : c->ssk_ready);
    ready = false;
    HIPCHK(c, hipSetDevice(c->device));
    auto transform = [&]() -> spf_status {
        HIPCHK(c, hipMemcpyAsync(p, words, bytes, hipMemcpyHostToDevice, c->stream));
        return launch_poly_fft(c, c->stream, n_words / c->prm.polynomial_degree, (const uint64_t*)p, (c64*)p);
    };
    s = transform();
    {
        // (no return before the stream is idle: the copy reads the caller's buffer)
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (s == SPF_OK && e != hipSuccess) s = fail(c, SPF_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    if (s == SPF_OK && which == 0) s = finish_bootstrap_key(c);
    if (s != SPF_OK) return s;
    ready = true;
    c->ggsw_const_ready = false;
    return SPF_OK;
}

spf_status spf_load_bootstrap_key_std(spf_ctx* c, const uint64_t* bsk, size_t n_words)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    return load_std_key(c, 0, "bootstrap", bsk, n_words, (size_t)c->prm.lwe_dimension * ggsw_fft_complex(c->prm, c->prm.pbs_radix_count));
}

spf_status spf_load_automorphism_key_std(spf_ctx* c, const uint64_t* ak, size_t n_words)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    return load_std_key(c, 2, "automorphism", ak, n_words, ak_complex(c->prm));
}

spf_status spf_load_scheme_switch_key_std(spf_ctx* c, const uint64_t* ssk, size_t n_words)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    return load_std_key(c, 3, "scheme-switch", ssk, n_words, ssk_complex(c->prm));
}

spf_status spf_mod_switch_trace_and_rotate_batch(spf_ctx* c, size_t B, const uint64_t* glwe_in, uint64_t* glev_out)
{
    if (!c || (B && (!glwe_in || !glev_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const BatchShape sh = trace_shape(c->prm);
    if (spf_status s = batch_limit(c, sh, B)) return s;
    return host_batch(c, sh, B, {{c->in, glwe_in}}, glev_out,
                      [&](const uint64_t* d_glwe, uint64_t* d_glev) { return spf_mod_switch_trace_and_rotate_dev(c, c->stream, B, d_glwe, d_glev); });
}

spf_status spf_scheme_switch_batch(spf_ctx* c, size_t B, const uint64_t* glev_in, double* ggsw_out)
{
    if (!c || (B && (!glev_in || !ggsw_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const BatchShape sh = spf_ops::shape(c->prm, spf_ops::OP_SCHEME_SWITCH);
    if (spf_status s = batch_limit(c, sh, B)) return s;
    return host_batch(c, sh, B, {{c->in, glev_in}}, ggsw_out,
                      [&](const uint64_t* d_glev, double* d_ggsw) { return spf_scheme_switch_dev(c, c->stream, B, d_glev, d_ggsw); });
}

spf_status spf_circuit_bootstrap_batch(spf_ctx* c, size_t B, const uint64_t* lwe0_in, double* ggsw_out)
{
    if (!c || (B && (!lwe0_in || !ggsw_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const BatchShape sh = spf_ops::shape(c->prm, spf_ops::OP_CBS);
    if (spf_status s = batch_limit(c, sh, B)) return s;
    return host_batch(c, sh, B, {{c->in, lwe0_in}}, ggsw_out,
                      [&](const uint64_t* d_lwe, double* d_ggsw) { return spf_circuit_bootstrap_dev(c, c->stream, B, d_lwe, d_ggsw); });
}

spf_status spf_keyswitch_circuit_bootstrap_batch(spf_ctx* c, size_t B, const uint64_t* lwe1_in, double* ggsw_out)
{
    if (!c || (B && (!lwe1_in || !ggsw_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const BatchShape sh = spf_ops::shape(c->prm, spf_ops::OP_GATE_CBS);
    if (spf_status s = batch_limit(c, sh, B)) return s;
    return host_batch(c, sh, B, {{c->in, lwe1_in}}, ggsw_out, [&](const uint64_t* d_lwe1, double* d_ggsw) {
        spf_status st = ensure(c, c->mid, B * lwe0_words(c->prm) * 8); // the level-0 LWE never leaves the device
        if (st == SPF_OK) st = launch_keyswitch(c, c->stream, B, d_lwe1, (uint64_t*)c->mid.p);
        if (st == SPF_OK) st = spf_circuit_bootstrap_dev(c, c->stream, B, (const uint64_t*)c->mid.p, d_ggsw);
        return st;
    });
}

spf_status spf_unpack_circuit_bootstrap_batch(spf_ctx* c, size_t B, size_t n_bits, const uint64_t* glwe, double* ggsw_out)
{
    spf_status s = packed_args(c, B, n_bits, glwe, ggsw_out);
    if (s != SPF_OK) return s;
    return host_batch(c, packed_shape(c->prm, n_bits, SPF_VAL_GLWE1, SPF_VAL_GGSW1, false), B, {{c->in, glwe}}, ggsw_out,
                      [&](const uint64_t* d_glwe, double* d_ggsw) { return spf_unpack_circuit_bootstrap_dev(c, c->stream, B, n_bits, d_glwe, d_ggsw); });
}

spf_status spf_gate_bootstrap_batch(spf_ctx* c, size_t B, const uint64_t* lwe1, uint64_t* glwe_out)
{
    if (!c || (B && (!lwe1 || !glwe_out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    const uint32_t log_v = ceil_log2(c->prm.cbs_radix_count);
    spf_status s = blind_rotate_args(c, B, 0, log_v);
    if (s != SPF_OK) return s;
    const BatchShape sh = gate_bootstrap_shape(c->prm), pbs = pbs_shape(c->prm, false); // (pbs: the second stage)
    return staged(c, {{c->in, lwe1, B * sh.in_words[0] * 8}}, B * sh.out_words * 8, [&] {
        spf_status st = ensure(c, c->mid, B * pbs.in_words[0] * 8); // the level-0 LWE never leaves the device
        if (st == SPF_OK) st = launch_keyswitch(c, c->stream, B, (const uint64_t*)c->in.p, (uint64_t*)c->mid.p);
        if (st != SPF_OK) return st;
        return bootstrap_sliced_to_host(c, B, (const uint64_t*)c->mid.p, c->d_cbs_lut, 0, 0, log_v, (uint64_t)1 << 62, pbs, false, glwe_out);
    });
}

// ---------------------------------------------------------------- measurement hooks

spf_status spf_set_timing(spf_ctx* c, int enabled)
{
    if (!c) return SPF_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    c->timing = enabled != 0;
    return SPF_OK;
}

spf_status spf_last_kernel_ms(spf_ctx* c, const char* kernel, double* avg_ms, int* launches)
{
    if (!c || !kernel || !avg_ms || !launches) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<TimedLaunch>* v = nullptr;
    for (int k = 0; k < T_COUNT; k++)
        if (!strcmp(kernel, kTimedNames[k])) v = &c->timed[k];
    if (!v) return fail(c, SPF_ERR_INVALID_ARGUMENT, "kernel must be \"pbs\", \"keyswitch\", \"trace\", \"scheme_switch\", \"cmux\", \"pufks_prepass\", \"lwe_linear_planes\", \"lwe_linear\", \"glwe_poly_linear\", \"glwe_keyswitch\" or \"lwe_ring_pack\"");
    double total = 0.0;
    int n = 0;
    for (auto& t : *v) {
        HIPCHK(c, hipEventSynchronize(t.stop));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, t.start, t.stop));
        total += ms; n++;
        (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop);
    }
    v->clear();
    *avg_ms = n ? total / n : 0.0;
    *launches = n;
    return SPF_OK;
}

// ---------------------------------------------------------------- host helpers without a GPU call

// `generate_lut` (ops/bootstrapping/programmable_bootstrapping.rs:129-185) as the trivial GLWE that
// `programmable_bootstrap_univariate` takes (zero mask, body = the table polynomial).  Closed form of the
// reference's fill / negate / rotate: with p = 2^bits inputs, stride = N / p coefficients per input and
// h = stride / 2, body[i] = sign * (f_id(x) << (64 - bits)) for m = (i + h) mod N, x = m / stride,
// id = (m % stride) % 2^ceil(log2 #maps) (0 when id >= #maps), sign = -1 for m < h.
spf_status spf_generate_lut(const spf_params* prm, const uint64_t* map_tables, size_t n_maps, uint32_t plaintext_bits,
                            uint64_t* lut_glwe_out)
{
    if (!prm || !map_tables || !lut_glwe_out || n_maps == 0)
        return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_generate_lut: null argument or no map");
    const size_t N = prm->polynomial_degree, k = prm->glwe_size;
    if (plaintext_bits == 0 || plaintext_bits >= 64 || ((size_t)1 << plaintext_bits) > N)
        return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_generate_lut: needs 1 <= plaintext_bits and 2^plaintext_bits <= N");
    const size_t p = (size_t)1 << plaintext_bits, stride = N / p, h = stride / 2;
    size_t ceil_v = 1;
    while (ceil_v < n_maps) ceil_v <<= 1;
    for (size_t i = 0; i < n_maps * p; i++)
        if (map_tables[i] >= p) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_generate_lut: a map value is not below 2^plaintext_bits");
    std::memset(lut_glwe_out, 0, k * N * sizeof(uint64_t));
    uint64_t* body = lut_glwe_out + k * N;
    for (size_t i = 0; i < N; i++) {
        const size_t m = (i + h) % N, x = m / stride, id = (m % stride) % ceil_v;
        const uint64_t v = id < n_maps ? map_tables[id * p + x] << (64 - plaintext_bits) : 0;
        body[i] = m < h ? (uint64_t)0 - v : v;
    }
    return SPF_OK;
}

// `BivariateLookupTable::trivial_from_fn` (entities/bivariate_lookup_table.rs:36-90) = `generate_bivariate_lut`
// (ops/bootstrapping/programmable_bootstrapping.rs:413-452): the univariate table U[x] = f((x >> p) mod 2^p, x mod 2^p) over
// x < 2^(p + c) (`bivariate_function`, the left operand taken mod 2^p), written by `generate_lut` at p + c bits.  With
// map_table[l * 2^p + r] = f(l, r) that index is x mod 2^(2p).
spf_status spf_generate_bivariate_lut(const spf_params* prm, const uint64_t* map_table, uint32_t plaintext_bits,
                                      uint32_t carry_bits, uint64_t* lut_glwe_out)
{
    if (!prm || !map_table || !lut_glwe_out) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_generate_bivariate_lut: null argument");
    const uint64_t bits = (uint64_t)plaintext_bits + carry_bits;
    if (plaintext_bits == 0 || plaintext_bits > carry_bits || bits >= 64 || ((uint64_t)1 << bits) > prm->polynomial_degree)
        return fail(nullptr, SPF_ERR_INVALID_ARGUMENT,
                    "spf_generate_bivariate_lut: needs 1 <= plaintext_bits <= carry_bits and 2^(plaintext_bits + carry_bits) <= N");
    const uint64_t p = (uint64_t)1 << plaintext_bits;
    for (uint64_t i = 0; i < p * p; i++)
        if (map_table[i] >= p)
            return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_generate_bivariate_lut: a map value is not below 2^plaintext_bits");
    std::vector<uint64_t> u;
    try {
        u.resize((size_t)1 << bits);
    } catch (const std::bad_alloc&) {
        return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_generate_bivariate_lut: out of host memory");
    }
    for (size_t x = 0; x < u.size(); x++) u[x] = map_table[x & (p * p - 1)];
    return spf_generate_lut(prm, u.data(), 1, (uint32_t)bits, lut_glwe_out);
}

// `safe_bincode::deserialize::<ComputeKey>` (parasol_runtime/src/safe_bincode.rs:16-28, crypto/keys.rs:294-318):
// bincode DefaultOptions + fixint: per field a u64 little-endian element count, then the elements
// (Complex<f64> = two LE f64, Torus<u64> = one LE u64); fields in declaration order bs_key, ks_key, ss_key,
// auto_key; trailing bytes allowed; every count must be exactly what the parameters need (the reference
// bounds the read by GetSize and then runs check_is_valid) — checked for ALL fields before any key is touched.
spf_status spf_load_compute_key_bincode(spf_ctx* c, const uint8_t* bytes, size_t len)
{
    if (!c || !bytes) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    struct Field { const char* name; size_t want, elem; const uint8_t* data; };
    Field f[4] = {{"bs_key", (size_t)c->prm.lwe_dimension * ggsw_fft_complex(c->prm, c->prm.pbs_radix_count), 16, nullptr},
                  {"ks_key", (size_t)c->prm.glwe_size * c->prm.polynomial_degree * c->prm.ks_radix_count * lwe0_words(c->prm), 8, nullptr},
                  {"ss_key", ssk_complex(c->prm), 16, nullptr},
                  {"auto_key", ak_complex(c->prm), 16, nullptr}};
    size_t off = 0;
    for (auto& x : f) {
        if (len - off < 8) return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string("ComputeKey: truncated before the length of ") + x.name);
        uint64_t n = 0;
        for (int b = 7; b >= 0; b--) n = (n << 8) | bytes[off + b]; // little-endian, any alignment
        off += 8;
        if (n != x.want)
            return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string("ComputeKey: ") + x.name + " has " + std::to_string(n) +
                                                         " elements, the parameters need " + std::to_string(x.want));
        if ((len - off) / x.elem < x.want) return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string("ComputeKey: truncated inside ") + x.name);
        x.data = bytes + off;
        off += x.want * x.elem;
    }
    // the loaders only memcpy from these (possibly unaligned) pointers; x86-64 little-endian host = wire order
    spf_status st = spf_load_bootstrap_key(c, reinterpret_cast<const double*>(f[0].data), f[0].want);
    if (st == SPF_OK) st = spf_load_keyswitch_key(c, reinterpret_cast<const uint64_t*>(f[1].data), f[1].want);
    if (st == SPF_OK) st = spf_load_scheme_switch_key(c, reinterpret_cast<const double*>(f[2].data), f[2].want);
    if (st == SPF_OK) st = spf_load_automorphism_key(c, reinterpret_cast<const double*>(f[3].data), f[3].want);
    return st;
}

// `safe_bincode::deserialize::<ComputeKeyNonFft>` + `ComputeKeyNonFft::fft` (crypto/keys.rs:145-159, :258-282): the same
// conventions, every element one little-endian u64 (Torus<u64>), fields in THAT struct's declaration order — bs_key, ks_key,
// auto_key, ss_key (ComputeKey has ss_key before auto_key).  All four counts are checked before any key is touched.
spf_status spf_load_compute_key_nonfft_bincode(spf_ctx* c, const uint8_t* bytes, size_t len)
{
    if (!c || !bytes) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    struct Field { const char* name; size_t want; const uint8_t* data; };
    Field f[4] = {{"bs_key", 2 * (size_t)c->prm.lwe_dimension * ggsw_fft_complex(c->prm, c->prm.pbs_radix_count), nullptr},
                  {"ks_key", (size_t)c->prm.glwe_size * c->prm.polynomial_degree * c->prm.ks_radix_count * lwe0_words(c->prm), nullptr},
                  {"auto_key", 2 * ak_complex(c->prm), nullptr},
                  {"ss_key", 2 * ssk_complex(c->prm), nullptr}};
    size_t off = 0;
    for (auto& x : f) {
        if (len - off < 8) return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string("ComputeKeyNonFft: truncated before the length of ") + x.name);
        uint64_t n = 0;
        for (int b = 7; b >= 0; b--) n = (n << 8) | bytes[off + b]; // little-endian, any alignment
        off += 8;
        if (n != x.want)
            return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string("ComputeKeyNonFft: ") + x.name + " has " + std::to_string(n) +
                                                         " elements, the parameters need " + std::to_string(x.want));
        if ((len - off) / 8 < x.want) return fail(c, SPF_ERR_INVALID_ARGUMENT, std::string("ComputeKeyNonFft: truncated inside ") + x.name);
        x.data = bytes + off;
        off += x.want * 8;
    }
    // the loaders only copy from these (possibly unaligned) pointers; x86-64 little-endian host = wire order
    spf_status st = spf_load_bootstrap_key_std(c, reinterpret_cast<const uint64_t*>(f[0].data), f[0].want);
    if (st == SPF_OK) st = spf_load_keyswitch_key(c, reinterpret_cast<const uint64_t*>(f[1].data), f[1].want);
    if (st == SPF_OK) st = spf_load_automorphism_key_std(c, reinterpret_cast<const uint64_t*>(f[2].data), f[2].want);
    if (st == SPF_OK) st = spf_load_scheme_switch_key_std(c, reinterpret_cast<const uint64_t*>(f[3].data), f[3].want);
    return st;
}

// Ciphertext wire format: see include/spf_hip.h.  (encryption.rs:23-110, 454-519; safe_bincode.rs:16-28.)
size_t spf_ciphertext_words(const spf_params* p, spf_value_kind kind)
{
    // (L1GgswCiphertext is not Serialize in the reference: the one kind that has a size in memory and none on the wire)
    if (!p || kind == SPF_VAL_GGSW1) return 0;
    return value_words(*p, kind);
}

static const char* wire_kind_name(spf_value_kind k)
{
    static const char* n[5] = {"L0LweCiphertext", "L1LweCiphertext", "L1GlweCiphertext", "L1GgswCiphertext", "L1GlevCiphertext"};
    return ((unsigned)k < 5) ? n[k] : "ciphertext";
}

spf_status spf_ciphertext_from_bincode(const spf_params* p, spf_value_kind kind, const uint8_t* bytes, size_t len,
                                       uint64_t* words_out)
{
    if (!p || !bytes || !words_out) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_ciphertext_from_bincode: null argument");
    if (kind == SPF_VAL_GGSW1)
        return fail(nullptr, SPF_ERR_UNSUPPORTED, "L1GgswCiphertext has no wire format in the reference (not Serialize)");
    const size_t want = spf_ciphertext_words(p, kind);
    if (want == 0) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_ciphertext_from_bincode: unknown ciphertext kind");
    const std::string what = wire_kind_name(kind);
    if (len < 8) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, what + ": truncated before the element count");
    uint64_t n = 0;
    for (int b = 7; b >= 0; b--) n = (n << 8) | bytes[b]; // little-endian, any alignment
    // the reference bounds the read at (want + 1) * 8 bytes (bincode's SizeLimit error for anything longer) and
    // check_is_valid rejects anything shorter: only the exact count passes
    if (n != want)
        return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, what + ": " + std::to_string(n) + " elements, the parameters need " + std::to_string(want));
    if ((len - 8) / 8 < want) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, what + ": truncated inside the data");
    for (size_t i = 0; i < want; i++) {
        uint64_t w = 0;
        for (int b = 7; b >= 0; b--) w = (w << 8) | bytes[8 + 8 * i + b];
        words_out[i] = w;
    }
    return SPF_OK;
}

spf_status spf_ciphertext_to_bincode(const spf_params* p, spf_value_kind kind, const uint64_t* words, uint8_t* out, size_t cap,
                                     size_t* written)
{
    if (!p || !words || !out || !written) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_ciphertext_to_bincode: null argument");
    if (kind == SPF_VAL_GGSW1)
        return fail(nullptr, SPF_ERR_UNSUPPORTED, "L1GgswCiphertext has no wire format in the reference (not Serialize)");
    const size_t n = spf_ciphertext_words(p, kind);
    if (n == 0) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_ciphertext_to_bincode: unknown ciphertext kind");
    if (cap < 8 + 8 * n) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "spf_ciphertext_to_bincode: output buffer too small");
    uint64_t v = n;
    for (int b = 0; b < 8; b++) out[b] = (uint8_t)(v >> (8 * b));
    for (size_t i = 0; i < n; i++)
        for (int b = 0; b < 8; b++) out[8 + 8 * i + b] = (uint8_t)(words[i] >> (8 * b));
    *written = 8 + 8 * n;
    return SPF_OK;
}

// l1ggsw_zero / l1ggsw_one as `Evaluation::new` makes them (crypto/evaluation.rs:161-197): the circuit bootstrap
// of the trivial level-0 LWE of the bit, under the loaded keys.  Built once per key set, kept in HBM.
static spf_status ensure_ggsw_constants(spf_ctx* c)
{
    if (c->ggsw_const_ready) return SPF_OK;
    const size_t sw = ggsw_fft_complex(c->prm, c->prm.cbs_radix_count) * 16, lw = lwe0_words(c->prm);
    if (!c->d_ggsw_const) HIPCHK(c, hipMalloc((void**)&c->d_ggsw_const, 2 * sw));
    std::vector<uint64_t> triv(2 * lw, 0);
    triv[2 * lw - 1] = (uint64_t)1 << 63; // trivial_lwe(1, l0, 1 plaintext bit): zero mask, body = 1 << 63
    spf_status st = ensure(c, c->aux, 2 * lw * 8);
    if (st != SPF_OK) return st;
    HIPCHK(c, hipMemcpyAsync(c->aux.p, triv.data(), 2 * lw * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // `triv` goes out of scope
    st = spf_circuit_bootstrap_dev(c, c->stream, 2, (const uint64_t*)c->aux.p, c->d_ggsw_const);
    if (st != SPF_OK) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ggsw_const_ready = true;
    return SPF_OK;
}

spf_status spf_l1ggsw_constant(spf_ctx* c, int bit, double* ggsw_fft_out)
{
    if (!c || !ggsw_fft_out || (bit != 0 && bit != 1)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument or bit not 0/1");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    spf_status st = ensure_ggsw_constants(c);
    if (st != SPF_OK) return st;
    const size_t sw = ggsw_fft_complex(c->prm, c->prm.cbs_radix_count) * 16;
    HIPCHK(c, hipMemcpy(ggsw_fft_out, (const char*)c->d_ggsw_const + (size_t)bit * sw, sw, hipMemcpyDeviceToHost));
    return SPF_OK;
}

// ---------------------------------------------------------------- public functional keyswitch
// `public_functional_keyswitch` (sunscreen_tfhe/src/ops/keyswitch/public_functional_keyswitch.rs:74-148), map "message j to
// coefficient j"; the kernels and the order of the arithmetic: spf_pufks.hpp.

// `PublicFunctionalKeyswitchKey<u64>` (entities/public_functional_keyswitch_key.rs), [n][count][k+1][N] words: into the key blob as
// they are, transformed there polynomial by polynomial (`PolynomialRef::fft`, entities/polynomial.rs:257-274).  Every check runs
// before the device is touched; the context is without this key from there until the end, and after any failure.
spf_status spf_load_public_functional_keyswitch_key_std(spf_ctx* c, const uint64_t* key, size_t n_words, size_t from_dimension,
                                                        uint32_t radix_log, uint32_t radix_count)
{
    if (!c) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    c->pufks_ready = false;
    if (!key) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (const char* why = pufks_key_shape_error(from_dimension, radix_log, radix_count)) return fail(c, SPF_ERR_INVALID_ARGUMENT, why);
    const size_t want = 2 * pufks_complex(c->prm, (uint32_t)from_dimension, radix_count);
    if (n_words != want)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "public functional keyswitch key length " + std::to_string(n_words) + " words != " +
                                                     std::to_string(want));
    c->pufks_n = (uint32_t)from_dimension; c->pufks_log = radix_log; c->pufks_count = radix_count;
    void* p; size_t bytes;
    spf_status s = spf_key_blob(c, 4, &p, &bytes);
    if (s != SPF_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    auto transform = [&]() -> spf_status {
        HIPCHK(c, hipMemcpyAsync(p, key, bytes, hipMemcpyHostToDevice, c->stream));
        const size_t n_polys = n_words / c->prm.polynomial_degree, step = (size_t)1 << 30; // (a grid dimension holds 2^31 - 1)
        for (size_t at = 0; at < n_polys; at += step) {
            const size_t nb = std::min(step, n_polys - at);
            uint64_t* q = (uint64_t*)p + at * c->prm.polynomial_degree;
            spf_status st = launch_poly_fft(c, c->stream, nb, q, (c64*)q);
            if (st != SPF_OK) return st;
        }
        return SPF_OK;
    };
    s = transform();
    {
        // (no return before the stream is idle: the copy reads the caller's buffer)
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (s == SPF_OK && e != hipSuccess) s = fail(c, SPF_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    if (s == SPF_OK) s = pufks_prepare(c);
    if (s != SPF_OK) return s;
    c->pufks_ready = true;
    return SPF_OK;
}

// why (B, lwe_count) is refused, or nullptr
static const char* pufks_shape_error(const spf_params& p, size_t B, size_t lwe_count)
{
    if (lwe_count == 0) return "lwe_count must be at least 1";
    if (lwe_count > p.polynomial_degree) return "lwe_count above polynomial_degree";
    if (B > pufks_shape(p, lwe_count, 0).max_batch) return "B * lwe_count above 0x0fffffff";
    return nullptr;
}

// What every form of the public functional keyswitch checks before the batch is touched, on `c` with its texts: the pointers (never
// null, whatever B), the shape of the call, the key; *sh: the batch shape for the loaded key's from_dimension.
static spf_status pufks_args(spf_ctx* c, size_t B, size_t lwe_count, const void* in, const void* out, BatchShape* sh)
{
    if (!c || !in || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (const char* why = pufks_shape_error(c->prm, B, lwe_count)) return fail(c, SPF_ERR_INVALID_ARGUMENT, why);
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (!c->pufks_ready) return fail(c, SPF_ERR_NO_KEY, "public functional keyswitch key not loaded");
    *sh = pufks_shape(c->prm, lwe_count, c->pufks_n);
    return SPF_OK;
}

// d_rows == null: the B * p rows are contiguous at d_in.  Otherwise row b * p + j is d_rows[b * p + j] (a device table of device
// pointers, d_in unused): the pre-pass reads the rows where they lie and leaves their bodies behind the digits of the launch —
// or, given d_gather, a buffer of B * p rows (the diagnostic SPF_PUFKS_ROWS_GATHER=1: the form the scattered pre-pass was
// measured against, tools/pbs_graph_bench.py), the rows are gathered there and the contiguous pre-pass runs on the copy.  The
// pre-pass of a launch, with its gather, is one "pufks_prepass" entry of spf_last_kernel_ms.
extern "C++" template <int LOGB, int L>
static spf_status launch_pufks_tuned(spf_ctx* c, hipStream_t s, size_t B, uint32_t p, const uint64_t* d_in, uint64_t* d_out,
                                     const uint64_t* const* d_rows = nullptr, uint64_t* d_gather = nullptr)
{
    const uint64_t* const* d_gather_from = nullptr;
    if (d_rows && d_gather) { d_gather_from = d_rows; d_rows = nullptr; d_in = d_gather; }
    const uint32_t n = c->pufks_n, pstride = (p + 31u) & ~31u;
    const size_t per_output = (size_t)n * pstride * sizeof(uint32_t), row_words = (size_t)n + 1, gw = glwe_words(c->prm);
    // outputs per launch: what keeps the digits of a launch within 8 GiB of scratch (half the bytes of the inputs they come from;
    // at n = 2048, p = 1024 that is the 1024 outputs that fill every CU: with 1 GiB the 128 outputs of a launch left half the
    // CUs idle, 311 ms per 1024 outputs), a multiple of the outputs per workgroup
    size_t chunk = std::max<size_t>(4, std::min<size_t>(4096, (((size_t)8 << 30) / per_output) & ~(size_t)3));
    chunk = std::min(chunk, (B + 3) & ~(size_t)3);
    spf_status st = ensure(c, c->pufks_dig, chunk * per_output + (d_rows ? chunk * pstride * sizeof(uint64_t) : 0));
    if (st != SPF_OK) return st;
    uint64_t* d_bodies = (uint64_t*)((char*)c->pufks_dig.p + chunk * per_output); // (per_output is a multiple of 128 bytes)
    // at most one output per CU: the four-waves-per-output latency shape.  Beyond, two outputs per workgroup while the call fills at
    // most two workgroups per CU (more CUs at work on a small batch), then four: each key row then serves four outputs from one
    // trip to memory.  One shape per call, whatever its launches hold.
    const bool latency = B <= (size_t)c->n_cu, four = B > 4 * (size_t)c->n_cu;
    for (size_t at = 0; at < B; at += chunk) {
        const size_t nb = std::min(chunk, B - at);
        const uint64_t* in = d_in + at * p * row_words;
        {
            TimedScope ts(c, s, T_PUFKS_PRE);
            st = ts.begin();
            if (st != SPF_OK) return st;
            if (d_gather_from) {
                st = spf_gather_rows_dev(c, s, nb * p, row_words, d_gather_from + at * p, d_gather + at * p * row_words);
                if (st != SPF_OK) return st;
            }
            if (d_rows)
                hipLaunchKernelGGL((pufks_digits_rows_kernel<L, LOGB>), dim3((n + 31) / 32, pstride / 32, (unsigned)nb), dim3(256), 0, s,
                                   d_rows + at * p, (uint32_t*)c->pufks_dig.p, d_bodies, n, p, pstride);
            else
                hipLaunchKernelGGL((pufks_digits_kernel<L, LOGB>), dim3((n + 31) / 32, pstride / 32, (unsigned)nb), dim3(256), 0, s, in,
                                   (uint32_t*)c->pufks_dig.p, n, p, pstride);
            st = ts.end();
            if (st != SPF_OK) return st;
        }
        PufksArgs a{c->d_pufks, (const uint32_t*)c->pufks_dig.p, d_rows ? d_bodies : in + n, d_rows ? (size_t)pstride : p * row_words,
                    d_rows ? (size_t)1 : row_words, d_out + at * gw, c->d_tables, (uint32_t)nb, n, p, pstride};
        if (latency) {
            c->last_pufks_kernel = L == 8 ? "pufks4_kernel<4,8>" : "pufks4_kernel<4,4>";
            hipLaunchKernelGGL((pufks4_kernel<LOGB, L>), dim3((unsigned)nb), dim3(256), kPufks4Lds, s, a);
        } else if (!four) {
            c->last_pufks_kernel = L == 8 ? "pufks_kernel<4,8,2>" : "pufks_kernel<4,4,2>";
            hipLaunchKernelGGL((pufks_kernel<LOGB, L, 2>), dim3((unsigned)((nb + 1) / 2)), dim3(256), cmux_lds_bytes(2), s, a);
        } else {
            c->last_pufks_kernel = L == 8 ? "pufks_kernel<4,8,4>" : "pufks_kernel<4,4,4>";
            hipLaunchKernelGGL((pufks_kernel<LOGB, L, 4>), dim3((unsigned)((nb + 3) / 4)), dim3(512), cmux_lds_bytes(4), s, a);
        }
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

spf_status spf_public_functional_keyswitch_enqueue(spf_ctx* c, void* stream, size_t B, size_t lwe_count, const uint64_t* d_lwe_in,
                                                   uint64_t* d_glwe_out)
{
    BatchShape sh;
    spf_status st = pufks_args(c, B, lwe_count, d_lwe_in, d_glwe_out, &sh);
    if (st != SPF_OK) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (B == 0) return SPF_OK;
    if (batch_overlaps(sh, B, d_glwe_out, d_lwe_in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    const size_t gw = sh.out_words;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (pufks_tuned(c))
        return c->pufks_count == 8 ? launch_pufks_tuned<4, 8>(c, s, B, (uint32_t)lwe_count, d_lwe_in, d_glwe_out)
                                   : launch_pufks_tuned<4, 4>(c, s, B, (uint32_t)lwe_count, d_lwe_in, d_glwe_out);
    GenericPufksArgs ga{};
    ga.g = generic_shape(c);
    ga.key = c->d_pufks; ga.n = c->pufks_n; ga.p = (uint32_t)lwe_count; ga.radix_log = c->pufks_log; ga.count = c->pufks_count;
    c->last_pufks_kernel = "generic_pufks_kernel";
    const size_t row_words = (size_t)c->pufks_n + 1;
    for (size_t at = 0; at < B; at += kMaxGridRows) {
        const size_t nb = std::min(B - at, kMaxGridRows);
        ga.lwe_in = d_lwe_in + at * lwe_count * row_words; ga.out = d_glwe_out + at * gw;
        hipLaunchKernelGGL(generic_pufks_kernel, dim3((unsigned)nb), dim3(kGenericThreads), generic_lds_bytes(ga.g.N, ga.g.k, false), s, ga);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// diagnostic, read at every call: the hand-written radices gather scattered rows and run the contiguous pre-pass (a graph planned
// without it is planned again)
static bool pufks_rows_gather()
{
    const char* e = getenv("SPF_PUFKS_ROWS_GATHER");
    return e && e[0] == '1';
}

// A gate graph's level of spf_graph_add_public_functional_keyswitch nodes: output b = the keyswitch of the rows
// d_rows[b * p .. b * p + p) (a device table of device pointers), read where they lie.  The hand-written radices run the pointer-table
// pre-pass and the main kernel over its digits and bodies; every other key gathers the rows into d_gather (B * p rows; the graph's
// stage buffer) and runs generic_pufks_kernel on them.  *launches counts what went on the stream.
static spf_status launch_pufks_rows(spf_ctx* c, hipStream_t s, size_t B, size_t p, const uint64_t* const* d_rows, uint64_t* d_gather,
                                    uint64_t* d_out, uint32_t* launches)
{
    if (const char* why = pufks_shape_error(c->prm, B, p)) return fail(c, SPF_ERR_INVALID_ARGUMENT, why);
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (!c->pufks_ready) return fail(c, SPF_ERR_NO_KEY, "public functional keyswitch key not loaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (pufks_tuned(c)) {
        const uint32_t pstride = ((uint32_t)p + 31u) & ~31u;
        const size_t per_output = (size_t)c->pufks_n * pstride * sizeof(uint32_t);
        const size_t chunk = std::max<size_t>(4, std::min<size_t>(4096, (((size_t)8 << 30) / per_output) & ~(size_t)3));
        uint64_t* gather_into = pufks_rows_gather() ? d_gather : nullptr;
        *launches += (gather_into ? 3 : 2) * (uint32_t)((B + chunk - 1) / chunk);
        return c->pufks_count == 8 ? launch_pufks_tuned<4, 8>(c, s, B, (uint32_t)p, nullptr, d_out, d_rows, gather_into)
                                   : launch_pufks_tuned<4, 4>(c, s, B, (uint32_t)p, nullptr, d_out, d_rows, gather_into);
    }
    if (!d_gather) return fail(c, SPF_ERR_INVALID_ARGUMENT, "public functional keyswitch over scattered rows: no gather buffer");
    spf_status st = spf_gather_rows_dev(c, s, B * p, (size_t)c->pufks_n + 1, d_rows, d_gather);
    if (st != SPF_OK) return st;
    *launches += 1 + (uint32_t)((B + kMaxGridRows - 1) / kMaxGridRows);
    return spf_public_functional_keyswitch_enqueue(c, s, B, p, d_gather, d_out);
}

spf_status spf_public_functional_keyswitch_batch(spf_ctx* c, size_t B, size_t lwe_count, const uint64_t* lwe_in, uint64_t* glwe_out)
{
    BatchShape sh;
    spf_status s = pufks_args(c, B, lwe_count, lwe_in, glwe_out, &sh);
    if (s != SPF_OK) return s;
    return host_batch(c, sh, B, {{c->in, lwe_in}}, glwe_out, [&](const uint64_t* d_in, uint64_t* d_out) {
        return spf_public_functional_keyswitch_enqueue(c, c->stream, B, lwe_count, d_in, d_out);
    });
}

const char* spf_last_public_functional_keyswitch_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_pufks_kernel;
}

// ---------------------------------------------------------------- private functional keyswitch
// `private_functional_keyswitch` (sunscreen_tfhe/src/ops/keyswitch/private_functional_keyswitch.rs:107-142) and
// `circuit_bootstrap_via_pfks` (ops/bootstrapping/circuit_bootstrapping.rs:162-219); kernels and arithmetic: spf_pfks.hpp.

// `PrivateFunctionalKeyswitchKey<u64>` (entities/private_functional_keyswitch_key.rs:44-46) x n_keys, back to back (n_keys = k+1,
// lwe_count = 1, n = k N: `CircuitBootstrappingKeyswitchKeys<u64>`, entities/circuit_bootstrapping_private_keyswitch_keys.rs:28-35).
// Every check runs before the device is touched; the context is without these keys from there until the end, and after any failure.
spf_status spf_load_private_functional_keyswitch_keys_std(spf_ctx* c, const uint64_t* keys, size_t n_words, size_t n_keys,
                                                          size_t from_dimension, size_t lwe_count, uint32_t radix_log, uint32_t radix_count)
{
    if (!c) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    c->pfks_ready = false;
    if (!keys) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    size_t want = 0;
    if (const char* why = pfks_key_shape_error(c->prm, n_keys, from_dimension, lwe_count, radix_log, radix_count, &want))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, why);
    if (n_words != want)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "private functional keyswitch key length " + std::to_string(n_words) + " words != " +
                                                     std::to_string(want));
    c->pfks_keys = (uint32_t)n_keys; c->pfks_n = (uint32_t)from_dimension; c->pfks_p = (uint32_t)lwe_count;
    c->pfks_log = radix_log; c->pfks_count = radix_count;
    void* p; size_t bytes;
    spf_status s = spf_key_blob(c, 5, &p, &bytes);
    if (s != SPF_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(p, keys, bytes, hipMemcpyHostToDevice));
    s = pfks_prepare(c);
    if (s != SPF_OK) return s;
    c->pfks_ready = true;
    return SPF_OK;
}

// M rows of lwe_count * (n+1) words against `nk` keys from `key0` on, each result where `dst` places it
static spf_status launch_pfks(spf_ctx* c, hipStream_t s, size_t M, const uint64_t* d_in, uint32_t key0, uint32_t nk, PfksDest dst)
{
    const size_t W = glwe_words(c->prm), rw = pfks_row_words(c), K = pfks_K(c), Kpad = pfks_Kpad(c);
    if (!c->d_pfks_planes) {
        c->last_pfks_kernel = "pfks_valu_kernel";
        const size_t step = kMaxGridRows / dst.rows_per_item * dst.rows_per_item; // whole items per launch
        for (size_t at = 0; at < M; at += step) {
            const size_t nb = std::min(M - at, step);
            PfksDest d = dst;
            d.out += (at / dst.rows_per_item) * dst.item_stride;
            PfksValuArgs a{d_in + at * rw, c->d_pfks + (size_t)key0 * K * W, d, (uint32_t)nb, (uint32_t)W, (uint32_t)rw, c->pfks_log, c->pfks_count};
            hipLaunchKernelGGL(pfks_valu_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)((nb + PFKS_VT - 1) / PFKS_VT), nk), dim3(256), 0, s, a);
        }
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    const uint32_t U = pfks_limbs(c->pfks_log);
    // rows per launch: what keeps the limbs of a launch within kPfksDigitCap, in whole row tiles of whole items (at least one: a
    // key whose single tile of rows exceeds the cap has no planes and is served above)
    const size_t unit = (size_t)PFKS_TILE * dst.rows_per_item;
    size_t chunk = std::max<size_t>(1, kPfksDigitCap / (Kpad * U) / unit) * unit;
    if (chunk > kMaxGridRows * PFKS_TILE) chunk = std::max<size_t>(1, kMaxGridRows * PFKS_TILE / unit) * unit; // (grid.y of the GEMM)
    chunk = std::min(chunk, (M + PFKS_TILE - 1) / PFKS_TILE * PFKS_TILE); // (then one launch holds the whole call)
    const uint32_t nseg = (uint32_t)((Kpad / 128 + kPfksSegRounds - 1) / kPfksSegRounds);
    spf_status st = ensure(c, c->pfks_dig, chunk * Kpad * U);
    if (st != SPF_OK) return st;
    st = ensure(c, c->pfks_rowsum, (size_t)nseg * U * chunk * sizeof(int));
    if (st != SPF_OK) return st;
    c->last_pfks_kernel = U == 1 ? "pfks_gemm_kernel<1>" : U == 2 ? "pfks_gemm_kernel<2>" : "pfks_gemm_kernel<3>";
    const size_t ncols = (size_t)nk * W;
    for (size_t at = 0; at < M; at += chunk) {
        const size_t nb = std::min(chunk, M - at), mpad = (nb + PFKS_TILE - 1) / PFKS_TILE * PFKS_TILE;
        hipLaunchKernelGGL(pfks_digits_kernel, dim3((unsigned)mpad), dim3(256), 0, s, d_in + at * rw, (int8_t*)c->pfks_dig.p, (uint32_t)rw,
                           (uint32_t)nb, (uint32_t)mpad, c->pfks_log, c->pfks_count, U, (uint32_t)K, (uint32_t)Kpad);
        hipLaunchKernelGGL(pfks_rowsum_kernel, dim3((unsigned)mpad, nseg * U), dim3(256), 0, s, (const int8_t*)c->pfks_dig.p,
                           (int*)c->pfks_rowsum.p, (uint32_t)mpad, U, (uint32_t)Kpad, kPfksSegRounds * 128u);
        PfksDest d = dst;
        d.out += (at / dst.rows_per_item) * dst.item_stride;
        PfksGemmArgs a{(const int8_t*)c->pfks_dig.p, c->d_pfks_planes + 8 * (size_t)key0 * W * Kpad, (const int*)c->pfks_rowsum.p, d,
                       (uint32_t)nb, (uint32_t)mpad, (uint32_t)Kpad, (uint32_t)W, (uint32_t)ncols};
        const dim3 grid((unsigned)((8 * ncols + PFKS_TILE - 1) / PFKS_TILE), (unsigned)(mpad / PFKS_TILE));
        if (U == 1) hipLaunchKernelGGL(pfks_gemm_kernel<1>, grid, dim3(256), 0, s, a);
        else if (U == 2) hipLaunchKernelGGL(pfks_gemm_kernel<2>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(pfks_gemm_kernel<3>, grid, dim3(256), 0, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return SPF_OK;
}

// What every form of the private functional keyswitch checks before the batch is touched, on `c` with its texts: the pointers (never
// null, whatever B), the keys, the key index, the batch limit; *sh: the batch shape for the loaded keys' row.
static spf_status pfks_args(spf_ctx* c, size_t key_index, size_t B, const void* in, const void* out, BatchShape* sh)
{
    if (!c || !in || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (!c->pfks_ready) return fail(c, SPF_ERR_NO_KEY, "private functional keyswitch keys not loaded");
    if (key_index >= c->pfks_keys) return fail(c, SPF_ERR_INVALID_ARGUMENT, "key_index >= n_keys");
    *sh = pfks_shape(c->prm, pfks_row_words(c));
    return batch_limit(c, *sh, B);
}

spf_status spf_private_functional_keyswitch_enqueue(spf_ctx* c, void* stream, size_t key_index, size_t B, const uint64_t* d_lwe_in,
                                                    uint64_t* d_glwe_out)
{
    BatchShape sh;
    spf_status st = pfks_args(c, key_index, B, d_lwe_in, d_glwe_out, &sh);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (batch_overlaps(sh, B, d_glwe_out, d_lwe_in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    HIPCHK(c, hipSetDevice(c->device));
    return launch_pfks(c, (hipStream_t)stream, B, d_lwe_in, (uint32_t)key_index, 1, PfksDest{d_glwe_out, 1, sh.out_words, 0, 0});
}

spf_status spf_private_functional_keyswitch_batch(spf_ctx* c, size_t key_index, size_t B, const uint64_t* lwe_in, uint64_t* glwe_out)
{
    BatchShape sh;
    spf_status st = pfks_args(c, key_index, B, lwe_in, glwe_out, &sh);
    if (st != SPF_OK) return st;
    return host_batch(c, sh, B, {{c->in, lwe_in}}, glwe_out, [&](const uint64_t* d_in, uint64_t* d_out) {
        return spf_private_functional_keyswitch_enqueue(c, c->stream, key_index, B, d_in, d_out);
    });
}

// what `apply_pfks_on_ggsw_components` needs of the loaded keys, or why not; under c->mu
static spf_status pfks_components_keys(spf_ctx* c)
{
    if (!c->pfks_ready) return fail(c, SPF_ERR_NO_KEY, "private functional keyswitch keys not loaded");
    if (c->pfks_keys != c->prm.glwe_size + 1 || c->pfks_p != 1 || c->pfks_n != c->prm.glwe_size * c->prm.polynomial_degree)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "the GGSW components need n_keys = k+1, lwe_count = 1 and from_dimension = k * N");
    return SPF_OK;
}

// ... and what both of its forms check before the batch is touched: the pointers (never null), the keys, the batch limit
static spf_status pfks_components_args(spf_ctx* c, size_t B, const void* in, const void* out, BatchShape* sh)
{
    if (!c || !in || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    spf_status st = pfks_components_keys(c);
    if (st != SPF_OK) return st;
    *sh = pfks_components_shape(c->prm, pfks_row_words(c));
    return batch_limit(c, *sh, B);
}

// where launch_pfks places row (r, level) of item b of B * cbs_radix_count rows: the reference's [k+1][l_cbs][k+1][N]
static PfksDest ggsw_components_dest(const spf_params& p, uint64_t* d_ggsw)
{
    return PfksDest{d_ggsw, p.cbs_radix_count, value_words(p, SPF_VAL_GGSW1), glwe_words(p), (size_t)p.cbs_radix_count * glwe_words(p)};
}

// `apply_pfks_on_ggsw_components` (circuit_bootstrapping.rs:485-514): GGSW row (r, level) = PFKS of LWE `level` under key r.  One
// launch sequence: a row's digits are computed once and meet all k+1 keys.
spf_status spf_apply_pfks_on_ggsw_components_enqueue(spf_ctx* c, void* stream, size_t B, const uint64_t* d_lwe_in, uint64_t* d_ggsw_out)
{
    BatchShape sh;
    spf_status st = pfks_components_args(c, B, d_lwe_in, d_ggsw_out, &sh);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (batch_overlaps(sh, B, d_ggsw_out, d_lwe_in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    HIPCHK(c, hipSetDevice(c->device));
    return launch_pfks(c, (hipStream_t)stream, B * c->prm.cbs_radix_count, d_lwe_in, 0, c->pfks_keys, ggsw_components_dest(c->prm, d_ggsw_out));
}

spf_status spf_apply_pfks_on_ggsw_components_batch(spf_ctx* c, size_t B, const uint64_t* lwe_in, uint64_t* ggsw_out)
{
    BatchShape sh;
    spf_status st = pfks_components_args(c, B, lwe_in, ggsw_out, &sh);
    if (st != SPF_OK) return st;
    return host_batch(c, sh, B, {{c->in, lwe_in}}, ggsw_out, [&](const uint64_t* d_in, uint64_t* d_out) {
        return spf_apply_pfks_on_ggsw_components_enqueue(c, c->stream, B, d_in, d_out);
    });
}

// what both context forms check before the batch is touched: the pointers (never null), the keys of both stages, the radix, the limit
static spf_status cbs_via_pfks_args(spf_ctx* c, size_t B, const void* in, const void* out, BatchShape* sh)
{
    if (!c || !in || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    spf_status st = pfks_components_keys(c);
    if (st != SPF_OK) return st;
    if (!c->bsk_ready) return fail(c, SPF_ERR_NO_KEY, "bootstrap key not loaded");
    if ((uint64_t)c->prm.cbs_radix_log * c->prm.cbs_radix_count + 1 > 64)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "cbs_radix_log * cbs_radix_count above 63");
    *sh = cbs_via_pfks_shape(c->prm);
    return batch_limit(c, *sh, B);
}

// `circuit_bootstrap_via_pfks` (circuit_bootstrapping.rs:162-219): hi_noise_lwe_to_lo_noise_glwe, extract_and_rotate_lo_noise_glwe,
// apply_pfks_on_ggsw_components, then every polynomial of the integer GGSW through the library's forward transform, in place
spf_status spf_circuit_bootstrap_via_pfks_enqueue(spf_ctx* c, void* stream, size_t B, const uint64_t* d_lwe0_in, double* d_ggsw_fft_out)
{
    BatchShape sh;
    spf_status st = cbs_via_pfks_args(c, B, d_lwe0_in, d_ggsw_fft_out, &sh);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (batch_overlaps(sh, B, d_ggsw_fft_out, d_lwe0_in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    const uint32_t L = c->prm.cbs_radix_count, N = c->prm.polynomial_degree, k = c->prm.glwe_size;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t gw = glwe_words(c->prm), rw = (size_t)k * N + 1;
    st = ensure(c, c->pfks_glwe, B * gw * 8);
    if (st != SPF_OK) return st;
    st = ensure(c, c->pfks_lwe, B * L * rw * 8);
    if (st != SPF_OK) return st;
    uint64_t* d_glwe = (uint64_t*)c->pfks_glwe.p;
    uint64_t* d_rows = (uint64_t*)c->pfks_lwe.p;
    st = launch_blind_rotate(c, s, B, d_lwe0_in, c->d_cbs_lut, 0, 0, ceil_log2(L), (uint64_t)1 << 62, d_glwe, gw, false);
    if (st != SPF_OK) return st;
    for (size_t at = 0; at < B * L; at += kMaxGridRows / L * L) {
        const size_t nb = std::min(B * L - at, kMaxGridRows / L * L);
        hipLaunchKernelGGL(pfks_extract_rotate_kernel, dim3((unsigned)((rw + 255) / 256), (unsigned)nb), dim3(256), 0, s,
                           d_glwe + at / L * gw, d_rows + at * rw, N, k, L, c->prm.cbs_radix_log);
    }
    HIPCHK(c, hipGetLastError());
    uint64_t* d_ggsw = reinterpret_cast<uint64_t*>(d_ggsw_fft_out);
    st = launch_pfks(c, s, B * L, d_rows, 0, c->pfks_keys, ggsw_components_dest(c->prm, d_ggsw));
    if (st != SPF_OK) return st;
    return launch_poly_fft(c, s, B * (k + 1) * L * (k + 1), d_ggsw, reinterpret_cast<c64*>(d_ggsw));
}

spf_status spf_circuit_bootstrap_via_pfks_batch(spf_ctx* c, size_t B, const uint64_t* lwe0_in, double* ggsw_fft_out)
{
    BatchShape sh;
    spf_status st = cbs_via_pfks_args(c, B, lwe0_in, ggsw_fft_out, &sh);
    if (st != SPF_OK) return st;
    return host_batch(c, sh, B, {{c->in, lwe0_in}}, ggsw_fft_out, [&](const uint64_t* d_in, double* d_out) {
        return spf_circuit_bootstrap_via_pfks_enqueue(c, c->stream, B, d_in, d_out);
    });
}

const char* spf_last_private_functional_keyswitch_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_pfks_kernel;
}

// ---------------------------------------------------------------- plaintext linear maps over LWE ciphertexts
// `scalar_mul_ciphertext_mad` + `add_lwe_inplace` (sunscreen_tfhe/src/ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18) for an
// integer matrix; kernels and arithmetic: spf_lwe_linear.hpp.

constexpr size_t kLweLinearWeightCap = (size_t)1 << 27; // weights of one slot (1 GiB of int64 on the device)
constexpr size_t kLweLinearImageCap = (size_t)1 << 30;  // bytes of a slot's limb image, and of the byte planes of one launch
// Whether the matrix-core path is taken where both are legal.  Measured (profiles/r24_lwe_linear.md), no constant M0 separates the
// two: at K = 256 the VALU kernel wins at every M up to 1024, at K = 4096 the matrix cores win from M = 64.  The two estimates
// below, in ms per 102 450 output words per row, are fitted to the 81 measured cells of that table (K 256 .. 4096, M 1 .. 1024,
// one to three limbs) and decide 79 of them as the measurement does; the other two are within 10 % and go to the VALU kernel.
//   VALU:         K times the larger of its memory floor and its 64-bit multiplies over the rows, in groups of LWE_LINEAR_VT
//   matrix cores: the planes pass, written and read again (per input column); per 128-row tile the folds and the epilogue, and
//                 the MFMA passes (per limb and column); the output stores (per row)
// The matrix cores are taken where their estimate is below the VALU kernel's by a tenth.
static bool lwe_linear_matrix_cores_pay(size_t M, size_t K, size_t Kpad, uint32_t U)
{
    const double valu = (double)K * std::max(2.4e-4, 1.55e-5 * (double)((M + LWE_LINEAR_VT - 1) / LWE_LINEAR_VT * LWE_LINEAR_VT));
    const double tiles = (double)((M + PFKS_TILE - 1) / PFKS_TILE);
    const double mfma = 6.6e-4 * (double)Kpad + tiles * (0.27 + 2.6e-4 * U * (double)Kpad) + 0.0022 * (double)M;
    return 1.1 * mfma < valu;
}

static void lwe_linear_drop(LweLinearSlot& l)
{
    for (void* p : {(void*)l.d_w, (void*)l.d_bias, (void*)l.d_A, (void*)l.d_rs})
        if (p) (void)hipFree(p);
    l = LweLinearSlot{};
}

// Synchronous, like a key load: the slot is empty from the first check that passes until the end, and after any failure.
spf_status spf_load_lwe_linear_weights(spf_ctx* c, uint32_t slot, size_t M, size_t K, const int64_t* weights, const uint64_t* bias)
{
    if (!c) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (slot >= SPF_LWE_LINEAR_SLOTS)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "slot " + std::to_string(slot) + " >= SPF_LWE_LINEAR_SLOTS = " + std::to_string(SPF_LWE_LINEAR_SLOTS));
    if (!weights) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (M == 0 || K == 0) return fail(c, SPF_ERR_INVALID_ARGUMENT, "a weight matrix needs M >= 1 and K >= 1");
    if (M > kLweLinearWeightCap / K)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "weight matrix of " + std::to_string(M) + " x " + std::to_string(K) + " weights > the cap of " +
                                                     std::to_string(kLweLinearWeightCap) + " weights per slot");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    LweLinearSlot& l = c->lin[slot];
    lwe_linear_drop(l);
    c->lin_epoch++;
    long long lo = weights[0], hi = weights[0];
    for (size_t i = 1; i < M * K; i++) { lo = std::min<long long>(lo, weights[i]); hi = std::max<long long>(hi, weights[i]); }
    LweLinearSlot n;
    n.M = M; n.K = K;
    n.Mpad = (M + PFKS_TILE - 1) / PFKS_TILE * PFKS_TILE;
    n.Kpad = (K + 127) & ~(size_t)127;
    n.nseg = (uint32_t)((n.Kpad / 128 + kPfksSegRounds - 1) / kPfksSegRounds);
    n.U = lwe_linear_limbs(lo, hi);
    // (grid.y of the GEMM; a matrix the first path declines is served by the VALU kernel)
    if (n.U && (n.Mpad / PFKS_TILE > 65535 || n.Mpad * n.Kpad > kLweLinearImageCap / n.U)) n.U = 0;
    auto build = [&]() -> spf_status {
        HIPCHK(c, hipMalloc((void**)&n.d_w, M * K * 8));
        HIPCHK(c, hipMemcpy(n.d_w, weights, M * K * 8, hipMemcpyHostToDevice));
        if (bias) {
            HIPCHK(c, hipMalloc((void**)&n.d_bias, M * 8));
            HIPCHK(c, hipMemcpy(n.d_bias, bias, M * 8, hipMemcpyHostToDevice));
        }
        if (!n.U) return SPF_OK;
        HIPCHK(c, hipMalloc((void**)&n.d_A, (size_t)n.U * n.Mpad * n.Kpad));
        HIPCHK(c, hipMalloc((void**)&n.d_rs, (size_t)n.nseg * n.U * n.Mpad * sizeof(int)));
        hipLaunchKernelGGL(lwe_linear_limbs_kernel, dim3((unsigned)n.Mpad), dim3(256), 0, c->stream, n.d_w, n.d_A, (uint32_t)M, (uint32_t)n.Mpad,
                           (uint32_t)K, (uint32_t)n.Kpad, n.U);
        hipLaunchKernelGGL(pfks_rowsum_kernel, dim3((unsigned)n.Mpad, n.nseg * n.U), dim3(256), 0, c->stream, (const int8_t*)n.d_A, n.d_rs,
                           (uint32_t)n.Mpad, n.U, (uint32_t)n.Kpad, kPfksSegRounds * 128u);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SPF_OK;
    };
    const spf_status st = build();
    if (st != SPF_OK) {
        lwe_linear_drop(n);
        return st;
    }
    n.ready = true;
    l = n;
    return SPF_OK;
}

// What every form of the linear maps checks before the batch is touched, on `c` with its texts: the pointers (never null, whatever
// B), the slot, the kind, the weights, the batch limit; *sh: the batch shape for the slot's M and K.
static spf_status lwe_linear_args(spf_ctx* c, uint32_t slot, spf_value_kind kind, size_t B, const void* in, const void* out, BatchShape* sh)
{
    if (!c || !in || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (slot >= SPF_LWE_LINEAR_SLOTS)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "slot " + std::to_string(slot) + " >= SPF_LWE_LINEAR_SLOTS = " + std::to_string(SPF_LWE_LINEAR_SLOTS));
    if (kind != SPF_VAL_LWE0 && kind != SPF_VAL_LWE1) return fail(c, SPF_ERR_INVALID_ARGUMENT, "kind must be SPF_VAL_LWE0 or SPF_VAL_LWE1");
    if (!c->lin[slot].ready) return fail(c, SPF_ERR_NO_KEY, "no weights loaded in slot " + std::to_string(slot));
    *sh = lwe_linear_batch_shape(c->prm, c->lin[slot].M, c->lin[slot].K, kind);
    return batch_limit(c, *sh, B);
}

// Which product kernel serves a call where both are legal: SPF_LWE_LINEAR_PATH=valu | mfma (diagnostic; read at every call)
static int lwe_linear_forced_path()
{
    const char* e = getenv("SPF_LWE_LINEAR_PATH");
    return !e ? 0 : !strcmp(e, "valu") ? 1 : !strcmp(e, "mfma") ? 2 : 0;
}

spf_status spf_lwe_linear_enqueue(spf_ctx* c, void* stream, uint32_t slot, spf_value_kind kind, size_t B, const uint64_t* d_lwe_in,
                                  uint64_t* d_lwe_out)
{
    BatchShape sh;
    spf_status st = lwe_linear_args(c, slot, kind, B, d_lwe_in, d_lwe_out, &sh);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (batch_overlaps(sh, B, d_lwe_out, d_lwe_in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    const LweLinearSlot& l = c->lin[slot];
    const size_t M = l.M, K = l.K, W = value_words(c->prm, kind);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->last_lin_launches = 0;
    const size_t item_planes = 8 * W * l.Kpad; // bytes of one item's byte planes
    const bool mfma_legal = l.U != 0 && item_planes <= kLweLinearImageCap;
    const int forced = lwe_linear_forced_path();
    const bool mfma = mfma_legal && (forced == 2 || (forced == 0 && lwe_linear_matrix_cores_pay(M, K, l.Kpad, l.U)));
    if (!mfma) {
        c->last_lin_kernel = "lwe_linear_valu_kernel";
        TimedScope ts(c, s, T_LIN);
        st = ts.begin();
        if (st != SPF_OK) return st;
        const size_t rows_step = (size_t)65535 * LWE_LINEAR_VT;
        for (size_t at = 0; at < B; at += 65535) {
            const size_t nb = std::min<size_t>(B - at, 65535);
            for (size_t m0 = 0; m0 < M; m0 += rows_step) {
                const size_t nm = std::min(M - m0, rows_step);
                LweLinearValuArgs a{d_lwe_in + at * K * W, l.d_w + m0 * K, l.d_bias ? l.d_bias + m0 : nullptr, d_lwe_out + (at * M + m0) * W,
                                    (uint32_t)nm, (uint32_t)M, (uint32_t)K, (uint32_t)W};
                hipLaunchKernelGGL(lwe_linear_valu_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)((nm + LWE_LINEAR_VT - 1) / LWE_LINEAR_VT), (unsigned)nb),
                                   dim3(256), 0, s, a);
                c->last_lin_launches++;
            }
        }
        HIPCHK(c, hipGetLastError());
        return ts.end();
    }
    // items per launch: what keeps the planes of a launch within kLweLinearImageCap, the plane rows within 32 bits and grid.z
    // of the planes pass within its limit (at least one: an item whose planes exceed the cap is served above).  The 2^28 / W term
    // is a guard, not a live limit: item_planes >= 1024 W, so the cap term is at most 2^20 / W for every W.
    size_t per = std::max<size_t>(1, kLweLinearImageCap / item_planes);
    per = std::min({per, B, (size_t)65535, std::max<size_t>(1, ((size_t)1 << 28) / W)});
    st = ensure(c, c->lin_planes, ((8 * per * W + PFKS_TILE - 1) / PFKS_TILE * PFKS_TILE) * l.Kpad);
    if (st != SPF_OK) return st;
    c->last_lin_kernel = l.U == 1 ? "pfks_gemm_kernel<1>" : l.U == 2 ? "pfks_gemm_kernel<2>" : "pfks_gemm_kernel<3>";
    for (size_t at = 0; at < B; at += per) {
        const size_t nb = std::min(per, B - at);
        {
            TimedScope ts(c, s, T_LIN_PLANES);
            st = ts.begin();
            if (st != SPF_OK) return st;
            hipLaunchKernelGGL(lwe_linear_planes_kernel, dim3((unsigned)(l.Kpad / 64), (unsigned)((W + 31) / 32), (unsigned)nb), dim3(256), 0, s,
                               d_lwe_in + at * K * W, (int8_t*)c->lin_planes.p, (uint32_t)W, (uint32_t)K, (uint32_t)l.Kpad);
            c->last_lin_launches++;
            HIPCHK(c, hipGetLastError());
            st = ts.end();
            if (st != SPF_OK) return st;
        }
        TimedScope ts(c, s, T_LIN);
        st = ts.begin();
        if (st != SPF_OK) return st;
        // output row m of item q, word col, at out[q][m][col]
        uint64_t* o = d_lwe_out + at * M * W;
        PfksGemmArgs a{l.d_A, (const int8_t*)c->lin_planes.p, l.d_rs, PfksDest{o, 1, W, 0, M * W},
                       (uint32_t)M, (uint32_t)l.Mpad, (uint32_t)l.Kpad, (uint32_t)W, (uint32_t)(nb * W)};
        const dim3 grid((unsigned)((8 * nb * W + PFKS_TILE - 1) / PFKS_TILE), (unsigned)(l.Mpad / PFKS_TILE));
        if (l.U == 1) hipLaunchKernelGGL(pfks_gemm_kernel<1>, grid, dim3(256), 0, s, a);
        else if (l.U == 2) hipLaunchKernelGGL(pfks_gemm_kernel<2>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(pfks_gemm_kernel<3>, grid, dim3(256), 0, s, a);
        if (l.d_bias)
            hipLaunchKernelGGL(lwe_linear_bias_kernel, dim3((unsigned)((nb * M + 255) / 256)), dim3(256), 0, s, o, (const uint64_t*)l.d_bias,
                               (uint32_t)M, (uint32_t)W, nb * M);
        c->last_lin_launches += l.d_bias ? 2 : 1;
        HIPCHK(c, hipGetLastError());
        st = ts.end();
        if (st != SPF_OK) return st;
    }
    return SPF_OK;
}

spf_status spf_lwe_linear_batch(spf_ctx* c, uint32_t slot, spf_value_kind kind, size_t B, const uint64_t* lwe_in, uint64_t* lwe_out)
{
    BatchShape sh;
    spf_status st = lwe_linear_args(c, slot, kind, B, lwe_in, lwe_out, &sh);
    if (st != SPF_OK) return st;
    if (batch_overlaps(sh, B, lwe_out, lwe_in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    return host_batch(c, sh, B, {{c->in, lwe_in}}, lwe_out, [&](const uint64_t* d_in, uint64_t* d_out) {
        return spf_lwe_linear_enqueue(c, c->stream, slot, kind, B, d_in, d_out);
    });
}

// The product over rows that are not contiguous (a level of a gate graph, spf_graph.hpp): d_rows is a device table of
// layers * K device pointers, layer-major, d_out layers * M contiguous rows that overlap none of them.  The caller has checked
// the slot against its nodes (M, K) and M <= SPF_GRAPH_LWE_LINEAR_MAX_ROWS: ONE launch of lwe_linear_rows_kernel whatever the
// shape (layers in grid.x), the VALU product whatever the size.
static spf_status launch_lwe_linear_rows(spf_ctx* c, hipStream_t s, uint32_t slot, spf_value_kind kind, size_t layers,
                                         const uint64_t* const* d_rows, uint64_t* d_out)
{
    const LweLinearSlot& l = c->lin[slot];
    const size_t W = value_words(c->prm, kind);
    if (layers > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "graph: more than 2^31 - 1 linear layers on one level");
    c->last_lin_kernel = "lwe_linear_rows_kernel";
    TimedScope ts(c, s, T_LIN);
    spf_status st = ts.begin();
    if (st != SPF_OK) return st;
    LweLinearRowsArgs a{d_rows, l.d_w, l.d_bias, d_out, (uint32_t)l.M, (uint32_t)l.K, (uint32_t)W};
    hipLaunchKernelGGL(lwe_linear_rows_kernel, dim3((unsigned)layers, (unsigned)((l.M + LWE_LINEAR_VT - 1) / LWE_LINEAR_VT), (unsigned)((W + 255) / 256)),
                       dim3(256), 0, s, a);
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

spf_status spf_lwe_linear_slot_shape(spf_ctx* c, uint32_t slot, size_t* M, size_t* K, int* has_bias)
{
    if (!c || !M || !K || !has_bias) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (slot >= SPF_LWE_LINEAR_SLOTS)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "slot " + std::to_string(slot) + " >= SPF_LWE_LINEAR_SLOTS = " + std::to_string(SPF_LWE_LINEAR_SLOTS));
    if (!c->lin[slot].ready) return fail(c, SPF_ERR_NO_KEY, "no weights loaded in slot " + std::to_string(slot));
    *M = c->lin[slot].M;
    *K = c->lin[slot].K;
    *has_bias = c->lin[slot].d_bias != nullptr;
    return SPF_OK;
}

const char* spf_last_lwe_linear_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_lin_kernel;
}

// ---------------------------------------------------------------- plaintext polynomial linear maps over GLWE ciphertexts
// `glwe_polynomial_mad`, `glwe_scalar_mad`, `sub_glwe_ciphertexts`, `glwe_negate_inplace`, `glwe_rotate`
// (sunscreen_tfhe/src/ops/ciphertext/glwe_ciphertext_ops.rs:164-183, :189-202, :121-141, :147-156, :285-305) for a matrix of sparse
// plaintext polynomials; checks and image: spf_glwe_poly_plan.hpp, kernels and arithmetic: spf_glwe_poly.hpp.

static void glwe_poly_drop(GlwePolySlot& l)
{
    for (void* p : {(void*)l.d_offsets, (void*)l.d_terms, (void*)l.d_scalars, (void*)l.d_bias})
        if (p) (void)hipFree(p);
    l = GlwePolySlot{};
}

// Synchronous, like a key load: the slot is empty from the first device call on until the end, and after any failure there.
spf_status spf_load_glwe_poly_weights(spf_ctx* c, uint32_t slot, size_t M, size_t K, const uint32_t* offsets, const uint32_t* exponents,
                                      const int64_t* coefficients, const uint64_t* bias)
{
    if (!c) return fail(nullptr, SPF_ERR_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    const size_t N = c->prm.polynomial_degree;
    const spf_glwe_poly::Verdict v = spf_glwe_poly::validate(slot, M, K, N, offsets, exponents, coefficients);
    if (v.status != SPF_OK) return fail(c, v.status, v.message);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    GlwePolySlot& l = c->gpoly[slot];
    glwe_poly_drop(l);
    c->gpoly_epoch++;
    const spf_glwe_poly::Image im = spf_glwe_poly::pack(M, K, offsets, exponents, coefficients);
    GlwePolySlot n;
    n.M = M; n.K = K; n.terms = im.terms.size();
    n.constants_only = im.cls == spf_glwe_poly::kConstantsOnly;
    auto upload = [&](auto** dst, const void* src, size_t bytes) -> spf_status {
        if (!bytes) return SPF_OK;
        HIPCHK(c, hipMalloc((void**)dst, bytes));
        HIPCHK(c, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return SPF_OK;
    };
    spf_status st = upload(&n.d_offsets, im.offsets.data(), im.offsets.size() * sizeof(uint32_t));
    if (st == SPF_OK) st = upload(&n.d_terms, im.terms.data(), im.terms.size() * sizeof(spf_glwe_poly::Term));
    if (st == SPF_OK) st = upload(&n.d_scalars, im.scalars.data(), im.scalars.size() * 8);
    if (st == SPF_OK && bias) st = upload(&n.d_bias, bias, M * N * 8);
    if (st != SPF_OK) {
        glwe_poly_drop(n);
        return st;
    }
    n.ready = true;
    l = n;
    return SPF_OK;
}

// What every form checks before the batch is touched, on `c` with its texts: the pointers (never null, whatever B), the slot, the
// weights, the batch limit; *sh: the batch shape for the slot's M and K.
static spf_status glwe_poly_args(spf_ctx* c, uint32_t slot, size_t B, const void* in, const void* out, BatchShape* sh)
{
    if (!c || !in || !out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (slot >= SPF_GLWE_POLY_SLOTS)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "slot " + std::to_string(slot) + " >= SPF_GLWE_POLY_SLOTS = " + std::to_string(SPF_GLWE_POLY_SLOTS));
    if (!c->gpoly[slot].ready) return fail(c, SPF_ERR_NO_KEY, "no polynomial weights loaded in slot " + std::to_string(slot));
    *sh = glwe_poly_batch_shape(c->prm, c->gpoly[slot].M, c->gpoly[slot].K);
    if (batch_limit(c, *sh, B) != SPF_OK) return SPF_ERR_INVALID_ARGUMENT;
    if (batch_overlaps(*sh, B, out, in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the input");
    return SPF_OK;
}

// Which kernel serves a constants-only slot: SPF_GLWE_POLY_PATH=lds | stream (diagnostic; read at every call).  A general slot
// has the LDS kernel only.
static int glwe_poly_forced_path()
{
    const char* e = getenv("SPF_GLWE_POLY_PATH");
    return !e ? 0 : !strcmp(e, "lds") ? 1 : !strcmp(e, "stream") ? 2 : 0;
}

// ONE launch whatever B and M: the items ride grid.x (B <= 2^28 by the batch shape), M <= SPF_GLWE_POLY_MAX_ROWS keeps grid.y in
// range, and grid.z is the polynomials of a GLWE or its words in groups of 256.
spf_status spf_glwe_poly_linear_enqueue(spf_ctx* c, void* stream, uint32_t slot, size_t B, const uint64_t* d_glwe_in, uint64_t* d_glwe_out)
{
    BatchShape sh;
    spf_status st = glwe_poly_args(c, slot, B, d_glwe_in, d_glwe_out, &sh);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    const GlwePolySlot& l = c->gpoly[slot];
    const uint32_t N = c->prm.polynomial_degree, k1 = c->prm.glwe_size + 1;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the default for a constants-only slot: the stream kernel (profiles/r28_glwe_poly_linear.md)
    const bool stream_kernel = l.constants_only && glwe_poly_forced_path() != 1;
    c->last_gpoly_kernel = stream_kernel ? "glwe_poly_stream_kernel" : "glwe_poly_lds_kernel";
    TimedScope ts(c, s, T_GLWE_POLY);
    st = ts.begin();
    if (st != SPF_OK) return st;
    GlwePolyArgs a{d_glwe_in, l.d_offsets, l.d_terms, l.d_scalars, l.d_bias, d_glwe_out, (uint32_t)l.M, (uint32_t)l.K, N, k1 - 1};
    const unsigned tiles = (unsigned)((l.M + GLWE_POLY_VT - 1) / GLWE_POLY_VT);
    if (stream_kernel) hipLaunchKernelGGL(glwe_poly_stream_kernel, dim3((unsigned)B, tiles, (k1 * N + 255) / 256), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(glwe_poly_lds_kernel, dim3((unsigned)B, tiles, k1), dim3(256), 0, s, a);
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

spf_status spf_glwe_poly_linear_batch(spf_ctx* c, uint32_t slot, size_t B, const uint64_t* glwe_in, uint64_t* glwe_out)
{
    BatchShape sh;
    spf_status st = glwe_poly_args(c, slot, B, glwe_in, glwe_out, &sh);
    if (st != SPF_OK) return st;
    return host_batch(c, sh, B, {{c->in, glwe_in}}, glwe_out, [&](const uint64_t* d_in, uint64_t* d_out) {
        return spf_glwe_poly_linear_enqueue(c, c->stream, slot, B, d_in, d_out);
    });
}

// The product over GLWEs that are not contiguous (a level of a gate graph, spf_graph.hpp): d_rows is a device table of layers * K
// device pointers, layer-major, d_out layers * M contiguous GLWEs that overlap none of them.  The caller has checked the slot
// against its nodes (M, K): ONE launch whatever layers and M (layers in grid.x, M <= SPF_GLWE_POLY_MAX_ROWS keeps grid.y <= 1024).
// `arena` is the base the table's pointers were made from: the rows kernels stage 16 bytes at a time.
static spf_status launch_glwe_poly_rows(spf_ctx* c, hipStream_t s, uint32_t slot, size_t layers, const void* arena,
                                        const uint64_t* const* d_rows, uint64_t* d_out)
{
    const GlwePolySlot& l = c->gpoly[slot];
    const uint32_t N = c->prm.polynomial_degree, k1 = c->prm.glwe_size + 1;
    if (layers > 0x7fffffffu) return fail(c, SPF_ERR_INVALID_ARGUMENT, "graph: more than 2^31 - 1 polynomial linear layers on one level");
    if (((uintptr_t)arena & 15) != 0 || N < 16 || N > (uint32_t)GLWE_POLY_MAX_N)
        return fail(c, SPF_ERR_UNSUPPORTED, "graph: the polynomial linear rows kernels need GLWEs on 16 bytes and 16 <= N <= 2048");
    const bool stream_kernel = l.constants_only && glwe_poly_forced_path() != 1;
    c->last_gpoly_kernel = stream_kernel ? "glwe_poly_stream_rows_kernel" : "glwe_poly_lds_rows_kernel";
    TimedScope ts(c, s, T_GLWE_POLY);
    spf_status st = ts.begin();
    if (st != SPF_OK) return st;
    GlwePolyRowsArgs a{d_rows, l.d_offsets, l.d_terms, l.d_scalars, l.d_bias, d_out, (uint32_t)l.M, (uint32_t)l.K, N, k1 - 1};
    const unsigned tiles = (unsigned)((l.M + GLWE_POLY_VT - 1) / GLWE_POLY_VT);
    if (stream_kernel) hipLaunchKernelGGL(glwe_poly_stream_rows_kernel, dim3((unsigned)layers, tiles, (k1 * N + 255) / 256), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(glwe_poly_lds_rows_kernel, dim3((unsigned)layers, tiles, k1), dim3(256), 0, s, a);
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

spf_status spf_glwe_poly_slot_shape(spf_ctx* c, uint32_t slot, size_t* M, size_t* K, size_t* terms, int* has_bias)
{
    if (!c || !M || !K || !terms || !has_bias) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (slot >= SPF_GLWE_POLY_SLOTS)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "slot " + std::to_string(slot) + " >= SPF_GLWE_POLY_SLOTS = " + std::to_string(SPF_GLWE_POLY_SLOTS));
    if (!c->gpoly[slot].ready) return fail(c, SPF_ERR_NO_KEY, "no polynomial weights loaded in slot " + std::to_string(slot));
    *M = c->gpoly[slot].M;
    *K = c->gpoly[slot].K;
    *terms = c->gpoly[slot].terms;
    *has_bias = c->gpoly[slot].d_bias != nullptr;
    return SPF_OK;
}

const char* spf_last_glwe_poly_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_gpoly_kernel;
}

// ---------------------------------------------------------------- GLWE keyswitch, automorphism round, homomorphic trace
// `keyswitch_glwe_to_glwe` (sunscreen_tfhe/src/ops/fft_ops.rs:457-495; integer twin ops/keyswitch/glwe_keyswitch.rs:26-55), one
// round of the trace's loop (`polynomial_pow_k`, ops/polynomial/mod.rs:62-84, then the keyswitch back: ops/automorphisms/mod.rs:72-83)
// and `trace` (ops/automorphisms/mod.rs:53-85) on B GLWEs; kernels: spf_glwe_keyswitch.hpp.

static spf_status glwe_ksk_slot_check(spf_ctx* c, uint32_t slot)
{
    if (slot >= SPF_GLWE_KSK_SLOTS)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "slot " + std::to_string(slot) + " >= SPF_GLWE_KSK_SLOTS = " + std::to_string(SPF_GLWE_KSK_SLOTS));
    return SPF_OK;
}

// Synchronous, like every key load: the slot is empty from the first device call on until the end, and after any failure there.
spf_status spf_load_glwe_keyswitch_key_std(spf_ctx* c, uint32_t slot, const uint64_t* key, size_t n_words, uint32_t radix_log, uint32_t radix_count)
{
    if (!c || !key) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (spf_status s = glwe_ksk_slot_check(c, slot)) return s;
    const std::string why = glwe_ks_radix_error(radix_log, radix_count);
    if (!why.empty()) return fail(c, SPF_ERR_INVALID_ARGUMENT, "GLWE keyswitch key: " + why);
    const size_t k = c->prm.glwe_size, N = c->prm.polynomial_degree, want = k * radix_count * (k + 1) * N;
    if (n_words != want)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "GLWE keyswitch key length " + std::to_string(n_words) + " words != glwe_size * radix_count * (glwe_size + 1) * N = " +
                                                     std::to_string(want));
    HIPCHK(c, hipSetDevice(c->device));
    if (!glwe_ks_tuned(c, radix_log, radix_count))
        if (spf_status s = glwe_ks_prepare_generic(c)) return s;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    GlweKskSlot& l = c->gksk[slot];
    if (l.d_key) (void)hipFree(l.d_key);
    l = GlweKskSlot{};
    c->gksk_epoch++;
    c64* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, n_words * 8));
    // the words go in as they are (same bytes as their spectra) and are transformed in place, as the other _std loaders do
    spf_status st = SPF_OK;
    {
        const hipError_t e = hipMemcpyAsync(d, key, n_words * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) st = fail(c, SPF_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    }
    if (st == SPF_OK) st = launch_poly_fft(c, c->stream, n_words / N, (const uint64_t*)d, d);
    {
        // (no return before the stream is idle: the copy reads the caller's buffer)
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (st == SPF_OK && e != hipSuccess) st = fail(c, SPF_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    if (st != SPF_OK) {
        (void)hipFree(d);
        return st;
    }
    l.d_key = d; l.radix_log = radix_log; l.radix_count = radix_count; l.ready = true;
    return SPF_OK;
}

spf_status spf_glwe_keyswitch_slot_shape(spf_ctx* c, uint32_t slot, uint32_t* radix_log, uint32_t* radix_count)
{
    if (!c || !radix_log || !radix_count) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (spf_status s = glwe_ksk_slot_check(c, slot)) return s;
    if (!c->gksk[slot].ready) return fail(c, SPF_ERR_NO_KEY, "no GLWE keyswitch key loaded in slot " + std::to_string(slot));
    *radix_log = c->gksk[slot].radix_log;
    *radix_count = c->gksk[slot].radix_count;
    return SPF_OK;
}

// What every form of the three operations checks before the batch is touched, on `c` with its texts.  mode: GlweKsMode; `arg` the
// slot (keyswitch) or the round (automorphism).  B = 0 is SPF_OK once these hold.
static spf_status glwe_ks_args(spf_ctx* c, int mode, uint32_t arg, size_t B, const void* in, const void* out)
{
    if (!c || (B && (!in || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (mode == GLWE_KS_KEYSWITCH) {
        if (spf_status s = glwe_ksk_slot_check(c, arg)) return s;
        if (!c->gksk[arg].ready) return fail(c, SPF_ERR_NO_KEY, "no GLWE keyswitch key loaded in slot " + std::to_string(arg));
    } else {
        if (mode == GLWE_KS_AUTOMORPHISM && (arg < 1 || arg > c->log_n))
            return fail(c, SPF_ERR_INVALID_ARGUMENT, "round " + std::to_string(arg) + " outside 1 .. log2 N = " + std::to_string(c->log_n));
        if (!c->ak_ready) return fail(c, SPF_ERR_NO_KEY, "automorphism key not loaded");
        if (!glwe_ks_tuned(c, c->prm.tr_radix_log, c->prm.tr_radix_count) && !c->glwe_ks_generic_ready)
            return fail(c, SPF_ERR_UNSUPPORTED, "the context's tr_radix is served by no GLWE keyswitch kernel: " +
                                                    glwe_ks_radix_error(c->prm.tr_radix_log, c->prm.tr_radix_count));
    }
    const BatchShape sh = glwe_ks_shape(c->prm);
    if (batch_limit(c, sh, B) != SPF_OK) return SPF_ERR_INVALID_ARGUMENT;
    if (B && out != in && batch_overlaps(sh, B, out, in))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output must be the input itself or must not overlap it");
    return SPF_OK;
}

// ONE launch whatever B <= kBatchMax: four items per workgroup (hand-written) or one (generic) on grid.x; no buffer of the context.
// With `d_rows` (a level of a gate graph, spf_graph.hpp): item b is d_rows[b], a device table of B device pointers, d_in is unused and
// d_out overlaps none of the items — the planner's guarantee: operands are rows of earlier levels, a level's outputs are fresh rows
// (the rows kernels park into d_out while other workgroups still read).  Still one launch.
static spf_status glwe_ks_launch(spf_ctx* c, void* stream, int mode, uint32_t arg, size_t B, const uint64_t* d_in,
                                 const uint64_t* const* d_rows, uint64_t* d_out);

static spf_status glwe_ks_enqueue(spf_ctx* c, void* stream, int mode, uint32_t arg, size_t B, const uint64_t* d_in, uint64_t* d_out)
{
    spf_status st = glwe_ks_args(c, mode, arg, B, d_in, d_out);
    if (st != SPF_OK || B == 0) return st;
    return glwe_ks_launch(c, stream, mode, arg, B, d_in, nullptr, d_out);
}

// The same over operands where they lie; the checks of glwe_ks_args that concern the key, none on the table's contents
static spf_status launch_glwe_ks_rows(spf_ctx* c, hipStream_t s, int mode, uint32_t arg, size_t B, const uint64_t* const* d_rows, uint64_t* d_out)
{
    spf_status st = glwe_ks_args(c, mode, arg, 0, nullptr, nullptr);
    if (st != SPF_OK) return st;
    if (batch_limit(c, glwe_ks_shape(c->prm), B) != SPF_OK) return SPF_ERR_INVALID_ARGUMENT;
    if (B == 0) return SPF_OK;
    if (!d_rows || !d_out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    return glwe_ks_launch(c, s, mode, arg, B, nullptr, d_rows, d_out);
}

static spf_status glwe_ks_launch(spf_ctx* c, void* stream, int mode, uint32_t arg, size_t B, const uint64_t* d_in,
                                 const uint64_t* const* d_rows, uint64_t* d_out)
{
    spf_status st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    const bool ks = mode == GLWE_KS_KEYSWITCH;
    const uint32_t radix_log = ks ? c->gksk[arg].radix_log : c->prm.tr_radix_log, count = ks ? c->gksk[arg].radix_count : c->prm.tr_radix_count;
    const uint32_t N = c->prm.polynomial_degree, k = c->prm.glwe_size;
    const size_t ksk_len = (size_t)k * count * (k + 1) * (N / 2); // complex values of one keyswitch key
    const c64* key = ks ? c->gksk[arg].d_key : mode == GLWE_KS_AUTOMORPHISM ? c->d_ak + (size_t)(arg - 1) * ksk_len : c->d_ak;
    const uint32_t kk = mode == GLWE_KS_AUTOMORPHISM ? (N >> (arg - 1)) + 1 : 1;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    TimedScope ts(c, s, T_GLWE_KS);
    st = ts.begin();
    if (st != SPF_OK) return st;
    if (glwe_ks_tuned(c, radix_log, count)) {
        const dim3 grid((unsigned)((B + kWavesPerBlock - 1) / kWavesPerBlock)), block(512);
        if (d_rows) {
            GlweKsRowsArgs a{d_rows, d_out, key, c->d_tables, (uint32_t)B, kk};
            if (mode == GLWE_KS_TRACE) hipLaunchKernelGGL((glwe_ks_rows_kernel<6, 7, GLWE_KS_TRACE>), grid, block, kTraceLds, s, a);
            else if (mode == GLWE_KS_AUTOMORPHISM) hipLaunchKernelGGL((glwe_ks_rows_kernel<6, 7, GLWE_KS_AUTOMORPHISM>), grid, block, kTraceLds, s, a);
            else hipLaunchKernelGGL((glwe_ks_rows_kernel<6, 7, GLWE_KS_KEYSWITCH>), grid, block, kTraceLds, s, a);
            c->last_glwe_ks_kernel = "glwe_ks_rows_kernel";
        } else {
            GlweKsArgs a{d_in, d_out, key, c->d_tables, (uint32_t)B, kk};
            if (mode == GLWE_KS_TRACE) hipLaunchKernelGGL((glwe_ks_kernel<6, 7, GLWE_KS_TRACE>), grid, block, kTraceLds, s, a);
            else if (mode == GLWE_KS_AUTOMORPHISM) hipLaunchKernelGGL((glwe_ks_kernel<6, 7, GLWE_KS_AUTOMORPHISM>), grid, block, kTraceLds, s, a);
            else hipLaunchKernelGGL((glwe_ks_kernel<6, 7, GLWE_KS_KEYSWITCH>), grid, block, kTraceLds, s, a);
            c->last_glwe_ks_kernel = "glwe_ks_kernel";
        }
    } else {
        GenericGlweKsArgs a{generic_shape(c), d_in, d_out, key, radix_log, count, (uint32_t)mode, kk};
        if (d_rows) hipLaunchKernelGGL(generic_glwe_ks_rows_kernel, dim3((unsigned)B), dim3(kGenericThreads), generic_trace_lds_bytes(N, k), s, a, d_rows);
        else hipLaunchKernelGGL(generic_glwe_ks_kernel, dim3((unsigned)B), dim3(kGenericThreads), generic_trace_lds_bytes(N, k), s, a);
        c->last_glwe_ks_kernel = d_rows ? "generic_glwe_ks_rows_kernel" : "generic_glwe_ks_kernel";
    }
    HIPCHK(c, hipGetLastError());
    return ts.end();
}

static spf_status glwe_ks_batch(spf_ctx* c, int mode, uint32_t arg, size_t B, const uint64_t* in, uint64_t* out)
{
    spf_status st = glwe_ks_args(c, mode, arg, B, in, out);
    if (st != SPF_OK) return st;
    return host_batch(c, glwe_ks_shape(c->prm), B, {{c->in, in}}, out,
                      [&](const uint64_t* d_in, uint64_t* d_out) { return glwe_ks_enqueue(c, c->stream, mode, arg, B, d_in, d_out); });
}

spf_status spf_glwe_keyswitch_enqueue(spf_ctx* c, void* stream, uint32_t slot, size_t B, const uint64_t* d_glwe_in, uint64_t* d_glwe_out)
{
    return glwe_ks_enqueue(c, stream, GLWE_KS_KEYSWITCH, slot, B, d_glwe_in, d_glwe_out);
}
spf_status spf_glwe_automorphism_enqueue(spf_ctx* c, void* stream, uint32_t round, size_t B, const uint64_t* d_glwe_in, uint64_t* d_glwe_out)
{
    return glwe_ks_enqueue(c, stream, GLWE_KS_AUTOMORPHISM, round, B, d_glwe_in, d_glwe_out);
}
spf_status spf_glwe_trace_enqueue(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe_in, uint64_t* d_glwe_out)
{
    return glwe_ks_enqueue(c, stream, GLWE_KS_TRACE, 0, B, d_glwe_in, d_glwe_out);
}
spf_status spf_glwe_keyswitch_batch(spf_ctx* c, uint32_t slot, size_t B, const uint64_t* glwe_in, uint64_t* glwe_out)
{
    return glwe_ks_batch(c, GLWE_KS_KEYSWITCH, slot, B, glwe_in, glwe_out);
}
spf_status spf_glwe_automorphism_batch(spf_ctx* c, uint32_t round, size_t B, const uint64_t* glwe_in, uint64_t* glwe_out)
{
    return glwe_ks_batch(c, GLWE_KS_AUTOMORPHISM, round, B, glwe_in, glwe_out);
}
spf_status spf_glwe_trace_batch(spf_ctx* c, size_t B, const uint64_t* glwe_in, uint64_t* glwe_out)
{
    return glwe_ks_batch(c, GLWE_KS_TRACE, 0, B, glwe_in, glwe_out);
}

// ---------------------------------------------------------------- ring packing: LWE / GLWE leaves into one GLWE (spf_lwe_ring_pack_*)
// p = 2^m leaves per output through p - 1 automorphism rounds in a tree and the first log2 N - m rounds of the trace, under the
// automorphism key: the composition include/spf_hip.h states; kernels spf_lwe_ring_pack.hpp, launches and rows
// spf_lwe_ring_pack_plan.hpp.

static size_t ring_pack_leaf_words(const spf_params& p, spf_value_kind kind)
{
    return kind == SPF_VAL_LWE1 ? (size_t)p.glwe_size * p.polynomial_degree + 1 : (size_t)(p.glwe_size + 1) * p.polynomial_degree;
}

// What every form checks before anything is touched, on `c` with its texts (B = 0 is SPF_OK once these hold; pointers are the
// caller's business below).
static spf_status ring_pack_args(spf_ctx* c, spf_value_kind leaf_kind, size_t p, size_t B)
{
    if (!c) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    const size_t N = c->prm.polynomial_degree;
    if (leaf_kind != SPF_VAL_LWE1 && leaf_kind != SPF_VAL_GLWE1)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "leaf kind " + std::to_string((int)leaf_kind) + ": the leaves are SPF_VAL_LWE1 (" +
                                                     std::to_string((int)SPF_VAL_LWE1) + ") or SPF_VAL_GLWE1 (" + std::to_string((int)SPF_VAL_GLWE1) + ")");
    if (!spf_ring_pack::valid_p(p, N))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "p = " + std::to_string(p) + ": the leaves per output are a power of two in 1 .. N = " + std::to_string(N));
    if (B > kBatchMaxRows / p)
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large: B * p = " + std::to_string(B) + " * " + std::to_string(p) + " > " + std::to_string(kBatchMaxRows));
    if (!c->ak_ready) return fail(c, SPF_ERR_NO_KEY, "automorphism key not loaded");
    if (!glwe_ks_tuned(c, c->prm.tr_radix_log, c->prm.tr_radix_count) && !c->glwe_ks_generic_ready)
        return fail(c, SPF_ERR_UNSUPPORTED, "the context's tr_radix is served by no GLWE keyswitch kernel: " +
                                                glwe_ks_radix_error(c->prm.tr_radix_log, c->prm.tr_radix_count));
    return SPF_OK;
}

// the launches of one slice (spf_lwe_ring_pack_plan.hpp) on `s`; no buffer of the context
static spf_status ring_pack_slice(spf_ctx* c, hipStream_t s, const spf_ring_pack::Slice& sl, spf_value_kind leaf_kind, const uint64_t* d_leaves,
                                  uint64_t* d_scratch, uint64_t* d_out)
{
    using namespace spf_ring_pack;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    const uint32_t N = c->prm.polynomial_degree, k = c->prm.glwe_size, count = c->prm.tr_radix_count, radix_log = c->prm.tr_radix_log;
    const size_t gw = (size_t)(k + 1) * N, lw = ring_pack_leaf_words(c->prm, leaf_kind);
    const size_t ksk_len = (size_t)k * count * (k + 1) * (N / 2);
    const bool tuned = glwe_ks_tuned(c, radix_log, count);
    c->last_ring_pack_kernel = tuned ? "ring_pack_kernel" : "generic_ring_pack_kernel";
    for (const Launch& l : sl.launches) {
        const bool leaves = l.src.space == LEAVES;
        const uint64_t* src = leaves ? d_leaves + l.src.row0 * lw : d_scratch + l.src.row0 * gw; // (a launch never reads the output)
        uint64_t* dst = l.dst.space == OUT ? d_out + l.dst.row0 * gw : d_scratch + l.dst.row0 * gw;
        const uint32_t src_kind = leaves ? (uint32_t)leaf_kind : (uint32_t)RING_PACK_ROWS, src_words = (uint32_t)(leaves ? lw : gw);
        TimedScope ts(c, s, T_RING_PACK);
        spf_status st = ts.begin();
        if (st != SPF_OK) return st;
        if (l.kind == LEAF) {
            hipLaunchKernelGGL(ring_pack_leaf_kernel, dim3(l.units), dim3(256), 0, s, src, dst, l.units, src_kind, src_words, N, k, c->log_n);
        } else {
            const c64* key = c->d_ak + (size_t)(l.round - 1) * ksk_len;
            const uint32_t kk = (N >> (l.round - 1)) + 1;
            if (tuned) {
                RingPackArgs a{src, dst, key, c->d_tables, l.units, l.cnt, kk, l.x, l.rounds, src_kind, src_words};
                const dim3 grid((l.units + kWavesPerBlock - 1) / kWavesPerBlock), block(512);
                if (l.kind == COMBINE) hipLaunchKernelGGL((ring_pack_kernel<6, 7, true>), grid, block, kTraceLds, s, a);
                else hipLaunchKernelGGL((ring_pack_kernel<6, 7, false>), grid, block, kTraceLds, s, a);
            } else {
                GenericRingPackArgs a{generic_shape(c), src, dst, key, radix_log, count, l.kind == COMBINE ? 1u : 0u,
                                      l.cnt, kk, l.x, l.rounds, src_kind, src_words};
                hipLaunchKernelGGL(generic_ring_pack_kernel, dim3(l.units), dim3(kGenericThreads), generic_trace_lds_bytes(N, k), s, a);
            }
        }
        HIPCHK(c, hipGetLastError());
        st = ts.end();
        if (st != SPF_OK) return st;
    }
    return SPF_OK;
}

spf_status spf_lwe_ring_pack_scratch_words(spf_ctx* c, size_t p, size_t B, size_t* words)
{
    if (!c || !words) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const size_t N = c->prm.polynomial_degree;
    if (!spf_ring_pack::valid_p(p, N))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "p = " + std::to_string(p) + ": the leaves per output are a power of two in 1 .. N = " + std::to_string(N));
    if (B > kBatchMaxRows / p) return fail(c, SPF_ERR_INVALID_ARGUMENT, "batch too large");
    *words = spf_ring_pack::scratch_words(B, p, N, c->prm.glwe_size);
    return SPF_OK;
}

spf_status spf_lwe_ring_pack_enqueue(spf_ctx* c, void* stream, spf_value_kind leaf_kind, size_t p, size_t B, const uint64_t* d_leaves,
                                     uint64_t* d_scratch, size_t scratch_words, uint64_t* d_glwe_out)
{
    spf_status st = ring_pack_args(c, leaf_kind, p, B);
    if (st != SPF_OK || B == 0) return st;
    if (!d_leaves || !d_glwe_out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const size_t N = c->prm.polynomial_degree, k = c->prm.glwe_size, gw = (k + 1) * N;
    const size_t need = spf_ring_pack::scratch_words(B, p, N, k);
    if (scratch_words < need || (need && !d_scratch))
        return fail(c, SPF_ERR_INVALID_ARGUMENT, "scratch of " + std::to_string(d_scratch ? scratch_words : 0) + " words: B = " + std::to_string(B) +
                                                     " outputs of p = " + std::to_string(p) + " leaves need " + std::to_string(need) +
                                                     " words (spf_lwe_ring_pack_scratch_words)");
    const size_t leaf_bytes = B * p * ring_pack_leaf_words(c->prm, leaf_kind) * 8;
    if (ranges_overlap(d_glwe_out, B * gw * 8, d_leaves, leaf_bytes)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the leaves");
    if (need && ranges_overlap(d_glwe_out, B * gw * 8, d_scratch, need * 8)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the scratch");
    if (need && ranges_overlap(d_scratch, need * 8, d_leaves, leaf_bytes)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the scratch overlaps the leaves");
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return ring_pack_slice(c, (hipStream_t)stream, spf_ring_pack::plan_slice(0, B, p, N), leaf_kind, d_leaves, d_scratch, d_glwe_out);
}

spf_status spf_lwe_ring_pack_batch(spf_ctx* c, spf_value_kind leaf_kind, size_t p, size_t B, const uint64_t* leaves, uint64_t* glwe_out)
{
    spf_status st = ring_pack_args(c, leaf_kind, p, B);
    if (st != SPF_OK || B == 0) return st;
    if (!leaves || !glwe_out) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    const size_t N = c->prm.polynomial_degree, k = c->prm.glwe_size, gw = (k + 1) * N;
    const size_t leaf_bytes = B * p * ring_pack_leaf_words(c->prm, leaf_kind) * 8;
    if (ranges_overlap(glwe_out, B * gw * 8, leaves, leaf_bytes)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output overlaps the leaves");
    // the slices of the call under the cap (the slice loop is the plan's), each with the whole scratch: the stream orders them
    const std::vector<spf_ring_pack::Slice> slices = spf_ring_pack::plan(B, p, N, k, spf_ring_pack::scratch_cap_bytes());
    return host_call(c, {HostIn{c->in, leaves, leaf_bytes}}, B * gw * 8, glwe_out, [&]() -> spf_status {
        spf_status s = ensure(c, c->ring_pack_scratch, spf_ring_pack::scratch_words(slices[0].nb, p, N, k) * 8);
        for (const spf_ring_pack::Slice& sl : slices) {
            if (s != SPF_OK) break;
            s = ring_pack_slice(c, c->stream, sl, leaf_kind, (const uint64_t*)c->in.p, (uint64_t*)c->ring_pack_scratch.p, (uint64_t*)c->out.p);
        }
        return s;
    });
}

const char* spf_last_lwe_ring_pack_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_ring_pack_kernel;
}

// ---------------------------------------------------------------- one launch over items with a parameter each (spf_*_each_*)
// SampleExtract (the index), MulXN (the amount), the GLWE keyswitch (the key slot) and one automorphism round (the round) with the
// parameter PER ITEM: `params` is a HOST array of B values, read during the call.  The kernels read item i through a pointer table
// and its parameter from a table beside it (spf_kernels.hpp, spf_generic.hpp), or, for the keyswitch kernels, through the segment
// plan of spf_each_plan.hpp (spf_glwe_keyswitch.hpp); the tables of a call are built in c->each_host and travel to c->each_tab on
// the call's stream: a buffer of the context, so one stream per context, and no _enqueue form.
static_assert(spf_each::kNoRow == kGlweKsNoRow, "the plan's padding mark is the kernels'");
static_assert(sizeof(GlweKsEachUnit) == 16 && sizeof(GlweKsEachWg) == 16, "the tables lie back to back, every entry aligned");

// What every per-item form checks before anything is queued, touching nothing: every parameter under the rule of op_param (the
// text carries position and value), then the keys, the batch limit and the ranges.  B = 0 is SPF_OK.
static spf_status each_args(spf_ctx* c, int op, size_t B, const void* in, const uint64_t* params, const void* out)
{
    if (!c || !spf_ops::has_each_form(op) || (B && (!in || !params || !out))) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument");
    if (B == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    const BatchShape sh = spf_ops::each_shape(c->prm, op);
    if (batch_limit(c, sh, B) != SPF_OK) return SPF_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < B; i++) {
        uint64_t v = params[i];
        const char* why = "";
        if (spf_ops::op_param(c->prm, op, &v, &why) != SPF_OK)
            return fail(c, SPF_ERR_INVALID_ARGUMENT, "parameter " + std::to_string(i) + " of " + std::to_string(B) + " is " + std::to_string(params[i]) + ": " + why);
    }
    if (op == spf_ops::OP_GLWE_KEYSWITCH) {
        for (size_t i = 0; i < B; i++)
            if (!c->gksk[params[i]].ready)
                return fail(c, SPF_ERR_NO_KEY, "no GLWE keyswitch key loaded in slot " + std::to_string(params[i]) + " (parameter " + std::to_string(i) + " of " + std::to_string(B) + ")");
    } else if (op == spf_ops::OP_GLWE_AUTOMORPHISM) {
        if (!c->ak_ready) return fail(c, SPF_ERR_NO_KEY, "automorphism key not loaded");
        if (!glwe_ks_tuned(c, c->prm.tr_radix_log, c->prm.tr_radix_count) && !c->glwe_ks_generic_ready)
            return fail(c, SPF_ERR_UNSUPPORTED, "the context's tr_radix is served by no GLWE keyswitch kernel: " +
                                                    glwe_ks_radix_error(c->prm.tr_radix_log, c->prm.tr_radix_count));
    }
    if (batch_overlaps(sh, B, out, in)) return fail(c, SPF_ERR_INVALID_ARGUMENT, "the output must not overlap the input");
    return SPF_OK;
}

// `image` -> c->each_tab on `s`, through the pinned c->each_host.  The previous call's copy has read the pinned image before it is
// overwritten (its event; that copy stands at the head of the previous call's work); the device table is overwritten behind the
// previous call's kernels: same stream.  Under c->mu.
static spf_status each_upload(spf_ctx* c, hipStream_t s, const std::vector<char>& image)
{
    if (!c->each_ev) HIPCHK(c, hipEventCreateWithFlags(&c->each_ev, hipEventDisableTiming));
    if (c->each_ev_recorded) HIPCHK(c, hipEventSynchronize(c->each_ev));
    c->each_ev_recorded = false;
    if (c->each_host_cap < image.size()) {
        if (c->each_host) HIPCHK(c, hipHostFree(c->each_host));
        c->each_host = nullptr; c->each_host_cap = 0;
        const size_t cap = std::max<size_t>(2 * image.size(), 4096);
        HIPCHK(c, hipHostMalloc(&c->each_host, cap, hipHostMallocDefault));
        c->each_host_cap = cap;
    }
    if (spf_status st = ensure(c, c->each_tab, c->each_host_cap)) return st;
    std::memcpy(c->each_host, image.data(), image.size());
    HIPCHK(c, hipMemcpyAsync(c->each_tab.p, c->each_host, image.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->each_ev, s));
    c->each_ev_recorded = true;
    return SPF_OK;
}

// The tables of one per-item call and what its launches need to know about them.  SampleExtract and MulXN: [B] operand pointers,
// then [B] parameters of 32 bits (a MulXN amount reduced mod 2N).  Keyswitch and automorphism: per launch — one per distinct
// (radix_log, radix_count) among the slots named; the automorphism has one — the unit table, then the workgroup table of its
// segment plan (spf_each_plan.hpp: four units per workgroup for the hand-written kernel, one for the generic one).
struct EachLaunch {
    uint32_t radix_log, count;
    std::vector<uint32_t> items;
    spf_each::Plan plan;
    size_t unit_at = 0, wg_at = 0; // byte offsets of its tables in the image
};
struct EachTables {
    std::vector<char> image;
    std::vector<EachLaunch> launches;
};

// Item i is rows[i] (a HOST array of device pointers), or d_in + i * words where `rows` is null; the parameters have been checked
// (each_args, or the pool's submit).  Under c->mu: the keys' pointers and shapes are read here.
static spf_status each_build(spf_ctx* c, int op, size_t B, const uint64_t* d_in, const uint64_t* const* rows, const uint64_t* params, EachTables& t)
{
    const size_t words = spf_ops::each_shape(c->prm, op).in_words[0];
    const uint32_t N = c->prm.polynomial_degree, k = c->prm.glwe_size;
    const auto row_of = [&](size_t i) { return rows ? rows[i] : d_in + i * words; };
    std::vector<char>& image = t.image;
    std::vector<EachLaunch>& launches = t.launches;
    using Launch = EachLaunch;
    try {
        if (op == spf_ops::OP_SAMPLE_EXTRACT || op == spf_ops::OP_MUL_XN) {
            image.resize(B * 12); // [B] pointers, then [B] parameters of 32 bits
            const uint64_t** rows_out = reinterpret_cast<const uint64_t**>(image.data());
            uint32_t* par = reinterpret_cast<uint32_t*>(image.data() + B * 8);
            for (size_t i = 0; i < B; i++) {
                uint64_t v = params[i];
                const char* why = "";
                (void)spf_ops::op_param(c->prm, op, &v, &why); // (checked above; reduces a MulXN amount mod 2N)
                rows_out[i] = row_of(i);
                par[i] = (uint32_t)v;
            }
        } else {
            const bool ks = op == spf_ops::OP_GLWE_KEYSWITCH;
            for (size_t i = 0; i < B; i++) {
                const uint32_t rl = ks ? c->gksk[params[i]].radix_log : c->prm.tr_radix_log, rc = ks ? c->gksk[params[i]].radix_count : c->prm.tr_radix_count;
                auto l = std::find_if(launches.begin(), launches.end(), [&](const Launch& x) { return x.radix_log == rl && x.count == rc; });
                if (l == launches.end()) l = launches.insert(l, Launch{rl, rc, {}, {}});
                l->items.push_back((uint32_t)i);
            }
            for (Launch& l : launches) {
                const size_t ksk_len = (size_t)k * l.count * (k + 1) * (N / 2); // complex values of one keyswitch key
                l.plan = spf_each::plan(params, l.items, B, glwe_ks_tuned(c, l.radix_log, l.count) ? (uint32_t)kWavesPerBlock : 1u);
                l.unit_at = image.size();
                l.wg_at = l.unit_at + l.plan.units() * sizeof(GlweKsEachUnit);
                image.resize(l.wg_at + l.plan.workgroups() * sizeof(GlweKsEachWg));
                GlweKsEachUnit* unit = reinterpret_cast<GlweKsEachUnit*>(image.data() + l.unit_at);
                GlweKsEachWg* wg = reinterpret_cast<GlweKsEachWg*>(image.data() + l.wg_at);
                for (size_t u = 0; u < l.plan.units(); u++) unit[u] = {row_of(l.plan.unit_item[u]), l.plan.unit_out[u], 0};
                for (size_t w = 0; w < l.plan.workgroups(); w++) {
                    const uint64_t p = l.plan.wg_param[w];
                    if (ks) wg[w] = {c->gksk[p].d_key, 1u, 0};
                    else wg[w] = {c->d_ak + (size_t)(p - 1) * ksk_len, (N >> (p - 1)) + 1, 0};
                }
            }
        }
    } catch (const std::bad_alloc&) {
        return fail(c, SPF_ERR_HIP, "out of host memory for the tables of a per-item launch");
    }
    return SPF_OK;
}

// The launches of a call over its tables at `base` (device-visible: c->each_tab, or a pool's pinned table).  SampleExtract and
// MulXN: one launch whatever B.  Keyswitch: one launch per distinct radix shape, the
// hand-written kernel at 6 x 7 bits on a tuned context, the generic one elsewhere; automorphism: one launch.  Under c->mu.
static spf_status each_run(spf_ctx* c, hipStream_t s, int op, size_t B, const char* base, const EachTables& t, uint64_t* d_out)
{
    spf_status st;
    const uint32_t N = c->prm.polynomial_degree, k = c->prm.glwe_size;
    const std::vector<EachLaunch>& launches = t.launches;
    using Launch = EachLaunch;
    if (op == spf_ops::OP_SAMPLE_EXTRACT || op == spf_ops::OP_MUL_XN) {
        const uint64_t* const* d_rows = reinterpret_cast<const uint64_t* const*>(base);
        const uint32_t* d_par = reinterpret_cast<const uint32_t*>(base + B * 8);
        const unsigned gy = (unsigned)std::min(B, kMaxGridRows); // (the kernels stride over the items: one launch whatever B)
        if (op == spf_ops::OP_SAMPLE_EXTRACT) {
            if (c->generic) hipLaunchKernelGGL(generic_sample_extract_each_kernel, dim3((k * N + 1 + 255) / 256, gy), dim3(256), 0, s, d_rows, d_par, d_out, (uint32_t)B, N, k);
            else hipLaunchKernelGGL(sample_extract_each_kernel, dim3((kN + 1 + 255) / 256, gy), dim3(256), 0, s, d_rows, d_par, d_out, (uint32_t)B);
        } else {
            if (c->generic) hipLaunchKernelGGL(generic_mul_xn_each_kernel, dim3(((k + 1) * N + 255) / 256, gy), dim3(256), 0, s, d_rows, d_par, d_out, (uint32_t)B, N, c->log_n, k);
            else hipLaunchKernelGGL(glwe_mul_xn_each_kernel, dim3(2 * kN / 256, gy), dim3(256), 0, s, d_rows, d_par, d_out, (uint32_t)B);
        }
        HIPCHK(c, hipGetLastError());
        return SPF_OK;
    }
    const int mode = op == spf_ops::OP_GLWE_KEYSWITCH ? GLWE_KS_KEYSWITCH : GLWE_KS_AUTOMORPHISM;
    for (const Launch& l : launches) {
        const GlweKsEachUnit* d_unit = reinterpret_cast<const GlweKsEachUnit*>(base + l.unit_at);
        const GlweKsEachWg* d_wg = reinterpret_cast<const GlweKsEachWg*>(base + l.wg_at);
        const dim3 grid((unsigned)l.plan.workgroups());
        TimedScope ts(c, s, T_GLWE_KS);
        st = ts.begin();
        if (st != SPF_OK) return st;
        if (glwe_ks_tuned(c, l.radix_log, l.count)) {
            GlweKsEachArgs a{d_unit, d_wg, d_out, c->d_tables};
            if (mode == GLWE_KS_AUTOMORPHISM) hipLaunchKernelGGL((glwe_ks_each_kernel<6, 7, GLWE_KS_AUTOMORPHISM>), grid, dim3(512), kTraceLds, s, a);
            else hipLaunchKernelGGL((glwe_ks_each_kernel<6, 7, GLWE_KS_KEYSWITCH>), grid, dim3(512), kTraceLds, s, a);
            c->last_glwe_ks_kernel = "glwe_ks_each_kernel";
        } else {
            GenericGlweKsArgs a{generic_shape(c), nullptr, d_out, nullptr, l.radix_log, l.count, (uint32_t)mode, 0};
            hipLaunchKernelGGL(generic_glwe_ks_each_kernel, grid, dim3(kGenericThreads), generic_trace_lds_bytes(N, k), s, a, d_unit, d_wg);
            c->last_glwe_ks_kernel = "generic_glwe_ks_each_kernel";
        }
        HIPCHK(c, hipGetLastError());
        st = ts.end();
        if (st != SPF_OK) return st;
    }
    return SPF_OK;
}

// The checks, the tables, the launches: B consecutive items at d_in, row i of d_out the result of item i under params[i]
static spf_status each_enqueue(spf_ctx* c, void* stream, int op, size_t B, const uint64_t* d_in, const uint64_t* params, uint64_t* d_out)
{
    spf_status st = each_args(c, op, B, d_in, params, d_out);
    if (st != SPF_OK || B == 0) return st;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    EachTables t;
    st = each_build(c, op, B, d_in, nullptr, params, t);
    if (st != SPF_OK) return st;
    st = each_upload(c, (hipStream_t)stream, t.image);
    if (st != SPF_OK) return st;
    return each_run(c, (hipStream_t)stream, op, B, static_cast<const char*>(c->each_tab.p), t, d_out);
}

// The same for a batch of a pool with mixed parameters (spf_pool_set_mixed_parameters): item i is rows[i], wherever it lies (by
// handle), or row i of the staged block d_in (by host pointer); the tables go to `table`, pinned memory of the batch's set that the
// kernels read in place (no buffer of the context: the pool's batches run on their sets' streams side by side).  The parameters
// and the keys were checked at the submits.
static spf_status each_launch_pool(spf_ctx* c, hipStream_t s, int op, size_t B, const uint64_t* d_in, const uint64_t* const* rows,
                                   const uint64_t* params, void* table, size_t table_bytes, uint64_t* d_out)
{
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    EachTables t;
    spf_status st = each_build(c, op, B, d_in, rows, params, t);
    if (st != SPF_OK) return st;
    if (t.image.size() > table_bytes) return fail(c, SPF_ERR_HIP, "the tables of a mixed-parameter batch outgrow the set's pinned table");
    std::memcpy(table, t.image.data(), t.image.size());
    return each_run(c, s, op, B, static_cast<const char*>(table), t, d_out);
}

static spf_status each_batch(spf_ctx* c, int op, size_t B, const uint64_t* in, const uint64_t* params, uint64_t* out)
{
    spf_status st = each_args(c, op, B, in, params, out);
    if (st != SPF_OK) return st;
    return host_batch(c, spf_ops::each_shape(c->prm, op), B, {{c->in, in}}, out,
                      [&](const uint64_t* d_in, uint64_t* d_out) { return each_enqueue(c, c->stream, op, B, d_in, params, d_out); });
}

spf_status spf_sample_extract_l1_each_batch(spf_ctx* c, size_t B, const uint64_t* glwe_in, const uint64_t* idx, uint64_t* lwe1_out)
{
    return each_batch(c, spf_ops::OP_SAMPLE_EXTRACT, B, glwe_in, idx, lwe1_out);
}
spf_status spf_sample_extract_l1_each_devptr(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe_in, const uint64_t* idx, uint64_t* d_lwe1_out)
{
    return each_enqueue(c, stream, spf_ops::OP_SAMPLE_EXTRACT, B, d_glwe_in, idx, d_lwe1_out);
}
spf_status spf_glwe_mul_xn_each_batch(spf_ctx* c, size_t B, const uint64_t* glwe_in, const uint64_t* amounts, uint64_t* glwe_out)
{
    return each_batch(c, spf_ops::OP_MUL_XN, B, glwe_in, amounts, glwe_out);
}
spf_status spf_glwe_mul_xn_each_devptr(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe_in, const uint64_t* amounts, uint64_t* d_glwe_out)
{
    return each_enqueue(c, stream, spf_ops::OP_MUL_XN, B, d_glwe_in, amounts, d_glwe_out);
}
spf_status spf_glwe_keyswitch_each_batch(spf_ctx* c, size_t B, const uint64_t* glwe_in, const uint64_t* slots, uint64_t* glwe_out)
{
    return each_batch(c, spf_ops::OP_GLWE_KEYSWITCH, B, glwe_in, slots, glwe_out);
}
spf_status spf_glwe_keyswitch_each_devptr(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe_in, const uint64_t* slots, uint64_t* d_glwe_out)
{
    return each_enqueue(c, stream, spf_ops::OP_GLWE_KEYSWITCH, B, d_glwe_in, slots, d_glwe_out);
}
spf_status spf_glwe_automorphism_each_batch(spf_ctx* c, size_t B, const uint64_t* glwe_in, const uint64_t* rounds, uint64_t* glwe_out)
{
    return each_batch(c, spf_ops::OP_GLWE_AUTOMORPHISM, B, glwe_in, rounds, glwe_out);
}
spf_status spf_glwe_automorphism_each_devptr(spf_ctx* c, void* stream, size_t B, const uint64_t* d_glwe_in, const uint64_t* rounds, uint64_t* d_glwe_out)
{
    return each_enqueue(c, stream, spf_ops::OP_GLWE_AUTOMORPHISM, B, d_glwe_in, rounds, d_glwe_out);
}

const char* spf_last_glwe_keyswitch_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_glwe_ks_kernel;
}

const char* spf_last_blind_rotate_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_pbs_kernel; // string literals: valid for the life of the library
}

const char* spf_last_cmux_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_cmux_kernel;
}

const char* spf_last_keyswitch_kernel(spf_ctx* c)
{
    if (!c) return "";
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return c->last_ks_kernel;
}

} // extern "C"

// ---------------------------------------------------------------- call-coalescing pool
// what a pool's launcher thread calls for a batch of a staging set: the set's own stream and intermediates, so that the batches of
// several sets run on the GPU at the same time, and the shape of the whole population of callers (per_wg_hint, launch_blind_rotate)
static spf_status pool_keyswitch(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_in, uint64_t* d_out, Scratch* sc)
{
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return launch_keyswitch(c, s, B, d_in, d_out, sc);
}
static spf_status pool_circuit_bootstrap(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_lwe, double* d_ggsw, Scratch* sc,
                                         int per_wg_hint)
{
    if (B == 0) return SPF_OK;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return circuit_bootstrap_chain(c, s, B, d_lwe, d_ggsw, sc, per_wg_hint);
}
// a set's intermediates sized for `cap` operations up front (growing them later would hipFree, i.e. wait for the whole device,
// with other batches in flight)
static spf_status scratch_reserve(spf_ctx* c, Scratch& sc, size_t cap, bool keyswitch, bool circuit_bootstrap)
{
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    spf_status st = SPF_OK;
    if (keyswitch && c->d_ksk_planes) {
        const size_t K = (size_t)c->prm.glwe_size * c->prm.polynomial_degree * c->prm.ks_radix_count;
        const size_t mpad = (cap + KSG_TILE - 1) / KSG_TILE * KSG_TILE;
        st = ensure(c, sc.ks_dig, mpad * K);
        if (st == SPF_OK) st = ensure(c, sc.ks_rowsum, mpad * sizeof(int));
    }
    if (st == SPF_OK && circuit_bootstrap) {
        st = ensure(c, sc.cbs_glwe, cap * glwe_words(c->prm) * 8);
        if (st == SPF_OK) st = ensure(c, sc.cbs_glev, cap * c->prm.cbs_radix_count * glwe_words(c->prm) * 8);
    }
    return st;
}
static spf_status pool_copy_in(spf_ctx* c, hipStream_t s, const void* src, void* dst, size_t bytes)
{
    const size_t words = bytes / 8;
    if (words == 0) return SPF_OK;
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 4 * (size_t)c->n_cu);
    hipLaunchKernelGGL(copy_words_kernel, dim3(blocks), dim3(256), 0, s, (const uint64_t*)src, (uint64_t*)dst, words);
    return hipGetLastError() == hipSuccess ? SPF_OK : SPF_ERR_HIP;
}
static void scratch_free(Scratch& sc)
{
    for (DevBuf* b : {&sc.ks_dig, &sc.ks_rowsum, &sc.cbs_glwe, &sc.cbs_glev}) {
        if (b->p) (void)hipFree(b->p);
        *b = DevBuf{};
    }
}

#include "spf_values.hpp"
#include "spf_pool.hpp"

extern "C" {

spf_status spf_pool_create(spf_ctx* c, size_t max_batch, uint32_t max_wait_us, spf_pool** out)
{
    if (!c || !out || max_batch == 0) return fail(c, SPF_ERR_INVALID_ARGUMENT, "null argument or max_batch == 0");
    spf_pool* p = new (std::nothrow) spf_pool();
    if (!p) return fail(c, SPF_ERR_HIP, "out of host memory");
    p->ctx = c; p->prm = c->prm; p->max_batch = max_batch;
    p->max_inflight = 4 * max_batch; // flow control: cf. the reference's bounded token channel (circuit_processor/mod.rs:139)
    p->max_wait = std::chrono::microseconds(max_wait_us);
    if (const char* e = getenv("SPF_POOL_GROUPS")) p->groups = (size_t)std::min(std::max(1, atoi(e)), spf_pool_impl::kMaxGroups);
    if (const char* e = getenv("SPF_POOL_PACE")) p->pace_div = atoi(e); // (experiments: -1 = no pacing)
    if (const char* e = getenv("SPF_POOL_SETS")) p->n_sets = std::min(std::max(1, atoi(e)), (int)spf_pool_impl::kSets);
    if (const char* e = getenv("SPF_POOL_SPLIT")) p->split = (size_t)std::min(std::max(1, atoi(e)), 16);
    if (const char* e = getenv("SPF_POOL_SPIN_US")) p->spin_us = std::max(0, atoi(e));
    if (const char* e = getenv("SPF_POOL_DEF_HEAVY")) p->max_def_heavy = std::max(0, atoi(e));
    if (const char* e = getenv("SPF_POOL_TABLE_SETS")) p->n_table_sets = std::min(std::max(1, atoi(e)), (int)spf_pool::kTableSets);
    if (const char* e = getenv("SPF_POOL_HOT_US")) p->hot_us = std::max(0, atoi(e)); // (0: the launcher never polls; completers complete every batch)
    if (const char* e = getenv("SPF_GLWE_KS_ROWS_GATHER")) p->glwe_ks_rows_gather = e[0] && e[0] != '0'; // (diagnostic: see enqueue_v)
    bool streams_ok = hipSetDevice(c->device) == hipSuccess && p->create_def_streams();
    for (auto& set : p->sets)
        streams_ok = streams_ok && hipStreamCreateWithFlags(&set.sk, hipStreamNonBlocking) == hipSuccess;
    if (!streams_ok) {
        p->free_sets();
        p->destroy_def_streams();
        delete p;
        return fail(c, SPF_ERR_HIP, "spf_pool_create: cannot create the pool's streams");
    }
    // Do the sets' streams really run side by side?  The library asks for GPU_MAX_HW_QUEUES=24 when it is loaded, but a host that
    // initialised HIP earlier keeps the runtime's default (4): the pool's resident batches then take turns (0.35-0.50 of the
    // device-resident rate instead of 0.8-0.97, profiles/r05_pool.md).  Measured, not guessed: a 200 us spin kernel on every
    // set's stream at once; streams that share a hardware queue run them one after the other.
    {
        const int n = spf_pool_impl::kSets;
        const uint64_t ticks = 20000; // 200 us of the 100 MHz constant-rate counter
        hipEvent_t e0 = nullptr, e1[spf_pool_impl::kSets] = {};
        bool ok = hipEventCreate(&e0) == hipSuccess;
        for (int i = 0; ok && i < n; i++) ok = hipEventCreate(&e1[i]) == hipSuccess;
        if (ok) {
            for (int i = 0; i < n; i++) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, p->sets[i].sk, (uint64_t)100); // (code object loaded, queues created)
            for (int i = 0; i < n; i++) (void)hipStreamSynchronize(p->sets[i].sk);
            // (the best of three: a device that is busy with somebody else's kernels delays the probe's, which reads as "serialised")
            for (int attempt = 0; attempt < 3 && p->stream_concurrency < n; attempt++) {
                (void)hipEventRecord(e0, p->sets[0].sk);
                (void)hipStreamSynchronize(p->sets[0].sk);
                for (int i = 0; i < n; i++) {
                    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, p->sets[i].sk, ticks);
                    (void)hipEventRecord(e1[i], p->sets[i].sk);
                }
                float worst = 0.f;
                for (int i = 0; i < n; i++) {
                    float ms = 0.f;
                    if (hipEventSynchronize(e1[i]) == hipSuccess && hipEventElapsedTime(&ms, e0, e1[i]) == hipSuccess) worst = std::max(worst, ms);
                }
                if (worst > 0.f) p->stream_concurrency = std::max(p->stream_concurrency, (int)std::min<double>(n, std::max(1.0, std::round(n * 0.2 / worst))));
            }
        }
        (void)hipGetLastError();
        if (e0) (void)hipEventDestroy(e0);
        for (hipEvent_t e : e1)
            if (e) (void)hipEventDestroy(e);
        if (p->stream_concurrency > 0 && p->stream_concurrency <= 5) { // (the runtime's default is four hardware queues)
            const char* q = getenv("GPU_MAX_HW_QUEUES");
            fail(c, SPF_OK, std::string("spf_pool_create: WARNING: only ~") + std::to_string(p->stream_concurrency) + " of the pool's " + std::to_string(n) +
                                " streams run concurrently (GPU_MAX_HW_QUEUES=" + (q ? q : "unset") +
                                " took effect too late or is too small: export GPU_MAX_HW_QUEUES=24 before the process first touches HIP); "
                                "resident batches will take turns");
        }
    }
    try {
        p->arena = std::make_shared<spf_value_impl::Arena>();
        p->arena->device = c->device;
        if (const char* e = getenv("SPF_VALUE_CACHE_MB")) p->arena->cache_limit = (size_t)std::max(0L, atol(e)) << 20;
        p->launcher = std::thread([p] {
            p->launch_loop();
            std::lock_guard<spf_pool::Mutex> lk(p->mu);
            p->launcher_gone = true;
            for (auto& cv : p->cv_fly) cv.notify_all();
        });
        for (int i = 0; i < spf_pool_impl::kSets; i++) p->completers[i] = std::thread([p, i] { p->complete_loop(i); });
    } catch (const std::exception& e) { // std::system_error: no thread to be had — must not cross extern "C"
        {
            std::lock_guard<spf_pool::Mutex> lk(p->mu);
            p->stop = true;
            p->launcher_gone = !p->launcher.joinable();
        }
        p->work_epoch++;
        p->cv_work.notify_all();
        if (p->launcher.joinable()) p->launcher.join();
        for (auto& cv : p->cv_fly) cv.notify_all();
        for (auto& t : p->completers)
            if (t.joinable()) t.join();
        p->free_sets();
        p->destroy_def_streams();
        delete p;
        return fail(c, SPF_ERR_HIP, std::string("spf_pool_create: cannot start the pool threads: ") + e.what());
    }
    ctx_retain(c); // (the pool's threads use the context's stream, mutex and scratch: it stays until spf_pool_destroy)
    *out = p;
    return SPF_OK;
}

spf_status spf_pool_set_max_inflight(spf_pool* p, size_t max_inflight)
{
    if (!p || max_inflight == 0) return SPF_ERR_INVALID_ARGUMENT;
    if (!p->members.empty()) { // a group pool: the bound applies to every member
        for (spf_pool* q : p->members) (void)spf_pool_set_max_inflight(q, max_inflight);
        return SPF_OK;
    }
    std::lock_guard<spf_pool::Mutex> lk(p->mu);
    p->max_inflight = max_inflight;
    p->cv_space.notify_all();
    return SPF_OK;
}

spf_status spf_pool_set_mixed_parameters(spf_pool* p, int on)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    if (!p->members.empty()) { // a group pool: every member, or none — refused as soon as one member has seen a submit
        for (spf_pool* q : p->members) {
            std::lock_guard<spf_pool::Mutex> lk(q->mu);
            if (q->submitted) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_pool_set_mixed_parameters: only before the pool's first submit");
        }
        for (spf_pool* q : p->members) (void)spf_pool_set_mixed_parameters(q, on);
        return SPF_OK;
    }
    std::lock_guard<spf_pool::Mutex> lk(p->mu);
    if (p->submitted) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_pool_set_mixed_parameters: only before the pool's first submit");
    p->mixed_parameters = on != 0;
    return SPF_OK;
}

static void group_release(struct spf_group* g); // spf_group.hpp

void spf_pool_destroy(spf_pool* p)
{
    if (!p) return;
    if (!p->members.empty()) { // a group pool owns one pool per member and no threads of its own
        for (spf_pool* q : p->members) spf_pool_destroy(q);
        spf_group* grp = p->grp;
        delete p;
        group_release(grp);
        return;
    }
    spf_ctx* ctx = p->ctx;
    {
        std::lock_guard<spf_pool::Mutex> lk(p->mu);
        p->stop = true;
    }
    // wake everything that can be parked on this pool: the launcher (it closes and enqueues what is pending, then
    // leaves), producers blocked on back-pressure or on a staging set (they return an error), and waiters (their
    // batches complete: the completion thread outlives the launcher)
    p->work_epoch++;
    p->cv_work.notify_all();
    p->cv_space.notify_all();
    p->cv_set.notify_all();
    if (p->launcher.joinable()) p->launcher.join();
    for (auto& cv : p->cv_fly) cv.notify_all();
    for (auto& t : p->completers)
        if (t.joinable()) t.join();
    {
        // nobody may still be inside submit() / spf_pool_wait() on the mutex and condition variables freed below
        std::unique_lock<spf_pool::Mutex> lk(p->mu);
        p->cv_set.notify_all();
        p->cv_idle.wait(lk, [&] { return p->blocked.load() == 0; });
        for (auto& b : p->collecting) // batches with tickets nobody collected
            b->destroy_events();
    }
    p->free_sets();
    p->destroy_def_streams();
    if (p->arena) p->arena->close(); // cached blocks go back to the driver; values still alive free theirs when they are released
    delete p;
    ctx_release(ctx);
}

} // extern "C"

// the pool an operation of the calling thread goes to: the pool itself, or — a group pool — the thread's home member
// (defined with the group, spf_group.hpp)
static spf_pool* pool_deal(spf_pool* top, int* member);

// The keys of a GLWE keyswitch, automorphism round or trace, looked at when the operation is SUBMITTED to the pool of context `c`
// (under the context's lock, let go again before the operation is queued): an empty slot or no automorphism key is
// SPF_ERR_NO_KEY with the batch entry points' text, and nothing is queued.  The launch reads the slot again — at run time, as a
// gate graph does; a caller that reloads a slot waits for its submissions on it first (spf_hip.h).  Any other operation: SPF_OK.
// `ks_shape`: the radix shape of a keyswitch's slot as it is now, (radix_log << 32) | radix_count — what a pool with mixed parameters
// keys its keyswitch batches by.
static spf_status pool_glwe_ks_keys(spf_ctx* c, int op, uint64_t param, uint64_t* ks_shape)
{
    *ks_shape = 0;
    if (!spf_ops::rows_in_place(op)) return SPF_OK;
    const int mode = op == spf_ops::OP_GLWE_KEYSWITCH ? GLWE_KS_KEYSWITCH : op == spf_ops::OP_GLWE_AUTOMORPHISM ? GLWE_KS_AUTOMORPHISM : GLWE_KS_TRACE;
    std::lock_guard<std::recursive_mutex> g(c->mu); // (the lock glwe_ks_args takes: the shape is read under the hold that checked the key)
    const spf_status st = glwe_ks_args(c, mode, (uint32_t)param, 0, nullptr, nullptr);
    if (st == SPF_OK && mode == GLWE_KS_KEYSWITCH) *ks_shape = (uint64_t)c->gksk[param].radix_log << 32 | c->gksk[param].radix_count;
    return st;
}

// a host-pointer submit: the null and parameter checks of every wrapper below, then the operation goes to the pool the calling
// thread is dealt to.  (Refusals are a bare status: no message is set.)
static spf_status pool_submit(spf_pool* p, int op, std::initializer_list<const void*> in, void* out, uint64_t* ticket, uint64_t param = 0)
{
    if (!p || !out || !ticket) return SPF_ERR_INVALID_ARGUMENT;
    const void* src[3] = {nullptr, nullptr, nullptr};
    size_t k = 0;
    for (const void* x : in) {
        if (!x) return SPF_ERR_INVALID_ARGUMENT;
        src[k++] = x;
    }
    const char* why = nullptr;
    if (spf_ops::op_param(p->prm, op, &param, &why) != SPF_OK) return SPF_ERR_INVALID_ARGUMENT;
    int member = 0;
    spf_pool* q = pool_deal(p, &member);
    if (!q) return SPF_ERR_HIP; // no member of the group is in rotation
    uint64_t ks_shape;
    if (spf_status ks = pool_glwe_ks_keys(q->ctx, op, param, &ks_shape)) return ks;
    const spf_status st = q->submit_impl(op, false, src, out, nullptr, nullptr, ticket, param, ks_shape);
    if (st == SPF_OK && q != p) *ticket |= (uint64_t)member << spf_pool::kMemberShift;
    return st;
}

extern "C" {

// one per `FheOp` kind of `CircuitProcessor::exec_op` (circuit_processor/mod.rs:341-540), and the KeyswitchL1toL0 -> CircuitBootstrap chain
spf_status spf_pool_submit_keyswitch(spf_pool* p, const uint64_t* in, uint64_t* out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_KEYSWITCH, {in}, out, ticket);
}
spf_status spf_pool_submit_circuit_bootstrap(spf_pool* p, const uint64_t* in, double* out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_CBS, {in}, out, ticket);
}
spf_status spf_pool_submit_keyswitch_circuit_bootstrap(spf_pool* p, const uint64_t* in, double* out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_GATE_CBS, {in}, out, ticket);
}
spf_status spf_pool_submit_cmux(spf_pool* p, const double* sel, const uint64_t* a, const uint64_t* b, uint64_t* out,
                                uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_CMUX, {sel, a, b}, out, ticket);
}
spf_status spf_pool_submit_sample_extract(spf_pool* p, const uint64_t* glwe_in, size_t idx, uint64_t* lwe1_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_SAMPLE_EXTRACT, {glwe_in}, lwe1_out, ticket, idx);
}
spf_status spf_pool_submit_not(spf_pool* p, const uint64_t* glwe_in, uint64_t* glwe_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_NOT, {glwe_in}, glwe_out, ticket);
}
spf_status spf_pool_submit_glwe_add(spf_pool* p, const uint64_t* a, const uint64_t* b, uint64_t* glwe_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_GLWE_ADD, {a, b}, glwe_out, ticket);
}
spf_status spf_pool_submit_mul_xn(spf_pool* p, const uint64_t* glwe_in, size_t n, uint64_t* glwe_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_MUL_XN, {glwe_in}, glwe_out, ticket, n);
}
spf_status spf_pool_submit_multiply_ggsw_glwe(spf_pool* p, const double* ggsw_fft, const uint64_t* glwe, uint64_t* glwe_out,
                                              uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_MULTIPLY_GGSW_GLWE, {ggsw_fft, glwe}, glwe_out, ticket);
}
spf_status spf_pool_submit_glev_cmux(spf_pool* p, const double* sel_ggsw_fft, const uint64_t* a, const uint64_t* b, uint64_t* glev_out,
                                     uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_GLEV_CMUX, {sel_ggsw_fft, a, b}, glev_out, ticket);
}
spf_status spf_pool_submit_scheme_switch(spf_pool* p, const uint64_t* glev_in, double* ggsw_fft_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_SCHEME_SWITCH, {glev_in}, ggsw_fft_out, ticket);
}
// (the slot / the round is part of the lane's key, as the SampleExtract index is: callers with different ones never share a launch)
spf_status spf_pool_submit_glwe_keyswitch(spf_pool* p, uint32_t slot, const uint64_t* glwe_in, uint64_t* glwe_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_GLWE_KEYSWITCH, {glwe_in}, glwe_out, ticket, slot);
}
spf_status spf_pool_submit_glwe_automorphism(spf_pool* p, uint32_t round, const uint64_t* glwe_in, uint64_t* glwe_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_GLWE_AUTOMORPHISM, {glwe_in}, glwe_out, ticket, round);
}
spf_status spf_pool_submit_glwe_trace(spf_pool* p, const uint64_t* glwe_in, uint64_t* glwe_out, uint64_t* ticket)
{
    return pool_submit(p, spf_ops::OP_GLWE_TRACE, {glwe_in}, glwe_out, ticket);
}

spf_status spf_pool_wait(spf_pool* p, uint64_t ticket)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    if (!p->members.empty()) {
        const uint64_t member = ticket >> spf_pool::kMemberShift;
        if (member >= p->members.size()) return SPF_ERR_INVALID_ARGUMENT;
        return p->members[member]->wait(ticket & (((uint64_t)1 << spf_pool::kMemberShift) - 1));
    }
    return p->wait(ticket);
}

spf_status spf_pool_stats(spf_pool* p, uint64_t* ops, uint64_t* launches)
{
    if (!p || !ops || !launches) return SPF_ERR_INVALID_ARGUMENT;
    if (!p->members.empty()) {
        *ops = *launches = 0;
        for (spf_pool* q : p->members) {
            uint64_t o = 0, l = 0;
            (void)spf_pool_stats(q, &o, &l);
            *ops += o; *launches += l;
        }
        return SPF_OK;
    }
    std::lock_guard<spf_pool::Mutex> lk(p->mu);
    *ops = p->n_ops; *launches = p->n_launches;
    return SPF_OK;
}

} // extern "C"

// ---------------------------------------------------------------- values: device-resident operands of the per-operation boundary
namespace {

// the pool of one context that a value of `member` belongs to: the pool itself, or — a group pool — that member's pool
// (member < 0: the calling thread's home member, dealt as for the host-pointer submits)
spf_pool* value_pool(spf_pool* top, int member, int* which)
{
    *which = 0;
    if (top->members.empty()) return (member <= 0) ? top : nullptr;
    if (member < 0) return pool_deal(top, which);
    if (member >= (int)top->members.size()) return nullptr;
    *which = member;
    return top->members[member];
}

// The pool of `top` that value `v` lives on, or null when the value is not this pool's.  Decided by the arena the value holds — which
// it keeps alive, so no later pool can come to own the same one — and by its member index: v->home is the address of a pool that
// may be gone (values may outlive their pool) and of whatever was allocated there since; nobody reads it before this has answered.
spf_pool* value_home(spf_pool* top, const spf_value* v)
{
    spf_pool* leaf = top;
    if (!top->members.empty()) leaf = (v->member >= 0 && v->member < (int)top->members.size()) ? top->members[(size_t)v->member] : nullptr;
    return (leaf && leaf->arena && leaf->arena == v->arena) ? leaf : nullptr;
}

// a submit by handle: the checks of every `_v` wrapper below.  `explain`: a refused parameter leaves its reason in the context's
// last error (spf_pool_submit_op_v) instead of a bare status (the named wrappers).
spf_status pool_submit_v(spf_pool* top, int op, const spf_value* const* vals, size_t n_vals, uint64_t param, spf_value** out,
                         uint64_t* ticket, bool explain = false)
{
    if (!top) return SPF_ERR_INVALID_ARGUMENT;
    const char* why = nullptr;
    if (spf_ops::op_param(top->prm, op, &param, &why) != SPF_OK) return explain ? fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, why) : SPF_ERR_INVALID_ARGUMENT;
    if (!out || !vals) return SPF_ERR_INVALID_ARGUMENT; // (ticket may be null: nobody will wait for this operation itself)
    const spf_ops::OpRow& info = spf_ops::row(op);
    if (n_vals != (size_t)info.arity) return fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: wrong number of operands");
    spf_value* v[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < info.arity; k++) {
        v[k] = const_cast<spf_value*>(vals[k]);
        if (!v[k]) return fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: null operand");
        if (v[k]->kind != info.in_kind[k]) return fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: operand has the wrong ciphertext type");
        if (v[k]->state.load(std::memory_order_acquire) == spf_value_impl::FAILED)
            return fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: the operation that was to produce this operand failed");
        if (v[k]->arena != v[0]->arena)
            return fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: operands live on different members of the group (spf_value_copy_to_member moves one)");
    }
    spf_pool* leaf = value_home(top, v[0]);
    const int member = v[0]->member;
    if (!leaf) return fail(top->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: operand belongs to another pool");
    uint64_t ks_shape;
    if (spf_status ks = pool_glwe_ks_keys(leaf->ctx, op, param, &ks_shape)) return ks; // (no value made, no ticket taken)
    spf_value* res = spf_value::make(leaf->arena, leaf, member, info.out_kind, value_bytes(leaf->prm, info.out_kind));
    if (!res) return fail(leaf->ctx, SPF_ERR_HIP, "out of host memory");
    const spf_status st = leaf->submit_impl(op, true, nullptr, nullptr, v, res, ticket, param, ks_shape);
    if (st != SPF_OK) {
        res->release();
        return st == SPF_ERR_INVALID_ARGUMENT ? fail(top->ctx, st, "pool operation by handle: refused (pool closing, or an operand's producing operation failed)") : st;
    }
    if (leaf != top && ticket) *ticket |= (uint64_t)member << spf_pool::kMemberShift;
    *out = res;
    return SPF_OK;
}
spf_status pool_submit_v(spf_pool* top, int op, std::initializer_list<const spf_value*> vals, uint64_t param, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(top, op, vals.begin(), vals.size(), param, out, ticket);
}

} // namespace

extern "C" {

spf_status spf_value_upload(spf_pool* p, int member, spf_value_kind kind, const void* host, spf_value** out)
{
    if (!p || !host || !out) return SPF_ERR_INVALID_ARGUMENT;
    int which = 0;
    spf_pool* leaf = value_pool(p, member, &which);
    if (!leaf) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_upload: no such member (or none in rotation)");
    const size_t bytes = value_bytes(leaf->prm, kind);
    if (!bytes) return fail(leaf->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_upload: unknown ciphertext kind");
    spf_value* v = spf_value::make(leaf->arena, leaf, which, kind, bytes);
    if (!v) return fail(leaf->ctx, SPF_ERR_HIP, "out of host memory");
    v->blk = spf_value_impl::Block::make(leaf->arena, bytes);
    if (!v->blk) {
        v->release();
        return fail(leaf->ctx, SPF_ERR_HIP, "spf_value_upload: out of device memory");
    }
    spf_value_impl::Arena::DeviceScope ds(leaf->ctx->device);
    const hipError_t e = ds.ok ? hipMemcpy(v->ptr(), host, bytes, hipMemcpyHostToDevice) : hipErrorInvalidDevice;
    if (e != hipSuccess) {
        v->release();
        return fail(leaf->ctx, SPF_ERR_HIP, std::string("spf_value_upload: ") + hipGetErrorString(e));
    }
    v->state.store(spf_value_impl::READY, std::memory_order_release);
    *out = v;
    return SPF_OK;
}

// n ciphertexts of one kind in ONE block and one copy (the bits of an encrypted integer): what spf_value_upload does n times,
// without n copies from pageable memory — and operations that take them in order find them consecutive (no gather pass)
spf_status spf_value_upload_batch(spf_pool* p, int member, spf_value_kind kind, size_t n, const void* host, spf_value** out)
{
    if (!p || !host || !out || n == 0) return SPF_ERR_INVALID_ARGUMENT;
    int which = 0;
    spf_pool* leaf = value_pool(p, member, &which);
    if (!leaf) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_upload_batch: no such member (or none in rotation)");
    const size_t bytes = value_bytes(leaf->prm, kind);
    if (!bytes) return fail(leaf->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_upload_batch: unknown ciphertext kind");
    if (n > ((size_t)1 << 40) / bytes) return fail(leaf->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_upload_batch: too many values");
    std::shared_ptr<spf_value_impl::Block> blk = spf_value_impl::Block::make(leaf->arena, n * bytes);
    if (!blk) return fail(leaf->ctx, SPF_ERR_HIP, "spf_value_upload_batch: out of device memory");
    {
        spf_value_impl::Arena::DeviceScope ds(leaf->ctx->device);
        const hipError_t e = ds.ok ? hipMemcpy(blk->p, host, n * bytes, hipMemcpyHostToDevice) : hipErrorInvalidDevice;
        if (e != hipSuccess) return fail(leaf->ctx, SPF_ERR_HIP, std::string("spf_value_upload_batch: ") + hipGetErrorString(e));
    }
    for (size_t i = 0; i < n; i++) {
        spf_value* v = spf_value::make(leaf->arena, leaf, which, kind, bytes);
        if (!v) {
            for (size_t j = 0; j < i; j++) { out[j]->release(); out[j] = nullptr; }
            return fail(leaf->ctx, SPF_ERR_HIP, "out of host memory");
        }
        v->blk = blk;
        v->off = i * bytes;
        v->state.store(spf_value_impl::READY, std::memory_order_release);
        out[i] = v;
    }
    return SPF_OK;
}

// n valid values of one kind and one context -> host, consecutive; ONE copy when they lie consecutively in one block (the
// results of one batch, or of spf_value_upload_batch), one copy each otherwise
spf_status spf_value_download_batch(size_t n, const spf_value* const* values, void* host)
{
    if (!values || !host || n == 0) return SPF_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; i++)
        if (!values[i] || !values[i]->ready() || values[i]->kind != values[0]->kind || values[i]->arena != values[0]->arena) return SPF_ERR_INVALID_ARGUMENT;
    const size_t bytes = values[0]->bytes;
    bool consecutive = true;
    for (size_t i = 1; i < n && consecutive; i++)
        consecutive = values[i]->blk == values[0]->blk && values[i]->off == values[0]->off + i * bytes;
    spf_value_impl::Arena::DeviceScope ds(values[0]->arena->device);
    if (!ds.ok) return SPF_ERR_HIP;
    if (consecutive) return hipMemcpy(host, values[0]->ptr(), n * bytes, hipMemcpyDeviceToHost) == hipSuccess ? SPF_OK : SPF_ERR_HIP;
    bool pool_alive;
    {
        std::lock_guard<std::mutex> lk(values[0]->arena->mu);
        pool_alive = !values[0]->arena->closed; // (values may outlive their pool: its context and stream are then gone)
    }
    if (n >= 4 && pool_alive) {
        // scattered (the outputs of a circuit come from different batches): packed on the device into one scratch block
        // (gather_rows_kernel reading a pointer table at the block's end), then ONE copy — a copy to pageable memory costs ~25 us
        // per call whatever its size
        spf_ctx* c = values[0]->home->ctx;
        const size_t table_at = (n * bytes + 255) / 256 * 256;
        std::shared_ptr<spf_value_impl::Block> tmp = spf_value_impl::Block::make(values[0]->arena, table_at + n * sizeof(void*));
        std::vector<const void*> ptrs;
        try {
            for (size_t i = 0; i < n; i++) ptrs.push_back(values[i]->ptr());
        } catch (const std::exception&) {
            tmp.reset();
        }
        if (tmp) {
            char* base = static_cast<char*>(tmp->p);
            std::lock_guard<std::recursive_mutex> g(c->mu);
            if (hipMemcpyAsync(base + table_at, ptrs.data(), n * sizeof(void*), hipMemcpyHostToDevice, c->stream) != hipSuccess) return SPF_ERR_HIP;
            spf_status st = spf_gather_rows_dev(c, c->stream, n, bytes / 8, (const uint64_t* const*)(base + table_at), (uint64_t*)base);
            if (st != SPF_OK) return st;
            if (hipMemcpyAsync(host, base, n * bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return SPF_ERR_HIP;
            return hipStreamSynchronize(c->stream) == hipSuccess ? SPF_OK : SPF_ERR_HIP;
        }
    }
    for (size_t i = 0; i < n; i++)
        if (hipMemcpy(static_cast<char*>(host) + i * bytes, values[i]->ptr(), bytes, hipMemcpyDeviceToHost) != hipSuccess) return SPF_ERR_HIP;
    return SPF_OK;
}

// FheOp::{Zero,One}{Lwe0,Lwe1,Glwe1,Glev1,Ggsw1} (fhe_circuit.rs:96-116) as values
spf_status spf_value_trivial(spf_pool* p, int member, spf_value_kind kind, uint64_t bit, spf_value** out)
{
    if (!p || !out || bit > 1) return SPF_ERR_INVALID_ARGUMENT;
    int which = 0;
    spf_pool* leaf = value_pool(p, member, &which);
    if (!leaf) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_trivial: no such member (or none in rotation)");
    const spf_params& prm = leaf->prm;
    const size_t bytes = value_bytes(prm, kind);
    if (!bytes) return fail(leaf->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_trivial: unknown ciphertext kind");
    if (kind != SPF_VAL_GGSW1) {
        // trivial_lwe / trivial_glwe / trivial_glev of a bit (crypto/encryption.rs:345-451): zero mask, body (coefficient 0) =
        // bit << 63, or bit * q / B^(j+1) for GLWE j of a GLEV — the same words spf_graph_add_trivial puts into a graph
        std::vector<uint64_t> w;
        try {
            w.assign(bytes / 8, 0);
        } catch (const std::exception&) {
            return fail(leaf->ctx, SPF_ERR_HIP, "out of host memory");
        }
        const size_t k = prm.glwe_size, N = prm.polynomial_degree;
        if (kind == SPF_VAL_GLEV1)
            for (size_t j = 0; j < prm.cbs_radix_count; j++) w[j * (k + 1) * N + k * N] = bit << (64 - prm.cbs_radix_log * (j + 1));
        else
            w[kind == SPF_VAL_LWE0 ? prm.lwe_dimension : k * N] = bit << 63;
        return spf_value_upload(p, which, kind, w.data(), out);
    }
    // l1ggsw_zero / l1ggsw_one: the context's circuit bootstraps of the trivial level-0 LWE (Evaluation::new, evaluation.rs:161-197)
    spf_ctx* c = leaf->ctx;
    spf_value* v = spf_value::make(leaf->arena, leaf, which, kind, bytes);
    if (!v) return fail(c, SPF_ERR_HIP, "out of host memory");
    v->blk = spf_value_impl::Block::make(leaf->arena, bytes);
    if (!v->blk) {
        v->release();
        return fail(c, SPF_ERR_HIP, "spf_value_trivial: out of device memory");
    }
    spf_status st;
    {
        spf_value_impl::Arena::DeviceScope ds(c->device);
        std::lock_guard<std::recursive_mutex> g(c->mu);
        st = ds.ok ? ensure_ggsw_constants(c) : fail(c, SPF_ERR_HIP, "hipSetDevice failed");
        // (a device-to-device hipMemcpy may return before the copy has run: the value is handed out only after the stream is idle —
        // the kernels that will read it run on the pool's own non-blocking streams, which do not wait for the null stream)
        if (st == SPF_OK && (hipMemcpy(v->ptr(), (const char*)c->d_ggsw_const + (size_t)bit * bytes, bytes, hipMemcpyDeviceToDevice) != hipSuccess ||
                             hipStreamSynchronize(nullptr) != hipSuccess))
            st = fail(c, SPF_ERR_HIP, "spf_value_trivial: device copy failed");
    }
    if (st != SPF_OK) {
        v->release();
        return st;
    }
    v->state.store(spf_value_impl::READY, std::memory_order_release);
    *out = v;
    return SPF_OK;
}

spf_status spf_value_download(const spf_value* v, void* host)
{
    if (!v || !host || !v->ready()) return SPF_ERR_INVALID_ARGUMENT;
    spf_value_impl::Arena::DeviceScope ds(v->arena->device);
    if (!ds.ok || hipMemcpy(host, v->ptr(), v->bytes, hipMemcpyDeviceToHost) != hipSuccess) return SPF_ERR_HIP;
    return SPF_OK;
}

spf_status spf_value_wait(const spf_value* v)
{
    if (!v) return SPF_ERR_INVALID_ARGUMENT;
    // (a value may outlive its pool, a PENDING one cannot: spf_pool_destroy drains every batch first)
    const int st = v->state.load(std::memory_order_acquire);
    if (st == spf_value_impl::READY) return SPF_OK;
    if (st == spf_value_impl::FAILED) return SPF_ERR_HIP;
    return v->home ? v->home->wait_value(v) : SPF_ERR_INVALID_ARGUMENT;
}

spf_status spf_pool_flush(spf_pool* p)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    auto one = [](spf_pool* q) {
        std::lock_guard<spf_pool::Mutex> lk(q->mu);
        q->flush_deferred();
    };
    if (p->members.empty()) one(p);
    else for (spf_pool* q : p->members) one(q);
    return SPF_OK;
}

spf_status spf_value_retain(spf_value* v)
{
    if (!v) return SPF_ERR_INVALID_ARGUMENT;
    v->retain();
    return SPF_OK;
}

void spf_value_release(spf_value* v)
{
    if (v) v->release();
}

spf_status spf_value_info(const spf_value* v, spf_value_kind* kind, size_t* bytes, int* member, int* ready)
{
    if (!v) return SPF_ERR_INVALID_ARGUMENT;
    if (kind) *kind = (spf_value_kind)v->kind;
    if (bytes) *bytes = v->bytes;
    if (member) *member = v->member;
    if (ready) *ready = v->ready() ? 1 : 0;
    return SPF_OK;
}

spf_status spf_value_device_ptr(const spf_value* v, void** dev_ptr)
{
    if (!v || !dev_ptr || !v->ready()) return SPF_ERR_INVALID_ARGUMENT;
    *dev_ptr = v->ptr();
    return SPF_OK;
}

spf_status spf_value_copy_to_member(spf_pool* p, const spf_value* v, int member, spf_value** out)
{
    if (!p || !v || !out || !v->ready()) return SPF_ERR_INVALID_ARGUMENT;
    int which = 0;
    spf_pool* leaf = value_pool(p, member, &which);
    if (!leaf || member < 0) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "spf_value_copy_to_member: no such member");
    spf_value* w = spf_value::make(leaf->arena, leaf, which, v->kind, v->bytes);
    if (!w) return fail(leaf->ctx, SPF_ERR_HIP, "out of host memory");
    w->blk = spf_value_impl::Block::make(leaf->arena, v->bytes);
    if (!w->blk) {
        w->release();
        return fail(leaf->ctx, SPF_ERR_HIP, "spf_value_copy_to_member: out of device memory");
    }
    spf_value_impl::Arena::DeviceScope ds(leaf->ctx->device);
    hipError_t e = !ds.ok ? hipErrorInvalidDevice
                   : (v->arena->device == leaf->ctx->device ? hipMemcpy(w->ptr(), v->ptr(), v->bytes, hipMemcpyDeviceToDevice)
                                                            : hipMemcpyPeer(w->ptr(), leaf->ctx->device, v->ptr(), v->arena->device, v->bytes));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr); // (a device-to-device copy may return before it has run; see spf_value_trivial)
    if (e != hipSuccess) {
        w->release();
        return fail(leaf->ctx, SPF_ERR_HIP, std::string("spf_value_copy_to_member: ") + hipGetErrorString(e));
    }
    w->state.store(spf_value_impl::READY, std::memory_order_release);
    *out = w;
    return SPF_OK;
}

spf_status spf_pool_value_stats(spf_pool* p, size_t* live_values, size_t* live_bytes, size_t* cached_bytes)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    size_t lv = 0, lb = 0, cb = 0;
    auto add = [&](spf_pool* q) {
        lv += q->arena->live_values.load();
        lb += q->arena->live_bytes.load();
        std::lock_guard<std::mutex> lk(q->arena->mu);
        cb += q->arena->cached_bytes;
    };
    if (p->members.empty()) add(p);
    else for (spf_pool* q : p->members) add(q);
    if (live_values) *live_values = lv;
    if (live_bytes) *live_bytes = lb;
    if (cached_bytes) *cached_bytes = cb;
    return SPF_OK;
}

spf_status spf_pool_trim(spf_pool* p)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    if (p->members.empty()) p->arena->trim();
    else for (spf_pool* q : p->members) q->arena->trim();
    return SPF_OK;
}

spf_status spf_pool_counters_get(spf_pool* p, spf_pool_counters* out)
{
    if (!p || !out) return SPF_ERR_INVALID_ARGUMENT;
    *out = spf_pool_counters{};
    auto add = [&](spf_pool* q) {
        std::lock_guard<spf_pool::Mutex> lk(q->mu);
        out->ops += q->n_ops; out->launches += q->n_launches;
        out->handle_ops += q->n_handle_ops; out->handle_launches += q->n_handle_launches;
        out->reclaimed += q->n_reclaimed;
        for (int i = 0; i < 3; i++) out->bootstrap_launches_by_shape[i] += q->n_shape[i];
        out->staging_sets = (uint64_t)q->n_sets;
        out->stream_concurrency = out->stream_concurrency ? std::min<uint64_t>(out->stream_concurrency, (uint64_t)q->stream_concurrency) : (uint64_t)q->stream_concurrency;
        out->value_mallocs += q->arena->n_malloc.load();
    };
    if (p->members.empty()) add(p);
    else for (spf_pool* q : p->members) add(q);
    return SPF_OK;
}

// ---- the pool's submits by handle
spf_status spf_pool_submit_keyswitch_v(spf_pool* p, const spf_value* lwe1, spf_value** lwe0_out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_KEYSWITCH, {lwe1}, 0, lwe0_out, ticket);
}
spf_status spf_pool_submit_circuit_bootstrap_v(spf_pool* p, const spf_value* lwe0, spf_value** ggsw_out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_CBS, {lwe0}, 0, ggsw_out, ticket);
}
spf_status spf_pool_submit_keyswitch_circuit_bootstrap_v(spf_pool* p, const spf_value* lwe1, spf_value** ggsw_out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_GATE_CBS, {lwe1}, 0, ggsw_out, ticket);
}
spf_status spf_pool_submit_cmux_v(spf_pool* p, const spf_value* sel, const spf_value* a, const spf_value* b, spf_value** out,
                                  uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_CMUX, {sel, a, b}, 0, out, ticket);
}
spf_status spf_pool_submit_sample_extract_v(spf_pool* p, const spf_value* glwe, size_t idx, spf_value** lwe1_out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_SAMPLE_EXTRACT, {glwe}, idx, lwe1_out, ticket);
}
spf_status spf_pool_submit_not_v(spf_pool* p, const spf_value* glwe, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_NOT, {glwe}, 0, out, ticket);
}
spf_status spf_pool_submit_glwe_add_v(spf_pool* p, const spf_value* a, const spf_value* b, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_GLWE_ADD, {a, b}, 0, out, ticket);
}
spf_status spf_pool_submit_mul_xn_v(spf_pool* p, const spf_value* glwe, size_t n, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_MUL_XN, {glwe}, n, out, ticket);
}
spf_status spf_pool_submit_multiply_ggsw_glwe_v(spf_pool* p, const spf_value* ggsw, const spf_value* glwe, spf_value** out,
                                                uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_MULTIPLY_GGSW_GLWE, {ggsw, glwe}, 0, out, ticket);
}
spf_status spf_pool_submit_glev_cmux_v(spf_pool* p, const spf_value* sel, const spf_value* a, const spf_value* b, spf_value** out,
                                       uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_GLEV_CMUX, {sel, a, b}, 0, out, ticket);
}
spf_status spf_pool_submit_scheme_switch_v(spf_pool* p, const spf_value* glev, spf_value** ggsw_out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_SCHEME_SWITCH, {glev}, 0, ggsw_out, ticket);
}
spf_status spf_pool_submit_glwe_keyswitch_v(spf_pool* p, uint32_t slot, const spf_value* glwe, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_GLWE_KEYSWITCH, &glwe, 1, slot, out, ticket, true); // (a refused parameter leaves its number in the last error)
}
spf_status spf_pool_submit_glwe_automorphism_v(spf_pool* p, uint32_t round, const spf_value* glwe, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_GLWE_AUTOMORPHISM, &glwe, 1, round, out, ticket, true); // (a refused parameter leaves its number in the last error)
}
spf_status spf_pool_submit_glwe_trace_v(spf_pool* p, const spf_value* glwe, spf_value** out, uint64_t* ticket)
{
    return pool_submit_v(p, spf_ops::OP_GLWE_TRACE, &glwe, 1, 0, out, ticket, true); // (a refused parameter leaves its number in the last error)
}

// `blind_rotation` (blind_rotation.rs:202-223) by handle: n_bits pushes of the rotate-CMUX kind, step i on the still-pending
// result of step i - 1 — the deferred table's (depth, kind, rotation) key then makes step i of every caller one scattered launch.
// Everything is checked before the first push; the intermediate values are the library's and are let go as the chain advances
// (each lives until the step that reads it has run: its batch holds it).
spf_status spf_pool_submit_blind_rotation_v(spf_pool* p, const spf_value* glwe, const spf_value* const* shift_ggsw, size_t n_bits,
                                            size_t log_stride, spf_value** out, uint64_t* ticket)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    if (!glwe || !shift_ggsw || !out) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool blind rotation: null pointer");
    if (const char* why = blind_rotation_shape_error(p->prm, 1, n_bits, log_stride))
        return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, std::string("pool blind rotation: ") + why);
    if (glwe->kind != SPF_VAL_GLWE1) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool blind rotation: operand is not an L1 GLWE");
    for (size_t i = 0; i < n_bits; i++) {
        if (!shift_ggsw[i]) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool blind rotation: null selector");
        if (shift_ggsw[i]->kind != SPF_VAL_GGSW1) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool blind rotation: selector is not an L1 GGSW");
        if (shift_ggsw[i]->arena != glwe->arena)
            return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool blind rotation: operands live on different members of the group (spf_value_copy_to_member moves one)");
        if (shift_ggsw[i]->state.load(std::memory_order_acquire) == spf_value_impl::FAILED)
            return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool blind rotation: the operation that was to produce a selector failed");
    }
    const spf_pool* leaf = value_home(p, glwe);
    if (!leaf) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "pool operation by handle: operand belongs to another pool");
    if (!leaf->ctx->generic && (leaf->prm.cbs_radix_log != 4 || leaf->prm.cbs_radix_count != 4))
        return fail(p->ctx, SPF_ERR_UNSUPPORTED, "cmux kernel is built for cbs_radix 4 x 4 bits");
    const spf_value* acc = glwe;
    for (size_t i = 0; i < n_bits; i++) {
        spf_value* next = nullptr;
        const spf_value* in[2] = {shift_ggsw[i], acc};
        const spf_status st = pool_submit_v(p, spf_ops::OP_ROT_CMUX, in, 2, (uint64_t)1 << (i + log_stride), &next,
                                            i + 1 == n_bits ? ticket : nullptr, true);
        if (acc != glwe) const_cast<spf_value*>(acc)->release(); // (step i holds it until it has run)
        if (st != SPF_OK) return st;
        acc = next;
    }
    *out = const_cast<spf_value*>(acc);
    return SPF_OK;
}

// one entry for `exec_op`'s whole match (circuit_processor/mod.rs:255-540): the operation as a spf_graph_op, operands in the
// order spf_graph_add_op takes them
spf_status spf_pool_submit_op_v(spf_pool* p, spf_graph_op op, const spf_value* const* inputs, size_t n_inputs, uint64_t param,
                                spf_value** out, uint64_t* ticket)
{
    if (!p) return SPF_ERR_INVALID_ARGUMENT;
    const int pop = spf_ops::pool_op_of(op);
    if (pop == spf_ops::kNone) return fail(p->ctx, SPF_ERR_INVALID_ARGUMENT, "unknown operation");
    return pool_submit_v(p, pop, inputs, n_inputs, param, out, ticket, true);
}

} // extern "C"

#include "spf_graph.hpp"
#include "spf_group.hpp"
