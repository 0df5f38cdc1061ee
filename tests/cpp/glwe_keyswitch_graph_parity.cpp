// Native parity test of `FheCircuit::glwe_keyswitch`, `glwe_automorphism` and `glwe_trace` (include/spf_evaluation.hpp) — test
// infrastructure.  One graph holds, over B input GLWEs taken out of order and with a repeat (the rows kernels), a keyswitch, an
// automorphism round and a trace of each; a second level holds the trace of every keyswitched node where it lies (the in-place
// kernel).  The same graph built through the C calls must give the same words, and both the driver's (the oracle's,
// tests/glwe_keyswitch_cases.py).  Links libspf_hip.so; built and run by tests/test_gpu_glwe_keyswitch_graph_cpp.py.
//   usage: glwe_keyswitch_graph_parity <dir> <B> <radix_log> <radix_count> <round> <pick 0> ... <pick B-1>
//   <dir>/ak.bin, ksk.bin, glwes.bin, want_keyswitch.bin, want_round.bin, want_trace.bin, want_chain.bin (uint64): raw little-endian,
//   the want_* files B GLWEs each in pick order
#include "spf_evaluation.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    std::printf("%-82s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}

bool read_file(const std::string& path, std::vector<uint64_t>& out, size_t count)
{
    out.resize(count);
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(out.data(), sizeof(uint64_t), count, f);
    const bool at_end = std::fgetc(f) == EOF;
    std::fclose(f);
    return got == count && at_end;
}

constexpr uint32_t kSlot = 6;

} // namespace

int main(int argc, char** argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <dir> <B> <radix_log> <radix_count> <round> <picks ...>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t B = std::strtoull(argv[2], nullptr, 10);
    const uint32_t radix_log = (uint32_t)std::strtoul(argv[3], nullptr, 10), radix_count = (uint32_t)std::strtoul(argv[4], nullptr, 10),
                   round = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    if ((size_t)argc != 6 + B) {
        std::fprintf(stderr, "expected %zu picks\n", B);
        return 2;
    }
    std::vector<size_t> picks;
    for (size_t i = 0; i < B; i++) picks.push_back(std::strtoull(argv[6 + i], nullptr, 10));
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 9; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, W = (k + 1) * N;
    size_t log_n = 0;
    while (((size_t)1 << log_n) < N) log_n++;
    const size_t bsk_words = p.lwe_dimension * (k + 1) * p.pbs_radix_count * (k + 1) * N;
    const size_t ak_words = log_n * k * p.tr_radix_count * (k + 1) * N, ksk_words = k * radix_count * (k + 1) * N;

    std::vector<uint64_t> ak, ksk, glwes, want_ks, want_round, want_trace, want_chain;
    if (!read_file(dir + "/ak.bin", ak, ak_words) || !read_file(dir + "/ksk.bin", ksk, ksk_words) || !read_file(dir + "/glwes.bin", glwes, B * W) ||
        !read_file(dir + "/want_keyswitch.bin", want_ks, B * W) || !read_file(dir + "/want_round.bin", want_round, B * W) ||
        !read_file(dir + "/want_trace.bin", want_trace, B * W) || !read_file(dir + "/want_chain.bin", want_chain, B * W)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<uint64_t> bsk(bsk_words, 0);
        spf::ComputeKeyNonFft ck{bsk.data(), bsk_words, nullptr, 0, ak.data(), ak_words};
        spf::Evaluation ev(ck, p, 0);
        using Node = spf::FheCircuit::Node;
        struct Outs { std::vector<uint64_t> ks, round, trace, chain; };
        auto sized = [&] { return Outs{std::vector<uint64_t>(B * W, 0x55), std::vector<uint64_t>(B * W, 0x55), std::vector<uint64_t>(B * W, 0x55), std::vector<uint64_t>(B * W, 0x55)}; };
        auto build = [&](spf::FheCircuit& g, Outs& o) {
            std::vector<Node> in;
            for (size_t i = 0; i < B; i++) in.push_back(g.input(SPF_VAL_GLWE1, glwes.data() + i * W));
            for (size_t i = 0; i < B; i++) {
                const Node x = in[picks[i]];
                const Node s = g.glwe_keyswitch(kSlot, x);
                g.output(s, o.ks.data() + i * W);
                g.output(g.glwe_automorphism(round, x), o.round.data() + i * W);
                g.output(g.glwe_trace(x), o.trace.data() + i * W);
                g.output(g.glwe_trace(s), o.chain.data() + i * W);
            }
        };
        {
            spf::FheCircuit g(ev);
            Outs o = sized();
            build(g, o); // built before the key is loaded: the slot is read by run()
            bool threw = false;
            try { g.run(); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
            expect(threw && o.ks[0] == 0x55 && o.chain[B * W - 1] == 0x55, "before the key is loaded: run() throws SPF_ERR_NO_KEY, nothing written");
            ev.load_glwe_keyswitch_key_std(kSlot, ksk.data(), ksk_words, radix_log, radix_count);
            g.run();
            expect(o.ks == want_ks, "FheCircuit::glwe_keyswitch over scattered inputs == the driver's words");
            expect(o.round == want_round, "FheCircuit::glwe_automorphism over scattered inputs == the driver's words");
            expect(o.trace == want_trace, "FheCircuit::glwe_trace over scattered inputs == the driver's words");
            expect(o.chain == want_chain, "FheCircuit::glwe_trace over the keyswitched rows in place == the driver's words");
            expect(std::string(spf_last_glwe_keyswitch_kernel(ev.raw())) == "glwe_ks_kernel", "  ... the second level on glwe_ks_kernel");

            // the same graph through the C calls
            spf_graph* cg = nullptr;
            Outs c = sized();
            bool ok = spf_graph_create(ev.raw(), &cg) == SPF_OK;
            std::vector<uint32_t> in(B);
            for (size_t i = 0; ok && i < B; i++) ok = spf_graph_add_input(cg, SPF_VAL_GLWE1, glwes.data() + i * W, &in[i]) == SPF_OK;
            for (size_t i = 0; ok && i < B; i++) {
                uint32_t s = 0, a = 0, t = 0, ch = 0;
                ok = spf_graph_add_glwe_keyswitch(cg, kSlot, in[picks[i]], &s) == SPF_OK && spf_graph_add_glwe_automorphism(cg, round, in[picks[i]], &a) == SPF_OK &&
                     spf_graph_add_glwe_trace(cg, in[picks[i]], &t) == SPF_OK && spf_graph_add_glwe_trace(cg, s, &ch) == SPF_OK &&
                     spf_graph_add_output(cg, s, c.ks.data() + i * W) == SPF_OK && spf_graph_add_output(cg, a, c.round.data() + i * W) == SPF_OK &&
                     spf_graph_add_output(cg, t, c.trace.data() + i * W) == SPF_OK && spf_graph_add_output(cg, ch, c.chain.data() + i * W) == SPF_OK;
            }
            ok = ok && spf_graph_run(cg) == SPF_OK;
            expect(ok && c.ks == o.ks && c.round == o.round && c.trace == o.trace && c.chain == o.chain, "  ... == the same graph through the C calls");
            uint32_t n_c = 0, lv_c = 0, la_c = 0;
            spf_graph_stats(cg, &n_c, &lv_c, &la_c);
            expect(n_c == 5 * B && lv_c == 2 && la_c == 4, "  ... 5 B nodes, 2 levels, 4 launches: one per mode and level");
            spf_graph_destroy(cg);

            struct Bad { const char* what; int which; uint32_t param; };
            for (const Bad& bad : {Bad{"  ... slot = SPF_GLWE_KSK_SLOTS throws", 0, SPF_GLWE_KSK_SLOTS}, Bad{"  ... round = 0 throws", 1, 0},
                                   Bad{"  ... round = log2 N + 1 throws", 1, (uint32_t)log_n + 1}}) {
                threw = false;
                try {
                    if (bad.which == 0) g.glwe_keyswitch(bad.param, 0);
                    else g.glwe_automorphism(bad.param, 0);
                } catch (const spf::Error& e) {
                    threw = e.status == SPF_ERR_INVALID_ARGUMENT;
                }
                expect(threw, bad.what);
            }
            threw = false;
            try { g.glwe_trace(0xFFFFFFF0u); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
            expect(threw, "  ... an operand that is no node throws");
            std::fill(o.chain.begin(), o.chain.end(), 0);
            g.run();
            expect(o.chain == want_chain, "  ... and the graph still runs");
        }
        { // a job of the whole Evaluation
            spf::FheCircuit job(ev, spf::FheCircuit::Job{});
            Outs o = sized();
            build(job, o);
            spf::FheCircuit::run_all(ev, {&job});
            expect(o.ks == want_ks && o.round == want_round && o.trace == want_trace && o.chain == want_chain, "the same nodes as a job of the group == the driver's words");
        }
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
