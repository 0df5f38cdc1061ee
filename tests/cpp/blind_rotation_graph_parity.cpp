// Native parity test of `FheCircuit::blind_rotation` and `PooledEvaluation::blind_rotation` (include/spf_evaluation.hpp) — test
// infrastructure.  Two GLWEs are rotated by shifts given as random selectors, as nodes of a gate graph and by handle (blocking
// and pushed); the expectation is `spf_blind_rotation_batch` on the same operands (`blind_rotation`, sunscreen_tfhe
// ops/bootstrapping/blind_rotation.rs:202-223).  Links libspf_hip.so; built and run by tests/test_gpu_blind_rotation_graph_cpp.py.
#include "spf_evaluation.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    std::printf("%-72s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}
bool same(const uint64_t* a, const uint64_t* b, size_t n) { return std::memcmp(a, b, n * 8) == 0; }

uint64_t state = 0xB16;
uint64_t next_word() // splitmix64
{
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

} // namespace

int main()
{
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 1; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, gw = (k + 1) * N;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);
    const size_t cbs_len = (k + 1) * p.cbs_radix_count * (k + 1) * (N / 2);
    const size_t B = 2, n_bits = 3, log_stride = 2;

    std::vector<uint64_t> in(B * gw);
    for (auto& x : in) x = next_word();
    std::vector<double> shift(B * n_bits * cbs_len * 2); // int-major: item b's selectors side by side
    for (auto& x : shift) x = (double)(int64_t)next_word() * 0.03125; // magnitudes up to 2^58
    auto selector = [&](size_t b, size_t i) { return shift.data() + (b * n_bits + i) * cbs_len * 2; };

    try {
        std::vector<double> bsk(ggsw_pbs * 2, 0.0);
        spf::ComputeKey key{bsk.data(), ggsw_pbs, nullptr, 0};
        spf::Evaluation ev(key, p, 0);
        std::vector<uint64_t> ref(B * gw);
        expect(spf_blind_rotation_batch(ev.raw(), B, n_bits, log_stride, shift.data(), in.data(), ref.data()) == SPF_OK,
               "spf_blind_rotation_batch (the expectation)");

        { // as nodes of a gate graph: both items in one graph, each with its own selectors
            spf::FheCircuit g(ev);
            std::vector<uint64_t> out(B * gw);
            for (size_t b = 0; b < B; b++) {
                std::vector<spf::FheCircuit::Node> sel;
                for (size_t i = 0; i < n_bits; i++) sel.push_back(g.input(SPF_VAL_GGSW1, selector(b, i)));
                g.output(g.blind_rotation(g.input(SPF_VAL_GLWE1, in.data() + b * gw), sel, log_stride), out.data() + b * gw);
            }
            g.run();
            expect(same(out.data(), ref.data(), B * gw), "FheCircuit::blind_rotation == spf_blind_rotation_batch");
            bool threw = false;
            try {
                g.blind_rotation(0, {0, 1, 2}, 9);
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... n_bits + log_stride = 12 throws");
        }
        for (int pushed = 0; pushed < 2; pushed++) { // by handle
            spf::PooledEvaluation pe(ev, 64, 100, pushed ? spf::PooledEvaluation::Mode::Pushed : spf::PooledEvaluation::Mode::Blocking);
            std::vector<spf::L1GlweCiphertext> outs(B);
            for (size_t b = 0; b < B; b++) {
                std::vector<spf::L1GgswCiphertext> sel;
                for (size_t i = 0; i < n_bits; i++) sel.push_back(pe.upload<spf::L1GgswCiphertext>(selector(b, i)));
                spf::L1GlweCiphertext x = pe.upload<spf::L1GlweCiphertext>(in.data() + b * gw);
                pe.blind_rotation(outs[b], sel, x, log_stride); // (the operands may go: the pool holds them until the steps have run)
            }
            std::vector<uint64_t> out(B * gw);
            for (size_t b = 0; b < B; b++) outs[b].download(out.data() + b * gw);
            expect(same(out.data(), ref.data(), B * gw), pushed ? "PooledEvaluation::blind_rotation, pushed == spf_blind_rotation_batch"
                                                                : "PooledEvaluation::blind_rotation, blocking == spf_blind_rotation_batch");
            bool threw = false;
            try {
                spf::L1GlweCiphertext x = pe.upload<spf::L1GlweCiphertext>(in.data()), y;
                pe.blind_rotation(y, nullptr, 0, x);
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... no selectors throws");
            outs.clear();
            size_t live = 1;
            expect(spf_pool_value_stats(pe.raw(), &live, nullptr, nullptr) == SPF_OK && live == 0, "  ... every value released");
        }
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
