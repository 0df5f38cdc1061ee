// Native parity test of `FheCircuit::lwe_linear` (include/spf_evaluation.hpp) — test infrastructure.  One graph holds
// "layer -> activation table -> layer -> keyswitch -> activation table": level-0 inputs -> lwe_linear (slot 0, scattered inputs)
// -> pbs_univariate -> lwe_linear (slot 1, on the bootstrap's level-1 results where they lie) -> keyswitch -> pbs_univariate; the
// expectation is the same rows through the `_dev` entry points (`scalar_mul_ciphertext_mad` + `add_lwe_inplace`, sunscreen_tfhe
// ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18; `programmable_bootstrap_univariate`, ops/bootstrapping/
// programmable_bootstrapping.rs:291).  The keys are uniform words and bounded spectra: parity needs no honest key.  Links
// libspf_hip.so; built and run by tests/test_gpu_lwe_linear_graph_cpp.py.
#include "spf_evaluation.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    std::printf("%-84s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}
bool same(const void* a, const void* b, size_t words) { return std::memcmp(a, b, words * 8) == 0; }

uint64_t state = 0xB27;
uint64_t next_word() // splitmix64
{
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
std::vector<uint64_t> words(size_t n)
{
    std::vector<uint64_t> v(n);
    for (auto& x : v) x = next_word();
    return v;
}
std::vector<double> spectra(size_t n_complex) // magnitudes up to 2^40
{
    std::vector<double> v(2 * n_complex);
    for (auto& x : v) x = (double)(int64_t)next_word() / 8388608.0;
    return v;
}

struct DeviceBuffers { // spf_device_alloc'd, freed at the end
    spf_ctx* c;
    std::vector<void*> all;
    template <class T> T* make(size_t bytes, const void* host = nullptr)
    {
        void* p = nullptr;
        if (spf_device_alloc(c, bytes, &p) != SPF_OK) throw spf::Error(SPF_ERR_HIP, "spf_device_alloc");
        all.push_back(p);
        if (host && spf_device_upload(c, p, host, bytes) != SPF_OK) throw spf::Error(SPF_ERR_HIP, "spf_device_upload");
        return static_cast<T*>(p);
    }
    ~DeviceBuffers() { for (void* p : all) spf_device_free(c, p); }
};

} // namespace

int main()
{
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 4; // four blind-rotation steps per bootstrap; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, n = p.lwe_dimension, h = N / 2;
    const size_t gw = (k + 1) * N, l1w = k * N + 1, l0w = n + 1;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * h;
    size_t log_n = 0;
    while (((size_t)1 << log_n) < N) log_n++;
    const size_t K = 3, M1 = 2, M2 = 3;
    const auto check = [](spf_status s, const char* what) {
        if (s != SPF_OK) throw spf::Error(s, what);
    };

    try {
        const std::vector<double> bsk = spectra(n * ggsw_pbs);
        const std::vector<uint64_t> ksk = words(k * N * p.ks_radix_count * l0w);
        const std::vector<double> ak = spectra(log_n * k * p.tr_radix_count * (k + 1) * h);
        const std::vector<double> ssk = spectra(k * (k + 1) / 2 * p.ss_radix_count * (k + 1) * h);
        spf::ComputeKey key{bsk.data(), bsk.size() / 2, ksk.data(), ksk.size(), ak.data(), ak.size() / 2, ssk.data(), ssk.size() / 2};
        spf::Evaluation ev(key, p, 0);
        const int64_t wa[M1 * K] = {3, -1, 0, INT64_MIN, 70000, -2}, wb[M2 * M1] = {1, 1, -5, 2, INT64_MAX, 0};
        const uint64_t ba[M1] = {7, ~0ull}, bb[M2] = {0, 1ull << 63, 12345};
        ev.load_lwe_linear_weights(0, M1, K, wa, ba);
        ev.load_lwe_linear_weights(1, M2, M1, wb, bb);
        size_t sm = 0, sk = 0;
        int has_bias = 0;
        expect(spf_lwe_linear_slot_shape(ev.raw(), 1, &sm, &sk, &has_bias) == SPF_OK && sm == M2 && sk == M1 && has_bias == 1,
               "spf_lwe_linear_slot_shape gives what was loaded");
        expect(spf_lwe_linear_slot_shape(ev.raw(), 2, &sm, &sk, &has_bias) == SPF_ERR_NO_KEY, "  ... an empty slot is SPF_ERR_NO_KEY");
        const std::vector<uint64_t> x = words(K * l0w), lut1 = words(gw), lut2 = words(gw);

        // ---- the expectation: the `_dev` entry points on one stream, one download at the end
        spf_ctx* c = ev.raw();
        DeviceBuffers dev{c, {}};
        uint64_t* d_x = dev.make<uint64_t>(K * l0w * 8, x.data());
        uint64_t* d_lut1 = dev.make<uint64_t>(gw * 8, lut1.data());
        uint64_t* d_lut2 = dev.make<uint64_t>(gw * 8, lut2.data());
        uint64_t* d_a = dev.make<uint64_t>(M1 * l0w * 8);
        uint64_t* d_h = dev.make<uint64_t>(M1 * l1w * 8);
        uint64_t* d_b = dev.make<uint64_t>(M2 * l1w * 8);
        uint64_t* d_b0 = dev.make<uint64_t>(M2 * l0w * 8);
        uint64_t* d_y = dev.make<uint64_t>(M2 * l1w * 8);
        check(spf_lwe_linear_enqueue(c, nullptr, 0, SPF_VAL_LWE0, 1, d_x, d_a), "layer A");
        check(spf_pbs_univariate_dev(c, nullptr, M1, d_a, d_lut1, 0, d_h), "table 1");
        check(spf_lwe_linear_enqueue(c, nullptr, 1, SPF_VAL_LWE1, 1, d_h, d_b), "layer B");
        check(spf_keyswitch_lwe_l1_lwe_l0_dev(c, nullptr, M2, d_b, d_b0), "keyswitch");
        check(spf_pbs_univariate_dev(c, nullptr, M2, d_b0, d_lut2, 0, d_y), "table 2");
        std::vector<uint64_t> want_a(M1 * l0w), want_b(M2 * l1w), want_y(M2 * l1w);
        check(spf_device_download(c, nullptr, want_a.data(), d_a, want_a.size() * 8), "download");
        check(spf_device_download(c, nullptr, want_b.data(), d_b, want_b.size() * 8), "download");
        check(spf_device_download(c, nullptr, want_y.data(), d_y, want_y.size() * 8), "download");

        auto chain = [&](spf::FheCircuit& g, uint64_t* a_out, uint64_t* b_out, uint64_t* y_out) {
            using Node = spf::FheCircuit::Node;
            const Node t1 = g.input(SPF_VAL_GLWE1, lut1.data()), t2 = g.input(SPF_VAL_GLWE1, lut2.data());
            std::vector<Node> xs;
            for (size_t i = 0; i < K; i++) xs.push_back(g.input(SPF_VAL_LWE0, x.data() + i * l0w));
            const std::vector<Node> a = g.lwe_linear(0, xs, M1);
            std::vector<Node> hidden;
            for (size_t m = 0; m < M1; m++) {
                g.output(a[m], a_out + m * l0w);
                hidden.push_back(g.pbs_univariate(a[m], t1));
            }
            const std::vector<Node> b = g.lwe_linear(1, hidden, M2);
            for (size_t m = 0; m < M2; m++) {
                g.output(b[m], b_out + m * l1w);
                g.output(g.pbs_univariate(g.op(SPF_OP_KEYSWITCH_L1_TO_L0, {b[m]}), t2), y_out + m * l1w);
            }
        };
        { // one graph of one context
            spf::FheCircuit g(ev);
            std::vector<uint64_t> a(M1 * l0w), b(M2 * l1w), y(M2 * l1w);
            chain(g, a.data(), b.data(), y.data());
            g.run();
            expect(same(a.data(), want_a.data(), a.size()), "FheCircuit::lwe_linear over inputs == spf_lwe_linear_enqueue");
            expect(same(b.data(), want_b.data(), b.size()), "FheCircuit::lwe_linear over bootstrap results == spf_lwe_linear_enqueue");
            expect(same(y.data(), want_y.data(), y.size()), "layer, table, layer, table in one graph == the _dev calls");
            bool threw = false;
            try {
                g.lwe_linear(0, {0, 1}, 0);
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... M = 0 throws");
            threw = false;
            try {
                g.lwe_linear(0, {}, 1);
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... no operands throw");
            threw = false;
            try {
                g.lwe_linear(SPF_LWE_LINEAR_SLOTS, {2}, 1);
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... slot = SPF_LWE_LINEAR_SLOTS throws");
            g.run();
            expect(same(y.data(), want_y.data(), y.size()), "  ... and the graph still runs");
        }
        { // a job of the whole Evaluation
            spf::FheCircuit job(ev, spf::FheCircuit::Job{});
            std::vector<uint64_t> a(M1 * l0w), b(M2 * l1w), y(M2 * l1w);
            chain(job, a.data(), b.data(), y.data());
            spf::FheCircuit::run_all(ev, {&job});
            expect(same(b.data(), want_b.data(), b.size()) && same(y.data(), want_y.data(), y.size()),
                   "the chain as a job of the group == the _dev calls");
        }
        { // a slot of another shape is an error of the run, with nothing written
            spf::FheCircuit g(ev);
            std::vector<uint64_t> out(l0w, 0x55);
            g.output(g.lwe_linear(1, {g.input(SPF_VAL_LWE0, x.data())}, 1)[0], out.data());
            bool threw = false;
            try {
                g.run();
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw && out[0] == 0x55 && out[l0w - 1] == 0x55, "a slot of another (M, K) than the nodes': run() throws");
        }
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
