// Native parity test of `FheCircuit::pbs_univariate` / `pbs_bivariate` / `public_functional_keyswitch` and of
// `PooledEvaluation::pbs_univariate` / `pbs_bivariate` (include/spf_evaluation.hpp) — test infrastructure.  One chain mixes the
// two computing styles in ONE graph: packed GLWE -> unpack -> keyswitch -> bivariate table -> keyswitch -> public functional
// keyswitch -> CMUX with a circuit-bootstrapped selector; the expectation is the same rows through the `_dev` entry points
// (`programmable_bootstrap_univariate` / `_bivariate`, sunscreen_tfhe ops/bootstrapping/programmable_bootstrapping.rs:291, 575-621;
// `public_functional_keyswitch`, ops/keyswitch/public_functional_keyswitch.rs:74-148).  The keys are uniform words and bounded
// spectra: parity needs no honest key.  Links libspf_hip.so; built and run by tests/test_gpu_pbs_graph_cpp.py.
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

uint64_t state = 0xB21;
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
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * h, cbs_len = (k + 1) * p.cbs_radix_count * (k + 1) * h;
    size_t log_n = 0;
    while (((size_t)1 << log_n) < N) log_n++;
    const size_t W = 4, bits = 2, pufks_log = 4, pufks_count = 4; // W digits -> W - 1 sums of neighbours
    const auto check = [](spf_status s, const char* what) {
        if (s != SPF_OK) throw spf::Error(s, what);
    };

    try {
        const std::vector<double> bsk = spectra(n * ggsw_pbs);
        const std::vector<uint64_t> ksk = words(k * N * p.ks_radix_count * l0w);
        const std::vector<double> ak = spectra(log_n * k * p.tr_radix_count * (k + 1) * h);
        const std::vector<double> ssk = spectra(k * (k + 1) / 2 * p.ss_radix_count * (k + 1) * h);
        const std::vector<uint64_t> pufks = words(n * pufks_count * gw);
        spf::ComputeKey key{bsk.data(), bsk.size() / 2, ksk.data(), ksk.size(), ak.data(), ak.size() / 2, ssk.data(), ssk.size() / 2};
        spf::Evaluation ev(key, p, 0);
        check(spf_group_load_public_functional_keyswitch_key_std(ev.group(), pufks.data(), pufks.size(), n, pufks_log, pufks_count),
              "load the public functional keyswitch key");
        const std::vector<uint64_t> packed = words(gw), lut = words(gw);

        // ---- the expectation: the `_dev` entry points on one stream, one download at the end
        spf_ctx* c = ev.raw();
        DeviceBuffers dev{c, {}};
        uint64_t* d_packed = dev.make<uint64_t>(gw * 8, packed.data());
        uint64_t* d_lut = dev.make<uint64_t>(gw * 8, lut.data());
        uint64_t* d_bits = dev.make<uint64_t>(W * l1w * 8);
        uint64_t* d_l0 = dev.make<uint64_t>(W * l0w * 8);
        uint64_t* d_sums = dev.make<uint64_t>((W - 1) * l1w * 8);
        uint64_t* d_uni = dev.make<uint64_t>(l1w * 8);
        uint64_t* d_sums0 = dev.make<uint64_t>((W - 1) * l0w * 8);
        uint64_t* d_glwe = dev.make<uint64_t>(gw * 8);
        double* d_sel = dev.make<double>(cbs_len * 16);
        uint64_t* d_out = dev.make<uint64_t>(gw * 8);
        check(spf_glwe_unpack_l1_dev(c, nullptr, 1, W, d_packed, d_bits), "unpack");
        check(spf_keyswitch_lwe_l1_lwe_l0_dev(c, nullptr, W, d_bits, d_l0), "keyswitch");
        check(spf_pbs_bivariate_dev(c, nullptr, W - 1, d_l0, d_l0 + l0w, d_lut, 0, bits, d_sums), "bivariate");
        check(spf_pbs_univariate_dev(c, nullptr, 1, d_l0, d_lut, 0, d_uni), "univariate");
        check(spf_keyswitch_lwe_l1_lwe_l0_dev(c, nullptr, W - 1, d_sums, d_sums0), "keyswitch of the sums");
        check(spf_public_functional_keyswitch_enqueue(c, nullptr, 1, W - 1, d_sums0, d_glwe), "public functional keyswitch");
        check(spf_circuit_bootstrap_dev(c, nullptr, 1, d_l0, d_sel), "circuit bootstrap");
        check(spf_cmux_dev(c, nullptr, 1, d_sel, d_glwe, d_packed, d_out), "cmux");
        std::vector<uint64_t> want_out(gw), want_glwe(gw), want_sums((W - 1) * l1w), want_uni(l1w), l0(W * l0w);
        check(spf_device_download(c, nullptr, want_out.data(), d_out, gw * 8), "download");
        check(spf_device_download(c, nullptr, want_glwe.data(), d_glwe, gw * 8), "download");
        check(spf_device_download(c, nullptr, want_sums.data(), d_sums, want_sums.size() * 8), "download");
        check(spf_device_download(c, nullptr, want_uni.data(), d_uni, l1w * 8), "download");
        check(spf_device_download(c, nullptr, l0.data(), d_l0, l0.size() * 8), "download");

        auto chain = [&](spf::FheCircuit& g, const uint64_t* in, uint64_t* out, uint64_t* glwe, uint64_t* sums, uint64_t* uni) {
            using Node = spf::FheCircuit::Node;
            const Node x = g.input(SPF_VAL_GLWE1, in), t = g.input(SPF_VAL_GLWE1, lut.data());
            std::vector<Node> digits;
            for (Node b : g.unpack(x, W)) digits.push_back(g.op(SPF_OP_KEYSWITCH_L1_TO_L0, {b}));
            std::vector<Node> low;
            for (size_t i = 0; i + 1 < W; i++) {
                const Node s = g.pbs_bivariate(digits[i], digits[i + 1], t, bits);
                g.output(s, sums + i * l1w);
                low.push_back(g.op(SPF_OP_KEYSWITCH_L1_TO_L0, {s}));
            }
            g.output(g.pbs_univariate(digits[0], t), uni);
            const Node together = g.public_functional_keyswitch(low);
            g.output(together, glwe);
            g.output(g.op(SPF_OP_CMUX, {g.op(SPF_OP_CIRCUIT_BOOTSTRAP, {digits[0]}), together, x}), out);
        };
        { // one graph of one context
            spf::FheCircuit g(ev);
            std::vector<uint64_t> out(gw), glwe(gw), sums((W - 1) * l1w), uni(l1w);
            chain(g, packed.data(), out.data(), glwe.data(), sums.data(), uni.data());
            g.run();
            expect(same(sums.data(), want_sums.data(), sums.size()), "FheCircuit::pbs_bivariate == spf_pbs_bivariate_dev");
            expect(same(uni.data(), want_uni.data(), l1w), "FheCircuit::pbs_univariate == spf_pbs_univariate_dev");
            expect(same(glwe.data(), want_glwe.data(), gw), "FheCircuit::public_functional_keyswitch == spf_public_functional_keyswitch_enqueue");
            expect(same(out.data(), want_out.data(), gw), "the whole chain in one graph == the _dev calls");
            bool threw = false;
            try {
                g.pbs_bivariate(0, 0, 1, 64);
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... plaintext_bits = 64 throws");
            threw = false;
            try {
                g.public_functional_keyswitch({});
            } catch (const spf::Error& e) {
                threw = e.status == SPF_ERR_INVALID_ARGUMENT;
            }
            expect(threw, "  ... no operands throw");
        }
        { // a job of the whole Evaluation
            spf::FheCircuit job(ev, spf::FheCircuit::Job{});
            std::vector<uint64_t> out(gw), glwe(gw), sums((W - 1) * l1w), uni(l1w);
            chain(job, packed.data(), out.data(), glwe.data(), sums.data(), uni.data());
            spf::FheCircuit::run_all(ev, {&job});
            expect(same(out.data(), want_out.data(), gw) && same(glwe.data(), want_glwe.data(), gw), "the chain as a job of the group == the _dev calls");
        }
        for (int pushed = 0; pushed < 2; pushed++) { // by handle
            spf::PooledEvaluation pe(ev, 64, 100, pushed ? spf::PooledEvaluation::Mode::Pushed : spf::PooledEvaluation::Mode::Blocking);
            {
                spf::L1GlweCiphertext t = pe.upload<spf::L1GlweCiphertext>(lut.data());
                spf::L0LweCiphertext a = pe.upload<spf::L0LweCiphertext>(l0.data()), b = pe.upload<spf::L0LweCiphertext>(l0.data() + l0w);
                spf::L1LweCiphertext s, u;
                pe.pbs_bivariate(s, a, b, t, bits);
                pe.pbs_univariate(u, a, t);
                std::vector<uint64_t> got(l1w);
                s.download(got.data());
                expect(same(got.data(), want_sums.data(), l1w), pushed ? "PooledEvaluation::pbs_bivariate, pushed == spf_pbs_bivariate_dev"
                                                                       : "PooledEvaluation::pbs_bivariate, blocking == spf_pbs_bivariate_dev");
                u.download(got.data());
                expect(same(got.data(), want_uni.data(), l1w), pushed ? "PooledEvaluation::pbs_univariate, pushed == spf_pbs_univariate_dev"
                                                                      : "PooledEvaluation::pbs_univariate, blocking == spf_pbs_univariate_dev");
                bool threw = false;
                try {
                    spf::L1LweCiphertext y;
                    pe.pbs_bivariate(y, a, b, t, 64);
                } catch (const spf::Error& e) {
                    threw = e.status == SPF_ERR_INVALID_ARGUMENT;
                }
                expect(threw, "  ... plaintext_bits = 64 throws");
            }
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
