// Native parity test of the standard-form (integer) keys of `Evaluation` (include/spf_evaluation.hpp) — test infrastructure.
// One `Evaluation` is built from a `ComputeKeyNonFft` (crypto/keys.rs:145-159: integer words, transformed on the device), a second
// from the `ComputeKey` that the CPU oracle's `PolynomialRef::fft` makes of the same words (`ComputeKeyNonFft::fft`,
// keys.rs:258-282: every polynomial through spfo_poly_fft); both must give the same words for a circuit bootstrap and a CMUX on
// its result, and `Evaluation::poly_fft` must give the oracle's bins.  The key words are uniform (parity does not need honest
// encryptions).  Links libspf_hip.so (product) and libspf_oracle.so (checker); built and run by tests/test_gpu_standard_keys.py.
#include "spf_evaluation.hpp"

extern "C" {
#include "spf_oracle.h"
}

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    std::printf("%-58s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}
template <class T> bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}
std::vector<uint64_t> uniform(spfo_rng* r, size_t n)
{
    std::vector<uint64_t> v(n);
    for (auto& x : v) x = spfo_rng_next(r);
    return v;
}
// `.fft()` of a key: a flat map over its polynomials
std::vector<double> oracle_fft(const std::vector<uint64_t>& words, size_t N)
{
    std::vector<double> out(words.size());
    for (size_t at = 0; at < words.size(); at += N) spfo_poly_fft(words.data() + at, N, reinterpret_cast<spfo_c64*>(out.data() + at));
    return out;
}

} // namespace

int main()
{
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 6; // a short blind rotation; every other parameter is DEFAULT_128
    const size_t n = p.lwe_dimension, N = p.polynomial_degree, k = p.glwe_size;
    size_t logn = 0;
    while (((size_t)1 << logn) < N) logn++;
    const size_t bsk_words = n * (k + 1) * p.pbs_radix_count * (k + 1) * N;
    const size_t ak_words = logn * k * p.tr_radix_count * (k + 1) * N;
    const size_t ssk_words = (k * (k + 1) / 2) * p.ss_radix_count * (k + 1) * N;
    const size_t ksk_words = k * N * p.ks_radix_count * (n + 1);
    const size_t cbs_doubles = 2 * (k + 1) * p.cbs_radix_count * (k + 1) * (N / 2), gw = (k + 1) * N;

    spfo_rng r;
    spfo_rng_seed(&r, 0x57D0);
    const std::vector<uint64_t> bsk = uniform(&r, bsk_words), ak = uniform(&r, ak_words), ssk = uniform(&r, ssk_words),
                                ksk = uniform(&r, ksk_words);
    const std::vector<double> bsk_fft = oracle_fft(bsk, N), ak_fft = oracle_fft(ak, N), ssk_fft = oracle_fft(ssk, N);

    try {
        spf::Evaluation std_ev(spf::ComputeKeyNonFft{bsk.data(), bsk.size(), ksk.data(), ksk.size(), ak.data(), ak.size(), ssk.data(), ssk.size()}, p);
        spf::Evaluation fft_ev(spf::ComputeKey{bsk_fft.data(), bsk_fft.size() / 2, ksk.data(), ksk.size(), ak_fft.data(), ak_fft.size() / 2,
                                               ssk_fft.data(), ssk_fft.size() / 2}, p);
        const size_t B = 3;
        const std::vector<uint64_t> lwe0 = uniform(&r, B * (n + 1)), a = uniform(&r, B * gw), b = uniform(&r, B * gw);
        std::vector<double> g_std(B * cbs_doubles), g_fft(B * cbs_doubles);
        std_ev.circuit_bootstrap(g_std.data(), lwe0.data(), B);
        fft_ev.circuit_bootstrap(g_fft.data(), lwe0.data(), B);
        expect(same(g_std, g_fft), "circuit_bootstrap: ComputeKeyNonFft == ComputeKey(oracle fft)");
        std::vector<uint64_t> c_std(B * gw), c_fft(B * gw);
        std_ev.cmux(c_std.data(), g_std.data(), a.data(), b.data(), B);
        fft_ev.cmux(c_fft.data(), g_fft.data(), a.data(), b.data(), B);
        expect(same(c_std, c_fft), "cmux on its result");

        // Evaluation::poly_fft against the oracle, full-range words and the conversion's corner words
        std::vector<uint64_t> polys = uniform(&r, 5 * N);
        for (size_t i = 0; i < N; i++) {
            polys[i] = i & 1 ? 0x7fffffffffffffffull : 0x8000000000000000ull;
            polys[N + i] = ((uint64_t)1 << 53) + 2 * i + 1;                   // exact ties of the i64 -> f64 conversion
            polys[2 * N + i] = (uint64_t)0 - (((uint64_t)1 << 62) + 512 * (2 * i + 1));
        }
        std::vector<double> got(polys.size());
        std_ev.poly_fft(got.data(), polys.data(), 5);
        expect(same(got, oracle_fft(polys, N)), "poly_fft == spfo_poly_fft");

        // a wrong length is refused and throws; the evaluation that exists stays usable
        bool threw = false;
        try {
            spf::Evaluation bad(spf::ComputeKeyNonFft{bsk.data(), bsk.size() / 2, ksk.data(), ksk.size(), nullptr, 0, nullptr, 0}, p);
        } catch (const spf::Error& e) {
            threw = e.status == SPF_ERR_INVALID_ARGUMENT;
        }
        expect(threw, "a BootstrapKey<u64> of the wrong length is refused");
    } catch (const spf::Error& e) {
        std::printf("spf::Error %d: %s\n", (int)e.status, e.what());
        return 2;
    }
    if (failures) return 1;
    std::printf("all equal\n");
    return 0;
}
