// Native parity test of `Evaluation::programmable_bootstrap_bivariate` (include/spf_evaluation.hpp) — test infrastructure.
// The expectation is the CPU oracle's composition of the reference's steps (programmable_bootstrapping.rs:575-621): pack
// left * 2^p + right, then the univariate bootstrap; the LUT is `generate_lut` at p + c bits of the expanded table
// (`generate_bivariate_lut`, :413-452).  Links libspf_hip.so (product) and libspf_oracle.so (checker); built and run by
// tests/test_gpu_bivariate.py.
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
bool same(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(uint64_t)) == 0;
}

} // namespace

int main()
{
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 10; // a short blind rotation keeps the oracle quick; every other parameter is DEFAULT_128
    const size_t n = p.lwe_dimension, N = p.polynomial_degree, k = p.glwe_size;
    const double lwe_std = 7.25e-5, glwe_std = 7e-16;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);
    const uint32_t pb = 2, cb = 2, m = 1u << pb; // plaintext and carry bits

    spfo_rng r;
    spfo_rng_seed(&r, 0xB1CAFE);
    std::vector<uint64_t> lwe_sk(n), glwe_sk(k * N);
    spfo_gen_binary_key(&r, lwe_sk.data(), n);
    spfo_gen_binary_key(&r, glwe_sk.data(), k * N);
    std::vector<spfo_c64> bsk(n * ggsw_pbs);
    spfo_gen_bsk_fft(&r, bsk.data(), lwe_sk.data(), n, glwe_sk.data(), N, k, p.pbs_radix_log, p.pbs_radix_count, glwe_std);

    // f(l, r) = (l + 3r) mod 4 as the table [l * 2^p + r], and the reference's LUT from the expanded table
    std::vector<uint64_t> table(m * m), u((size_t)1 << (pb + cb)), lut((k + 1) * N), lut_ref((k + 1) * N, 0);
    for (uint32_t l = 0; l < m; l++)
        for (uint32_t x = 0; x < m; x++) table[l * m + x] = (l + 3 * x) % m;
    for (size_t x = 0; x < u.size(); x++) u[x] = table[((x >> pb) % m) * m + x % m];
    spfo_generate_lut(lut_ref.data() + k * N, N, u.data(), 1, pb + cb);
    expect(spf_generate_bivariate_lut(&p, table.data(), pb, cb, lut.data()) == SPF_OK && same(lut, lut_ref),
           "spf_generate_bivariate_lut");

    const size_t B = 6, lw = n + 1, ow = k * N + 1;
    std::vector<uint64_t> left(B * lw), right(B * lw), packed(B * lw);
    for (size_t i = 0; i < B; i++) {
        spfo_encrypt_lwe(&r, left.data() + i * lw, lwe_sk.data(), n, (uint64_t)(i % m) << (63 - pb - cb), lwe_std);
        spfo_encrypt_lwe(&r, right.data() + i * lw, lwe_sk.data(), n, (uint64_t)((i / m) % m) << (63 - pb - cb), lwe_std);
    }
    for (size_t j = 0; j < B * lw; j++) packed[j] = left[j] * m + right[j]; // unsigned: wraps mod 2^64
    std::vector<uint64_t> ref(B * ow);
    for (size_t i = 0; i < B; i++)
        spfo_pbs_univariate(ref.data() + i * ow, packed.data() + i * lw, lut_ref.data(), bsk.data(), n, N, k, p.pbs_radix_log,
                            p.pbs_radix_count);

    try {
        spf::ComputeKey key{reinterpret_cast<const double*>(bsk.data()), bsk.size(), nullptr, 0, nullptr, 0, nullptr, 0};
        spf::Evaluation ev(key, p, 0);
        std::vector<uint64_t> out(B * ow), one(ow), self(ow), self_ref(ow);
        ev.programmable_bootstrap_bivariate(out.data(), left.data(), right.data(), lut.data(), pb, B);
        expect(same(out, ref), "Evaluation::programmable_bootstrap_bivariate (B = 6)");
        ev.programmable_bootstrap_bivariate(one.data(), left.data() + 5 * lw, right.data() + 5 * lw, lut.data(), pb);
        expect(same(one, std::vector<uint64_t>(ref.begin() + 5 * ow, ref.end())), "  ... one ciphertext");
        ev.programmable_bootstrap_bivariate(self.data(), left.data(), left.data(), lut.data(), pb);
        std::vector<uint64_t> pk(lw);
        for (size_t j = 0; j < lw; j++) pk[j] = left[j] * m + left[j];
        spfo_pbs_univariate(self_ref.data(), pk.data(), lut_ref.data(), bsk.data(), n, N, k, p.pbs_radix_log, p.pbs_radix_count);
        expect(same(self, self_ref), "  ... left and right the same ciphertext: f(x, x)");
        bool threw = false;
        try { ev.programmable_bootstrap_bivariate(one.data(), left.data(), right.data(), lut.data(), 64); } catch (const spf::Error&) { threw = true; }
        expect(threw, "  ... plaintext_bits = 64 throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
