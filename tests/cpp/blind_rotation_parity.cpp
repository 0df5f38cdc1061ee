// Native parity test of `Evaluation::blind_rotation` (include/spf_evaluation.hpp) — test infrastructure.
// Rotates a batch of two GLWEs by shifts given as random selectors; the expectations are the C call on the same operands and the
// CPU oracle's composition of the reference's steps (`blind_rotation`, sunscreen_tfhe ops/bootstrapping/blind_rotation.rs:202-223:
// `rotate_glwe_negative_monomial_negacyclic` then `cmux` per bit).  Links libspf_hip.so (product) and libspf_oracle.so
// (checker); built and run by tests/test_gpu_blind_rotation_cpp.py.
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

    spfo_rng r;
    spfo_rng_seed(&r, 0xB12);
    std::vector<uint64_t> in(B * gw);
    for (auto& x : in) x = spfo_rng_next(&r);
    std::vector<double> shift(B * n_bits * cbs_len * 2);
    for (auto& x : shift) x = (double)(int64_t)spfo_rng_next(&r) * 0.03125; // magnitudes up to 2^58

    std::vector<uint64_t> ref(B * gw), high(gw), acc(gw), next(gw);
    for (size_t b = 0; b < B; b++) {
        std::memcpy(acc.data(), in.data() + b * gw, gw * 8);
        for (size_t i = 0; i < n_bits; i++) {
            spfo_glwe_mul_xn(high.data(), acc.data(), 2 * N - ((size_t)1 << (i + log_stride)), N, k);
            spfo_cmux(next.data(), acc.data(), high.data(), reinterpret_cast<const spfo_c64*>(shift.data()) + (b * n_bits + i) * cbs_len, N, k,
                      p.cbs_radix_log, p.cbs_radix_count);
            acc.swap(next);
        }
        std::memcpy(ref.data() + b * gw, acc.data(), gw * 8);
    }

    try {
        std::vector<double> bsk(ggsw_pbs * 2, 0.0);
        spf::ComputeKey key{bsk.data(), ggsw_pbs, nullptr, 0};
        spf::Evaluation ev(key, p, 0);
        std::vector<uint64_t> out(B * gw), c_out(B * gw), one(gw);
        ev.blind_rotation(out.data(), shift.data(), in.data(), n_bits, log_stride, B);
        spf_status st = spf_blind_rotation_batch(ev.raw(), B, n_bits, log_stride, shift.data(), in.data(), c_out.data());
        expect(st == SPF_OK && same(out, c_out), "Evaluation::blind_rotation == spf_blind_rotation_batch (B = 2)");
        expect(same(out, ref), "  ... == the oracle's mul_xn + cmux loop");
        ev.blind_rotation(one.data(), shift.data() + n_bits * cbs_len * 2, in.data() + gw, n_bits, log_stride);
        expect(same(one, std::vector<uint64_t>(ref.begin() + gw, ref.end())), "  ... one ciphertext");
        bool threw = false;
        try { ev.blind_rotation(out.data(), shift.data(), in.data(), n_bits, 9, B); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... n_bits + log_stride = 12 throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
