// Native parity test of `Evaluation::lwe_linear` (include/spf_evaluation.hpp) — test infrastructure.
// Calls through the C++ mirror (`scalar_mul_ciphertext_mad` + `add_lwe_inplace`, sunscreen_tfhe ops/ciphertext/
// lwe_ciphertext_ops.rs:48-66, :4-18) on weights, a bias and inputs the Python driver wrote, compared with the words the driver
// wrote (tests/lwe_linear_cases.py's linear_ref) and with the C call.  Links libspf_hip.so; built and run by
// tests/test_gpu_lwe_linear_cpp.py.
//   usage: lwe_linear_parity <dir> <M> <K> <B>
//   <dir>/weights.bin (int64), bias.bin, lwes.bin, want.bin: raw little-endian 64-bit words; the ciphertexts are L0 LWEs
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
    std::printf("%-66s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}

bool read_words(const std::string& path, std::vector<uint64_t>& out, size_t words)
{
    out.resize(words);
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(out.data(), 8, words, f);
    const bool at_end = std::fgetc(f) == EOF;
    std::fclose(f);
    return got == words && at_end;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s <dir> <M> <K> <B>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t M = std::strtoull(argv[2], nullptr, 10), K = std::strtoull(argv[3], nullptr, 10), B = std::strtoull(argv[4], nullptr, 10);
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 9; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, W = p.lwe_dimension + 1;
    const size_t bsk_complex = p.lwe_dimension * (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);

    std::vector<uint64_t> weights, bias, lwes, want;
    if (!read_words(dir + "/weights.bin", weights, M * K) || !read_words(dir + "/bias.bin", bias, M) ||
        !read_words(dir + "/lwes.bin", lwes, B * K * W) || !read_words(dir + "/want.bin", want, B * M * W)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    const int64_t* w = reinterpret_cast<const int64_t*>(weights.data());
    try {
        std::vector<double> bsk(bsk_complex * 2, 0.0);
        spf::ComputeKey ck{bsk.data(), bsk_complex, nullptr, 0};
        spf::Evaluation ev(ck, p, 0);
        std::vector<uint64_t> out(B * M * W), c_out(B * M * W), one(M * W);
        bool threw = false;
        try { ev.lwe_linear(out.data(), lwes.data(), 7, SPF_VAL_LWE0, B); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
        expect(threw, "before the weights are loaded: SPF_ERR_NO_KEY");
        ev.load_lwe_linear_weights(7, M, K, w, bias.data());
        ev.lwe_linear(out.data(), lwes.data(), 7, SPF_VAL_LWE0, B);
        expect(out == want, "Evaluation::lwe_linear == the driver's words");
        spf_status st = spf_lwe_linear_batch(ev.raw(), 7, SPF_VAL_LWE0, B, lwes.data(), c_out.data());
        expect(st == SPF_OK && out == c_out, "  ... == spf_lwe_linear_batch");
        ev.lwe_linear(one.data(), lwes.data() + (B - 1) * K * W, 7);
        expect(std::memcmp(one.data(), want.data() + (B - 1) * M * W, M * W * 8) == 0, "  ... the last input vector alone");
        threw = false;
        try { ev.lwe_linear(out.data(), lwes.data(), SPF_LWE_LINEAR_SLOTS, SPF_VAL_LWE0, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... slot = SPF_LWE_LINEAR_SLOTS throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
