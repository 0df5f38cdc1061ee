// Native parity test of `Evaluation::glwe_poly_linear` (include/spf_evaluation.hpp) — test infrastructure.
// Calls through the C++ mirror (`glwe_polynomial_mad`, `glwe_scalar_mad`, `sub_glwe_ciphertexts`, `glwe_negate_inplace`,
// `glwe_rotate`: sunscreen_tfhe ops/ciphertext/glwe_ciphertext_ops.rs:164-183, :189-202, :121-141, :147-156, :285-305) on a CSR
// matrix, a bias and inputs the Python driver wrote, compared with the words the driver wrote (tests/glwe_poly_cases.py's
// poly_linear_ref) and with the C call.  Links libspf_hip.so; built and run by tests/test_gpu_glwe_poly_linear_cpp.py.
//   usage: glwe_poly_linear_parity <dir> <M> <K> <B> <T>
//   <dir>/offsets.bin, exponents.bin (uint32), coefficients.bin (int64), bias.bin, glwes.bin, want.bin (uint64): raw little-endian
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

template <class T> bool read_file(const std::string& path, std::vector<T>& out, size_t count)
{
    out.resize(count);
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(out.data(), sizeof(T), count, f);
    const bool at_end = std::fgetc(f) == EOF;
    std::fclose(f);
    return got == count && at_end;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <dir> <M> <K> <B> <T>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t M = std::strtoull(argv[2], nullptr, 10), K = std::strtoull(argv[3], nullptr, 10), B = std::strtoull(argv[4], nullptr, 10),
                 T = std::strtoull(argv[5], nullptr, 10);
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 9; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, W = (k + 1) * N;
    const size_t bsk_complex = p.lwe_dimension * (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);

    std::vector<uint32_t> offsets, exponents;
    std::vector<int64_t> coefficients;
    std::vector<uint64_t> bias, glwes, want;
    if (!read_file(dir + "/offsets.bin", offsets, M * K + 1) || !read_file(dir + "/exponents.bin", exponents, T) ||
        !read_file(dir + "/coefficients.bin", coefficients, T) || !read_file(dir + "/bias.bin", bias, M * N) ||
        !read_file(dir + "/glwes.bin", glwes, B * K * W) || !read_file(dir + "/want.bin", want, B * M * W)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<double> bsk(bsk_complex * 2, 0.0);
        spf::ComputeKey ck{bsk.data(), bsk_complex, nullptr, 0};
        spf::Evaluation ev(ck, p, 0);
        std::vector<uint64_t> out(B * M * W), c_out(B * M * W), one(M * W);
        bool threw = false;
        try { ev.glwe_poly_linear(out.data(), glwes.data(), 7, B); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
        expect(threw, "before the weights are loaded: SPF_ERR_NO_KEY");
        ev.load_glwe_poly_weights(7, M, K, offsets.data(), exponents.data(), coefficients.data(), bias.data());
        ev.glwe_poly_linear(out.data(), glwes.data(), 7, B);
        expect(out == want, "Evaluation::glwe_poly_linear == the driver's words");
        size_t m_ = 0, k_ = 0, t_ = 0;
        int has_bias = 0;
        spf_status st = spf_glwe_poly_slot_shape(ev.raw(), 7, &m_, &k_, &t_, &has_bias);
        expect(st == SPF_OK && m_ == M && k_ == K && t_ == T && has_bias == 1, "  ... spf_glwe_poly_slot_shape gives the shape back");
        expect(std::string(spf_last_glwe_poly_kernel(ev.raw())) == "glwe_poly_lds_kernel", "  ... on glwe_poly_lds_kernel");
        st = spf_glwe_poly_linear_batch(ev.raw(), 7, B, glwes.data(), c_out.data());
        expect(st == SPF_OK && out == c_out, "  ... == spf_glwe_poly_linear_batch");
        ev.glwe_poly_linear(one.data(), glwes.data() + (B - 1) * K * W, 7);
        expect(std::memcmp(one.data(), want.data() + (B - 1) * M * W, M * W * 8) == 0, "  ... the last item alone");
        threw = false;
        try { ev.glwe_poly_linear(out.data(), glwes.data(), SPF_GLWE_POLY_SLOTS, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... slot = SPF_GLWE_POLY_SLOTS throws");
        threw = false;
        exponents[T - 1] = (uint32_t)N;
        try { ev.load_glwe_poly_weights(7, M, K, offsets.data(), exponents.data(), coefficients.data()); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... an exponent = N throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
