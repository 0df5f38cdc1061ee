// Native parity test of `Evaluation::public_functional_keyswitch` (include/spf_evaluation.hpp) — test infrastructure.
// One call through the C++ mirror (`public_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/public_functional_keyswitch.rs:
// 74-148) on a key and inputs the Python driver wrote, compared with the words the driver wrote (tests/pufks_cases.py's
// pufks_oracle) and with the C call.  Links libspf_hip.so; built and run by tests/test_gpu_public_functional_keyswitch_cpp.py.
//   usage: public_functional_keyswitch_parity <dir> <from_dimension> <radix_log> <radix_count> <lwe_count> <B>
//   <dir>/key.bin, lwes.bin, want.bin: raw little-endian uint64 words
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
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <dir> <from_dimension> <radix_log> <radix_count> <lwe_count> <B>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t n = std::strtoull(argv[2], nullptr, 10), log = std::strtoull(argv[3], nullptr, 10), count = std::strtoull(argv[4], nullptr, 10);
    const size_t p_in = std::strtoull(argv[5], nullptr, 10), B = std::strtoull(argv[6], nullptr, 10);
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 1; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, gw = (k + 1) * N;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);

    std::vector<uint64_t> key, lwes, want;
    if (!read_words(dir + "/key.bin", key, n * count * gw) || !read_words(dir + "/lwes.bin", lwes, B * p_in * (n + 1)) ||
        !read_words(dir + "/want.bin", want, B * gw)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<double> bsk(ggsw_pbs * 2, 0.0);
        spf::ComputeKey ck{bsk.data(), ggsw_pbs, nullptr, 0};
        spf::Evaluation ev(ck, p, 0);
        std::vector<uint64_t> out(B * gw), c_out(B * gw), one(gw);
        bool threw = false;
        try { ev.public_functional_keyswitch(out.data(), lwes.data(), p_in, B); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
        expect(threw, "before the key is loaded: SPF_ERR_NO_KEY");
        ev.load_public_functional_keyswitch_key(key.data(), key.size(), n, (uint32_t)log, (uint32_t)count);
        ev.public_functional_keyswitch(out.data(), lwes.data(), p_in, B);
        expect(out == want, "Evaluation::public_functional_keyswitch == the driver's words");
        spf_status st = spf_public_functional_keyswitch_batch(ev.raw(), B, p_in, lwes.data(), c_out.data());
        expect(st == SPF_OK && out == c_out, "  ... == spf_public_functional_keyswitch_batch");
        ev.public_functional_keyswitch(one.data(), lwes.data() + (B - 1) * p_in * (n + 1), p_in);
        expect(std::memcmp(one.data(), want.data() + (B - 1) * gw, gw * 8) == 0, "  ... the last output alone");
        threw = false;
        try { ev.public_functional_keyswitch(out.data(), lwes.data(), N + 1, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... lwe_count = N + 1 throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
