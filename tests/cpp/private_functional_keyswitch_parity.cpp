// Native parity test of `Evaluation::private_functional_keyswitch` (include/spf_evaluation.hpp) — test infrastructure.
// Calls through the C++ mirror (`private_functional_keyswitch`, sunscreen_tfhe ops/keyswitch/private_functional_keyswitch.rs:
// 107-142) on keys and inputs the Python driver wrote, compared with the words the driver wrote (tests/pfks_cases.py's pfks_ref)
// and with the C call.  Links libspf_hip.so; built and run by tests/test_gpu_private_functional_keyswitch_cpp.py.
//   usage: private_functional_keyswitch_parity <dir> <n_keys> <from_dimension> <lwe_count> <radix_log> <radix_count> <B>
//   <dir>/keys.bin, lwes.bin, want.bin (n_keys x B outputs, key-major): raw little-endian uint64 words
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
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s <dir> <n_keys> <from_dimension> <lwe_count> <radix_log> <radix_count> <B>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t nk = std::strtoull(argv[2], nullptr, 10), n = std::strtoull(argv[3], nullptr, 10), p_in = std::strtoull(argv[4], nullptr, 10);
    const size_t log = std::strtoull(argv[5], nullptr, 10), count = std::strtoull(argv[6], nullptr, 10), B = std::strtoull(argv[7], nullptr, 10);
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 1; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, gw = (k + 1) * N;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);

    std::vector<uint64_t> keys, lwes, want;
    if (!read_words(dir + "/keys.bin", keys, nk * p_in * (n + 1) * count * gw) || !read_words(dir + "/lwes.bin", lwes, B * p_in * (n + 1)) ||
        !read_words(dir + "/want.bin", want, nk * B * gw)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<double> bsk(ggsw_pbs * 2, 0.0);
        spf::ComputeKey ck{bsk.data(), ggsw_pbs, nullptr, 0};
        spf::Evaluation ev(ck, p, 0);
        std::vector<uint64_t> out(B * gw), c_out(B * gw), one(gw);
        bool threw = false;
        try { ev.private_functional_keyswitch(out.data(), lwes.data(), 0, B); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
        expect(threw, "before the keys are loaded: SPF_ERR_NO_KEY");
        ev.load_private_functional_keyswitch_keys(keys.data(), keys.size(), nk, n, p_in, (uint32_t)log, (uint32_t)count);
        for (size_t q = 0; q < nk; q++) {
            ev.private_functional_keyswitch(out.data(), lwes.data(), q, B);
            expect(std::memcmp(out.data(), want.data() + q * B * gw, B * gw * 8) == 0, "Evaluation::private_functional_keyswitch == the driver's words");
            spf_status st = spf_private_functional_keyswitch_batch(ev.raw(), q, B, lwes.data(), c_out.data());
            expect(st == SPF_OK && out == c_out, "  ... == spf_private_functional_keyswitch_batch");
        }
        ev.private_functional_keyswitch(one.data(), lwes.data() + (B - 1) * p_in * (n + 1), nk - 1);
        expect(std::memcmp(one.data(), want.data() + ((nk - 1) * B + B - 1) * gw, gw * 8) == 0, "  ... the last output alone");
        threw = false;
        try { ev.private_functional_keyswitch(out.data(), lwes.data(), nk, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... key_index = n_keys throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
