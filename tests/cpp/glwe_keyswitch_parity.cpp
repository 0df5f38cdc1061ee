// Native parity test of `Evaluation::keyswitch_glwe_to_glwe`, `glwe_automorphism` and `trace` (include/spf_evaluation.hpp) — test
// infrastructure.  Calls through the C++ mirror (`keyswitch_glwe_to_glwe`, sunscreen_tfhe ops/fft_ops.rs:457-495; `trace`,
// ops/automorphisms/mod.rs:53-85) on keys and GLWEs the Python driver wrote, compared with the words the driver wrote (the oracle's,
// tests/glwe_keyswitch_cases.py) and with the C calls.  Links libspf_hip.so; built and run by tests/test_gpu_glwe_keyswitch_cpp.py.
//   usage: glwe_keyswitch_parity <dir> <B> <radix_log> <radix_count> <round>
//   <dir>/ak.bin, ksk.bin, glwes.bin, want_keyswitch.bin, want_round.bin, want_trace.bin (uint64): raw little-endian
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

bool read_file(const std::string& path, std::vector<uint64_t>& out, size_t count)
{
    out.resize(count);
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(out.data(), sizeof(uint64_t), count, f);
    const bool at_end = std::fgetc(f) == EOF;
    std::fclose(f);
    return got == count && at_end;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <dir> <B> <radix_log> <radix_count> <round>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t B = std::strtoull(argv[2], nullptr, 10);
    const uint32_t radix_log = (uint32_t)std::strtoul(argv[3], nullptr, 10), radix_count = (uint32_t)std::strtoul(argv[4], nullptr, 10),
                   round = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 9; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, W = (k + 1) * N;
    size_t log_n = 0;
    while (((size_t)1 << log_n) < N) log_n++;
    const size_t bsk_words = p.lwe_dimension * (k + 1) * p.pbs_radix_count * (k + 1) * N;
    const size_t ak_words = log_n * k * p.tr_radix_count * (k + 1) * N, ksk_words = k * radix_count * (k + 1) * N;

    std::vector<uint64_t> ak, ksk, glwes, want_ks, want_round, want_trace;
    if (!read_file(dir + "/ak.bin", ak, ak_words) || !read_file(dir + "/ksk.bin", ksk, ksk_words) || !read_file(dir + "/glwes.bin", glwes, B * W) ||
        !read_file(dir + "/want_keyswitch.bin", want_ks, B * W) || !read_file(dir + "/want_round.bin", want_round, B * W) ||
        !read_file(dir + "/want_trace.bin", want_trace, B * W)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<uint64_t> bsk(bsk_words, 0);
        spf::ComputeKeyNonFft ck{bsk.data(), bsk_words, nullptr, 0, ak.data(), ak_words};
        spf::Evaluation ev(ck, p, 0);
        std::vector<uint64_t> out(B * W), c_out(B * W), one(W);
        bool threw = false;
        try { ev.keyswitch_glwe_to_glwe(out.data(), glwes.data(), 5, B); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
        expect(threw, "before the key is loaded: SPF_ERR_NO_KEY");
        ev.load_glwe_keyswitch_key_std(5, ksk.data(), ksk_words, radix_log, radix_count);
        uint32_t lg = 0, cnt = 0;
        spf_status st = spf_glwe_keyswitch_slot_shape(ev.raw(), 5, &lg, &cnt);
        expect(st == SPF_OK && lg == radix_log && cnt == radix_count, "spf_glwe_keyswitch_slot_shape gives the radix back");

        ev.keyswitch_glwe_to_glwe(out.data(), glwes.data(), 5, B);
        expect(out == want_ks, "Evaluation::keyswitch_glwe_to_glwe == the driver's words");
        expect(std::string(spf_last_glwe_keyswitch_kernel(ev.raw())) == "glwe_ks_kernel", "  ... on glwe_ks_kernel");
        st = spf_glwe_keyswitch_batch(ev.raw(), 5, B, glwes.data(), c_out.data());
        expect(st == SPF_OK && out == c_out, "  ... == spf_glwe_keyswitch_batch");
        ev.keyswitch_glwe_to_glwe(one.data(), glwes.data() + (B - 1) * W, 5);
        expect(std::memcmp(one.data(), want_ks.data() + (B - 1) * W, W * 8) == 0, "  ... the last item alone");

        ev.glwe_automorphism(out.data(), glwes.data(), round, B);
        expect(out == want_round, "Evaluation::glwe_automorphism == the driver's words");
        ev.trace(out.data(), glwes.data(), B);
        expect(out == want_trace, "Evaluation::trace == the driver's words");
        st = spf_glwe_trace_batch(ev.raw(), B, glwes.data(), c_out.data());
        expect(st == SPF_OK && out == c_out, "  ... == spf_glwe_trace_batch");
        c_out = glwes;
        ev.trace(c_out.data(), c_out.data(), B);
        expect(c_out == want_trace, "  ... in place");

        threw = false;
        try { ev.keyswitch_glwe_to_glwe(out.data(), glwes.data(), SPF_GLWE_KSK_SLOTS, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "slot = SPF_GLWE_KSK_SLOTS throws");
        threw = false;
        try { ev.glwe_automorphism(out.data(), glwes.data(), (uint32_t)log_n + 1, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "round = log2 N + 1 throws");
        threw = false;
        try { ev.load_glwe_keyswitch_key_std(5, ksk.data(), ksk_words - 1, radix_log, radix_count); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "a key one word short throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
