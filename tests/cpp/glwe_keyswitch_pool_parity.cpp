// Native parity test of `PooledEvaluation::keyswitch_glwe_to_glwe`, `glwe_automorphism` and `trace` (include/spf_evaluation.hpp) —
// test infrastructure.  On a generic context (the driver's N = 16 shape), in pushed mode:
//   * scattered: B GLWEs uploaded one at a time with other uploads in between and taken by descending device address, so that no
//     operand row lies behind the one before; each of the three operations pushed on all of them, one wait: ONE launch of
//     generic_glwe_ks_rows_kernel, the driver's words (the oracle's, tests/glwe_keyswitch_cases.py), the operands unchanged;
//   * pending: mul_xn(x, 2N - 3) -> trace -> sample_extract(0), and on the trace's pending result a keyswitch under slot 0 then one
//     under slot 1 — nothing valid before the single wait, then the driver's words;
//   * refusals throw with their status and leave the output as it was.
// Links libspf_hip.so; built and run by tests/test_gpu_glwe_keyswitch_pool_cpp.py.
//   usage: glwe_keyswitch_pool_parity <dir> <B> <round> <the thirteen spf_params fields in the header's order>
//   <dir>/ak.bin, ksk0.bin, ksk1.bin, glwes.bin, ones.bin, want_keyswitch.bin, want_round.bin, want_trace.bin (B GLWEs each, in
//   item order), want_chain_trace.bin, want_chain_extract.bin, want_chain_k0.bin, want_chain_k1.bin (uint64, raw little-endian)
#include "spf_evaluation.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    std::printf("%-96s %s\n", what, ok ? "ok" : "MISMATCH");
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

bool valid(const spf_value* v)
{
    spf_value_kind kind = SPF_VAL_LWE0;
    int member = 0, ready = 0;
    size_t bytes = 0;
    return spf_value_info(v, &kind, &bytes, &member, &ready) == SPF_OK && ready != 0;
}

uintptr_t address(const spf_value* v)
{
    void* p = nullptr;
    return spf_value_device_ptr(v, &p) == SPF_OK ? (uintptr_t)p : 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 4 + 13) {
        std::fprintf(stderr, "usage: %s <dir> <B> <round> <13 spf_params fields>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t B = std::strtoull(argv[2], nullptr, 10);
    const uint32_t round = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    spf_params p;
    uint32_t* fields[13] = {&p.lwe_dimension, &p.polynomial_degree, &p.glwe_size, &p.pbs_radix_log, &p.pbs_radix_count, &p.cbs_radix_log, &p.cbs_radix_count,
                            &p.ks_radix_log, &p.ks_radix_count, &p.tr_radix_log, &p.tr_radix_count, &p.ss_radix_log, &p.ss_radix_count};
    for (int i = 0; i < 13; i++) *fields[i] = (uint32_t)std::strtoul(argv[4 + i], nullptr, 10);
    const size_t N = p.polynomial_degree, k = p.glwe_size, W = (k + 1) * N, L1 = k * N + 1;
    size_t log_n = 0;
    while (((size_t)1 << log_n) < N) log_n++;
    const size_t bsk_words = (size_t)p.lwe_dimension * (k + 1) * p.pbs_radix_count * (k + 1) * N;
    const size_t ak_words = log_n * k * p.tr_radix_count * (k + 1) * N, ksk_words = k * p.tr_radix_count * (k + 1) * N;

    std::vector<uint64_t> ak, ksk0, ksk1, glwes, ones, want_ks, want_round, want_trace, want_t, want_se, want_k0, want_k1;
    if (!read_file(dir + "/ak.bin", ak, ak_words) || !read_file(dir + "/ksk0.bin", ksk0, ksk_words) || !read_file(dir + "/ksk1.bin", ksk1, ksk_words) ||
        !read_file(dir + "/glwes.bin", glwes, B * W) || !read_file(dir + "/ones.bin", ones, W) || !read_file(dir + "/want_keyswitch.bin", want_ks, B * W) ||
        !read_file(dir + "/want_round.bin", want_round, B * W) || !read_file(dir + "/want_trace.bin", want_trace, B * W) ||
        !read_file(dir + "/want_chain_trace.bin", want_t, W) || !read_file(dir + "/want_chain_extract.bin", want_se, L1) ||
        !read_file(dir + "/want_chain_k0.bin", want_k0, W) || !read_file(dir + "/want_chain_k1.bin", want_k1, W)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<uint64_t> bsk(bsk_words, 0);
        spf::ComputeKeyNonFft ck{bsk.data(), bsk_words, nullptr, 0, ak.data(), ak_words};
        spf::Evaluation ev(ck, p, 0);
        ev.load_glwe_keyswitch_key_std(0, ksk0.data(), ksk_words, p.tr_radix_log, p.tr_radix_count);
        ev.load_glwe_keyswitch_key_std(1, ksk1.data(), ksk_words, p.tr_radix_log, p.tr_radix_count);
        // pushed: a call returns at once with a pending ciphertext; the quiet time (100 ms) is never waited out — a wait closes what was pushed
        spf::PooledEvaluation pe(ev, 64, 100000, spf::PooledEvaluation::Mode::Pushed);
        size_t live_at_start = 0;
        spf_pool_value_stats(pe.raw(), &live_at_start, nullptr, nullptr);
        {
            // ---- scattered operands
            std::vector<spf::L1GlweCiphertext> in(B), between(B);
            for (size_t i = 0; i < B; i++) {
                in[i] = pe.upload<spf::L1GlweCiphertext>(glwes.data() + i * W);
                between[i] = pe.upload<spf::L1GlweCiphertext>(glwes.data() + ((i + 1) % B) * W);
            }
            std::vector<size_t> order(B);
            for (size_t i = 0; i < B; i++) order[i] = i;
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return address(in[a].raw()) > address(in[b].raw()); });
            bool apart = true;
            for (size_t i = 0; i + 1 < B; i++) apart = apart && address(in[order[i + 1]].raw()) != address(in[order[i]].raw()) + 8 * W;
            expect(apart && address(in[0].raw()) != 0, "scattered: no operand row lies behind the one before");
            struct Mode { const char* what; int which; const std::vector<uint64_t>* want; };
            for (const Mode& m : {Mode{"PooledEvaluation::keyswitch_glwe_to_glwe, scattered, one launch of the rows kernel == the driver's words", 0, &want_ks},
                                  Mode{"PooledEvaluation::glwe_automorphism, scattered, one launch of the rows kernel == the driver's words", 1, &want_round},
                                  Mode{"PooledEvaluation::trace, scattered, one launch of the rows kernel == the driver's words", 2, &want_trace}}) {
                spf_pool_counters before{}, after{};
                spf_pool_counters_get(pe.raw(), &before);
                std::vector<spf::L1GlweCiphertext> out(B);
                for (size_t i = 0; i < B; i++) {
                    const spf::L1GlweCiphertext& x = in[order[i]];
                    if (m.which == 0) pe.keyswitch_glwe_to_glwe(out[i], x, 0);
                    else if (m.which == 1) pe.glwe_automorphism(out[i], x, round);
                    else pe.trace(out[i], x);
                }
                bool pending = true;
                for (size_t i = 0; i < B; i++) pending = pending && out[i] && !valid(out[i].raw());
                out[B - 1].wait();
                const std::string kernel = spf_last_glwe_keyswitch_kernel(ev.raw());
                spf_pool_counters_get(pe.raw(), &after);
                bool ok = pending && kernel == "generic_glwe_ks_rows_kernel" && after.handle_ops - before.handle_ops == B && after.handle_launches - before.handle_launches == 1;
                std::vector<uint64_t> got(W);
                for (size_t i = 0; i < B; i++) {
                    out[i].download(got.data());
                    ok = ok && std::equal(got.begin(), got.end(), m.want->begin() + order[i] * W);
                }
                expect(ok, m.what);
            }
            bool unchanged = true;
            std::vector<uint64_t> got(W);
            for (size_t i = 0; i < B; i++) {
                in[i].download(got.data());
                unchanged = unchanged && std::equal(got.begin(), got.end(), glwes.begin() + i * W);
            }
            expect(unchanged, "  ... the operands are unchanged");
        }
        {
            // ---- pending operands, one wait
            spf::L1GlweCiphertext x = pe.upload<spf::L1GlweCiphertext>(ones.data()), m, t, k0, k1;
            spf::L1LweCiphertext se;
            pe.mul_xn(m, x, 2 * N - 3);
            pe.trace(t, m);
            pe.sample_extract_l1(se, t, 0);
            pe.keyswitch_glwe_to_glwe(k0, t, 0);
            pe.keyswitch_glwe_to_glwe(k1, k0, 1);
            expect(!valid(m.raw()) && !valid(t.raw()) && !valid(se.raw()) && !valid(k0.raw()) && !valid(k1.raw()), "pending: nothing is valid before the wait");
            k1.wait();
            expect(valid(t.raw()) && valid(se.raw()) && valid(k0.raw()) && valid(k1.raw()), "  ... everything the chain passed through is valid behind it");
            std::vector<uint64_t> got(W), got_se(L1);
            t.download(got.data());
            expect(got == want_t, "  ... trace(mul_xn(x, 2N - 3)) == the driver's words");
            se.download(got_se.data());
            expect(got_se == want_se, "  ... sample_extract(0) of it == the driver's words");
            k0.download(got.data());
            expect(got == want_k0, "  ... its keyswitch under slot 0 == the driver's words");
            k1.download(got.data());
            expect(got == want_k1, "  ... and that one's keyswitch under slot 1 == the driver's words");

            // ---- refusals: the status, the output left as it was
            struct Bad { const char* what; int which; uint32_t param; spf_status status; };
            for (const Bad& bad : {Bad{"  ... slot = SPF_GLWE_KSK_SLOTS throws SPF_ERR_INVALID_ARGUMENT", 0, SPF_GLWE_KSK_SLOTS, SPF_ERR_INVALID_ARGUMENT},
                                   Bad{"  ... an empty slot throws SPF_ERR_NO_KEY", 0, 9, SPF_ERR_NO_KEY},
                                   Bad{"  ... round = 0 throws SPF_ERR_INVALID_ARGUMENT", 1, 0, SPF_ERR_INVALID_ARGUMENT},
                                   Bad{"  ... round = log2 N + 1 throws SPF_ERR_INVALID_ARGUMENT", 1, (uint32_t)log_n + 1, SPF_ERR_INVALID_ARGUMENT}}) {
                bool threw = false;
                spf_value* const was = k1.raw();
                try {
                    if (bad.which == 0) pe.keyswitch_glwe_to_glwe(k1, x, bad.param);
                    else pe.glwe_automorphism(k1, x, bad.param);
                } catch (const spf::Error& e) {
                    threw = e.status == bad.status;
                }
                expect(threw && k1.raw() == was, bad.what);
            }
        }
        size_t live_at_end = 0;
        spf_pool_value_stats(pe.raw(), &live_at_end, nullptr, nullptr);
        expect(live_at_end == live_at_start, "every value has been let go");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
