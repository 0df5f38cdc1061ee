// glwe_keyswitch_pool_driver.cpp — the blocking callers of tools/glwe_keyswitch_pool_bench.py: T host threads, each calling the
// GLWE keyswitch, an automorphism round or the trace on ONE ciphertext synchronously (submit, wait), again and again, as the
// reference's processor calls its evaluator (circuit_processor/mod.rs:192-253).  Python threads cannot generate that load.
// Uses the public C ABI only; built by the bench beside the library:
//   g++ -O2 -std=c++17 -shared -fPIC -pthread -I include -o tools/bin/libglwe_keyswitch_pool_driver.so
//       tools/glwe_keyswitch_pool_driver.cpp -L spf_amd/lib -lspf_hip
#include "spf_hip.h"

#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

extern "C" {

// `threads` callers loop spf_pool_submit_op_v(op, inputs[t], params[t % n_params]) + spf_pool_wait + release of the result for
// `seconds`.  Returns the operations completed, -1 on an error status; *elapsed_s: first submit to last wait.
long glwe_ks_drive_v(spf_pool* pool, int op, const uint32_t* params, size_t n_params, int threads, double seconds, spf_value* const* inputs,
                     double* elapsed_s)
{
    std::atomic<long> done{0};
    std::atomic<int> failed{0};
    std::vector<std::thread> th;
    const auto t0 = std::chrono::steady_clock::now();
    const auto until = t0 + std::chrono::duration<double>(seconds);
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            const uint64_t param = params[(size_t)t % n_params];
            while (std::chrono::steady_clock::now() < until && !failed.load()) {
                uint64_t ticket = 0;
                spf_value* out = nullptr;
                const spf_value* in = inputs[t];
                if (spf_pool_submit_op_v(pool, (spf_graph_op)op, &in, 1, param, &out, &ticket) != SPF_OK) { failed.store(1); break; }
                const spf_status st = spf_pool_wait(pool, ticket);
                spf_value_release(out);
                if (st != SPF_OK) { failed.store(1); break; }
                done.fetch_add(1);
            }
        });
    for (auto& x : th) x.join();
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return failed.load() ? -1 : done.load();
}

// the same by host pointer: every caller owns a copy of `glwe` (`words` words) and its output
long glwe_ks_drive(spf_pool* pool, int op, const uint32_t* params, size_t n_params, int threads, double seconds, const uint64_t* glwe, size_t words,
                   double* elapsed_s)
{
    std::atomic<long> done{0};
    std::atomic<int> failed{0};
    std::vector<std::thread> th;
    std::vector<std::vector<uint64_t>> in((size_t)threads), out((size_t)threads);
    for (int t = 0; t < threads; t++) {
        in[(size_t)t].assign(glwe, glwe + words);
        in[(size_t)t][0] += (uint64_t)t;
        out[(size_t)t].assign(words, 0);
    }
    const auto t0 = std::chrono::steady_clock::now();
    const auto until = t0 + std::chrono::duration<double>(seconds);
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            const uint32_t param = params[(size_t)t % n_params];
            while (std::chrono::steady_clock::now() < until && !failed.load()) {
                uint64_t ticket = 0;
                const uint64_t* x = in[(size_t)t].data();
                uint64_t* y = out[(size_t)t].data();
                const spf_status st = op == SPF_OP_GLWE_KEYSWITCH      ? spf_pool_submit_glwe_keyswitch(pool, param, x, y, &ticket)
                                      : op == SPF_OP_GLWE_AUTOMORPHISM ? spf_pool_submit_glwe_automorphism(pool, param, x, y, &ticket)
                                                                       : spf_pool_submit_glwe_trace(pool, x, y, &ticket);
                if (st != SPF_OK || spf_pool_wait(pool, ticket) != SPF_OK) { failed.store(1); break; }
                done.fetch_add(1);
            }
        });
    for (auto& x : th) x.join();
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return failed.load() ? -1 : done.load();
}

} // extern "C"
