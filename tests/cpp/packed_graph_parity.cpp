// Native parity test of `FheCircuit::unpack` / `FheCircuit::pack` (include/spf_evaluation.hpp) — test infrastructure.
// One graph takes a random packed GLWE apart and puts it together again the way the reference's fluent layer does
// (`graph_input -> unpack -> convert ... pack -> collect_output`, fluent/packed_dynamic_generic_int_graph_node.rs:24-60,
// fluent/dynamic_generic_int_graph_nodes.rs:139-200): unpack (n_bits = N) -> KeyswitchL1toL0 -> CircuitBootstrap ->
// MultiplyGgswGlwe with the trivial one -> pack.  An unpacked bit is an LWE and a packed bit a GLWE, and
// sum_i X^i * sample_extract(x, i) is not the identity on ciphertexts, so nothing is held to the input's words: every
// unpacked row is held to the closed form of `sample_extract` and the packed result to the closed form
// sum_i X^i * row_i (mod X^N + 1, mod 2^64) of the GLWE rows the graph itself produced, both computed here on the host.
// A second pack reads an input, a NOT node and the first pack's result, one of them twice.
// Links libspf_hip.so (product) and libspf_oracle.so (keys only); built and run by tests/test_gpu_packed_graph.py.
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
    std::printf("%-66s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}

// out = sum_i X^i * rows[i] on every polynomial, negacyclic, wrapping
std::vector<uint64_t> closed_form_pack(const std::vector<const uint64_t*>& rows, size_t N, size_t k)
{
    std::vector<uint64_t> out((k + 1) * N, 0);
    for (size_t i = 0; i < rows.size(); i++)
        for (size_t p = 0; p <= k; p++)
            for (size_t j = 0; j < N; j++)
                out[p * N + j] += j >= i ? rows[i][p * N + j - i] : (uint64_t)0 - rows[i][p * N + j + N - i];
    return out;
}

// sample_extract(glwe, h): mask word p*N + j = a[p*N + h - j] when j <= h, else -a[p*N + h + N - j]; body b[h]
std::vector<uint64_t> closed_form_extract(const uint64_t* glwe, size_t h, size_t N, size_t k)
{
    std::vector<uint64_t> out(k * N + 1);
    for (size_t p = 0; p < k; p++)
        for (size_t j = 0; j < N; j++)
            out[p * N + j] = j <= h ? glwe[p * N + h - j] : (uint64_t)0 - glwe[p * N + h + N - j];
    out[k * N] = glwe[k * N + h];
    return out;
}

} // namespace

int main()
{
    spf_params p;
    spf_default_params(&p);
    // the smallest generic shape: N = 16, k = 1 (every kernel of the chain in its generic form)
    p.lwe_dimension = 5; p.polynomial_degree = 16; p.glwe_size = 1;
    p.pbs_radix_log = 6; p.pbs_radix_count = 2; p.cbs_radix_log = 5; p.cbs_radix_count = 3;
    p.ks_radix_log = 2; p.ks_radix_count = 6; p.tr_radix_log = 6; p.tr_radix_count = 5; p.ss_radix_log = 5; p.ss_radix_count = 6;
    const size_t n = p.lwe_dimension, N = p.polynomial_degree, k = p.glwe_size, gw = (k + 1) * N, lw = k * N + 1;
    size_t logn = 0;
    while (((size_t)1 << logn) < N) logn++;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);
    const size_t ak_len = logn * k * p.tr_radix_count * (k + 1) * (N / 2);
    const size_t ssk_len = (k * (k + 1) / 2) * p.ss_radix_count * (k + 1) * (N / 2);

    spfo_rng r;
    spfo_rng_seed(&r, 0x9AC7);
    std::vector<uint64_t> lwe_sk(n), glwe_sk(k * N);
    spfo_gen_binary_key(&r, lwe_sk.data(), n);
    spfo_gen_binary_key(&r, glwe_sk.data(), k * N);
    std::vector<spfo_c64> bsk(n * ggsw_pbs), ak(ak_len), ssk(ssk_len);
    spfo_gen_bsk_fft(&r, bsk.data(), lwe_sk.data(), n, glwe_sk.data(), N, k, p.pbs_radix_log, p.pbs_radix_count, 0.0);
    std::vector<uint64_t> ksk(k * N * p.ks_radix_count * (n + 1));
    spfo_gen_ksk(&r, ksk.data(), glwe_sk.data(), k * N, lwe_sk.data(), n, p.ks_radix_log, p.ks_radix_count, 0.0);
    spfo_gen_auto_key_fft(&r, ak.data(), glwe_sk.data(), N, k, p.tr_radix_log, p.tr_radix_count, 0.0);
    spfo_gen_ssk_fft(&r, ssk.data(), glwe_sk.data(), N, k, p.ss_radix_log, p.ss_radix_count, 0.0);

    std::vector<uint64_t> x(gw);
    for (auto& w : x) w = spfo_rng_next(&r);

    try {
        spf::ComputeKey key{reinterpret_cast<const double*>(bsk.data()), bsk.size(), ksk.data(), ksk.size(),
                            reinterpret_cast<const double*>(ak.data()), ak.size(), reinterpret_cast<const double*>(ssk.data()), ssk.size()};
        spf::Evaluation ev(key, p, 0);
        spf::FheCircuit g(ev);
        using Node = spf::FheCircuit::Node;
        const Node in = g.input(SPF_VAL_GLWE1, x.data());
        const Node one = g.trivial(SPF_VAL_GLWE1, 1);
        const std::vector<Node> bits = g.unpack(in, N);
        std::vector<Node> rows;
        for (Node b : bits) {
            const Node sel = g.op(SPF_OP_CIRCUIT_BOOTSTRAP, {g.op(SPF_OP_KEYSWITCH_L1_TO_L0, {b})});
            rows.push_back(g.op(SPF_OP_MULTIPLY_GGSW_GLWE, {sel, one}));
        }
        const Node packed = g.pack(rows);
        const Node nx = g.op(SPF_OP_NOT, {in});
        const Node again = g.pack({nx, packed, in, nx});
        std::vector<uint64_t> lwe(N * lw), row_words(N * gw), out(gw), out2(gw), nx_words(gw);
        for (size_t i = 0; i < N; i++) {
            g.output(bits[i], lwe.data() + i * lw);
            g.output(rows[i], row_words.data() + i * gw);
        }
        g.output(packed, out.data());
        g.output(nx, nx_words.data());
        g.output(again, out2.data());
        g.run();

        bool ok = true;
        for (size_t i = 0; i < N; i++)
            ok &= std::memcmp(lwe.data() + i * lw, closed_form_extract(x.data(), i, N, k).data(), lw * 8) == 0;
        expect(ok, "FheCircuit::unpack (n_bits = N): every row == sample_extract closed form");
        std::vector<const uint64_t*> ptrs;
        for (size_t i = 0; i < N; i++) ptrs.push_back(row_words.data() + i * gw);
        expect(out == closed_form_pack(ptrs, N, k), "FheCircuit::pack (n_bits = N) == sum X^i * row_i closed form");
        bool nonzero = false;
        for (uint64_t w : out) nonzero |= w != 0;
        expect(nonzero, "  ... and is not all zero");
        expect(out2 == closed_form_pack({nx_words.data(), out.data(), x.data(), nx_words.data()}, N, k),
               "FheCircuit::pack of a NOT node, a pack node and an input, one repeated");
        bool threw = false;
        try { g.unpack(in, N + 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... unpack with n_bits = N + 1 throws");
        threw = false;
        try { g.pack({bits[0]}); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... pack of an LWE node throws");
        std::vector<uint64_t> first = out;
        g.run();
        expect(out == first, "  ... the graph still runs, same words");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
