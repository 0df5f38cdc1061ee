// Native parity test of `FheCircuit::glwe_poly_linear` (include/spf_evaluation.hpp) — test infrastructure.
// One graph holds a layer over scattered inputs (slot 0: the K input GLWEs in the order the driver names, out of order and with a
// repeat) and a layer over that layer's rows where they lie (slot 1, K = the first layer's M): the polynomial linear maps
// (`glwe_polynomial_mad` and its kin, sunscreen_tfhe ops/ciphertext/glwe_ciphertext_ops.rs:164-183) as gate-graph nodes.  The two
// CSR matrices, the bias, the inputs and the expected words of both layers (tests/glwe_poly_cases.py's poly_linear_ref) are
// written by the Python driver.  Links libspf_hip.so; built and run by tests/test_gpu_glwe_poly_linear_graph_cpp.py.
//   usage: glwe_poly_linear_graph_parity <dir> <M1> <K> <M2> <T1> <T2> <pick 0> ... <pick K-1>
//   <dir>/a_offsets.bin, a_exponents.bin, b_offsets.bin, b_exponents.bin (uint32), a_coefficients.bin, b_coefficients.bin (int64),
//   a_bias.bin, glwes.bin, want_a.bin, want_b.bin (uint64): raw little-endian
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
    std::printf("%-82s %s\n", what, ok ? "ok" : "MISMATCH");
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
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s <dir> <M1> <K> <M2> <T1> <T2> <picks ...>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const size_t M1 = std::strtoull(argv[2], nullptr, 10), K = std::strtoull(argv[3], nullptr, 10), M2 = std::strtoull(argv[4], nullptr, 10),
                 T1 = std::strtoull(argv[5], nullptr, 10), T2 = std::strtoull(argv[6], nullptr, 10);
    if ((size_t)argc != 7 + K) {
        std::fprintf(stderr, "expected %zu picks\n", K);
        return 2;
    }
    std::vector<size_t> picks;
    for (size_t i = 0; i < K; i++) picks.push_back(std::strtoull(argv[7 + i], nullptr, 10));
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 9; // no bootstrap runs here; every other parameter is DEFAULT_128
    const size_t N = p.polynomial_degree, k = p.glwe_size, W = (k + 1) * N;
    const size_t bsk_complex = p.lwe_dimension * (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);

    std::vector<uint32_t> a_off, a_exp, b_off, b_exp;
    std::vector<int64_t> a_coef, b_coef;
    std::vector<uint64_t> a_bias, glwes, want_a, want_b;
    if (!read_file(dir + "/a_offsets.bin", a_off, M1 * K + 1) || !read_file(dir + "/a_exponents.bin", a_exp, T1) ||
        !read_file(dir + "/a_coefficients.bin", a_coef, T1) || !read_file(dir + "/a_bias.bin", a_bias, M1 * N) ||
        !read_file(dir + "/b_offsets.bin", b_off, M2 * M1 + 1) || !read_file(dir + "/b_exponents.bin", b_exp, T2) ||
        !read_file(dir + "/b_coefficients.bin", b_coef, T2) || !read_file(dir + "/glwes.bin", glwes, K * W) ||
        !read_file(dir + "/want_a.bin", want_a, M1 * W) || !read_file(dir + "/want_b.bin", want_b, M2 * W)) {
        std::fprintf(stderr, "cannot read the driver's files in %s\n", dir.c_str());
        return 2;
    }
    try {
        std::vector<double> bsk(bsk_complex * 2, 0.0);
        spf::ComputeKey ck{bsk.data(), bsk_complex, nullptr, 0};
        spf::Evaluation ev(ck, p, 0);
        using Node = spf::FheCircuit::Node;
        auto layers = [&](spf::FheCircuit& g, uint64_t* a_out, uint64_t* b_out) {
            std::vector<Node> in, ops;
            for (size_t i = 0; i < K; i++) in.push_back(g.input(SPF_VAL_GLWE1, glwes.data() + i * W));
            for (size_t i : picks) ops.push_back(in[i]);
            const std::vector<Node> a = g.glwe_poly_linear(0, ops, M1);
            const std::vector<Node> b = g.glwe_poly_linear(1, a, M2);
            for (size_t m = 0; m < M1; m++) g.output(a[m], a_out + m * W);
            for (size_t m = 0; m < M2; m++) g.output(b[m], b_out + m * W);
        };
        {
            spf::FheCircuit g(ev);
            std::vector<uint64_t> a(M1 * W, 0x55), b(M2 * W, 0x55);
            layers(g, a.data(), b.data()); // built before the slots are loaded: they are read by run()
            bool threw = false;
            try { g.run(); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_NO_KEY; }
            expect(threw && a[0] == 0x55 && b[M2 * W - 1] == 0x55, "before the weights are loaded: run() throws SPF_ERR_NO_KEY, nothing written");
            ev.load_glwe_poly_weights(0, M1, K, a_off.data(), a_exp.data(), a_coef.data(), a_bias.data());
            ev.load_glwe_poly_weights(1, M2, M1, b_off.data(), b_exp.data(), b_coef.data());
            g.run();
            expect(a == want_a, "FheCircuit::glwe_poly_linear over scattered inputs == the driver's words");
            expect(b == want_b, "FheCircuit::glwe_poly_linear over a layer's rows in place == the driver's words");
            expect(std::string(spf_last_glwe_poly_kernel(ev.raw())) == "glwe_poly_lds_kernel", "  ... the second layer on glwe_poly_lds_kernel");
            for (const auto& bad : std::vector<std::pair<const char*, std::vector<size_t>>>{{"  ... M = 0 throws", {0, 1, 0}},
                                                                                         {"  ... no operands throw", {0, 0, 1}},
                                                                                         {"  ... slot = SPF_GLWE_POLY_SLOTS throws", {SPF_GLWE_POLY_SLOTS, 1, 1}}}) {
                threw = false;
                try {
                    g.glwe_poly_linear((uint32_t)bad.second[0], std::vector<Node>(bad.second[1], 0), bad.second[2]);
                } catch (const spf::Error& e) {
                    threw = e.status == SPF_ERR_INVALID_ARGUMENT;
                }
                expect(threw, bad.first);
            }
            std::fill(b.begin(), b.end(), 0);
            g.run();
            expect(b == want_b, "  ... and the graph still runs");
        }
        { // a job of the whole Evaluation
            spf::FheCircuit job(ev, spf::FheCircuit::Job{});
            std::vector<uint64_t> a(M1 * W), b(M2 * W);
            layers(job, a.data(), b.data());
            spf::FheCircuit::run_all(ev, {&job});
            expect(a == want_a && b == want_b, "the two layers as a job of the group == the driver's words");
        }
        { // a slot of another shape is an error of the run, with nothing written
            spf::FheCircuit g(ev);
            std::vector<uint64_t> out(W, 0x55);
            g.output(g.glwe_poly_linear(1, {g.input(SPF_VAL_GLWE1, glwes.data())}, 1)[0], out.data());
            bool threw = false;
            try { g.run(); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
            expect(threw && out[0] == 0x55 && out[W - 1] == 0x55, "a slot of another (M, K) than the nodes': run() throws");
        }
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
