// Stand-alone test of spf_amd/csrc/spf_glwe_poly_plan.hpp — test infrastructure.  Built from the HIP-free header alone with the
// system g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process by tests/test_glwe_poly_plan.py.
// Every rejection of a load of plaintext polynomial weights with its message, the term cap read from the last offset alone, the
// classification of a slot, the packed image, and seeded random CSR descriptions with mutated offsets and exponents through the
// validator and the packer: an out-of-bounds read of the caller's arrays is the sanitizer's to report.
//   usage: glwe_poly_plan            prints one line per check, "glwe_poly_plan ok" last
#include "../../spf_amd/csrc/spf_glwe_poly_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using namespace spf_glwe_poly;

namespace {

int failures = 0;
void expect(bool ok, const std::string& what)
{
    std::printf("%-90s %s\n", what.c_str(), ok ? "ok" : "FAILED");
    if (!ok) failures++;
}

bool has(const Verdict& v, std::initializer_list<const char*> parts)
{
    if (v.status != SPF_ERR_INVALID_ARGUMENT) return false;
    for (const char* p : parts)
        if (v.message.find(p) == std::string::npos) return false;
    return true;
}

// the arrays of a description, each allocated at exactly its size so that one word past an end is the sanitizer's
struct Csr {
    size_t M, K;
    std::vector<uint32_t> off, exp;
    std::vector<int64_t> coef;
    Verdict check(uint32_t slot, size_t N) const { return validate(slot, M, K, N, off.data(), exp.data(), coef.data()); }
};

Csr random_csr(std::mt19937_64& rng, size_t N, bool constants)
{
    Csr c;
    c.M = 1 + rng() % 6;
    c.K = 1 + rng() % 5;
    c.off.push_back(0);
    for (size_t i = 0; i < c.M * c.K; i++) {
        const size_t terms = rng() % 4 == 0 ? 0 : rng() % 5;
        for (size_t t = 0; t < terms; t++) {
            c.exp.push_back(constants ? 0 : (uint32_t)(rng() % N));
            c.coef.push_back((int64_t)rng());
        }
        c.off.push_back((uint32_t)c.exp.size());
    }
    c.off.shrink_to_fit(); c.exp.shrink_to_fit(); c.coef.shrink_to_fit();
    return c;
}

// the image against the description, term by term
bool image_matches(const Csr& c, const Image& im)
{
    if (im.offsets != c.off || im.terms.size() != c.exp.size()) return false;
    bool constants = true;
    for (size_t t = 0; t < c.exp.size(); t++) {
        if (im.terms[t].coefficient != (uint64_t)c.coef[t] || im.terms[t].exponent != c.exp[t] || im.terms[t].zero != 0) return false;
        constants = constants && c.exp[t] == 0;
    }
    if ((im.cls == kConstantsOnly) != constants) return false;
    if (!constants) return im.scalars.empty();
    if (im.scalars.size() != c.M * c.K) return false;
    for (size_t i = 0; i < c.M * c.K; i++) {
        uint64_t s = 0;
        for (size_t t = c.off[i]; t < c.off[i + 1]; t++) s += (uint64_t)c.coef[t];
        if (im.scalars[i] != s) return false;
    }
    return true;
}

} // namespace

int main()
{
    const size_t N = 128;
    const std::vector<uint32_t> off2 = {0, 1, 2}, exp2 = {0, 5};
    const std::vector<int64_t> coef2 = {INT64_MIN, -1};

    // ---- every rejection, with its numbers
    expect(validate(0, 1, 2, N, off2.data(), exp2.data(), coef2.data()).status == SPF_OK, "a legal description passes (INT64_MIN included)");
    expect(validate(63, 1, 2, N, off2.data(), exp2.data(), coef2.data()).status == SPF_OK, "slot 63 passes");
    expect(has(validate(64, 1, 2, N, off2.data(), exp2.data(), coef2.data()), {"slot 64", "SPF_GLWE_POLY_SLOTS = 64"}), "slot 64");
    expect(has(validate(0, 1, 2, N, nullptr, exp2.data(), coef2.data()), {"null"}), "null offsets");
    expect(has(validate(0, 1, 2, N, off2.data(), nullptr, coef2.data()), {"null"}), "null exponents with terms");
    expect(has(validate(0, 1, 2, N, off2.data(), exp2.data(), nullptr), {"null"}), "null coefficients with terms");
    expect(has(validate(0, 0, 2, N, off2.data(), exp2.data(), coef2.data()), {"M = 0", "K = 2"}), "M = 0");
    expect(has(validate(0, 2, 0, N, off2.data(), exp2.data(), coef2.data()), {"M = 2", "K = 0"}), "K = 0");
    expect(has(validate(0, 4097, 1, N, off2.data(), exp2.data(), coef2.data()), {"M = 4097", "SPF_GLWE_POLY_MAX_ROWS = 4096"}),
           "M above SPF_GLWE_POLY_MAX_ROWS (before an offset is read)");
    expect(has(validate(0, 4096, 1025, N, off2.data(), exp2.data(), coef2.data()), {"4096 x 1025", "4194304"}),
           "M * K above 2^22 (before an offset is read)");
    {
        const std::vector<uint32_t> off = {1, 1, 2};
        expect(has(validate(0, 1, 2, N, off.data(), exp2.data(), coef2.data()), {"offsets[0] = 1"}), "offsets that do not start at 0");
    }
    {
        const std::vector<uint32_t> off = {0, 2, 1, 2};
        const std::vector<uint32_t> e = {0, 0};
        expect(has(validate(0, 1, 3, N, off.data(), e.data(), coef2.data()), {"offsets[1] = 2", "offsets[2] = 1"}), "offsets that decrease");
    }
    {
        // the cap from the last offset alone: two one-word term arrays stand behind 2^24 + 1 claimed terms, and the offsets in
        // between decrease as well — neither is looked at
        const std::vector<uint32_t> off = {0, 9, (1u << 24) + 1};
        const std::vector<uint32_t> e = {0};
        const std::vector<int64_t> co = {1};
        expect(has(validate(0, 1, 2, N, off.data(), e.data(), co.data()), {"16777217", "SPF_GLWE_POLY_MAX_TERMS = 16777216"}),
               "more than SPF_GLWE_POLY_MAX_TERMS terms, read from the last offset alone");
        expect(has(validate(0, 1, 2, N, off.data(), nullptr, nullptr), {"16777217"}), "  ... before the term pointers are looked at");
        const std::vector<uint32_t> at = {0, 0, 1u << 24};
        const Verdict v = validate(0, 1, 2, N, at.data(), nullptr, nullptr);
        expect(has(v, {"null"}), "  ... exactly SPF_GLWE_POLY_MAX_TERMS terms pass the cap (and need their arrays)");
    }
    {
        const std::vector<uint32_t> e = {0, (uint32_t)N};
        expect(has(validate(0, 1, 2, N, off2.data(), e.data(), coef2.data()), {"exponents[1] = 128", "polynomial_degree = 128"}), "an exponent = N");
        const std::vector<uint32_t> last = {0, (uint32_t)N - 1};
        expect(validate(0, 1, 2, N, off2.data(), last.data(), coef2.data()).status == SPF_OK, "an exponent = N - 1 passes");
    }
    {
        const std::vector<uint32_t> off = {0, 0, 0};
        expect(validate(0, 2, 1, N, off.data(), nullptr, nullptr).status == SPF_OK, "no terms at all: the term arrays may be null");
        const Image im = pack(2, 1, off.data(), nullptr, nullptr);
        expect(im.cls == kConstantsOnly && im.terms.empty() && im.scalars == std::vector<uint64_t>{0, 0}, "  ... constants only, all zero");
    }

    // ---- classification and image
    expect(classify(2, exp2.data()) == kGeneral && classify(1, exp2.data()) == kConstantsOnly && classify(0, nullptr) == kConstantsOnly,
           "a slot is constants-only iff every exponent is 0");
    {
        const std::vector<uint32_t> off = {0, 3, 3}, e = {0, 0, 0};
        const std::vector<int64_t> co = {INT64_MAX, INT64_MAX, 2};
        const Image im = pack(1, 2, off.data(), e.data(), co.data());
        expect(im.cls == kConstantsOnly && im.scalars == std::vector<uint64_t>{0, 0}, "duplicate constants add, wrapping: 2 (2^63 - 1) + 2 = 0");
    }

    // ---- seeded random descriptions, then one mutation each
    std::mt19937_64 rng(0x9e3779b97f4a7c15ull);
    int legal = 0, refused = 0, wrong = 0;
    for (int round = 0; round < 400; round++) {
        Csr c = random_csr(rng, N, round % 3 == 0);
        const Verdict v = c.check((uint32_t)(rng() % 64), N);
        if (v.status != SPF_OK || !image_matches(c, pack(c.M, c.K, c.off.data(), c.exp.data(), c.coef.data()))) { wrong++; continue; }
        legal++;
        Csr m = c;
        const size_t P = c.M * c.K, T = c.exp.size();
        bool must_fail = true;
        switch (rng() % 5) {
        case 0: m.off[0] = 1 + (uint32_t)(rng() % 7); break;                                   // does not start at 0
        case 1: m.off[P] = (1u << 24) + 1 + (uint32_t)(rng() % 1000); break;                   // past the cap: nothing else is read
        case 2: {                                                                               // a decrease somewhere
            const size_t i = rng() % P;
            m.off[i] = m.off[i + 1] + 1;                                                        // (i = 0: no longer starts at 0)
            break;
        }
        case 3:                                                                                 // an exponent at or above N
            if (T) m.exp[rng() % T] = (uint32_t)(N + rng() % 3); else must_fail = false;
            break;
        default:                                                                                // a last offset past the arrays' claim:
            m.off[P] = (uint32_t)T;                                                             // (unchanged: still legal)
            must_fail = false;
        }
        const Verdict w = m.check(0, N);
        if (must_fail ? w.status != SPF_ERR_INVALID_ARGUMENT || w.message.empty() : w.status != SPF_OK) wrong++;
        else refused += must_fail;
    }
    std::printf("random: %d descriptions, %d legal, %d mutations refused, %d failed\n", 400, legal, refused, wrong);
    if (wrong || legal != 400) failures++;

    std::printf("%s\n", failures ? "FAILED" : "glwe_poly_plan ok");
    return failures ? 1 : 0;
}
