// spf_glwe_poly_plan.hpp — what a load of plaintext polynomial weights (spf_load_glwe_poly_weights, spf_glwe_poly.hpp) decides on
// the host before a device is touched: whether the CSR description is legal, which kernel family serves it, and the image the
// kernels read.
//
// A weight matrix is M x K polynomials of R = Z_2^64[X]/(X^N + 1), given sparse: polynomial (m, k) is the sum of
// coefficients[t] * X^exponents[t] over t in [offsets[m K + k], offsets[m K + k + 1]).  Duplicate exponents inside a polynomial
// are legal and add; a polynomial without terms is zero; any int64 coefficient is legal.
//
// Free of HIP (as spf_arena_plan.hpp and spf_wake.hpp): tests/cpp/glwe_poly_plan.cpp drives it on the CPU under the sanitizers.
#pragma once
#include "../../include/spf_hip.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace spf_glwe_poly {

constexpr size_t kMaxPolys = (size_t)1 << 22; // M * K of one slot (the offsets are 16 MiB at most)

struct Verdict {
    spf_status status = SPF_OK;
    std::string message; // the offending numbers, where the status is not SPF_OK
};

inline Verdict refuse(const std::string& message) { return {SPF_ERR_INVALID_ARGUMENT, message}; }

// Every check of a load, in the order the header states them.  The term cap is checked on the LAST offset before any other offset
// and before any term is read, so a caller's description is never walked past what the cap admits.  exponents and coefficients may
// be null where the matrix has no term at all.
inline Verdict validate(uint32_t slot, size_t M, size_t K, size_t N, const uint32_t* offsets, const uint32_t* exponents,
                        const int64_t* coefficients)
{
    const auto n = [](size_t v) { return std::to_string(v); };
    if (slot >= SPF_GLWE_POLY_SLOTS) return refuse("slot " + n(slot) + " >= SPF_GLWE_POLY_SLOTS = " + n(SPF_GLWE_POLY_SLOTS));
    if (!offsets) return refuse("null argument");
    if (M == 0 || K == 0) return refuse("a weight matrix needs M >= 1 and K >= 1, got M = " + n(M) + ", K = " + n(K));
    if (M > SPF_GLWE_POLY_MAX_ROWS) return refuse("M = " + n(M) + " > SPF_GLWE_POLY_MAX_ROWS = " + n(SPF_GLWE_POLY_MAX_ROWS));
    if (K > kMaxPolys / M) return refuse("weight matrix of " + n(M) + " x " + n(K) + " polynomials > the cap of " + n(kMaxPolys) + " per slot");
    const size_t P = M * K;
    if (offsets[0] != 0) return refuse("offsets[0] = " + n(offsets[0]) + ", must be 0");
    const size_t T = offsets[P];
    if (T > SPF_GLWE_POLY_MAX_TERMS) return refuse("offsets[" + n(P) + "] = " + n(T) + " terms > SPF_GLWE_POLY_MAX_TERMS = " + n(SPF_GLWE_POLY_MAX_TERMS));
    for (size_t i = 0; i < P; i++)
        if (offsets[i] > offsets[i + 1])
            return refuse("offsets decrease: offsets[" + n(i) + "] = " + n(offsets[i]) + " > offsets[" + n(i + 1) + "] = " + n(offsets[i + 1]));
    if (T != 0 && (!exponents || !coefficients)) return refuse("null argument");
    for (size_t t = 0; t < T; t++)
        if (exponents[t] >= N) return refuse("exponents[" + n(t) + "] = " + n(exponents[t]) + " >= polynomial_degree = " + n(N));
    return {};
}

// Which kernels serve a slot.  Constants only: every term has exponent 0 (scalar weights: weighted sums, subtraction, negation; a
// matrix without terms is one) — the product needs no rotation and a dense M x K matrix of words describes it.  General: the rest.
enum Class { kConstantsOnly = 0, kGeneral = 1 };

inline Class classify(size_t terms, const uint32_t* exponents)
{
    for (size_t t = 0; t < terms; t++)
        if (exponents[t] != 0) return kGeneral;
    return kConstantsOnly;
}

// One term as the kernels read it: 16 bytes, one scalar load.
struct Term {
    uint64_t coefficient; // the int64 as a word of the torus
    uint32_t exponent;    // < N
    uint32_t zero;
};
static_assert(sizeof(Term) == 16, "a term is one 16-byte load");

struct Image {
    Class cls = kConstantsOnly;
    std::vector<uint32_t> offsets; // [M K + 1], as given
    std::vector<Term> terms;       // [T]
    std::vector<uint64_t> scalars; // constants only: [M][K], the wrapping sum of each polynomial's coefficients; else empty
};

// The device image of a description that validate() has passed.
inline Image pack(size_t M, size_t K, const uint32_t* offsets, const uint32_t* exponents, const int64_t* coefficients)
{
    Image im;
    const size_t P = M * K, T = offsets[P];
    im.cls = classify(T, exponents);
    im.offsets.assign(offsets, offsets + P + 1);
    im.terms.resize(T);
    for (size_t t = 0; t < T; t++) im.terms[t] = Term{(uint64_t)coefficients[t], exponents[t], 0};
    if (im.cls == kConstantsOnly) {
        im.scalars.assign(P, 0);
        for (size_t i = 0; i < P; i++)
            for (size_t t = offsets[i]; t < offsets[i + 1]; t++) im.scalars[i] += (uint64_t)coefficients[t];
    }
    return im;
}

} // namespace spf_glwe_poly
