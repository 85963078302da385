// tests/cpp/test_shim_smul_g2.cc -- the shim's batched G2 calls, libff::lsa_scalar_mul_batch on G2 points and
// libff::lsa_mtxmultiexp on columns of (G2 value, row) entries, against the shim's own host `Fr * G2` and `+`: the
// Galbraith-Scott ladder of csrc/smul_host.h, a second, independent implementation (valid here because every point is a
// multiple of the generator).  Built against legosnark_amd/shim only.  Needs the GPU.  Also prints the time per product of
// the host loop and of the batched call (tools/bench_smul_g2.py reads the host figure).
#include <chrono>
#include <cstdio>
#include <vector>

#include "libff/lsa_libff.hpp"

using namespace libff;
typedef alt_bn128_Fr Fr_;
typedef alt_bn128_G2 G2_;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Entry {                                                   // the members lsa_mtxmultiexp reads (CoeffPos, src/utils/matrix.h:35-42)
    G2_ val;
    size_t pos;
};
typedef std::vector<Entry> Col;

int main() {
    alt_bn128_pp::init_public_params();
    const size_t n = 200;
    // bases as the host additions leave them (Z != 1), infinity and a normalised point among them
    std::vector<G2_> pts;
    std::vector<Fr_> sc;
    G2_ step = Fr_(12345L) * G2_::one(), p = Fr_(1000003L) * G2_::one();
    for (size_t i = 0; i < n; i++) {
        p = p + step;
        if (i == 17) pts.push_back(G2_::zero());
        else if (i % 7 == 3) { G2_ q = p; q.to_affine_coordinates(); pts.push_back(q); }
        else if (i % 11 == 5) pts.push_back(-p);
        else pts.push_back(p);
        sc.push_back(i == 0 ? Fr_::zero() : i == 1 ? Fr_::one() : i == 2 ? -Fr_::one() : Fr_::random_element());
    }
    auto t0 = std::chrono::steady_clock::now();
    std::vector<G2_> want(n);
    for (size_t i = 0; i < n; i++) want[i] = sc[i] * pts[i];
    const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / n;
    std::vector<G2_> got = lsa_scalar_mul_batch(pts, sc);         // (the first call pays the library's start-up)
    t0 = std::chrono::steady_clock::now();
    got = lsa_scalar_mul_batch(pts, sc);
    const double call_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    CHECK(got.size() == n);
    size_t bad = 0;
    for (size_t i = 0; i < n && i < got.size(); i++) bad += !(got[i] == want[i]);
    CHECK(bad == 0);
    CHECK(got[17].is_zero() && got[0].is_zero() && got[1] == pts[1] && got[2] == -pts[2]);
    printf("host operator*: %.1f us per product; lsa_scalar_mul_batch: %.1f us for %zu products\n", host_us, call_us, n);

    // a matrix: 12 rows, 30 ragged columns (empty ones, repeated rows, P and -P under one exponent)
    const size_t nrows = 12, ncols = 30;
    std::vector<Fr_> exps(nrows);
    for (Fr_ &e : exps) e = Fr_::random_element();
    exps[3] = Fr_::zero();
    exps[4] = Fr_::one();
    std::vector<Col> M(ncols);
    for (size_t j = 0; j < ncols; j++)
        for (size_t e = 0; e < j % 6; e++) M[j].push_back({pts[(7 * j + 3 * e) % n], (5 * j + e * e) % nrows});
    M[29] = {{pts[5], 2}, {-pts[5], 2}};
    std::vector<G2_> out;
    lsa_mtxmultiexp(out, exps, M);
    CHECK(out.size() == ncols);
    for (size_t j = 0; j < ncols && j < out.size(); j++) {
        G2_ acc = G2_::zero();
        for (const Entry &e : M[j]) acc = acc + exps[e.pos] * e.val;
        CHECK(out[j] == acc);
    }
    CHECK(out[0].is_zero() && out[6].is_zero() && out[29].is_zero());
    printf(fails ? "FAILED %d\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
