// tests/cpp/test_shim_points_io.cc -- libff::lsa_dump_points / lsa_load_points of the shim (one library call per vector) against
// the reference's per-element loops (cputil::dumpIntoFile / loadFromFile, src/utils/util.h:56-96, restated below), under the
// serialisation macros it is compiled with.  Needs the GPU.
//   (no argument)          300 G1 and 300 G2 points, infinity and un-normalised representatives among them: same bytes out, same
//                          points in, the state of external_point_seen()
//   dump FILE              writes the 300 G2 points to FILE with lsa_dump_points
//   load FILE CHECK        lsa_load_points<G2>(FILE, check_subgroup = CHECK): prints "LOADED n", or "REJECTED <what()>"
#include <string.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "libff/lsa_libff.hpp"

using namespace libff;
typedef alt_bn128_Fr Fr_;
typedef alt_bn128_G1 G1_;
typedef alt_bn128_G2 G2_;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

template <class T>
static std::string dump_loop(const std::vector<T> &v) {
    std::ostringstream os;
    os << v.size() << "\n";
    for (const T &x : v) os << x << "\n";
    return os.str();
}
template <class T>
static std::vector<T> load_loop(const std::string &s) {
    std::istringstream is(s);
    size_t sz;
    is >> sz;
    std::vector<T> v(sz);
    for (size_t i = 0; i < sz; i++) is >> v[i];
    return v;
}
template <class T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp((const void *)a.data(), (const void *)b.data(), a.size() * sizeof(T)) == 0);
}

// 300 points: multiples of the generator as the host additions leave them (Z != 1), a few normalised, infinity at both ends
// and in the middle
template <class G>
static std::vector<G> points() {
    std::vector<G> v;
    G step = Fr_(12345L) * G::one(), p = Fr_(1000003L) * G::one();
    v.push_back(G::zero());
    while (v.size() < 299) {
        p = p + step;
        if (v.size() % 50 == 7) v.push_back(G::zero());
        else if (v.size() % 7 == 3) { G q = p; q.to_affine_coordinates(); v.push_back(q); }
        else if (v.size() % 11 == 5) v.push_back(-p);
        else v.push_back(p);
    }
    v.push_back(G::zero());
    return v;
}

template <class G>
static void round_trip(const char *name) {
    const std::vector<G> v = points<G>();
    CHECK(v.size() == 300);
    const std::string want = dump_loop(v);
    std::ostringstream os;
    lsa_dump_points(os, v);
    CHECK(os.str() == want);                                     // byte for byte what the per-element loop writes
    std::vector<G> norm = v;
    for (G &p : norm) p.to_affine_coordinates();                 // host normalisation: (X, Y, one) or (0, 1, 0)
    std::vector<G> got;
    {
        std::istringstream is(want);
        lsa_load_points(is, got);
    }
    CHECK(same_bytes(got, norm));
#if !defined(BINARY_OUTPUT)
    CHECK(same_bytes(got, load_loop<G>(want)));                  // exactly what loadFromFile returns
#endif
    {
        std::istringstream is(want);
        std::vector<G> again(5);
        lsa_load_points(is, again, false);
        CHECK(same_bytes(again, norm));
    }
    std::vector<G> none(3);
    {
        std::ostringstream e;
        lsa_dump_points(e, std::vector<G>());
        CHECK(e.str() == dump_loop(std::vector<G>()));
        std::istringstream is(e.str());
        lsa_load_points(is, none);
        CHECK(none.empty());
    }
    printf("%s: %zu points, %zu bytes\n", name, v.size(), want.size());
}

int main(int argc, char **argv) {
    alt_bn128_pp::init_public_params();
    if (argc >= 3 && std::string(argv[1]) == "dump") {
        std::ofstream f(argv[2], std::ios::binary);
        lsa_dump_points(f, points<G2_>());
        printf(f ? "PASS\n" : "FAIL write\n");
        return f ? 0 : 1;
    }
    if (argc >= 4 && std::string(argv[1]) == "load") {
        std::ifstream f(argv[2], std::ios::binary);
        std::vector<G2_> v;
        try {
            lsa_load_points(f, v, argv[3][0] == '1');
            printf("LOADED %zu\n", v.size());
        } catch (const std::runtime_error &e) {
            printf("REJECTED %s\n", e.what());
        }
        printf("external_point_seen %d\n", (int)G2_::external_point_seen().load());
        printf("PASS\n");
        return 0;
    }
    round_trip<G1_>("G1");
    // G2: a checked load proves every point to lie in G2 and leaves the flag alone ...
    const std::vector<G2_> v = points<G2_>();
    {
        std::ostringstream os;
        lsa_dump_points(os, v);
        std::istringstream is(os.str());
        std::vector<G2_> got;
        lsa_load_points(is, got);
        CHECK(got.size() == v.size());
    }
    CHECK(!G2_::external_point_seen().load());
    // ... one operator>> sets it (the per-element loop inside round_trip reads with it, as does an unchecked load)
    {
        std::ostringstream os;
        os << v[1];
        std::istringstream is(os.str());
        G2_ q;
        is >> q;
        CHECK(q == v[1]);
    }
    CHECK(G2_::external_point_seen().load());
    round_trip<G2_>("G2");
    printf(fails ? "FAILED %d\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
