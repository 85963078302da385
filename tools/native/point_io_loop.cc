// tools/native/point_io_loop.cc -- the yardstick of tools/bench_point_load.py: reading and writing a vector of 2^LOG points the
// way the reference does (cputil::dumpIntoFile / loadFromFile, src/utils/util.h:56-96: one operator<< / operator>> per element,
// on one host core; the read performs no subgroup test), beside the shim's bulk lsa_dump_points / lsa_load_points on the same
// points.  Compressed text format (the default macros).  Usage: point_io_loop LOG REPS -- one JSON line per group.
#include <algorithm>
#include <chrono>
#include <sstream>
#include <string>
#include <vector>

#include "libff/lsa_libff.hpp"

using namespace libff;

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; }

template <class G>
static void run(const char *name, size_t n, int reps) {
    std::vector<alt_bn128_Fr> sc(n);
    alt_bn128_Fr s(7L);
    for (size_t i = 0; i < n; i++) { sc[i] = s; s = s * s + alt_bn128_Fr(3L); }
    std::vector<G> v(n);
    const G base = G::one();
    if (detail::group_id<G>::value == 1) lsa_require(lsa_g1_batch_exp(&base, sc.data(), n, v.data(), 0), "batch_exp");
    else lsa_require(lsa_g2_batch_exp(&base, sc.data(), n, v.data(), 0), "batch_exp");
    std::vector<double> dump_loop, load_loop, dump_bulk, load_bulk, load_bulk_nocheck;
    std::string text;
    for (int r = 0; r < reps + 1; r++) {                          // the first pass warms up and is dropped
        double t0 = now_ms();
        std::ostringstream os;
        os << v.size() << "\n";
        for (const G &x : v) os << x << "\n";
        const double t_dump = now_ms() - t0;
        text = os.str();
        std::vector<G> back(n);
        t0 = now_ms();
        {
            std::istringstream is(text);
            size_t sz;
            is >> sz;
            for (size_t i = 0; i < sz; i++) is >> back[i];
        }
        const double t_load = now_ms() - t0;
        t0 = now_ms();
        std::ostringstream ob;
        lsa_dump_points(ob, v);
        const double t_dump_bulk = now_ms() - t0;
        if (ob.str() != text) { printf("FAIL: lsa_dump_points differs from the loop\n"); exit(1); }
        std::vector<G> b1, b2;
        t0 = now_ms();
        { std::istringstream is(text); lsa_load_points(is, b1, true); }
        const double t_load_bulk = now_ms() - t0;
        t0 = now_ms();
        { std::istringstream is(text); lsa_load_points(is, b2, false); }
        const double t_load_nocheck = now_ms() - t0;
        if (memcmp((const void *)b1.data(), (const void *)back.data(), n * sizeof(G)) != 0 || memcmp((const void *)b2.data(), (const void *)back.data(), n * sizeof(G)) != 0) {
            printf("FAIL: lsa_load_points differs from the loop\n");
            exit(1);
        }
        if (r == 0) continue;
        dump_loop.push_back(t_dump); load_loop.push_back(t_load); dump_bulk.push_back(t_dump_bulk); load_bulk.push_back(t_load_bulk);
        load_bulk_nocheck.push_back(t_load_nocheck);
    }
    printf("{\"yardstick\": \"%s\", \"n\": %zu, \"reps\": %d, \"loop_write_ms\": %.3f, \"loop_read_ms\": %.3f, \"lsa_dump_points_ms\": %.3f, "
           "\"lsa_load_points_checked_ms\": %.3f, \"lsa_load_points_unchecked_ms\": %.3f}\n",
           name, n, reps, median(dump_loop), median(load_loop), median(dump_bulk), median(load_bulk), median(load_bulk_nocheck));
    fflush(stdout);
}

int main(int argc, char **argv) {
    const int log = argc > 1 ? atoi(argv[1]) : 16, reps = argc > 2 ? atoi(argv[2]) : 3;
    alt_bn128_pp::init_public_params();
    run<alt_bn128_G1>("g1", (size_t)1 << log, reps);
    run<alt_bn128_G2>("g2", (size_t)1 << log, reps);
    return 0;
}
