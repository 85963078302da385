// tools/w12_rows_check.hip -- the device-only forms of the pairing engines run on the device at the limits of their operand
// contract ("operands < 2p, tight limbs; result < 2p, tight") and compared on the host: the one-phase Fq12 row product
// w12_rows (csrc/w12.h: product, Frobenius map and line product, every aliasing of destination and operands), the 256-lane
// final exponentiation w12_final_exponentiation_h with its helper wavefront, the inline-assembly branch of lin2 (fp29.h)
// and wt_swap / wt_xi_comp (tmiller.h).  The library's C-ABI converts every input with a Montgomery product
// (F29::from_mont256), so no caller can choose the limbs these functions see; here a workgroup copies RAW 9-limb
// operands (tests/cpp/w12_edge_cases.h: 0, 1, p - 1, p, p + 1, 2p - 1, the tight maxima below p and 2p, v and v + p, one-hot
// elements) from global memory into LDS verbatim, runs ONE call and copies the destination's raw limbs back.  The host
// computes the expected value with the tower code over canonical residues and compares canonical 256-bit values; every
// raw result is also held to the contract the next chain link relies on (limbs 0..7 below 2^29, value below 2p).  lin2,
// wt_swap and wt_xi_comp are compared limb for limb with the host's branch of the same function.
// Prints one line per section and "PASS" or "FAILED"; exit status 0 only when everything agrees.  Adds no symbol to the
// library.  Build: make -C legosnark_amd/csrc ../w12_rows_check
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "tmiller.h"
#include "w12_edge_cases.h"

using namespace lsa;
using namespace w12edge;

#define HIP_OK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("FAILED %s: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__); return 2; } } while (0)

enum Op {
    OP_MUL, OP_MUL_NOALIAS, OP_MUL_DA, OP_MUL_DB,        // D apart (NOALIAS false / true), D == A, D == B
    OP_SQR, OP_SQR_DA,                                   // A == B, D == A == B
    OP_FROB1, OP_FROB2, OP_FROB3, OP_FROB1_DA, OP_FROB2_DA, OP_FROB3_DA,
    OP_LINE, OP_LINE_NOALIAS, OP_LINE_DA,
    N_OPS
};
static constexpr int ELT_WORDS = 12 * 9;                 // one slot: six Fq2S
static_assert(sizeof(Fq2S) == 18 * sizeof(uint32_t), "an Fq2S is 18 limbs and nothing else");
struct RowCase { uint32_t op; uint32_t a[ELT_WORDS], b[ELT_WORDS]; };
struct RowOut { uint32_t d[ELT_WORDS]; };
struct Lin2Case { F29 u, v; int32_t cu, cv, K; };

// one case per workgroup of 192 lanes: slot 0 the destination (filled with ones: an engine that stores nothing is seen),
// slot 1 = A, slot 2 = B, raw words
__global__ __launch_bounds__(192) void k_rows(const RowCase *__restrict__ in, RowOut *__restrict__ out, uint32_t n) {
    __shared__ Fq2S lds[3 * 6];
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    const unsigned lane = threadIdx.x;
    uint32_t *w = reinterpret_cast<uint32_t *>(lds);
    if (lane < (unsigned)ELT_WORDS) {
        w[lane] = 0xffffffffu;
        w[ELT_WORDS + lane] = in[c].a[lane];
        w[2 * ELT_WORDS + lane] = in[c].b[lane];
    }
    __syncthreads();
    Fq2S *const D = lds, *const A = lds + 6, *const B = lds + 12, *res = D;
#if defined(__HIP_DEVICE_COMPILE__)                      // (w12.h's row engine is device code only)
    switch (in[c].op) {                                  // (the same for every lane of the workgroup)
    case OP_MUL: w12_rows<W12_MUL>(D, A, B, nullptr); break;
    case OP_MUL_NOALIAS: w12_rows<W12_MUL, false, true>(D, A, B, nullptr); break;
    case OP_MUL_DA: w12_rows<W12_MUL>(A, A, B, nullptr); res = A; break;
    case OP_MUL_DB: w12_rows<W12_MUL>(B, A, B, nullptr); res = B; break;
    case OP_SQR: w12_rows<W12_MUL>(D, A, A, nullptr); break;
    case OP_SQR_DA: w12_rows<W12_MUL>(A, A, A, nullptr); res = A; break;
    case OP_FROB1: w12_rows<W12_FROB>(D, A, nullptr, &LSA_FROB_ROWS[0][0][0][0][0]); break;
    case OP_FROB2: w12_rows<W12_FROB>(D, A, nullptr, &LSA_FROB_ROWS[1][0][0][0][0]); break;
    case OP_FROB3: w12_rows<W12_FROB>(D, A, nullptr, &LSA_FROB_ROWS[2][0][0][0][0]); break;
    case OP_FROB1_DA: w12_rows<W12_FROB>(A, A, nullptr, &LSA_FROB_ROWS[0][0][0][0][0]); res = A; break;
    case OP_FROB2_DA: w12_rows<W12_FROB>(A, A, nullptr, &LSA_FROB_ROWS[1][0][0][0][0]); res = A; break;
    case OP_FROB3_DA: w12_rows<W12_FROB>(A, A, nullptr, &LSA_FROB_ROWS[2][0][0][0][0]); res = A; break;
    case OP_LINE: w12_rows<W12_LINE>(D, A, B, nullptr); break;
    case OP_LINE_NOALIAS: w12_rows<W12_LINE, false, true>(D, A, B, nullptr); break;
    case OP_LINE_DA: w12_rows<W12_LINE>(A, A, B, nullptr); res = A; break;
    default: break;
    }
#endif
    if (lane < (unsigned)ELT_WORDS) out[c].d[lane] = reinterpret_cast<const uint32_t *>(res)[lane];
}

// one element per workgroup of 256 lanes: slot 0 in, the whole chain, slot 0 out
__global__ __launch_bounds__(256) void k_final_exp(const RowOut *__restrict__ in, RowOut *__restrict__ out, uint32_t n) {
    __shared__ Fq2S lds[W12_LDS_FQ2];
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    const unsigned lane = threadIdx.x;
    if (lane < (unsigned)ELT_WORDS) reinterpret_cast<uint32_t *>(lds)[lane] = in[c].d[lane];
    __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)
    w12_final_exponentiation_h(lds);
#endif
    if (lane < (unsigned)ELT_WORDS) out[c].d[lane] = reinterpret_cast<const uint32_t *>(lds)[lane];
}

__global__ __launch_bounds__(64) void k_lin2(const Lin2Case *__restrict__ in, F29 *__restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    out[t] = lin2(in[t].u, in[t].cu, in[t].v, in[t].cv, in[t].K);
}

// n a multiple of 64 (every lane of a wavefront holds a value: the swap reads its neighbour's registers)
__global__ __launch_bounds__(64) void k_wt(const F29 *__restrict__ in, F29 *__restrict__ swapped, F29 *__restrict__ xi) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const F29 mine = in[t];
#if defined(__HIP_DEVICE_COMPILE__)
    const F29 other = wt_swap(mine);
    swapped[t] = other;
    xi[t] = wt_xi_comp(t & 1u, mine, other);
#endif
}

struct LoopExec {
    template <class F> void par(F f) { for (unsigned l = 0; l < 64; l++) f(l); }
    unsigned nlanes() const { return 64; }
};

static void put(uint32_t *w, const Elt &e) { for (int c = 0; c < 12; c++) for (int i = 0; i < 9; i++) w[9 * c + i] = e[c].l[i]; }
static Elt get(const uint32_t *w) { Elt e; for (int c = 0; c < 12; c++) for (int i = 0; i < 9; i++) e[c].l[i] = w[9 * c + i]; return e; }

static int fails = 0;
static void report(const char *section, const char *name_a, const char *name_b, int op, const char *what) {
    if (fails++ < 20) printf("  %s: %s [%s | %s] form %d\n", section, what, name_a, name_b, op);
}

int main() {
    const std::vector<Named> el = elements(20261019);
    const int ne = (int)el.size();
    for (const Named &x : el) if (!within_contract(x.e)) { printf("FAILED an operand class outside the contract: %s\n", x.name); return 2; }

    // ---- the row engine: product, Frobenius maps, line product ----
    std::vector<RowCase> rc;
    std::vector<std::pair<int, int>> who;
    auto add = [&](int op, int a, int b) { RowCase c; c.op = (uint32_t)op; put(c.a, el[a].e); put(c.b, el[b].e); rc.push_back(c); who.push_back({a, b}); };
    const std::vector<std::pair<int, int>> pr = pairs(ne);
    for (const auto &ab : pr) for (int op = OP_MUL; op <= OP_MUL_DB; op++) add(op, ab.first, ab.second);
    for (int a = 0; a < ne; a++) { add(OP_SQR, a, a); add(OP_SQR_DA, a, a); }
    const size_t n_mul = rc.size();
    for (int a = 0; a < ne; a++) for (int op = OP_FROB1; op <= OP_FROB3_DA; op++) add(op, a, a);
    const size_t n_frob = rc.size() - n_mul;
    for (const auto &ab : pr) for (int op = OP_LINE; op <= OP_LINE_DA; op++) add(op, ab.first, ab.second);
    const size_t n_line = rc.size() - n_mul - n_frob;
    {
        const uint32_t n = (uint32_t)rc.size();
        RowCase *d_in; RowOut *d_out;
        std::vector<RowOut> out(n);
        HIP_OK(hipMalloc(&d_in, n * sizeof(RowCase))); HIP_OK(hipMalloc(&d_out, n * sizeof(RowOut)));
        HIP_OK(hipMemcpy(d_in, rc.data(), n * sizeof(RowCase), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xff, n * sizeof(RowOut)));
        hipLaunchKernelGGL(k_rows, dim3(n), dim3(192), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(RowOut), hipMemcpyDeviceToHost));
        int bad[3] = {0, 0, 0}, loose[3] = {0, 0, 0};
        for (uint32_t t = 0; t < n; t++) {
            const int op = (int)rc[t].op, sec = op <= OP_SQR_DA ? 0 : (op <= OP_FROB3_DA ? 1 : 2);
            const Elt &a = el[who[t].first].e, &b = el[who[t].second].e;
            const Fq12S ta = to_tower(a);
            Fq12S want;
            if (sec == 0) want = fq12_mul(ta, to_tower(b));
            else if (op == OP_FROB1 || op == OP_FROB1_DA) want = fq12_frobenius<1>(ta);
            else if (op == OP_FROB2 || op == OP_FROB2_DA) want = fq12_frobenius<2>(ta);
            else if (sec == 1) want = fq12_frobenius<3>(ta);
            else want = fq12_mul(ta, to_tower(embed_line(b)));
            const Elt got = get(out[t].d);
            static const char *const SEC[3] = {"rows product", "rows frobenius", "rows line"};
            if (!within_contract(got)) { loose[sec]++; report(SEC[sec], el[who[t].first].name, el[who[t].second].name, op, "result outside the contract"); }
            if (!same_value(got, want)) { bad[sec]++; report(SEC[sec], el[who[t].first].name, el[who[t].second].name, op, "wrong value"); }
        }
        printf("rows product: %zu workgroups (%zu pairs x 4 forms, %d squares x 2 forms): values differ in %d, results outside the contract in %d\n",
               n_mul, pr.size(), ne, bad[0], loose[0]);
        printf("rows frobenius: %zu workgroups (%d elements x 3 powers x 2 forms): values differ in %d, results outside the contract in %d\n",
               n_frob, ne, bad[1], loose[1]);
        printf("rows line: %zu workgroups (%zu pairs x 3 forms): values differ in %d, results outside the contract in %d\n",
               n_line, pr.size(), bad[2], loose[2]);
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }

    // ---- the 256-lane final exponentiation, whole ----
    {
        std::vector<int> pick;
        for (int c = 0; c < N_CLS; c++) pick.push_back(c);                                  // all <class>: "all 0" and "all p" are zero
        for (int i = N_CLS; i < ne; i += 5) pick.push_back(i);                              // singles, mixed, one-hot
        const uint32_t n = (uint32_t)pick.size();
        std::vector<RowOut> in(n), out(n);
        for (uint32_t t = 0; t < n; t++) put(in[t].d, el[pick[t]].e);
        RowOut *d_in, *d_out;
        HIP_OK(hipMalloc(&d_in, n * sizeof(RowOut))); HIP_OK(hipMalloc(&d_out, n * sizeof(RowOut)));
        HIP_OK(hipMemcpy(d_in, in.data(), n * sizeof(RowOut), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xff, n * sizeof(RowOut)));
        hipLaunchKernelGGL(k_final_exp, dim3(n), dim3(256), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(RowOut), hipMemcpyDeviceToHost));
        std::vector<Fq2S> lds(W12_LDS_FQ2);
        LoopExec ex;
        W12<LoopExec> w{ex, lds.data(), lds.data() + 6 * W12_SLOTS};
        const Fq12S zero12{Fq6T<Fs>::zero(), Fq6T<Fs>::zero()};
        int bad = 0, loose = 0, zeros = 0;
        for (uint32_t t = 0; t < n; t++) {
            const Fq12S f = to_tower(el[pick[t]].e);
            w.store_tower(0, f);
            w.final_exponentiation();
            const Fq12S want = w.load_tower(0);
            const Elt got = get(out[t].d);
            if (!within_contract(got)) { loose++; report("final exponentiation", el[pick[t]].name, "", 0, "result outside the contract"); }
            if (!same_value(got, want)) { bad++; report("final exponentiation", el[pick[t]].name, "", 0, "wrong value"); }
            if (f == zero12) {
                zeros++;
                if (!same_value(got, zero12)) { bad++; report("final exponentiation", el[pick[t]].name, "", 0, "zero does not give zero"); }
            } else if (!(fq12_mul(want, want.unitary_inverse()) == Fq12S::one())) { bad++; report("final exponentiation", el[pick[t]].name, "", 0, "the host chain's result is not unitary"); }
        }
        printf("final exponentiation: %u elements (%d of them zero): values differ in %d, results outside the contract in %d\n", n, zeros, bad, loose);
        if (zeros != 2) { printf("FAILED expected the two zero elements\n"); fails++; }
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }

    // ---- lin2: the multiply-add branch of the device against the host's ----
    {
        Gen g(7);
        std::vector<Lin2Case> c;
        std::vector<F29> vals;
        for (int k = 0; k < N_CLS; k++) vals.push_back(g.value(k));
        for (int s = 0; s < 8; s++) {                                                       // the eight triples of w12_rows
            const int cu = (int)(int8_t)(W12_ROW_C0 >> (8 * s)), cv = (int)(int8_t)(W12_ROW_C1 >> (8 * s)), K = (int)(int8_t)(W12_ROW_K >> (8 * s));
            for (const F29 &u : vals) for (const F29 &v : vals) c.push_back({u, v, cu, cv, K});
        }
        const size_t n_rows = c.size();
        for (int t = 0; t < 7; t++) {                                                       // K p - u of w12_comp_mul_k, u < K p
            const int K = GP_KLIST[t];
            std::vector<F29> us = vals;
            us.push_back(tight_max((uint32_t)K));
            us.push_back(kp_minus((uint32_t)K, 1));
            for (const F29 &u : us) { c.push_back({u, F29::zero(), -1, 0, K}); c.push_back({u, tight_max(2), -1, 0, K}); }
        }
        const uint32_t n = (uint32_t)c.size();
        Lin2Case *d_in; F29 *d_out;
        std::vector<F29> out(n);
        HIP_OK(hipMalloc(&d_in, n * sizeof(Lin2Case))); HIP_OK(hipMalloc(&d_out, n * sizeof(F29)));
        HIP_OK(hipMemcpy(d_in, c.data(), n * sizeof(Lin2Case), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xff, n * sizeof(F29)));
        hipLaunchKernelGGL(k_lin2, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(F29), hipMemcpyDeviceToHost));
        int bad = 0, loose = 0;
        for (uint32_t t = 0; t < n; t++) {
            const F29 want = lin2(c[t].u, c[t].cu, c[t].v, c[t].cv, c[t].K);
            if (!same_limbs(out[t], want)) { bad++; if (fails++ < 20) printf("  lin2: limbs differ at (%d, %d, %d), case %u\n", c[t].cu, c[t].cv, c[t].K, t); }
            if (!tight_below(want, 41) || (int32_t)want.l[8] < 0) { loose++; fails++; }     // (the host's own result: non-negative, tight, at most 40p)
        }
        printf("lin2: %u lanes (%zu on the row product's eight triples, %zu on (-1, 0, K) for the seven bounds): limbs differ in %d, results outside the contract in %d\n",
               n, n_rows, c.size() - n_rows, bad, loose);
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
    }

    // ---- wt_swap / wt_xi_comp ----
    {
        Gen g(11);
        std::vector<F29> in;
        for (int a = 0; a < N_CLS; a++) for (int b = 0; b < N_CLS; b++) { in.push_back(g.value(a)); in.push_back(g.value(b)); }
        while (in.size() % 64) in.push_back(g.value(C_RAND_PP));
        const uint32_t n = (uint32_t)in.size();
        F29 *d_in, *d_sw, *d_xi;
        std::vector<F29> sw(n), xi(n);
        HIP_OK(hipMalloc(&d_in, n * sizeof(F29))); HIP_OK(hipMalloc(&d_sw, n * sizeof(F29))); HIP_OK(hipMalloc(&d_xi, n * sizeof(F29)));
        HIP_OK(hipMemcpy(d_in, in.data(), n * sizeof(F29), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_sw, 0xff, n * sizeof(F29))); HIP_OK(hipMemset(d_xi, 0xff, n * sizeof(F29)));
        hipLaunchKernelGGL(k_wt, dim3(n / 64), dim3(64), 0, 0, d_in, d_sw, d_xi);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(sw.data(), d_sw, n * sizeof(F29), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(xi.data(), d_xi, n * sizeof(F29), hipMemcpyDeviceToHost));
        int bad_sw = 0, bad_xi = 0, loose = 0;
        for (uint32_t t = 0; t < n; t++) {
            if (!same_limbs(sw[t], in[t ^ 1u])) { bad_sw++; fails++; }
            const F29 want = wt_xi_comp(t & 1u, in[t], in[t ^ 1u]);
            if (!same_limbs(xi[t], want)) { bad_xi++; fails++; }
            if (!tight_below(xi[t], 20)) { loose++; fails++; }
        }
        printf("wt_swap / wt_xi_comp: %u lanes: swapped limbs differ in %d, xi limbs differ in %d, results outside the contract in %d\n", n, bad_sw, bad_xi, loose);
        HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_sw)); HIP_OK(hipFree(d_xi));
    }
    printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
