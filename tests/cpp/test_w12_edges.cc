// Host unit test of the host-compilable forms of the pairing engines (csrc/w12.h, fp29.h) at the limits of their operand
// contract: the operand classes of w12_edge_cases.h (0, 1, p - 1, p, p + 1, 2p - 1, every low limb 2^29 - 1 below p and
// below 2p, v and v + p, one-hot elements) as RAW limbs -- nothing goes through from_mont256 -- through mul_lanes,
// w12_reduce_lane12, w12_xi_times, csqr_lanes and the three forms of w12_comp_mul for every bound of GP_KLIST, values
// against canonical arithmetic and results against "< 2p, tight"; and a 128-bit model of the 64-bit columns and of the
// integer sums T of dot2 / dot4 / the one-phase row product at the limb maxima (the row product's T is built from the
// packed words W12_ROW_C0 / C1 / K that the device code reads).  tools/w12_rows_check.hip runs the same classes through
// the device-only forms.
#include <cstdio>
#include <vector>
#include "tmiller.h"
#include "w12_edge_cases.h"
using namespace lsa;
using namespace w12edge;
typedef unsigned __int128 u128;
static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { if (fails < 20) printf("FAIL %s (line %d)\n", msg, __LINE__); fails++; } } while (0)
struct LoopExec {
    template <class F> void par(F f) { for (unsigned l = 0; l < 64; l++) f(l); }
    unsigned nlanes() const { return 64; }
};
static const double P2_58 = 288230376151711744.0;

// the largest 64-bit accumulator value of a serial n-product chain (mul, dot2, dot4): the limb products of a column, the
// m_i * p_(k-i) terms with m_i <= 2^29 - 1, and the carry of the column before
static u128 dot_column_max(const F29 *a, const F29 *b, int n) {
    u128 worst = 0, carry = 0;
    for (int k = 0; k < 17; k++) {
        u128 col = carry;
        for (int i = 0; i < 9; i++) {
            const int j = k - i;
            if (j < 0 || j > 8) continue;
            for (int t = 0; t < n; t++) col += (u128)a[t].l[i] * b[t].l[j];
            col += (u128)F29::MASK * F29::p(j);
        }
        if (col > worst) worst = col;
        carry = col >> 29;
    }
    return worst;
}
// units * p^2 / 2^261 + p < 4p  <=>  units * p < 3 * 2^261 (bit 261 is bit 29 of limb 8)
static bool reduces_below_4p(uint32_t units) { return kp_minus(units, 0).l[8] < (3u << 29); }
static double bound_in_p(uint32_t units) { return units / 169.2788 + 1.0; }       // 2^261 / p = 169.2788...

template <int KB> static F29 comp_mul_t(unsigned part, const Fq2S &a, const Fq2S &b) { return w12_comp_mul<KB>(part, a, b); }
static F29 comp_mul_static(int K, unsigned part, const Fq2S &a, const Fq2S &b) {
    switch (K) {
    case 2: return comp_mul_t<2>(part, a, b);
    case 4: return comp_mul_t<4>(part, a, b);
    case 5: return comp_mul_t<5>(part, a, b);
    case 6: return comp_mul_t<6>(part, a, b);
    case 8: return comp_mul_t<8>(part, a, b);
    case 10: return comp_mul_t<10>(part, a, b);
    default: return comp_mul_t<40>(part, a, b);
    }
}

int main() {
    const std::vector<Named> el = elements(20261019);
    const int ne = (int)el.size();
    for (const Named &x : el) CHECK(within_contract(x.e), "an operand class inside the contract");
    CHECK(same_limbs(tight_max(1), F29::from_limbs({F29::MASK, F29::MASK, F29::MASK, F29::MASK, F29::MASK, F29::MASK, F29::MASK, F29::MASK, 0x30644du})), "tight maximum below p");
    CHECK(less_than(tight_max(1), kp_minus(1, 0)) && less_than(tight_max(2), kp_minus(2, 0)) && !less_than(tight_max(2), kp_minus(1, 0)), "tight maxima");
    std::vector<Fq2S> lds(W12_LDS_FQ2);
    LoopExec ex;
    W12<LoopExec> w{ex, lds.data(), lds.data() + 6 * W12_SLOTS};

    // ---- mul_lanes: every aliasing of destination and operands ----
    {
        int n = 0;
        auto run = [&](int d, int a, int b, const Elt &ea, const Elt &eb, const char *what) {
            to_slots(ea, w.slot(1));
            to_slots(eb, w.slot(2));
            w.mul_lanes(d, a, b);
            const Elt got = from_slots(w.slot(d));
            CHECK(within_contract(got), what);
            CHECK(same_value(got, fq12_mul(to_tower(ea), to_tower(a == b ? ea : eb))), what);
            n++;
        };
        for (const auto &ab : pairs(ne)) {
            const Elt &a = el[ab.first].e, &b = el[ab.second].e;
            run(3, 1, 2, a, b, "mul_lanes, D apart");
            run(1, 1, 2, a, b, "mul_lanes, D == A");
            run(2, 1, 2, a, b, "mul_lanes, D == B");
        }
        for (const Named &x : el) { run(3, 1, 1, x.e, x.e, "mul_lanes, A == B"); run(1, 1, 1, x.e, x.e, "mul_lanes, D == A == B"); }
        printf("mul_lanes: %d products\n", n);
    }
    // ---- w12_reduce_lane12: 36 partial products of one class each, and mixed ----
    {
        Gen g(3);
        int n = 0;
        for (int c = 0; c < N_CLS + 6; c++) {
            std::vector<Fq2S> P(36), D(6);
            for (Fq2S &x : P) x = Fq2S{Fs{g.value(c < N_CLS ? c : (int)(g.rng() % N_CLS))}, Fs{g.value(c < N_CLS ? c : (int)(g.rng() % N_CLS))}};
            for (unsigned lane = 0; lane < 12; lane++) w12_reduce_lane12(lane, P.data(), D.data());
            const Fq nine = Fq::from_u32(9);
            for (int k = 0; k < 6; k++) {
                Fq lo0 = Fq::zero(), lo1 = Fq::zero(), hi0 = Fq::zero(), hi1 = Fq::zero();
                for (int i = 0; i <= k; i++) { lo0 = lo0 + residue(P[i * 6 + k - i].c0.v); lo1 = lo1 + residue(P[i * 6 + k - i].c1.v); }
                for (int i = k + 1; i <= 5; i++) { hi0 = hi0 + residue(P[i * 6 + k + 6 - i].c0.v); hi1 = hi1 + residue(P[i * 6 + k + 6 - i].c1.v); }
                // the lane multiplies its sum by the Montgomery form of 1: the same residue
                CHECK(D[k].c0.to_mont256() == lo0 + nine * hi0 - hi1, "reduce_lane12 c0");
                CHECK(D[k].c1.to_mont256() == lo1 + nine * hi1 + hi0, "reduce_lane12 c1");
                CHECK(tight_below(D[k].c0.v, 2) && tight_below(D[k].c1.v, 2), "reduce_lane12 result < 2p, tight");
                n += 2;
            }
        }
        printf("w12_reduce_lane12: %d components\n", n);
    }
    // ---- w12_xi_times: every class beside every class ----
    {
        Gen g(4);
        const Fq nine = Fq::from_u32(9);
        for (int a = 0; a < N_CLS; a++) for (int b = 0; b < N_CLS; b++) {
            const F29x2 t{g.value(a), g.value(b)}, r = w12_xi_times(t);
            const Fq t0 = residue(t.c0), t1 = residue(t.c1);
            CHECK(tight_below(r.c0, 20) && tight_below(r.c1, 20), "xi_times result < 20p, tight");
            CHECK(residue(r.c0) == nine * t0 - t1 && residue(r.c1) == nine * t1 + t0, "xi_times value");
        }
    }
    // ---- csqr_lanes: cyclotomic elements, every component canonical / stored as v + p / a mix ----
    {
        Gen g(5);
        int n = 0;
        for (int t = 0; t < 6; t++) {
            const Fq12S a = to_tower(g.all_of(C_RAND));
            Fq12S e = fq12_mul(a.unitary_inverse(), fq12_inverse(a));           // f^(p^6 - 1)
            e = fq12_mul(fq12_frobenius<2>(e), e);                              // ^(p^2 + 1)
            w.store_tower(1, e);
            Elt canon = from_slots(w.slot(1));
            for (F29 &c : canon) c = c.canonical();
            const F29 p = kp_minus(1, 0);
            for (int form = 0; form < 4; form++) {
                Elt in = canon;
                for (int c = 0; c < 12; c++) if (form == 1 || (form == 2 && (c & 1)) || (form == 3 && (g.rng() & 1))) in[c] = add_lazy(canon[c], p).norm();
                CHECK(within_contract(in), "csqr operand inside the contract");
                to_slots(in, w.slot(1));
                w.csqr_lanes(2, 1);
                const Elt got = from_slots(w.slot(2));
                CHECK(within_contract(got), "csqr_lanes result < 2p, tight");
                CHECK(same_value(got, fq12_sqr(e)), "csqr_lanes value");
                n++;
            }
        }
        printf("csqr_lanes: %d squarings\n", n);
    }
    // ---- w12_comp_mul<KB>, w12_comp_mul_k, w12_comp_mul_lift for every bound K of GP_KLIST ----
    // b's components up to the tight maximum below K p, a's up to the tight maximum below A p, A the largest with 2 A K < 169
    {
        Gen g(6);
        int n = 0;
        for (int t = 0; t < 7; t++) {
            const int K = GP_KLIST[t], A = 168 / (2 * K);
            CHECK(2 * A * K < 169 && 2 * (A + 1) * K >= 169, "largest bound of a");
            uint32_t lift[9];
            w12_lift_kp(K, lift);
            std::vector<F29> as = {tight_max((uint32_t)A), kp_minus((uint32_t)A, 1), F29::zero()}, bs = {tight_max((uint32_t)K), kp_minus((uint32_t)K, 1), F29::zero()};
            for (int c = 1; c < N_CLS; c++) { as.push_back(g.value(c)); bs.push_back(g.value(c)); }
            for (size_t ia = 0; ia < as.size(); ia++) for (size_t ib = 0; ib < bs.size(); ib++) {
                // the extremes against each other in all four components; otherwise a second component drawn at random
                const Fq2S a{Fs{as[ia]}, Fs{ia < 2 ? as[ia] : as[g.rng() % as.size()]}}, b{Fs{bs[ib]}, Fs{ib < 2 ? bs[ib] : bs[g.rng() % bs.size()]}};
                const Fq a0 = residue(a.c0.v), a1 = residue(a.c1.v), b0 = residue(b.c0.v), b1 = residue(b.c1.v);
                for (unsigned part = 0; part < 2; part++) {
                    // (a0 y0 + a1 y1) / 2^261: in libff's form (x 2^256) the product of the two 2^256-forms
                    const Fq want = part ? a0 * b1 + a1 * b0 : a0 * b0 - a1 * b1;
                    const F29 r0 = comp_mul_static(K, part, a, b), r1 = w12_comp_mul_k(part, a, b, K), r2 = w12_comp_mul_lift(part, a, b, lift);
                    CHECK(tight_below(r0, 2) && tight_below(r1, 2) && tight_below(r2, 2), "comp_mul result < 2p, tight");
                    // (the lifted form adds p where b1 is within K p mod 2^203 of K p: the same residue, other limbs)
                    CHECK(same_limbs(r0, r1) && (same_limbs(r0, r2) || b.c1.v.l[8] == kp_minus((uint32_t)K, 0).l[8]), "the three forms of comp_mul agree limb for limb");
                    CHECK(residue(r0) == want && residue(r2) == want, "comp_mul value");
                    n++;
                }
            }
        }
        printf("w12_comp_mul (three forms, seven bounds): %d components\n", n);
    }
    // ---- 64-bit columns and integer sums at the limb maxima, in 128-bit integers ----
    {
        const u128 lim = (u128)1 << 64;
        // dot2 in w12_comp_mul<KB> / _k: a < A p tight, y0 = b < K p tight, y1 = K p - b1 <= K p tight; _lift: y1 with limbs 0..6 below
        // 2^30 (the lifted K p itself, b1 = 0).  mul_lanes: a = xi * a_i < 20p, K = 2.
        double worst2 = 0, worst2l = 0;
        for (int t = 0; t < 7; t++) {
            const int K = GP_KLIST[t], A = 168 / (2 * K);
            F29 y1 = kp_minus((uint32_t)K, 0);
            for (int i = 0; i < 8; i++) y1.l[i] = F29::MASK;                      // (limb maxima of a tight value <= K p)
            const F29 a[2] = {tight_max((uint32_t)A), tight_max((uint32_t)A)}, b[2] = {tight_max((uint32_t)K), y1};
            const u128 m = dot_column_max(a, b, 2);
            uint32_t lift[9];
            w12_lift_kp(K, lift);
            F29 yl;
            for (int i = 0; i < 9; i++) yl.l[i] = lift[i];
            if ((int32_t)yl.l[7] < 0) yl.l[7] = 0;                                  // (limb 7 of K p zero: the borrow makes it tight again)
            for (int i = 0; i < 7; i++) CHECK(yl.l[i] < (1u << 30), "lifted limbs below 2^30");
            for (int i = 0; i < 9; i++) yl.l[i] += F29::p(i);                      // (+ p where limb 8 had nothing left to lend: every limb's bound at once)
            for (int i = 0; i < 8; i++) CHECK(yl.l[i] < 3u << 29, "lifted limbs + p below 3 * 2^29");
            const F29 bl[2] = {tight_max((uint32_t)K), yl};
            const u128 ml = dot_column_max(a, bl, 2);
            CHECK(m < lim && ml < lim, "dot2 columns of comp_mul below 2^64");
            if ((double)m > worst2) worst2 = (double)m;
            if ((double)ml > worst2l) worst2l = (double)ml;
            CHECK(2 * A * K < 169, "dot2: T < 169 p^2");
        }
        {
            const F29 a[2] = {tight_max(20), tight_max(20)}, b[2] = {tight_max(2), tight_max(2)};
            const u128 m = dot_column_max(a, b, 2);
            CHECK(m < lim, "dot2 columns of mul_lanes below 2^64");
            if ((double)m > worst2) worst2 = (double)m;
        }
        printf("dot2 column maxima / 2^58: comp_mul %.3f  comp_mul_lift %.3f  (limit 64)\n", worst2 / P2_58, worst2l / P2_58);
        // dot4 in the Granger-Scott rows: from the table, L_i <= (|fa| + |fb|) * 2p, R_i <= 2p * (positive coefficients) + K p with
        // K p covering the negative ones, the fourth product s * (+-2) with both factors < 2p (2p - two <= 2p)
        uint32_t worst_r = 0, worst_t = 0;
        double worst4 = 0;
        for (unsigned type = 0; type < 3; type++) for (unsigned part = 0; part < 2; part++) {
            const W12SqRow &row = w12_sq_row(type, part);
            uint32_t T = 2 * 2;
            F29 a[4], b[4];
            a[3] = tight_max(2); b[3] = tight_max(2);
            for (int i = 0; i < 3; i++) {
                const W12SqTerm &t = row.t[i];
                const int lb = 2 * ((t.fa < 0 ? -t.fa : t.fa) + (t.fb < 0 ? -t.fb : t.fb));
                const int pos = (t.ca > 0 ? t.ca : 0) + (t.cb > 0 ? t.cb : 0), neg = (t.ca < 0 ? -t.ca : 0) + (t.cb < 0 ? -t.cb : 0);
                CHECK(t.fa >= 0 && t.fb >= 0, "L is a plain sum");
                CHECK(t.K >= 2 * neg, "K p keeps R non-negative");
                const uint32_t rb = (uint32_t)(2 * pos + t.K);
                if (rb > worst_r) worst_r = rb;
                T += (uint32_t)lb * rb;
                a[i] = lb ? tight_max((uint32_t)lb) : F29::zero();
                b[i] = rb ? tight_max(rb) : F29::zero();
            }
            if (T > worst_t) worst_t = T;
            const u128 m = dot_column_max(a, b, 4);
            CHECK(m < lim, "dot4 columns below 2^64");
            if ((double)m > worst4) worst4 = (double)m;
        }
        CHECK(worst_r <= 120, "Granger-Scott rows: R_i <= 120 p");
        CHECK(reduces_below_4p(worst_t), "Granger-Scott rows: T / 2^261 + p < 4p");
        printf("dot4 (Granger-Scott rows): R <= %u p, T <= %u p^2 -> < %.3f p, column maximum / 2^58: %.3f  (limit 64)\n", worst_r, worst_t, bound_in_p(worst_t), worst4 / P2_58);
        // the one-phase row product: row (k, part), lane (i, h) multiplies L = a_ih < 2p by R = c0 b_j0 + c1 b_j1 + K p, b < 2p; the
        // three small integers come from the packed words the device code reads
        uint32_t worst_row = 0, worst_rr = 0;
        for (unsigned k = 0; k < 6; k++) for (unsigned part = 0; part < 2; part++) {
            uint32_t T = 0;
            for (unsigned i = 0; i < 6; i++) for (unsigned h = 0; h < 2; h++) {
                const unsigned sh = 8u * ((i > k ? 4u : 0u) | (part << 1) | h);
                const int c0 = (int)(int8_t)(W12_ROW_C0 >> sh), c1 = (int)(int8_t)(W12_ROW_C1 >> sh), K = (int)(int8_t)(W12_ROW_K >> sh);
                const int pos = (c0 > 0 ? c0 : 0) + (c1 > 0 ? c1 : 0), neg = (c0 < 0 ? -c0 : 0) + (c1 < 0 ? -c1 : 0);
                CHECK(K >= 2 * neg, "row product: K p keeps R non-negative");
                const uint32_t rb = (uint32_t)(2 * pos + K);
                if (rb > worst_rr) worst_rr = rb;
                T += 2 * rb;
            }
            if (T > worst_row) worst_row = T;
        }
        CHECK(worst_rr == 20, "row product: R <= 20 p");
        CHECK(worst_row == 408, "row product: T <= 408 p^2 (ten wrapped lanes at 2p * 20p, two plain ones at 2p * 2p)");
        CHECK(reduces_below_4p(worst_row), "row product: T / 2^261 + p < 4p");
        // its columns: a lane's plain product (no m * p terms), the sums of eight tight limbs in 32 bits, the top limb, and the
        // reduction's columns t_k + u_k + sum m_i p_(k-i) + carry
        u128 wide = 0, top = 0, carry = 0;
        const F29 L = tight_max(2), R = tight_max(20);
        for (int k = 0; k < 17; k++) {
            u128 col = 0;
            for (int i = 0; i < 9; i++) if (k - i >= 0 && k - i < 9) col += (u128)L.l[i] * R.l[k - i];
            if (col > wide) wide = col;
            carry = (carry + col) >> 29;
        }
        top = carry;                                                                  // limb 17 of L * R
        u128 redc = 0;
        carry = 0;
        for (int k = 0; k < 17; k++) {
            u128 col = carry + (u128)16 * F29::MASK;
            for (int i = 0; i < 9; i++) if (k - i >= 1 && k - i < 9 && i <= k) col += (u128)F29::MASK * F29::p(k - i);
            if (k < 9) col += (u128)F29::MASK * F29::p(0);
            if (col > redc) redc = col;
            carry = col >> 29;
        }
        CHECK(wide < lim && redc < lim, "row product: columns below 2^64");
        CHECK((u128)8 * F29::MASK < ((u128)1 << 32), "row product: sums of eight tight limbs in 32 bits");
        CHECK(carry + 16 * top < ((u128)1 << 32), "row product: top limb in 32 bits");
        printf("row product: R <= %u p, T <= %u p^2 -> < %.3f p, column maxima / 2^58: lane product %.3f  reduction %.3f  (limit 64)\n",
               worst_rr, worst_row, bound_in_p(worst_row), (double)wide / P2_58, (double)redc / P2_58);
    }
    printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
