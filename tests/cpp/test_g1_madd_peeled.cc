// Host unit test of the G1 bucket accumulation's arithmetic (csrc/fp29.h): the signed mixed addition
// (xyzz29_madd_signed), the affine + affine head of a bucket list (xyzz29_add_affine), the packed-base wrappers the
// kernels call (g1_madd_packed / g1_madd_head) and the carry-free subtractions (sub_loose), against xyzz29_madd on an
// explicitly negated base and against the canonical 32-bit-limb code of ec.h, as field values (X/ZZ, Y/ZZZ).
// The bucket walk below is the one of msm_accumulate.h's accumulate_body.  Build: g++ -std=c++17 -O2 -I legosnark_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "ec.h"
#include "fp29.h"

using namespace lsa;
static std::mt19937_64 rng(20261018);
static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { printf("FAIL %s (line %d)\n", msg, __LINE__); fails++; } } while (0)
typedef unsigned __int128 u128;

static Aff<Fq> rand_point() {   // k*G by double-and-add from (1,2)
    Aff<Fq> g{Fq::from_u32(1), Fq::from_u32(2)};
    XYZZ<Fq> acc = XYZZ<Fq>::inf(), cur = XYZZ<Fq>::from_affine(g);
    uint64_t k = rng() | 1;
    for (int i = 0; i < 64; i++) { if ((k >> i) & 1) acc = xyzz_add(acc, cur); cur = xyzz_dbl(cur); }
    Fq zi = acc.ZZ.inverse(), zzi = acc.ZZZ.inverse();
    return {acc.X * zi, acc.Y * zzi};
}
static AffPacked pack(const Aff<Fq> &a) {            // what CurveG1::from_affine stores
    AffPacked r;
    for (int i = 0; i < 8; i++) { r.x[i] = 0; r.y[i] = 0; }
    if (!a.is_inf()) { F29::from_mont256(a.x).canonical().pack256(r.x); F29::from_mont256(a.y).canonical().pack256(r.y); }
    return r;
}
// equal as points: both infinity, or the same X/ZZ and Y/ZZZ
static bool same(const XYZZ29 &a, const XYZZ29 &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    Fq ax = a.X.to_mont256() * a.ZZ.to_mont256().inverse(), ay = a.Y.to_mont256() * a.ZZZ.to_mont256().inverse();
    Fq bx = b.X.to_mont256() * b.ZZ.to_mont256().inverse(), by = b.Y.to_mont256() * b.ZZZ.to_mont256().inverse();
    return ax == bx && ay == by;
}
static bool same(const XYZZ29 &a, const XYZZ<Fq> &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    Fq ax = a.X.to_mont256() * a.ZZ.to_mont256().inverse(), ay = a.Y.to_mont256() * a.ZZZ.to_mont256().inverse();
    return ax == b.X * b.ZZ.inverse() && ay == b.Y * b.ZZZ.inverse();
}
static const uint32_t PTOP = 0x30644fu;              // (p >> 232) + 1
static bool in_bounds(const XYZZ29 &a) {
    if (a.is_inf()) return a.X.limbs_zero() && a.Y.limbs_zero() && a.ZZZ.limbs_zero();     // infinity is all zeros
    for (int i = 0; i < 8; i++) if ((a.X.l[i] | a.Y.l[i] | a.ZZ.l[i] | a.ZZZ.l[i]) >> 29) return false;
    return a.X.l[8] <= 8 * PTOP && a.Y.l[8] <= 4 * PTOP && a.ZZ.l[8] <= 2 * PTOP && a.ZZZ.l[8] <= 2 * PTOP;
}

struct Entry { AffPacked b; bool neg, endo; };
// the walk of accumulate_body (msm_accumulate.h), one lane per bucket
template <bool ENDO>
static XYZZ29 walk_new(const std::vector<Entry> &e) {
    XYZZ29 acc = XYZZ29::inf();
    size_t j = 0;
    if (e.size() >= 2 && !packed_is_inf(e[0].b) && !packed_is_inf(e[1].b)) {
        acc = g1_madd_head<ENDO>(e[0].b, e[0].neg, e[0].endo, e[1].b, e[1].neg, e[1].endo);
        CHECK(in_bounds(acc), "head bounds");
        j = 2;
    }
    for (; j < e.size(); j++) { acc = g1_madd_packed<ENDO>(acc, e[j].b, e[j].neg, e[j].endo); CHECK(in_bounds(acc), "madd bounds"); }
    return acc;
}
// the same list through the unchanged xyzz29_madd, on an explicitly negated base
static XYZZ29 walk_ref(const std::vector<Entry> &e) {
    XYZZ29 acc = XYZZ29::inf();
    for (const Entry &t : e) {
        Aff29 q = unpack_affine(t.b);                 // (nothing of the new helpers on this side)
        if (q.is_inf()) continue;
        if (t.endo) {                                 // phi(x, y) = (beta * x, y)
            const uint32_t BETA[9] = {0x0a337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu, 0x0176f16du, 0x0eed93bau, 0x14291140u, 0x000c0afeu};
            q.x = mul(q.x, F29::from_limbs(BETA));
        }
        if (t.neg) q.y = sub_k<1>(F29::zero(), q.y);
        acc = xyzz29_madd(acc, q);
    }
    return acc;
}
static void check_list(const std::vector<Entry> &e, const char *what, bool want_inf = false) {
    XYZZ29 r = walk_ref(e), n = walk_new<true>(e);
    CHECK(same(n, r), what);
    if (want_inf) CHECK(n.is_inf() && r.is_inf(), what);
    bool any_endo = false;
    for (const Entry &t : e) any_endo |= t.endo;
    if (!any_endo) CHECK(same(walk_new<false>(e), r), what);
}

// limb-wise maxima of the columns of dot2(a0, b0, a1, b1), reduction terms and carries included, in 128 bits
static u128 dot2_column_max(const F29 &a0, const F29 &b0, const F29 &a1, const F29 &b1) {
    u128 worst = 0, carry = 0;
    for (int k = 0; k < 17; k++) {
        u128 col = carry;
        for (int i = 0; i < 9; i++) {
            const int j = k - i;
            if (j < 0 || j > 8) continue;
            col += (u128)a0.l[i] * b0.l[j] + (u128)a1.l[i] * b1.l[j];
            col += (u128)F29::MASK * F29::p(j);                                 // m_i * p_(k-i), m_i <= 2^29 - 1
        }
        if (col > worst) worst = col;
        carry = col >> 29;
    }
    return worst;
}
static F29 tight_max(int kp_top) {                    // every limb at its maximum for a tight value < kp_top * p
    F29 r;
    for (int i = 0; i < 8; i++) r.l[i] = F29::MASK;
    r.l[8] = (uint32_t)kp_top * PTOP;
    return r;
}

int main() {
    const XYZZ29 I = XYZZ29::inf();
    // ---- the subtraction helpers as field operations, random and at the limb maxima ------------------------------------
    for (int t = 0; t < 3000; t++) {
        Aff<Fq> P = rand_point(), Q = rand_point();   // any field values will do
        Fq a = P.x, b = P.y, c = Q.x;
        F29 A = F29::from_mont256(a), B = F29::from_mont256(b), C = F29::from_mont256(c);      // < 2p, tight
        if (t % 3 == 1) { A = tight_max(2); A.l[8] = 2 * PTOP - 3; a = A.to_mont256(); }      // all low limbs 2^29 - 1, just below 2p
        if (t % 3 == 2) { B = tight_max(2); B.l[8] = 2 * PTOP - 3; b = B.to_mont256(); }
        CHECK(sub_k_signed<6>(A, add_lazy(B, B).norm(), 0u).to_mont256() == a - (b + b), "signed +");
        CHECK(sub_k_signed<6>(A, add_lazy(B, B).norm(), ~0u).to_mont256() == (a + b + b).neg(), "signed -");
        CHECK(sub_k_signed<2>(A.canonical(), B.canonical(), ~0u).to_mont256() == (a + b).neg(), "signed - 2p");
        CHECK(sub_k_signed<2>(A.canonical(), B.canonical(), 0u).to_mont256() == a - b, "signed + 2p");
        for (int s = 0; s < 2; s++) {
            F29 r = sub_k_signed<6>(A, B, s ? ~0u : 0u);
            bool tight = true;
            for (int i = 0; i < 8; i++) tight = tight && (r.l[i] >> 29) == 0;
            CHECK(tight && r.l[8] <= 8 * PTOP, "signed tight");
        }
        // loose differences: limbs within the stated bound, value right (through a product with a tight partner)
        F29 X3 = add_lazy(add_lazy(A, A), add_lazy(B, B)).norm();                              // 2a + 2b < 8p, in the place of X3
        F29 L = sub_loose<10>(C, X3), Lz = sub_loose<6>(F29::zero(), add_lazy(A, B).norm()), L3 = sub_loose<3>(F29::zero(), A);
        bool ok = true;
        for (int i = 0; i < 8; i++) ok = ok && L.l[i] <= 3u * (1u << 29) - 2 && Lz.l[i] <= 3u * (1u << 29) - 2 && L3.l[i] <= 3u * (1u << 29) - 2;
        ok = ok && L.l[8] <= 12 * PTOP && Lz.l[8] <= 6 * PTOP && L3.l[8] <= 3 * PTOP && (int32_t)L.l[8] >= 0 && (int32_t)Lz.l[8] >= 0 && (int32_t)L3.l[8] >= 0;
        CHECK(ok, "loose limb bounds");
        Fq two = Fq::from_u32(2);
        CHECK(mul(L, B).to_mont256() == (c - two * (a + b)) * b, "loose 10p value");
        CHECK(mul(Lz, C).to_mont256() == (a + b).neg() * c, "loose 6p value");
        CHECK(dot2(B, L, Lz, C).to_mont256() == b * (c - two * (a + b)) + (a + b).neg() * c, "dot2 of two loose operands");
    }
    // ---- column maxima of dot2 at the three call sites, from the largest limbs each operand can have ------------------
    {
        const u128 lim = (u128)1 << 64;
        // xyzz29_madd_signed: R < 8p tight, Q < 2p, X3 >= 0, Y1 >= 0, PPP < 2p tight
        u128 m1 = dot2_column_max(tight_max(8), sub_loose<10>(tight_max(2), F29::zero()), sub_loose<6>(F29::zero(), F29::zero()), tight_max(2));
        // xyzz29_add_affine: R < 3p, (3p - y1)
        u128 m2 = dot2_column_max(tight_max(3), sub_loose<10>(tight_max(2), F29::zero()), sub_loose<3>(F29::zero(), F29::zero()), tight_max(2));
        printf("dot2 column maxima / 2^58: madd %.3f  head %.3f  (limit 64)\n", (double)m1 / 288230376151711744.0, (double)m2 / 288230376151711744.0);
        CHECK(m1 < lim && m2 < lim, "dot2 columns below 2^64");
        CHECK(m1 < lim - (lim >> 4), "dot2 columns keep a margin of 2^60");
    }
    // ---- bucket lists ----------------------------------------------------------------------------------------------------
    const AffPacked INF = pack(Aff<Fq>::inf());
    for (int t = 0; t < 60; t++) {
        Aff<Fq> P = rand_point(), Q = rand_point(), S = rand_point();
        AffPacked p = pack(P), q = pack(Q), s = pack(S), pn = pack(P.neg());
        // random lists, both signs, with and without the endomorphism
        for (int len = 1; len <= 6; len++) {
            std::vector<Entry> e;
            for (int i = 0; i < len; i++) e.push_back({pack(rand_point()), (rng() & 1) != 0, false});
            check_list(e, "random list");
            for (Entry &x : e) x.endo = (rng() & 1) != 0;
            check_list(e, "random list with endo");
        }
        for (int sg = 0; sg < 2; sg++) {
            const bool n = sg != 0;
            check_list({{p, n, false}}, "single");
            check_list({{p, n, false}, {q, !n, false}}, "pair, opposite signs");
            check_list({{p, n, false}, {q, n, false}}, "pair, same signs");
            // second entry equal to the first: the head doubles
            check_list({{p, n, false}, {p, n, false}}, "head doubles");
            check_list({{p, n, false}, {p, n, false}, {q, false, false}}, "head doubles, goes on");
            check_list({{p, n, true}, {p, n, true}, {q, true, true}}, "head doubles under endo");
            check_list({{p, n, false}, {pn, !n, false}}, "head doubles through the negated base");
            // second entry the negative of the first: infinity, and a third entry lands on an infinity accumulator
            check_list({{p, n, false}, {p, !n, false}}, "head cancels", true);
            check_list({{p, n, false}, {pn, n, false}}, "head cancels through the negated base", true);
            check_list({{p, n, false}, {p, !n, false}, {q, n, false}}, "third entry on infinity");
            check_list({{p, n, false}, {p, !n, false}, {q, n, false}, {s, !n, false}}, "twoth after infinity");
            // doubling and cancellation at entry 2 (in the loop)
            check_list({{p, n, false}, {q, !n, false}, {q, n, false}}, "entry 2 undoes entry 1");
            check_list({{p, n, false}, {q, false, false}, {p, !n, false}}, "entry 2 undoes entry 0");
            // an infinity base at positions 0, 1, 2 (and everywhere)
            check_list({{INF, n, false}, {p, n, false}, {q, !n, false}}, "infinity at 0");
            check_list({{p, n, false}, {INF, n, false}, {q, !n, false}}, "infinity at 1");
            check_list({{p, n, false}, {q, !n, false}, {INF, n, false}}, "infinity at 2");
            check_list({{p, n, false}, {q, !n, false}, {INF, n, false}, {s, n, false}}, "infinity at 2, goes on");
            check_list({{INF, n, false}}, "only infinity", true);
            check_list({{INF, n, false}, {INF, !n, false}, {INF, n, false}}, "all infinity", true);
            check_list({{INF, n, false}, {INF, !n, false}, {p, n, false}}, "two infinities, then a point");
        }
        // the mixed addition where the accumulator IS the (signed) base: doubling; and its negative: infinity
        for (int sg = 0; sg < 2; sg++) {
            const uint32_t m = sg ? ~0u : 0u;
            XYZZ29 acc = walk_ref({{q, false, false}, {s, true, false}, {p, false, false}});       // Q - S + P, a projective accumulator
            Aff<Fq> A;                                                                              // its affine form
            { Fq x = acc.X.to_mont256() * acc.ZZ.to_mont256().inverse(), y = acc.Y.to_mont256() * acc.ZZZ.to_mont256().inverse(); A = {x, y}; }
            Aff29 a29 = unpack_affine(pack(A)), a29n = unpack_affine(pack(A.neg()));
            Aff29 ref_b = sg ? a29n : a29;
            CHECK(same(xyzz29_madd_signed(acc, a29, m), xyzz29_madd(acc, ref_b)), "madd_signed: acc +- its own point");
            CHECK(same(xyzz29_madd_signed(acc, a29n, m), xyzz29_madd(acc, sg ? a29 : a29n)), "madd_signed: acc +- its negative");
            CHECK(xyzz29_madd_signed(acc, sg ? a29 : a29n, m).is_inf(), "madd_signed: cancels to infinity");
        }
        // accumulator coordinates at the top of their invariants: X < 8p, Y < 4p, ZZ, ZZZ < 2p
        {
            XYZZ29 acc = walk_ref({{q, false, false}, {s, true, false}});
            F29 P1 = sub_k<1>(F29::zero(), F29::zero());                                           // p, tight
            F29 X = acc.X.canonical(), Y = acc.Y.canonical(), ZZ = acc.ZZ.canonical(), ZZZ = acc.ZZZ.canonical();
            XYZZ29 top = {sub_k<7>(X, F29::zero()), sub_k<3>(Y, F29::zero()), add_lazy(ZZ, P1).norm(), add_lazy(ZZZ, P1).norm()};
            CHECK(in_bounds(top) && same(top, acc), "top-of-invariant accumulator");
            CHECK(top.X.l[8] >= 7 * (PTOP - 1) && top.Y.l[8] >= 3 * (PTOP - 1) && top.ZZ.l[8] >= PTOP - 1 && top.ZZZ.l[8] >= PTOP - 1, "top limbs at the top");
            Aff29 b = unpack_affine(p);
            for (int sg = 0; sg < 2; sg++) {
                Aff29 bs = b;
                if (sg) bs.y = sub_k<1>(F29::zero(), b.y);
                XYZZ29 r = xyzz29_madd_signed(top, b, sg ? ~0u : 0u);
                CHECK(same(r, xyzz29_madd(top, bs)) && same(r, xyzz29_madd(acc, bs)) && in_bounds(r), "madd_signed at the top of the invariants");
            }
            // every limb at its stated maximum: the low limbs all 2^29 - 1, the top limbs just below 8p, 4p, 2p, 2p.  Not a
            // point of the curve, but both forms are the same polynomial identities: coordinate by coordinate as field values
            {
                XYZZ29 mx = {tight_max(8), tight_max(4), tight_max(2), tight_max(2)};
                mx.X.l[8] = 8 * (PTOP - 1) - 1; mx.Y.l[8] = 4 * (PTOP - 1) - 1; mx.ZZ.l[8] = 2 * (PTOP - 1) - 1; mx.ZZZ.l[8] = 2 * (PTOP - 1) - 1;
                CHECK(in_bounds(mx), "all-limbs-maximal accumulator within the invariants");
                for (int sg = 0; sg < 2; sg++) {
                    Aff29 bs = b;
                    if (sg) bs.y = sub_k<1>(F29::zero(), b.y);
                    XYZZ29 r = xyzz29_madd_signed(mx, b, sg ? ~0u : 0u), w = xyzz29_madd(mx, bs);
                    CHECK(in_bounds(r) && !r.is_inf(), "madd_signed with every limb maximal: bounds");
                    CHECK(r.X.to_mont256() == w.X.to_mont256() && r.Y.to_mont256() == w.Y.to_mont256() &&
                          r.ZZ.to_mont256() == w.ZZ.to_mont256() && r.ZZZ.to_mont256() == w.ZZZ.to_mont256(), "madd_signed with every limb maximal");
                }
            }
            // the general addition against the canonical 32-bit-limb code, both operands at the top
            XYZZ29 o = walk_ref({{p, true, false}, {s, false, false}, {q, false, false}});
            XYZZ29 otop = {sub_k<7>(o.X.canonical(), F29::zero()), sub_k<3>(o.Y.canonical(), F29::zero()),
                           add_lazy(o.ZZ.canonical(), P1).norm(), add_lazy(o.ZZZ.canonical(), P1).norm()};
            XYZZ<Fq> fa = {acc.X.to_mont256(), acc.Y.to_mont256(), acc.ZZ.to_mont256(), acc.ZZZ.to_mont256()};
            XYZZ<Fq> fo = {o.X.to_mont256(), o.Y.to_mont256(), o.ZZ.to_mont256(), o.ZZZ.to_mont256()};
            XYZZ29 sum = xyzz29_add(top, otop);
            CHECK(same(sum, xyzz_add(fa, fo)) && in_bounds(sum), "add at the top of the invariants");
            CHECK(same(xyzz29_add(acc, o), xyzz_add(fa, fo)), "add");
            CHECK(same(xyzz29_add(top, top), xyzz_dbl(fa)), "add doubles");
            CHECK(xyzz29_add(top, xyzz29_neg(acc)).is_inf(), "add cancels");
            CHECK(same(xyzz29_add(I, otop), fo) && same(xyzz29_add(otop, I), fo), "add with infinity");
        }
    }
    printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
    return fails ? 1 : 0;
}
