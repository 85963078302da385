// legosnark_amd/csrc/ecntt.h -- the discrete Fourier transform on group elements (lsa_g1_ecntt / lsa_g2_ecntt; kernels and
// host orchestration: ecntt.hip): where the butterflies of each stage find their operands, and what one butterfly computes.
// Kept in a header so that the host tests (tests/cpp/test_ecntt.cc) run the very same code.
//
// The network is the textbook radix-2 decimation in time: n = 2^log_n elements e, stages s = 1 .. log_n, stage s pairs
// e = g 2^s + j with e + 2^(s-1) (group g < n / 2^s, j < 2^(s-1)) under the twiddle w^(j n / 2^s):
//     x[e], x[e + 2^(s-1)]  <-  x[e] + [w^(j n / 2^s)] x[e + 2^(s-1)],  x[e] - [w^(j n / 2^s)] x[e + 2^(s-1)]
// with x[e] = in[bitrev(e)] before stage 1 and out[k] = x[k] = sum_i [w^(ik)] in[i] after stage log_n.
//
// What is particular here is where a stage keeps its elements.  Every butterfly multiplies its second operand by a scalar,
// and both ladders (smul.h, smul_g2.h) want that operand affine, so a stage's second operands are batch-normalised before it
// runs (prepare_bases).  The stages therefore work out of place on two buffers, and stage s - 1 writes every element where
// stage s wants it: butterfly b of stage s reads its first operand at slot b and its second at slot n/2 + b -- the second
// operands are the contiguous upper half, one prepare_bases call -- and the butterflies are numbered j-first,
//     b = j (n / 2^s) + g,
// so that the twiddle index (into the table w^t, t < n/2) is b with its low log_n - s bits cleared, the butterflies with the
// twiddle 1 (no ladder) are the first n / 2^s of the stage, and in the early stages a wavefront's lanes share one twiddle.
// Stage 1 reads the caller's array (bit-reversed index), stage log_n writes natural order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ec.h"
#include "fp29.h"
#include "fp29x2.h"
#include "smul.h"
#include "smul_g2.h"

namespace lsa {

static constexpr unsigned ECNTT_MAX_LOG = 24;      // lsa_g*_ecntt: log_n <= 24

LSA_HD size_t ecntt_bitrev(size_t e, unsigned log_n) {
    size_t r = 0;
    for (unsigned i = 0; i < log_n; i++) r |= ((e >> i) & 1) << (log_n - 1 - i);
    return r;
}

// where stage s (2 <= s <= log_n) finds network element e in its source buffer; s == log_n + 1: natural order, the result
LSA_HD size_t ecntt_slot(unsigned log_n, unsigned s, size_t e) {
    if (s > log_n) return e;
    const size_t half = (size_t)1 << (s - 1), b = ((e & (half - 1)) << (log_n - s)) + (e >> s);
    return ((e >> (s - 1)) & 1) ? ((size_t)1 << (log_n - 1)) + b : b;
}

// Butterfly b < n/2 of stage s (1 <= s <= log_n): the network elements ea < eb it combines, where it reads them (src_a,
// src_b: indices into the caller's array for s == 1, slots of the source buffer otherwise), where it writes the sum (dst_a:
// element ea) and the difference (dst_b: element eb) for stage s + 1, and the index tw of its twiddle in the table w^t, t < n/2.
struct EcnttBfly {
    size_t ea, eb, src_a, src_b, dst_a, dst_b, tw;
};
LSA_HD EcnttBfly ecntt_bfly(unsigned log_n, unsigned s, size_t b) {
    const unsigned low = log_n - s;                          // log2 of the number of groups
    const size_t g = b & (((size_t)1 << low) - 1), j = b >> low;
    EcnttBfly r;
    r.ea = (g << s) + j;
    r.eb = r.ea + ((size_t)1 << (s - 1));
    r.tw = j << low;
    if (s == 1) {
        r.src_a = ecntt_bitrev(r.ea, log_n);
        r.src_b = ecntt_bitrev(r.eb, log_n);
    } else {
        r.src_a = b;
        r.src_b = ((size_t)1 << (log_n - 1)) + b;
    }
    r.dst_a = ecntt_slot(log_n, s + 1, r.ea);
    r.dst_b = ecntt_slot(log_n, s + 1, r.eb);
    return r;
}

// ---- G1.  libff Jacobian -> XYZZ (ZZ = Z^2, ZZZ = Z^3) and an affine base as XYZZ: the operands of the additions
LSA_HD XYZZ29 ecntt_from_jac(const Jac<Fq> &p) {
    if (p.Z.is_zero()) return XYZZ29::inf();
    const F29 z = F29::from_mont256(p.Z), zz = sqr(z);
    return {F29::from_mont256(p.X), F29::from_mont256(p.Y), zz, mul(zz, z)};
}
LSA_HD XYZZ29 ecntt_from_affine(const Aff29 &P) {
    if (P.is_inf()) return XYZZ29::inf();
    return {P.x, P.y, F29::one(), F29::one()};                         // (smul_glv's own T[0])
}
// [w] B for a butterfly's second operand B (affine, canonical) and the canonical words w of its twiddle.  one: the twiddle
// is known to be 1 (tw == 0) and no ladder runs.  T: SMUL_TBL entries of scratch owned by the caller.
LSA_HD XYZZ29 ecntt_twiddled(const Aff29 &B, const uint32_t w[8], bool one, XYZZ29 *T) {
    return one ? ecntt_from_affine(B) : smul_glv(B, w, T);
}
// A + T and A - T, complete: A == T (doubling), A == -T, either side infinite.  A: from ecntt_from_jac (X, Y < p); T: from
// ecntt_twiddled, within the accumulator invariants of fp29.h; -T has Y <= 4p as in smul_glv's negated table entries.
LSA_HD void ecntt_combine(const XYZZ29 &A, const XYZZ29 &T, XYZZ29 &sum, XYZZ29 &diff) {
    sum = xyzz29_add(A, T);
    diff = xyzz29_add(A, xyzz29_neg(T));
}

// ---- G2, over any representation E of Fq2 (fp29x2.h): F29x2 on the host, the lane pair's F29h in the kernels
template <class E>
LSA_HD XyzzE<E> ecntt_from_affine(const AffE<E> &P) {
    if (P.is_inf()) return XyzzE<E>::inf();
    return {P.x, P.y, E::one(), E::one()};                             // [<1, <1, <1, <1; tight]  (smul_g2's own T[0])
}
// the integer multiple [w] B: the transform of the header only for points of the order-r subgroup (the twiddles compose mod r)
template <class E>
LSA_HD XyzzE<E> ecntt_twiddled(const AffE<E> &B, const uint32_t w[8], bool one, XyzzE<E> *T) {
    return one ? ecntt_from_affine(B) : smul_g2(B, w, T);
}
// A: X, Y < 1 (from Jacobian words) or within the accumulator invariants; T: [<4, <4, <2, <2]; -T: Y <= 4 as in smul_g2
template <class E>
LSA_HD void ecntt_combine(const XyzzE<E> &A, const XyzzE<E> &T, XyzzE<E> &sum, XyzzE<E> &diff) {
    sum = g2_add(A, T);
    XyzzE<E> nT = T;
    if (!T.is_inf()) nT.Y = sub_k<4>(E::zero(), T.Y);                  // 4p - Y  [<= 4; tight]
    diff = g2_add(A, nT);
}
LSA_HD XYZZ29x2 ecntt_from_jac(const Jac<Fq2> &p) {
    if (p.Z.is_zero()) return XYZZ29x2::inf();
    const F29x2 z = f29x2_from_mont256(p.Z), zz = sqr<2>(z);
    return {f29x2_from_mont256(p.X), f29x2_from_mont256(p.Y), zz, mul<2>(zz, z)};
}

}  // namespace lsa
