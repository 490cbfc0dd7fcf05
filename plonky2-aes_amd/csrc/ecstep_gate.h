// EcStepGate: one double-and-add step of an ecGFp5 scalar multiplication per row,
//     mid = 2 acc,   out = mid + bit Q,
// in the complete (X:Z:U:T) formulas of ecgfp5.h (Point::add; pdbl and padd_mixed in circuits), written once over an abstract
// field the way poseidon_gate.h is: the quotient-side kernel (base field, per LDE point), the host verifier and the GPU verifier
// (GF(p^2), at zeta) and the witness generator share it.  Wire layout in circuit.h (EG_*); the row's two gate constants are 0.
//
// K = GF(p)[z]/(z^5 - 3), curve constant b = 263 z.  Both halves end in the same tail (ec_tail): with
//     doubling:        t1 = X^2,   t2 = Z^2, t3 = U^2,   t4 = T^2, t5 = 2 X Z,    t6 = 2 U T
//     mixed addition:  t1 = X qx,  t2 = Z,   t3 = U qu,  t4 = T,   t5 = Z qx + X, t6 = T qu + U      (q = bit Q, Z2 = T2 = 1)
//     t7 = b t2 + t1, t8 = t4 t7, w9 = 2 b t5 + 2 t7, Z' = t8 - t3 w9, T' = 2 t8 - Z', d = (2 t3 + t4)(t5 + t7) - t8, X' = b d,
//     U' = t6 (b t2 - t1).
// 10 + 8 = 18 products in K.  Degrees: mid - dbl(acc) is 4 in acc; with q of degree 2, t1 t3 t5 t6 t7 w9 s qq e are 3, t8 is 4,
// Z' T' d X' U' are 6: the gate's degree is 6.  `bit` is not constrained to be boolean here.
#pragma once
#include "circuit.h"
#include "gl.h"
#include "poseidon_gate.h"

namespace p2 {

static const gl::u64 EG_B1 = 263;  // ecgfp5::B1
// every loop here runs over the five coefficients of an element with constant bounds: unrolled in device code, an element is
// five registers and never an indexed array in memory (the host compiler is left to choose: forced, its pass over the
// flattened 18 products takes many minutes)
#if defined(__HIP_DEVICE_COMPILE__)
#define EG_UNROLL _Pragma("unroll")
#else
#define EG_UNROLL
#endif

template <class F>
struct Q5 {
    typename F::T c[5];
};

template <class F>
GL_HD Q5<F> q5_add(const Q5<F>& a, const Q5<F>& b) {
    Q5<F> r;
    EG_UNROLL
    for (int i = 0; i < 5; i++) r.c[i] = F::add(a.c[i], b.c[i]);
    return r;
}
template <class F>
GL_HD Q5<F> q5_sub(const Q5<F>& a, const Q5<F>& b) {
    Q5<F> r;
    EG_UNROLL
    for (int i = 0; i < 5; i++) r.c[i] = F::sub(a.c[i], b.c[i]);
    return r;
}
template <class F>
GL_HD Q5<F> q5_dbl(const Q5<F>& a) {
    return q5_add<F>(a, a);
}
// a * (k z)
template <class F>
GL_HD Q5<F> q5_mul_k1(const Q5<F>& a, gl::u64 k) {
    Q5<F> r;
    r.c[0] = F::mul_base(a.c[4], 3 * k);
    EG_UNROLL
    for (int i = 1; i < 5; i++) r.c[i] = F::mul_base(a.c[i - 1], k);
    return r;
}
// a * s for s in the coefficient field
template <class F>
GL_HD Q5<F> q5_scale(const Q5<F>& a, typename F::T s) {
    Q5<F> r;
    EG_UNROLL
    for (int i = 0; i < 5; i++) r.c[i] = F::mul(a.c[i], s);
    return r;
}
template <class F>
GL_HD Q5<F> q5_mul(const Q5<F>& a, const Q5<F>& b) {
    typedef typename F::T T;
    Q5<F> r;
    EG_UNROLL
    for (int k = 0; k < 5; k++) {
        T lo = F::mul(a.c[0], b.c[k]);
        EG_UNROLL
        for (int i = 1; i <= k; i++) lo = F::add(lo, F::mul(a.c[i], b.c[k - i]));
        if (k < 4) {
            T hi = F::mul(a.c[k + 1], b.c[4]);
            EG_UNROLL
            for (int i = k + 2; i < 5; i++) hi = F::add(hi, F::mul(a.c[i], b.c[k + 5 - i]));
            lo = F::add(lo, F::mul_base(hi, 3));
        }
        r.c[k] = lo;
    }
    return r;
}

template <class F>
struct EcPoint {
    Q5<F> X, Z, U, T;
};

// the shared second half of both formulas (4 products)
template <class F>
GL_HD EcPoint<F> ec_tail(const Q5<F>& t1, const Q5<F>& t2, const Q5<F>& t3, const Q5<F>& t4, const Q5<F>& t5, const Q5<F>& t6) {
    const Q5<F> bt2 = q5_mul_k1<F>(t2, EG_B1);
    const Q5<F> t7 = q5_add<F>(bt2, t1);
    const Q5<F> t8 = q5_mul<F>(t4, t7);
    const Q5<F> w9 = q5_add<F>(q5_mul_k1<F>(t5, 2 * EG_B1), q5_dbl<F>(t7));
    EcPoint<F> r;
    r.Z = q5_sub<F>(t8, q5_mul<F>(t3, w9));
    r.T = q5_sub<F>(q5_dbl<F>(t8), r.Z);
    const Q5<F> d = q5_sub<F>(q5_mul<F>(q5_add<F>(q5_dbl<F>(t3), t4), q5_add<F>(t5, t7)), t8);
    r.X = q5_mul_k1<F>(d, EG_B1);
    r.U = q5_mul<F>(t6, q5_sub<F>(bt2, t1));
    return r;
}
// 2 p (6 products and the tail)
template <class F>
GL_HD EcPoint<F> ec_double(const EcPoint<F>& p) {
    return ec_tail<F>(q5_mul<F>(p.X, p.X), q5_mul<F>(p.Z, p.Z), q5_mul<F>(p.U, p.U), q5_mul<F>(p.T, p.T), q5_dbl<F>(q5_mul<F>(p.X, p.Z)),
                      q5_dbl<F>(q5_mul<F>(p.U, p.T)));
}
// p + (qx, qu) for an affine second operand; complete, so (0, 0) adds nothing (4 products and the tail)
template <class F>
GL_HD EcPoint<F> ec_add_mixed(const EcPoint<F>& p, const Q5<F>& qx, const Q5<F>& qu) {
    return ec_tail<F>(q5_mul<F>(p.X, qx), p.Z, q5_mul<F>(p.U, qu), p.T, q5_add<F>(q5_mul<F>(p.Z, qx), p.X), q5_add<F>(q5_mul<F>(p.T, qu), p.U));
}

template <class F, class WireFn>
GL_HD Q5<F> eg_load(WireFn wire, u32 first) {
    Q5<F> r;
    EG_UNROLL
    for (int i = 0; i < 5; i++) r.c[i] = wire(first + i);
    return r;
}
template <class F, class WireFn>
GL_HD EcPoint<F> eg_load_point(WireFn wire, u32 first) {
    EcPoint<F> p;
    p.X = eg_load<F>(wire, first), p.Z = eg_load<F>(wire, first + 5), p.U = eg_load<F>(wire, first + 10), p.T = eg_load<F>(wire, first + 15);
    return p;
}

// wire(i) -> value of wire i of the row; emit(k, c) receives constraint k = 0..39 in order: 0..19 mid - 2 acc, 20..39
// out - (mid + bit Q), each as X, Z, U, T with five coefficients.  The wires are asked for when they are needed (acc; then mid;
// then Q, bit; then out), so a caller that loads on demand never holds the whole row.
template <class F, class WireFn, class EmitFn>
GL_HD void ecstep_gate_constraints(WireFn wire, EmitFn emit) {
    int k = 0;
    const EcPoint<F> dbl = ec_double<F>(eg_load_point<F>(wire, EG_ACC));
    const EcPoint<F> mid = eg_load_point<F>(wire, EG_MID);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(mid.X.c[i], dbl.X.c[i]));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(mid.Z.c[i], dbl.Z.c[i]));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(mid.U.c[i], dbl.U.c[i]));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(mid.T.c[i], dbl.T.c[i]));
    const typename F::T bit = wire(EG_BIT);
    const EcPoint<F> sum = ec_add_mixed<F>(mid, q5_scale<F>(eg_load<F>(wire, EG_Q), bit), q5_scale<F>(eg_load<F>(wire, EG_Q + 5), bit));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(wire(EG_OUT + i), sum.X.c[i]));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(wire(EG_OUT + 5 + i), sum.Z.c[i]));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(wire(EG_OUT + 10 + i), sum.U.c[i]));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(k++, F::sub(wire(EG_OUT + 15 + i), sum.T.c[i]));
}

// The generator: in(i) -> wires 0..30 of the row (canonical); emit(col, v) receives wires 31..70 in column order.
template <class InFn, class Emit>
GL_HD void ecstep_row_walk(InFn in, Emit emit) {
    typedef FBase F;
    const EcPoint<F> mid = ec_double<F>(eg_load_point<F>(in, EG_ACC));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_MID + i, mid.X.c[i]);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_MID + 5 + i, mid.Z.c[i]);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_MID + 10 + i, mid.U.c[i]);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_MID + 15 + i, mid.T.c[i]);
    const gl::u64 bit = in(EG_BIT);
    const EcPoint<F> out = ec_add_mixed<F>(mid, q5_scale<F>(eg_load<F>(in, EG_Q), bit), q5_scale<F>(eg_load<F>(in, EG_Q + 5), bit));
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_OUT + i, out.X.c[i]);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_OUT + 5 + i, out.Z.c[i]);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_OUT + 10 + i, out.U.c[i]);
    EG_UNROLL
    for (int i = 0; i < 5; i++) emit(EG_OUT + 15 + i, out.T.c[i]);
}
// w[0..30] (acc, Q, bit) are given; fills w[31..70] (mid, out).
GL_HD void ecstep_gate_witness(gl::u64* w) {
    ecstep_row_walk([&](u32 i) { return w[i]; }, [&](u32 col, gl::u64 v) { w[col] = v; });
}

}  // namespace p2
