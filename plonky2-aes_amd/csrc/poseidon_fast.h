// Poseidon-12 for the hashing kernels: same permutation as gl::poseidon (gl.h), restructured for VALU issue slots (the plain
// 30-round form compiles to 41 k VALU instructions per permutation, round 1's restructuring to 28 k, the sparse partial rounds
// that this file used until the block form to 15.5 k, PMC-counted: profiles/r02_valu.json, r03_valu.json):
//   * lazy reduction -- state words are arbitrary u64 representatives (not < p) inside the permutation; every product is
//     reduced once from 128 bits without canonicalisation; outputs are canonicalised;
//   * multiply-reduce built from v_mad_u64_u32 (gl::mulr_add_dev): the mad is a 64-bit adder with a free multiplier and a
//     carry-out, and costs what ONE 32-bit add-with-carry costs (tools/microbench/valu_rates.hip);
//   * round constants are never added on their own: every linear layer starts its accumulators from the constants of the
//     layer that follows;
//   * the 22 partial rounds run in blocks of three (tools/gen_poseidon_fast.py, "block form"): the linear maps between the
//     S-boxes of a block are composed into small-integer matrices (entries below 2^21), so that every term is one
//     v_mad_u64_u32 per 32-bit half, as in a full round's MDS, with no carry counts and one fold per output word; inside a
//     block only row 0, the next S-box's input, is evaluated, and all twelve rows once at its end.  The sparse-matrix form
//     (fewest multiplications, but every constant a 64-bit field element: 8 slots a term, 12 with its reduction) remains
//     for poseidon_coop, where a lane holds one word, and as poseidon_sparse for the verifier's Merkle path walks;
//   * the tree kernels never run the whole of it: permute_known / sponge_permute leave out the S-boxes and MDS terms of words
//     that enter as 0 (the capacity in front of a first chunk, a chunk of known-zero columns) and the last round's MDS rows
//     of outputs the sponge overwrites or never reads;
//   * poseidon_coop: one state over 12 lanes of a 16-lane group, for the sequential Fiat-Shamir chain.
// The host build of the same functions (plain 64-bit arithmetic on the same tables) is what p2_selftest_host and the CPU tests
// exercise.
#pragma once
#include "gl.h"

namespace glf {
using gl::u32;
using gl::u64;

#if defined(__HIP_DEVICE_COMPILE__)
#define P2F_DECL __device__ __constant__ static
#else
#define P2F_DECL static
#endif
#include "poseidon_fast.inc"
P2F_DECL const unsigned long long PF_ZERO12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the addends of the last round's rows

GL_HD void mul128(u64 a, u64 b, u64& hi, u64& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    // 4 x (32x32 + 64 -> 64) = 4 v_mad_u64_u32; every partial sum below provably fits 64 bits
    u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    u64 p00 = (u64)a0 * b0;
    u64 mid = (u64)a0 * b1 + (p00 >> 32);
    u64 mid2 = (u64)a1 * b0 + (u32)mid;
    lo = (mid2 << 32) | (u32)p00;
    hi = (u64)a1 * b1 + (mid >> 32) + (mid2 >> 32);
#else
    unsigned __int128 m = (unsigned __int128)a * b;
    lo = (u64)m;
    hi = (u64)(m >> 64);
#endif
}
// hi*2^64 + lo  ->  some u64 congruent mod p (2^64 = 2^32 - 1, 2^96 = -1; no canonicalisation).
// T = lo + (hl << 32) - (hl + hh) is formed with 32-bit add/subtract-with-carry chains; the number of 2^64 wraps,
// net = carry - borrow in {-1, 0, 1}, is folded back as T - net * p = T - (net << 32) ... + net, again on the halves, so no
// 64-bit compare-and-select is needed: the compiler's version of plonky2's reduce128 spends two of those per reduction
// (v_cmp_lt_u64 + 64-bit add + two v_cndmask, and a v_cndmask on VCC alone costs 23 cycles -- tools/microbench/valu_rates.hip).
// The result T - net * p lies in [0, 2^64) for every input (checked against 128-bit arithmetic on 2*10^8 inputs and all
// combinations of extreme halves).
GL_HD u64 red128(u64 hi, u64 lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    return gl::red128_dev(hi, lo);  // one mad, two subtracts, the wave-uniform correction (gl.h)
#endif
    const u32 l0 = (u32)lo, l1 = (u32)(lo >> 32), hl = (u32)hi, hh = (u32)(hi >> 32);
    u32 C, cv, b, B;
    const u32 u1 = __builtin_addc(l1, hl, 0u, &C);   // lo + (hl << 32): carry C
    const u32 mC = 0u - C;
    const u32 v0 = __builtin_addc(hl, hh, 0u, &cv);  // v = hl + hh, 33 bits
    const u32 w0 = __builtin_subc(l0, v0, 0u, &b);
    u32 w1 = __builtin_subc(u1, cv, b, &B);          // w = u - v: borrow B
    const u32 net = 0u - mC - B;                     // C - B
    w1 += net;                                       // + net * 2^32
    const u32 sx = (u32)((int)net >> 31);
    u32 r0 = __builtin_subc(w0, net, 0u, &b);        // - net (sign-extended)
    u32 r1 = __builtin_subc(w1, sx, b, &B);
#if defined(__HIP_DEVICE_COMPILE__)
    // Value barrier.  ROCm 7.2's AMDGPU backend folds "x - borrow" into a following add-with-carry as "+ 0xFFFFFFFF", which
    // keeps the sum but not the carry-out: a reduction whose result feeds an add-with-carry chain in the same basic block
    // was miscompiled that way (tools/microbench/reduce_check.hip shows it: 4.7 % wrong results when a carry-based
    // canonicalisation follows directly).  The empty asm makes r0, r1 opaque to that combine; it emits nothing.
    asm("" : "+v"(r0), "+v"(r1));
#endif
    return ((u64)r1 << 32) | r0;
}
// a * b mod p as some u64 (a, b arbitrary u64): gl::mulr_add_dev on the device (see gl.h for the sequence).
GL_HD u64 mulr(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return gl::mulr_add_dev<false>(a, b, 0);
#else
    u64 hi, lo;
    mul128(a, b, hi, lo);
    return red128(hi, lo);
#endif
}
GL_HD u64 canon(u64 a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return gl::canon_dev(a);
#else
    return a >= gl::P ? a - gl::P : a;
#endif
}
GL_HD u64 sbox7(u64 x) {
    u64 x2 = mulr(x, x), x3 = mulr(x2, x), x4 = mulr(x2, x2);
    return mulr(x3, x4);
}
// Accumulator for sums of 64x64-bit products (dot products of a sparse/dense matrix row with the state).
// Carries are never propagated between words: each of the four 32x32 partial products is accumulated with one
// v_mad_u64_u32 into its own aligned 64-bit lane (E01: a0*b0, O01: a0*b1 + a1*b0 (weight 2^32), E23: a1*b1 (weight
// 2^64)) and the carry-out of every mad is counted in a 32-bit counter.  8 VALU instructions per term, no moves; the
// four carry SGPR pairs are distinct and each is consumed >= 2 issue slots after it is produced, which is the wait
// gfx950 requires between a VALU SGPR write and its VALU reader (the compiler pads its own carry chains with
// s_nop/v_mov for this reason).  reduce() folds the five words once.
struct Acc {
    u64 e01, o01, e23;
    u32 ce0, co, ce2;
    GL_HD void init() {
        e01 = o01 = e23 = 0;
        ce0 = co = ce2 = 0;
    }
    GL_HD void fma(u64 a, u64 b) {
        u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
        unsigned long long s1, s2, s3, s4;
        asm("v_mad_u64_u32 %[e01], %[s1], %[a0], %[b0], %[e01]\n\t"
            "v_mad_u64_u32 %[o01], %[s2], %[a0], %[b1], %[o01]\n\t"
            "v_mad_u64_u32 %[e23], %[s3], %[a1], %[b1], %[e23]\n\t"
            "v_addc_co_u32_e64 %[ce0], %[s1], 0, %[ce0], %[s1]\n\t"
            "v_mad_u64_u32 %[o01], %[s4], %[a1], %[b0], %[o01]\n\t"
            "v_addc_co_u32_e64 %[co], %[s2], 0, %[co], %[s2]\n\t"
            "v_addc_co_u32_e64 %[ce2], %[s3], 0, %[ce2], %[s3]\n\t"
            "v_addc_co_u32_e64 %[co], %[s4], 0, %[co], %[s4]"
            : [e01] "+v"(e01), [o01] "+v"(o01), [e23] "+v"(e23), [ce0] "+v"(ce0), [co] "+v"(co), [ce2] "+v"(ce2), [s1] "=&s"(s1), [s2] "=&s"(s2),
              [s3] "=&s"(s3), [s4] "=&s"(s4)
            : [a0] "v"(a0), [a1] "v"(a1), [b0] "v"(b0), [b1] "v"(b1));
#else
        u64 p, t;
        p = (u64)a0 * b0; t = e01 + p; ce0 += t < p; e01 = t;
        p = (u64)a0 * b1; t = o01 + p; co += t < p; o01 = t;
        p = (u64)a1 * b1; t = e23 + p; ce2 += t < p; e23 = t;
        p = (u64)a1 * b0; t = o01 + p; co += t < p; o01 = t;
#endif
    }
    // the same with `k` a UNIFORM table constant (PF_E, PF_WHAT rows fetched by scalar loads): its halves are read straight
    // from SGPRs -- every mad here has exactly one scalar source -- instead of being copied into VGPRs first
    GL_HD void fma_k(u64 k, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
        const u32 a0 = (u32)k, a1 = (u32)(k >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
        unsigned long long s1, s2, s3, s4;
        asm("v_mad_u64_u32 %[e01], %[s1], %[a0], %[b0], %[e01]\n\t"
            "v_mad_u64_u32 %[o01], %[s2], %[a0], %[b1], %[o01]\n\t"
            "v_mad_u64_u32 %[e23], %[s3], %[a1], %[b1], %[e23]\n\t"
            "v_addc_co_u32_e64 %[ce0], %[s1], 0, %[ce0], %[s1]\n\t"
            "v_mad_u64_u32 %[o01], %[s4], %[a1], %[b0], %[o01]\n\t"
            "v_addc_co_u32_e64 %[co], %[s2], 0, %[co], %[s2]\n\t"
            "v_addc_co_u32_e64 %[ce2], %[s3], 0, %[ce2], %[s3]\n\t"
            "v_addc_co_u32_e64 %[co], %[s4], 0, %[co], %[s4]"
            : [e01] "+v"(e01), [o01] "+v"(o01), [e23] "+v"(e23), [ce0] "+v"(ce0), [co] "+v"(co), [ce2] "+v"(ce2), [s1] "=&s"(s1), [s2] "=&s"(s2),
              [s3] "=&s"(s3), [s4] "=&s"(s4)
            : [a0] "s"(a0), [a1] "s"(a1), [b0] "v"(b0), [b1] "v"(b1));
#else
        fma(k, b);
#endif
    }
    // a < 2^32: only the two products with a's low half exist
    GL_HD void fma_small(u32 a0, u64 b) {
        u32 b0 = (u32)b, b1 = (u32)(b >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
        unsigned long long s1, s2;
        asm("v_mad_u64_u32 %[e01], %[s1], %[a0], %[b0], %[e01]\n\t"
            "v_mad_u64_u32 %[o01], %[s2], %[a0], %[b1], %[o01]\n\t"
            "s_nop 0\n\t"
            "v_addc_co_u32_e64 %[ce0], %[s1], 0, %[ce0], %[s1]\n\t"
            "v_addc_co_u32_e64 %[co], %[s2], 0, %[co], %[s2]"
            : [e01] "+v"(e01), [o01] "+v"(o01), [ce0] "+v"(ce0), [co] "+v"(co), [s1] "=&s"(s1), [s2] "=&s"(s2)
            : [a0] "v"(a0), [b0] "v"(b0), [b1] "v"(b1));
#else
        u64 p, t;
        p = (u64)a0 * b0; t = e01 + p; ce0 += t < p; e01 = t;
        p = (u64)a0 * b1; t = o01 + p; co += t < p; o01 = t;
#endif
    }
    // value = e01 + 2^32*o01 + 2^64*(e23 + ce0 + 2^32*co) + 2^128*ce2, summed limb by limb with carry chains (no 64-bit
    // compares), then 2^128 = -2^32 (mod p).  Some u64 congruent to the value; not canonical.
    GL_HD u64 reduce() const {
        u32 k1, k2, k2b, k3, k3b, b, b2;
        const u32 L0 = (u32)e01;
        const u32 L1 = __builtin_addc((u32)(e01 >> 32), (u32)o01, 0u, &k1);
        u32 L2 = __builtin_addc((u32)(o01 >> 32), (u32)e23, k1, &k2);
        L2 = __builtin_addc(L2, ce0, 0u, &k2b);
        u32 L3 = __builtin_addc((u32)(e23 >> 32), co, k2, &k3);
        L3 = __builtin_addc(L3, 0u, k2b, &k3b);
        const u32 L4 = ce2 + k3 + k3b;  // multiples of 2^128: tiny
        const u64 r = red128(((u64)L3 << 32) | L2, ((u64)L1 << 32) | L0);
        // r - L4 * 2^32; a borrow is worth -2^64 = -(2^32 - 1)
        const u32 h1 = __builtin_subc((u32)(r >> 32), L4, 0u, &b);
        u32 lo = __builtin_subc((u32)r, 0u - b, 0u, &b2);
        u32 hi = h1 - b2;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("" : "+v"(lo), "+v"(hi));  // value barrier, see red128
#endif
        return ((u64)hi << 32) | lo;
    }
};

// a arbitrary u64, c canonical (< p) -> some u64 congruent to a + c.  The wrap is folded back as + EPS, which cannot
// wrap again (a + c - 2^64 < c <= p - 1).  Carry chains only: a 64-bit compare-and-select costs a v_cmp_*_u64 plus two
// v_cndmask_b32 on VCC, and tools/microbench/valu_rates.hip measures the latter at 23 cycles each on gfx950.
GL_HD u64 add_wrap(u64 a, u64 c) {
    u32 k, K, b, b2;
    const u32 lo = __builtin_addc((u32)a, (u32)c, 0u, &k);
    const u32 hi = __builtin_addc((u32)(a >> 32), (u32)(c >> 32), k, &K);
    // + K * (2^32 - 1):  lo - K, hi + K - borrow
    u32 r0 = __builtin_subc(lo, 0u, K, &b);
    u32 r1 = __builtin_addc(hi, 0u, K, &b2);
    r1 -= b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(r0), "+v"(r1));  // value barrier, see red128
#endif
    return ((u64)r1 << 32) | r0;
}

// value = al + 2^32 * ah with al, ah < 2^57  ->  some u64 congruent to it.  A full round's MDS gives al, ah < 2^43 (at most 13
// products of a 32-bit half with a coefficient < 2^6, plus a 32-bit half of a round constant), the end of a block of three
// partial rounds al, ah < 2^56 (coefficients summing to less than 2^24; the generator proves the bounds used here row by row).
//   ah' = ah + (al >> 32) < 2^58;  value = x0 + 2^32 x1 + 2^64 x2  with x0 = lo32(al), (x1, x2) = halves of ah', x2 < 2^26
//   = {x1:x0} + x2 * (2^32 - 1): ONE v_mad_u64_u32 (the 64-bit add rides on the multiply; a 32-bit add-with-carry costs
//   the same issue time as the whole mad, valu_rates.hip), and its carry-out -- possible only when x1 >= 2^32 - x2 --
//   is folded back by a second mad, which cannot wrap (the wrapped sum is < x2 * 2^32 < 2^58).
// ALWAYS: for al, ah up to 2^64 - 1 with ah + (al >> 32) < 2^64 still (the end rows of a block of four layers, merged_middle: the
// generator proves it per row).  x2 is then any 32-bit value and the first mad wraps on every second lane, so the second step
// runs branch-free on all of them: a 0/1 select on the carry mask and the mad, two wait states behind the mad that wrote the mask
// (as gl::one_where pays them).  It cannot wrap either: the wrapped sum is < x2 (2^32 - 1) <= 2^64 - 2^33 + 1.
template <bool ALWAYS = false>
GL_HD u64 fold_al_ah(u64 al, u64 ah) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u64 ah2 = gl::add_u32(ah, (u32)(al >> 32));  // through the multiplier: no zero-extension of al's high half
#else
    const u64 ah2 = ah + (al >> 32);
#endif
    const u32 x2 = (u32)(ah2 >> 32);
    const u64 base = (ah2 << 32) | (u32)al;
#if defined(__HIP_DEVICE_COMPILE__)
    // the carry needs x1 >= 2^32 - x2: once in 2^20 on random data after a full round and about one lane in 250 at the end of a
    // block of partial rounds (a wave in four), so its fold sits behind a wave-uniform branch
    gl::sg sc, dead;
    if (ALWAYS) {
        u64 r = base;   // in place: the 0/1 select lands in x2's register, which the first mad has consumed
        u32 c01 = x2;
        asm("v_mad_u64_u32 %[r], %[sc], %[c], -1, %[r]\n\t"
            "s_nop 1\n\t"
            "v_cndmask_b32_e64 %[c], 0, 1, %[sc]\n\t"
            "v_mad_u64_u32 %[r], %[d], %[c], -1, %[r]"
            : [r] "+v"(r), [c] "+v"(c01), [sc] "=&s"(sc), [d] "=&s"(dead));
        return r;
    }
    u64 r = gl::mad_eps_co(x2, base, sc);
    if (__builtin_expect(sc != 0, 0)) r = gl::mad_eps_co(gl::one_where(sc), r, dead);
    return r;
#else
    const u64 t = base + (u64)x2 * gl::EPS;
    return t < base ? t + gl::EPS : t;
#endif
}

// MDS layer of a full round, with the NEXT round's constants folded into the accumulators (rc == nullptr: none):
//   out[r] = rc[r] + sum_i circ[i] * s[(i + r) % 12] + 8 * s[0] (r == 0)      as some u64 representative.
// Evaluated on 32-bit halves: every accumulator stays below 2^43, one fold per output word.
// Only the rows whose bit is set in `rows` are evaluated; the other words keep their input (nobody reads them: last_round).
GL_HD void mds_full(u64* s, const unsigned long long* rc, const u32 rows = 0xFFF) {
#if defined(__HIP_DEVICE_COMPILE__)
    // Every term is one v_mad_u64_u32 with the coefficient as an inline constant (gl::madk: the coefficients 2, 8 and 16 must
    // not become shift-adds on zero-extended operands), and the round constant is the ADDEND of the first one, read from its
    // SGPR pair: no separate additions, no moves.
    u32 l[12], h[12];
    u64 res[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        l[i] = (u32)s[i];
        h[i] = (u32)(s[i] >> 32);
    }
    // One asm block per output word: 24 (26) mads on two accumulators.  As separate statements each mad is followed by the
    // compiler's boundary pad (it defines an SGPR pair, the unused carry-out, and the compiler cannot see that nobody reads
    // it): 2 500 s_nop per permutation.  29 operands -- the limit is 30.  (The macros serve mds_row0 as well.)
#define P2_MDS_T(n, K) "v_mad_u64_u32 %[al], %[d], %[l" #n "], " #K ", %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h" #n "], " #K ", %[ah]\n\t"
#define P2_MDS_TAIL P2_MDS_T(1, 15) P2_MDS_T(2, 41) P2_MDS_T(3, 16) P2_MDS_T(4, 2) P2_MDS_T(5, 28) P2_MDS_T(6, 13) P2_MDS_T(7, 13) \
                    P2_MDS_T(8, 39) P2_MDS_T(9, 18) P2_MDS_T(10, 34) P2_MDS_T(11, 20)
#define P2_MDS_IN(r)                                                                                                                          \
    [l0] "v"(l[(0 + r) % 12]), [h0] "v"(h[(0 + r) % 12]), [l1] "v"(l[(1 + r) % 12]), [h1] "v"(h[(1 + r) % 12]), [l2] "v"(l[(2 + r) % 12]),     \
        [h2] "v"(h[(2 + r) % 12]), [l3] "v"(l[(3 + r) % 12]), [h3] "v"(h[(3 + r) % 12]), [l4] "v"(l[(4 + r) % 12]), [h4] "v"(h[(4 + r) % 12]), \
        [l5] "v"(l[(5 + r) % 12]), [h5] "v"(h[(5 + r) % 12]), [l6] "v"(l[(6 + r) % 12]), [h6] "v"(h[(6 + r) % 12]), [l7] "v"(l[(7 + r) % 12]), \
        [h7] "v"(h[(7 + r) % 12]), [l8] "v"(l[(8 + r) % 12]), [h8] "v"(h[(8 + r) % 12]), [l9] "v"(l[(9 + r) % 12]), [h9] "v"(h[(9 + r) % 12]), \
        [l10] "v"(l[(10 + r) % 12]), [h10] "v"(h[(10 + r) % 12]), [l11] "v"(l[(11 + r) % 12]), [h11] "v"(h[(11 + r) % 12])
#pragma unroll
    for (int r = 0; r < 12; r++) {
        res[r] = s[r];
        if (!((rows >> r) & 1)) continue;
        u64 al, ah;
        gl::sg dead;
        if (rc) {
            const u64 rl = (u64)(u32)rc[r], rh = (u64)(rc[r] >> 32);
            if (r == 0)
                asm("v_mad_u64_u32 %[al], %[d], %[l0], 17, %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 17, %[rh]\n\t" P2_MDS_TAIL
                    "v_mad_u64_u32 %[al], %[d], %[l0], 8, %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 8, %[ah]"
                    : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
                    : [rl] "s"(rl), [rh] "s"(rh), P2_MDS_IN(r));
            else
                asm("v_mad_u64_u32 %[al], %[d], %[l0], 17, %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 17, %[rh]\n\t" P2_MDS_TAIL
                    : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
                    : [rl] "s"(rl), [rh] "s"(rh), P2_MDS_IN(r));
        } else {
            if (r == 0)
                asm("v_mad_u64_u32 %[al], %[d], %[l0], 17, 0\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 17, 0\n\t" P2_MDS_TAIL
                    "v_mad_u64_u32 %[al], %[d], %[l0], 8, %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 8, %[ah]"
                    : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
                    : P2_MDS_IN(r));
            else
                asm("v_mad_u64_u32 %[al], %[d], %[l0], 17, 0\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 17, 0\n\t" P2_MDS_TAIL
                    : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
                    : P2_MDS_IN(r));
        }
        res[r] = fold_al_ah(al, ah);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = res[i];
    return;
#endif
    const u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    u64 lo[12], hi[12], out[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        lo[i] = s[i] & gl::EPS;
        hi[i] = s[i] >> 32;
    }
#pragma unroll
    for (int r = 0; r < 12; r++) {
        out[r] = s[r];
        if (!((rows >> r) & 1)) continue;
        u64 al = rc ? (u64)(u32)rc[r] : 0, ah = rc ? (u64)(rc[r] >> 32) : 0;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            int j = (i + r) % 12;
            al += lo[j] * C[i];
            ah += hi[j] * C[i];
        }
        if (r == 0) {
            al += lo[0] * 8;
            ah += hi[0] * 8;
        }
        out[r] = fold_al_ah(al, ah);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = out[i];
}

// Row 0 of the MDS alone: rc + sum_i circ[i] * s[i] + 8 * s[0]
GL_HD u64 mds_row0(const u64* s, u64 rc) {
#if defined(__HIP_DEVICE_COMPILE__)
    {
        u32 l[12], h[12];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            l[i] = (u32)s[i];
            h[i] = (u32)(s[i] >> 32);
        }
        const u64 rl = (u64)(u32)rc, rh = rc >> 32;
        u64 al, ah;
        gl::sg dead;
        asm("v_mad_u64_u32 %[al], %[d], %[l0], 17, %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 17, %[rh]\n\t" P2_MDS_TAIL
            "v_mad_u64_u32 %[al], %[d], %[l0], 8, %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], 8, %[ah]"
            : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
            : [rl] "s"(rl), [rh] "s"(rh), P2_MDS_IN(0));
        return fold_al_ah(al, ah);
    }
#endif
    const u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    u64 al = (u32)rc, ah = rc >> 32;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        al += (s[i] & gl::EPS) * C[i];
        ah += (s[i] >> 32) * C[i];
    }
    al += (s[0] & gl::EPS) * 8;
    ah += (s[0] >> 32) * 8;
    return fold_al_ah(al, ah);
}
#if defined(__HIP_DEVICE_COMPILE__)
#undef P2_MDS_T
#undef P2_MDS_TAIL
#undef P2_MDS_IN
#endif

// One full round on a state that already carries this round's constants: S-box, then MDS + next constants.
GL_HD void full_round(u64* s, const unsigned long long* rc_next) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = sbox7(s[i]);
    mds_full(s, rc_next);
}

// a * b + c mod p as some u64 (a, b, c arbitrary u64): the addend rides on the multiply-adds (gl.h)
GL_HD u64 mulr_add(u64 a, u64 b, u64 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return gl::mulr_add_dev<true>(a, b, c);
#else
    unsigned __int128 m = (unsigned __int128)a * b + c;
    return red128((u64)(m >> 64), (u64)m);
#endif
}

// the same with a uniform table constant as the first factor
GL_HD u64 mulr_add_k(u64 k, u64 b, u64 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return gl::mulr_add_dev<true, true>(k, b, c);
#else
    return mulr_add(k, b, c);
#endif
}

// ---- The permutation in three parts.  A sponge never needs all of it: the capacity words 8..11 are 0 in front of the first
// permutation of every hash, an absorbed chunk of known-zero columns puts 0 into the rate words 0..7, and of the twelve outputs
// only the words that the next chunk does not overwrite (or the digest words 0..3) are read.
//   first_round    + constants, S-box, MDS, with the words known to be 0 left out: such a word leaves the S-box as the constant
//                  RC[k]^7, and its MDS terms are part of the row's addend (RC1_ZCAP / RC1_ZRATE, tools/gen_poseidon_fast.py);
//   middle         full rounds 1..3, the 22 partial rounds, full rounds 26..28;
//   last_round     S-box, then only the MDS rows somebody reads, canonicalised.
// `kind` and `rows` are compile-time constants (first_round<KIND>, last_round<ROWS>) or WAVE-UNIFORM run-time values (the leaf
// kernels, whose chunks differ): then every group of terms sits behind a scalar branch and there is still one copy of each.
enum : u32 { FR_GENERAL = 0, FR_ZERO_CAP = 1, FR_ZERO_RATE = 2 };           // which words enter as 0: none, 8..11, 0..7
enum : u32 { ROWS_ALL = 0xFFF, ROWS_DIGEST = 0x00F, ROWS_CAPACITY = 0xF00 };  // bit r = output word r is read

// The output words a sponge still needs when the NEXT chunk overwrites words 0..m-1 (overwrite mode, hash_n_to_hash_no_pad):
// no next chunk (m <= 0): the digest; a full chunk: the capacity; a partial one: the rate words it leaves, and the capacity.
GL_HD constexpr u32 rows_before_chunk(int m) { return m <= 0 ? 0x00Fu : m >= 8 ? 0xF00u : (0xFFFu & ~((1u << m) - 1u)); }

// coefficient of state word j in MDS row r (circulant + the diagonal 8 at (0, 0)); at most 25: an inline constant
GL_HD constexpr u32 mds_coef(int r, int j) {
    constexpr u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    return C[(j - r + 12) % 12] + ((r == 0 && j == 0) ? 8u : 0u);
}

#if defined(__HIP_DEVICE_COMPILE__)
// MDS row R split at the rate / capacity boundary, the per-term form of mds_full's blocks: the terms of words 0..7 on a
// uniform addend (SGPR pairs), and the terms of words 8..11 on top of running accumulators.
#define P2_FR_T(n) "v_mad_u64_u32 %[al], %[d], %[l" #n "], %[k" #n "], %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h" #n "], %[k" #n "], %[ah]\n\t"
template <int R>
GL_D void mds_rate_terms(u64& al, u64& ah, const u32* l, const u32* h, u64 rl, u64 rh) {
    gl::sg dead;
    asm("v_mad_u64_u32 %[al], %[d], %[l0], %[k0], %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[h0], %[k0], %[rh]\n\t"  //
        P2_FR_T(1) P2_FR_T(2) P2_FR_T(3) P2_FR_T(4) P2_FR_T(5) P2_FR_T(6) "v_mad_u64_u32 %[al], %[d], %[l7], %[k7], %[al]\n\t"
        "v_mad_u64_u32 %[ah], %[d], %[h7], %[k7], %[ah]"
        : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
        : [rl] "s"(rl), [rh] "s"(rh), [l0] "v"(l[0]), [h0] "v"(h[0]), [l1] "v"(l[1]), [h1] "v"(h[1]), [l2] "v"(l[2]), [h2] "v"(h[2]),
          [l3] "v"(l[3]), [h3] "v"(h[3]), [l4] "v"(l[4]), [h4] "v"(h[4]), [l5] "v"(l[5]), [h5] "v"(h[5]), [l6] "v"(l[6]), [h6] "v"(h[6]),
          [l7] "v"(l[7]), [h7] "v"(h[7]), [k0] "n"(mds_coef(R, 0)), [k1] "n"(mds_coef(R, 1)), [k2] "n"(mds_coef(R, 2)),
          [k3] "n"(mds_coef(R, 3)), [k4] "n"(mds_coef(R, 4)), [k5] "n"(mds_coef(R, 5)), [k6] "n"(mds_coef(R, 6)), [k7] "n"(mds_coef(R, 7)));
}
// ADDEND: the capacity terms open the row (a zero rate) and start from the addend themselves
template <int R, bool ADDEND>
GL_D void mds_cap_terms(u64& al, u64& ah, const u32* l, const u32* h, u64 rl, u64 rh) {
    gl::sg dead;
#define P2_FR_CAP_IN                                                                                                                      \
    [l8] "v"(l[8]), [h8] "v"(h[8]), [l9] "v"(l[9]), [h9] "v"(h[9]), [l10] "v"(l[10]), [h10] "v"(h[10]), [l11] "v"(l[11]), [h11] "v"(h[11]), \
        [k8] "n"(mds_coef(R, 8)), [k9] "n"(mds_coef(R, 9)), [k10] "n"(mds_coef(R, 10)), [k11] "n"(mds_coef(R, 11))
    if (ADDEND)
        asm("v_mad_u64_u32 %[al], %[d], %[l8], %[k8], %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[h8], %[k8], %[rh]\n\t"  //
            P2_FR_T(9) P2_FR_T(10) "v_mad_u64_u32 %[al], %[d], %[l11], %[k11], %[al]\n\t"
            "v_mad_u64_u32 %[ah], %[d], %[h11], %[k11], %[ah]"
            : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
            : [rl] "s"(rl), [rh] "s"(rh), P2_FR_CAP_IN);
    else
        asm(P2_FR_T(8) P2_FR_T(9) P2_FR_T(10) "v_mad_u64_u32 %[al], %[d], %[l11], %[k11], %[al]\n\t"
            "v_mad_u64_u32 %[ah], %[d], %[h11], %[k11], %[ah]"
            : [al] "+v"(al), [ah] "+v"(ah), [d] "=&s"(dead)
            : P2_FR_CAP_IN);
#undef P2_FR_CAP_IN
}
#undef P2_FR_T
template <int R>
GL_D u64 first_round_row(const u32 kind, const u32* l, const u32* h, const u64 add) {  // kind != FR_ZERO_RATE
    u64 al, ah;
    mds_rate_terms<R>(al, ah, l, h, (u64)(u32)add, add >> 32);
    if (kind != FR_ZERO_CAP) mds_cap_terms<R, false>(al, ah, l, h, 0, 0);
    return fold_al_ah(al, ah);
}
template <int R>
GL_D u64 zero_rate_row(const u32* l, const u32* h, const u64 add) {
    u64 al, ah;
    mds_cap_terms<R, true>(al, ah, l, h, (u64)(u32)add, add >> 32);
    return fold_al_ah(al, ah);
}
#endif

// One full round with the words that `kind` (FR_*) declares zero left out; they are not read.  In two stages, because round 3
// runs the first alone (its MDS is the first layer of merged_middle):
//   sbox_layer_known    pre: the constants the S-box inputs still lack (the first round) or nullptr (the state carries them);
//   linear_layer_known  add: the addend of every MDS row.
GL_HD void sbox_layer_known(u64* s, const u32 kind, const unsigned long long* pre) {
#if defined(__HIP_DEVICE_COMPILE__)
    // A zero rate is a region of its own in both stages (four S-boxes, twelve rows of eight terms) and not a third arm of every
    // row below: with three arms per row the register allocator needed 22 more VGPRs in k_hash_leaves and spilled.
    if (kind == FR_ZERO_RATE) {
#pragma unroll
        for (int i = 8; i < 12; i++) s[i] = sbox7(pre ? add_wrap(s[i], pre[i]) : s[i]);
        return;
    }
    if (pre) {
#pragma unroll
        for (int i = 0; i < 8; i++) s[i] = add_wrap(s[i], pre[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = sbox7(s[i]);
    if (kind != FR_ZERO_CAP) {
        if (pre) {
#pragma unroll
            for (int i = 8; i < 12; i++) s[i] = add_wrap(s[i], pre[i]);
        }
#pragma unroll
        for (int i = 8; i < 12; i++) s[i] = sbox7(s[i]);
    }
#else
    const int j0 = kind == FR_ZERO_RATE ? 8 : 0, j1 = kind == FR_ZERO_CAP ? 8 : 12;
    for (int j = j0; j < j1; j++) s[j] = sbox7(pre ? add_wrap(s[j], pre[j]) : s[j]);
#endif
}
GL_HD void linear_layer_known(u64* s, const u32 kind, const unsigned long long* add) {
#if defined(__HIP_DEVICE_COMPILE__)
    u32 l[12], h[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        l[i] = (u32)s[i];
        h[i] = (u32)(s[i] >> 32);
    }
    if (kind == FR_ZERO_RATE) {
#define P2_FR_ROW(r) s[r] = zero_rate_row<r>(l, h, add[r]);
        P2_FR_ROW(0) P2_FR_ROW(1) P2_FR_ROW(2) P2_FR_ROW(3) P2_FR_ROW(4) P2_FR_ROW(5) P2_FR_ROW(6) P2_FR_ROW(7) P2_FR_ROW(8) P2_FR_ROW(9)
        P2_FR_ROW(10) P2_FR_ROW(11)
#undef P2_FR_ROW
        return;
    }
#define P2_FR_ROW(r) s[r] = first_round_row<r>(kind, l, h, add[r]);
    P2_FR_ROW(0) P2_FR_ROW(1) P2_FR_ROW(2) P2_FR_ROW(3) P2_FR_ROW(4) P2_FR_ROW(5) P2_FR_ROW(6) P2_FR_ROW(7) P2_FR_ROW(8) P2_FR_ROW(9)
    P2_FR_ROW(10) P2_FR_ROW(11)
#undef P2_FR_ROW
#else
    const int j0 = kind == FR_ZERO_RATE ? 8 : 0, j1 = kind == FR_ZERO_CAP ? 8 : 12;
    u64 out[12];
    for (int r = 0; r < 12; r++) {
        u64 al = (u32)add[r], ah = add[r] >> 32;
        for (int j = j0; j < j1; j++) {
            al += (s[j] & gl::EPS) * mds_coef(r, j);
            ah += (s[j] >> 32) * mds_coef(r, j);
        }
        out[r] = fold_al_ah(al, ah);
    }
    for (int i = 0; i < 12; i++) s[i] = out[i];
#endif
}
GL_HD void full_round_known(u64* s, const u32 kind, const unsigned long long* pre, const unsigned long long* add) {
    sbox_layer_known(s, kind, pre);
    linear_layer_known(s, kind, add);
}
GL_HD const unsigned long long* poseidon_rc() {
#if defined(__HIP_DEVICE_COMPILE__)
    return (const unsigned long long*)gl::D_POSEIDON_RC;
#else
    return (const unsigned long long*)gl::H_POSEIDON_RC;
#endif
}
// Out: the state in front of the second round's S-boxes.
GL_HD void first_round_any(u64* s, const u32 kind) {
    full_round_known(s, kind, poseidon_rc(), kind == FR_ZERO_CAP ? RC1_ZCAP : kind == FR_ZERO_RATE ? RC1_ZRATE : poseidon_rc() + 12);
}
template <u32 KIND>
GL_HD void first_round(u64* s) {
    static_assert(KIND <= FR_ZERO_RATE, "FR_GENERAL, FR_ZERO_CAP or FR_ZERO_RATE");
    first_round_any(s, KIND);
}

// ---- The 22 partial rounds, in blocks of three (and one round left over), on a state that carries round 4's constants; out:
// the state carries round 26's.  With y = (s_0^7, s_1, .., s_11), the state in front of a block's linear maps, and t_1, t_2 the
// outputs of its second and third S-box (tools/gen_poseidon_fast.py has the derivation and proves the accumulator bounds):
//   input of the second S-box   M[0] . y + K1                                       mds_row0: inline coefficients
//   input of the third          PB_ROW0_D2 . y + 25 t_1 + K2                        block_row0_d2
//   the block's end, row r      PB_END[r][1..] . y + PB_END[r][0] t_1 + M[r][0] t_2 + K[r]     block_end
// Every term is one v_mad_u64_u32 per half: the half in a VGPR, the coefficient in an SGPR (scalar loads) or, where it is an
// MDS entry, an inline constant.  A VOP3 instruction reads one SGPR operand, so a row cannot start from its K in the mad of a
// term whose coefficient is in an SGPR: the term with the inline coefficient opens the row and carries K as its addend.
// The block of one round (the last: 22 = 7 * 3 + 1) is the same end stage on the table of M itself with t_1 = t_2 = 0.
#if defined(__HIP_DEVICE_COMPILE__)
#define P2_PB_T(n) "v_mad_u64_u32 %[al], %[d], %[l" #n "], %[k" #n "], %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h" #n "], %[k" #n "], %[ah]\n\t"
#define P2_PB_LAST(n) "v_mad_u64_u32 %[al], %[d], %[l" #n "], %[k" #n "], %[al]\n\tv_mad_u64_u32 %[ah], %[d], %[h" #n "], %[k" #n "], %[ah]"
#define P2_PB_IN(n) [l##n] "v"(l[n]), [h##n] "v"(h[n]), [k##n] "s"(c[n])
// Asm statements take 30 operands, a row of fourteen terms needs 45: two statements a row (29 + 21 operands, 25 + 21).
GL_D u64 block_row0_d2(const u32* l, const u32* h, const u64 t1, const unsigned int* c, const u64 k) {
    const u64 rl = (u64)(u32)k, rh = k >> 32;
    u64 al, ah;
    gl::sg dead;
    asm("v_mad_u64_u32 %[al], %[d], %[lt], 25, %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[ht], 25, %[rh]\n\t"  //
        P2_PB_T(0) P2_PB_T(1) P2_PB_T(2) P2_PB_T(3) P2_PB_T(4) P2_PB_LAST(5)
        : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
        : [rl] "s"(rl), [rh] "s"(rh), [lt] "v"((u32)t1), [ht] "v"((u32)(t1 >> 32)), P2_PB_IN(0), P2_PB_IN(1), P2_PB_IN(2), P2_PB_IN(3),
          P2_PB_IN(4), P2_PB_IN(5));
    asm(P2_PB_T(6) P2_PB_T(7) P2_PB_T(8) P2_PB_T(9) P2_PB_T(10) P2_PB_LAST(11)
        : [al] "+v"(al), [ah] "+v"(ah), [d] "=&s"(dead)
        : P2_PB_IN(6), P2_PB_IN(7), P2_PB_IN(8), P2_PB_IN(9), P2_PB_IN(10), P2_PB_IN(11));
    return fold_al_ah(al, ah);
}
template <int R>
GL_D u64 block_end_row(const u32* l, const u32* h, const u64 t1, const u64 t2, const unsigned int* e, const u64 k) {
    const u64 rl = (u64)(u32)k, rh = k >> 32;
    const unsigned int* c = e + 1;
    u64 al, ah;
    gl::sg dead;
    asm("v_mad_u64_u32 %[al], %[d], %[lu], %[ku], %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[hu], %[ku], %[rh]\n\t"  //
        P2_PB_T(t) P2_PB_T(0) P2_PB_T(1) P2_PB_T(2) P2_PB_T(3) P2_PB_T(4) P2_PB_LAST(5)
        : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
        : [rl] "s"(rl), [rh] "s"(rh), [lu] "v"((u32)t2), [hu] "v"((u32)(t2 >> 32)), [ku] "n"(mds_coef(R, 0)), [lt] "v"((u32)t1),
          [ht] "v"((u32)(t1 >> 32)), [kt] "s"(e[0]), P2_PB_IN(0), P2_PB_IN(1), P2_PB_IN(2), P2_PB_IN(3), P2_PB_IN(4), P2_PB_IN(5));
    asm(P2_PB_T(6) P2_PB_T(7) P2_PB_T(8) P2_PB_T(9) P2_PB_T(10) P2_PB_LAST(11)
        : [al] "+v"(al), [ah] "+v"(ah), [d] "=&s"(dead)
        : P2_PB_IN(6), P2_PB_IN(7), P2_PB_IN(8), P2_PB_IN(9), P2_PB_IN(10), P2_PB_IN(11));
    return fold_al_ah(al, ah);
}
// The rows merged_middle adds (below): row 0 at depth 3 (fourteen terms: 29 + 21 operands) and an end row of up to four layers
// (fifteen terms: 29 + 24).  e: the row's table entries, the coefficients of the earlier t first.
static_assert((PM_ALWAYS_ROW0 & 3) == 0, "mds_row0 and block_row0_d2 fold with the rare-carry branch");
GL_D u64 merged_row0_d3(const u32* l, const u32* h, const u64 t1, const u64 t2, const unsigned int* e, const u64 k) {
    const u64 rl = (u64)(u32)k, rh = k >> 32;
    const unsigned int* c = e + 1;
    u64 al, ah;
    gl::sg dead;
    asm("v_mad_u64_u32 %[al], %[d], %[lu], 25, %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[hu], 25, %[rh]\n\t"  //
        P2_PB_T(t) P2_PB_T(0) P2_PB_T(1) P2_PB_T(2) P2_PB_T(3) P2_PB_T(4) P2_PB_LAST(5)
        : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
        : [rl] "s"(rl), [rh] "s"(rh), [lu] "v"((u32)t2), [hu] "v"((u32)(t2 >> 32)), [lt] "v"((u32)t1), [ht] "v"((u32)(t1 >> 32)),
          [kt] "s"(e[0]), P2_PB_IN(0), P2_PB_IN(1), P2_PB_IN(2), P2_PB_IN(3), P2_PB_IN(4), P2_PB_IN(5));
    asm(P2_PB_T(6) P2_PB_T(7) P2_PB_T(8) P2_PB_T(9) P2_PB_T(10) P2_PB_LAST(11)
        : [al] "+v"(al), [ah] "+v"(ah), [d] "=&s"(dead)
        : P2_PB_IN(6), P2_PB_IN(7), P2_PB_IN(8), P2_PB_IN(9), P2_PB_IN(10), P2_PB_IN(11));
    return fold_al_ah<((PM_ALWAYS_ROW0 >> 2) & 1) != 0>(al, ah);
}
template <int R>
GL_D u64 merged_end_row(const u32* l, const u32* h, const u64 t1, const u64 t2, const u64 t3, const unsigned int* e, const u64 k) {
    const u64 rl = (u64)(u32)k, rh = k >> 32;
    const unsigned int* c = e + 2;
    u64 al, ah;
    gl::sg dead;
    asm("v_mad_u64_u32 %[al], %[d], %[lu], %[ku], %[rl]\n\tv_mad_u64_u32 %[ah], %[d], %[hu], %[ku], %[rh]\n\t"  //
        P2_PB_T(t) P2_PB_T(v) P2_PB_T(0) P2_PB_T(1) P2_PB_T(2) P2_PB_T(3) P2_PB_LAST(4)
        : [al] "=&v"(al), [ah] "=&v"(ah), [d] "=&s"(dead)
        : [rl] "s"(rl), [rh] "s"(rh), [lu] "v"((u32)t3), [hu] "v"((u32)(t3 >> 32)), [ku] "n"(mds_coef(R, 0)), [lt] "v"((u32)t1),
          [ht] "v"((u32)(t1 >> 32)), [kt] "s"(e[0]), [lv] "v"((u32)t2), [hv] "v"((u32)(t2 >> 32)), [kv] "s"(e[1]), P2_PB_IN(0), P2_PB_IN(1),
          P2_PB_IN(2), P2_PB_IN(3), P2_PB_IN(4));
    asm(P2_PB_T(5) P2_PB_T(6) P2_PB_T(7) P2_PB_T(8) P2_PB_T(9) P2_PB_T(10) P2_PB_LAST(11)
        : [al] "+v"(al), [ah] "+v"(ah), [d] "=&s"(dead)
        : P2_PB_IN(5), P2_PB_IN(6), P2_PB_IN(7), P2_PB_IN(8), P2_PB_IN(9), P2_PB_IN(10), P2_PB_IN(11));
    // one copy of the row serves both depths: the second step runs always if either table's row needs it
    return fold_al_ah<(((PM_ALWAYS_END4 | PM_ALWAYS_END3) >> R) & 1) != 0>(al, ah);
}
#undef P2_PB_T
#undef P2_PB_LAST
#undef P2_PB_IN
#else
// one row on the host: k + c . y (+ ct1 t_1 + ct2 t_2) on halves, in 64-bit accumulators, as the device forms it
GL_HD u64 block_row(const u64* y, const unsigned int* c, const u64 t1, const u32 ct1, const u64 t2, const u32 ct2, const u64 k) {
    u64 al = (u64)(u32)k + (t1 & gl::EPS) * ct1 + (t2 & gl::EPS) * ct2, ah = (k >> 32) + (t1 >> 32) * ct1 + (t2 >> 32) * ct2;
    for (int j = 0; j < 12; j++) {
        al += (y[j] & gl::EPS) * c[j];
        ah += (y[j] >> 32) * c[j];
    }
    return fold_al_ah(al, ah);
}
// the same with a third t: the rows of merged_middle
GL_HD u64 merged_row(const u64* y, const unsigned int* c, const u64 t1, const u32 ct1, const u64 t2, const u32 ct2, const u64 t3, const u32 ct3,
                     const u64 k) {
    u64 al = (u64)(u32)k + (t1 & gl::EPS) * ct1 + (t2 & gl::EPS) * ct2 + (t3 & gl::EPS) * ct3;
    u64 ah = (k >> 32) + (t1 >> 32) * ct1 + (t2 >> 32) * ct2 + (t3 >> 32) * ct3;
    for (int j = 0; j < 12; j++) {
        al += (y[j] & gl::EPS) * c[j];
        ah += (y[j] >> 32) * c[j];
    }
    return fold_al_ah<true>(al, ah);   // on the host both forms of the fold are the same compare
}
#endif
// s = the twelve rows of a block's end; e: the block's table (PB_END or its second half), k: its twelve constants
GL_HD void block_end(u64* s, const u64 t1, const u64 t2, const unsigned int* e, const unsigned long long* k) {
    u64 res[12];
#if defined(__HIP_DEVICE_COMPILE__)
    u32 l[12], h[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        l[i] = (u32)s[i];
        h[i] = (u32)(s[i] >> 32);
    }
#define P2_PB_ROW(r) res[r] = block_end_row<r>(l, h, t1, t2, e + 13 * r, k[r]);
    P2_PB_ROW(0) P2_PB_ROW(1) P2_PB_ROW(2) P2_PB_ROW(3) P2_PB_ROW(4) P2_PB_ROW(5) P2_PB_ROW(6) P2_PB_ROW(7) P2_PB_ROW(8) P2_PB_ROW(9)
    P2_PB_ROW(10) P2_PB_ROW(11)
#undef P2_PB_ROW
#else
    for (int r = 0; r < 12; r++) res[r] = block_row(s, e + 13 * r + 1, t1, e[13 * r], t2, mds_coef(r, 0), k[r]);
#endif
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = res[i];
}
// ONE copy of the block body per kernel: a rolled loop whose last trip skips the two inner S-boxes and reads M's own table.
GL_HD void partial_block(u64* s) {
#pragma nounroll
    for (int b = 0; b < 8; b++) {
        const unsigned long long* K = PB_K + 14 * b;
        const bool three = b < 7;
        s[0] = sbox7(s[0]);
        u64 t1 = 0, t2 = 0;
        if (three) {
            t1 = sbox7(mds_row0(s, K[0]));
#if defined(__HIP_DEVICE_COMPILE__)
            u32 l[12], h[12];
#pragma unroll
            for (int i = 0; i < 12; i++) {
                l[i] = (u32)s[i];
                h[i] = (u32)(s[i] >> 32);
            }
            t2 = sbox7(block_row0_d2(l, h, t1, PB_ROW0_D2, K[1]));
#else
            t2 = sbox7(block_row(s, PB_ROW0_D2, t1, mds_coef(0, 0), 0, 0, K[1]));
#endif
        }
        block_end(s, t1, t2, PB_END + (three ? 0 : 12 * 13), K + 2);
    }
}

// ---- The merged middle: round 3's MDS and the 22 partial rounds as ONE chain of 23 linear layers, M after round 3's S-boxes and
// then [S-box on word 0, M] x 22, in five blocks of four layers and one of three (PM_DEPTH).  Round 3's MDS on its own was twelve
// rows that fed one S-box and more linear maps; as the first layer of the first block it costs that block one more column of
// coefficients.  In: round 3's twelve S-box outputs (any u64); out: the state carries round 26's constants.  A block of four:
//   t_1 = S(M[0] . y + K1)   t_2 = S(PB_ROW0_D2 . y + 25 t_1 + K2)   t_3 = S(PM_ROW0_D3[1..] . y + PM_ROW0_D3[0] t_1 + 25 t_2 + K3)
//   end, row r               PM_END[r][2..] . y + PM_END[r][0] t_1 + PM_END[r][1] t_2 + M[r][0] t_3 + K[r]
// with y = (s_0^7, s_1, .., s_11), and y = s in the first block: round 3's S-box layer has run.  The coefficients at depth four
// reach 2^28.3 and a row's sum 2^31.8, so the half-accumulators come close to 2^64 and the end rows fold with the always-on
// second step (fold_al_ah<true>; tools/gen_poseidon_fast.py proves the bounds per row and emits PM_ALWAYS_*).
// ONE rolled copy of the body: the trip of depth three skips the third stage (t_3 = 0) and reads the second end table, in which
// the slot of t_2, its last real t, holds M[r][0].
GL_HD void merged_end(u64* s, const u64 t1, const u64 t2, const u64 t3, const unsigned int* e, const unsigned long long* k) {
    u64 res[12];
#if defined(__HIP_DEVICE_COMPILE__)
    u32 l[12], h[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        l[i] = (u32)s[i];
        h[i] = (u32)(s[i] >> 32);
    }
#define P2_PM_ROW(r) res[r] = merged_end_row<r>(l, h, t1, t2, t3, e + 14 * r, k[r]);
    P2_PM_ROW(0) P2_PM_ROW(1) P2_PM_ROW(2) P2_PM_ROW(3) P2_PM_ROW(4) P2_PM_ROW(5) P2_PM_ROW(6) P2_PM_ROW(7) P2_PM_ROW(8) P2_PM_ROW(9)
    P2_PM_ROW(10) P2_PM_ROW(11)
#undef P2_PM_ROW
#else
    for (int r = 0; r < 12; r++) res[r] = merged_row(s, e + 14 * r + 2, t1, e[14 * r], t2, e[14 * r + 1], t3, mds_coef(r, 0), k[r]);
#endif
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = res[i];
}
GL_HD void merged_middle(u64* s) {
#pragma nounroll
    for (int b = 0; b < 6; b++) {
        const unsigned long long* K = PM_K + 15 * b;
        const bool four = PM_DEPTH[b] == 4;
        if (b) s[0] = sbox7(s[0]);
        const u64 t1 = sbox7(mds_row0(s, K[0]));
        u64 t3 = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        u32 l[12], h[12];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            l[i] = (u32)s[i];
            h[i] = (u32)(s[i] >> 32);
        }
        const u64 t2 = sbox7(block_row0_d2(l, h, t1, PB_ROW0_D2, K[1]));
        if (four) t3 = sbox7(merged_row0_d3(l, h, t1, t2, PM_ROW0_D3, K[2]));
#else
        const u64 t2 = sbox7(block_row(s, PB_ROW0_D2, t1, mds_coef(0, 0), 0, 0, K[1]));
        if (four) t3 = sbox7(merged_row(s, PM_ROW0_D3 + 1, t1, PM_ROW0_D3[0], t2, mds_coef(0, 0), 0, 0, K[2]));
#endif
        merged_end(s, t1, t2, t3, PM_END + (four ? 0 : 12 * 14), K + 3);
    }
}
// Everything between the first and the last full round; the same for every use of the permutation.
GL_HD void middle(u64* s) {
    const unsigned long long* RC = poseidon_rc();
    for (int r = 1; r < 3; r++) full_round(s, RC + 12 * (r + 1));
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = sbox7(s[i]);
    merged_middle(s);
    for (int r = 26; r < 29; r++) full_round(s, RC + 12 * (r + 1));
}

// The words whose bit is set in `rows` come out canonical; the others are unspecified.
GL_HD void last_round_any(u64* s, const u32 rows) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = sbox7(s[i]);
    mds_full(s, PF_ZERO12, rows);
#pragma unroll
    for (int i = 0; i < 12; i++)
        if ((rows >> i) & 1) s[i] = canon(s[i]);
}
template <u32 ROWS>
GL_HD void last_round(u64* s) {
    static_assert(ROWS != 0 && ROWS <= ROWS_ALL, "a mask of output words 0..11");
    last_round_any(s, ROWS);
}

// first_round(kind), middle, last_round(rows) as the kernels run them: the first round is the first trip of the loop over
// rounds 0..3 and the last round the last trip of the loop over rounds 26..29, so a kernel holds ONE copy of each loop body
// whatever it knows about its inputs (the hash kernels are larger than the instruction cache as it is).
// Round 3 is an S-box layer only: its MDS opens merged_middle.  Two ways to leave it out, chosen per kernel by what the register
// allocator makes of them (the state is one 12-word register tuple to it, and every join of two paths costs a copy of the tuple):
//   !OWN_SBOX3  one loop body serves rounds 0..3: a trip is the MDS of round r - 1 (skipped, wave-uniformly, on the first) and
//               the S-boxes of round r.  The tree kernels' form (k_merkle_level 82 VGPRs, k_merkle_top 84, no spill).
//   OWN_SBOX3   rounds 0..2 as whole rounds and round 3's twelve S-boxes as a copy of their own, 11 KB more code: the sponge
//               kernels' form.  With the skip inside the loop k_hash_leaves needs 98 VGPRs where five waves leave 96, and
//               with the loop left between the two stages of round 3 it spills the state once per MDS row.
template <bool OWN_SBOX3 = false>
GL_HD void permute_known_any(u64* s, const u32 kind, const u32 rows) {
    const unsigned long long* RC = poseidon_rc();
    const unsigned long long* add0 = kind == FR_ZERO_CAP ? RC1_ZCAP : kind == FR_ZERO_RATE ? RC1_ZRATE : RC + 12;
    if (OWN_SBOX3) {
#pragma nounroll
        for (int r = 0; r < 3; r++) full_round_known(s, r == 0 ? kind : (u32)FR_GENERAL, r == 0 ? RC : nullptr, r == 0 ? add0 : RC + 12 * (r + 1));
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = sbox7(s[i]);
    } else {
#pragma nounroll
        for (int r = 0; r < 4; r++) {
            if (r) linear_layer_known(s, r == 1 ? kind : (u32)FR_GENERAL, r == 1 ? add0 : RC + 12 * r);
            sbox_layer_known(s, r == 0 ? kind : (u32)FR_GENERAL, r == 0 ? RC : nullptr);
        }
    }
    merged_middle(s);
#pragma nounroll
    for (int r = 26; r < 30; r++) {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = sbox7(s[i]);
        mds_full(s, r < 29 ? RC + 12 * (r + 1) : PF_ZERO12, r < 29 ? (u32)ROWS_ALL : rows);
    }
#pragma unroll
    for (int i = 0; i < 12; i++)
        if ((rows >> i) & 1) s[i] = canon(s[i]);
}
template <u32 KIND, u32 ROWS>
GL_HD void permute_known(u64* s) {
    static_assert(KIND <= FR_ZERO_RATE && ROWS != 0 && ROWS <= ROWS_ALL, "FR_* and a mask of output words 0..11");
    permute_known_any(s, KIND, ROWS);
}

// The whole permutation on twelve unknown words.  In: canonical or not; out: canonical.
// Round constants are never added on their own (except the very first ones): each layer's linear step starts its
// accumulators from the constants of the layer that follows.
template <bool MERGED = true>
GL_HD void poseidon(u64* s) {
    const unsigned long long* RC = poseidon_rc();
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = add_wrap(s[i], RC[i]);
    if (MERGED) {
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int i = 0; i < 12; i++) s[i] = sbox7(s[i]);
            if (r < 3) mds_full(s, RC + 12 * (r + 1));   // round 3's MDS opens merged_middle
        }
        merged_middle(s);
    } else {   // k_pow: the merged form costs it nine spilled SGPRs and a wave of occupancy (66 VGPRs), so it keeps the blocks of three
        for (int r = 0; r < 4; r++) full_round(s, RC + 12 * (r + 1));
        partial_block(s);
    }
    for (int r = 26; r < 29; r++) full_round(s, RC + 12 * (r + 1));
    full_round(s, nullptr);
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = canon(s[i]);
}

// ---- The sparse-matrix form of the same rounds (tools/gen_poseidon_fast.py, form 1), as these kernels ran them until the block
// form: the fourth full round with the dense 11x11 layer merged into its linear step (PF_E), then 23 multiply-accumulates per
// round on 64-bit constants.  One user is left: PoseidonTree (kernels_verify.h), the Merkle path walks of the verifier and the
// compressor.  tests/test_public_inputs_host.py holds k_vfy_queries to the register count it has with this form, so those two
// kernels keep it; they hash a few hundred nodes per proof and are not where the time goes.
GL_HD u64 mds_row0_terms(const u64* s, u64 rc) {
#if defined(__HIP_DEVICE_COMPILE__)
    {
        u64 al = gl::madk_s<17>((u32)s[0], (u64)(u32)rc), ah = gl::madk_s<17>((u32)(s[0] >> 32), rc >> 32);
#define P2_MDS_TERM(i, K)                       \
    al = gl::madk<K>((u32)s[i], al);            \
    ah = gl::madk<K>((u32)(s[i] >> 32), ah);
        P2_MDS_TERM(1, 15) P2_MDS_TERM(2, 41) P2_MDS_TERM(3, 16) P2_MDS_TERM(4, 2) P2_MDS_TERM(5, 28) P2_MDS_TERM(6, 13)
        P2_MDS_TERM(7, 13) P2_MDS_TERM(8, 39) P2_MDS_TERM(9, 18) P2_MDS_TERM(10, 34) P2_MDS_TERM(11, 20) P2_MDS_TERM(0, 8)
#undef P2_MDS_TERM
        return fold_al_ah(al, ah);
    }
#endif
    return mds_row0(s, rc);
}
// In: the state in front of the fourth full round's S-boxes; out: the state carries round 26's constants.
GL_HD void partial_block_sparse(u64* s) {
    {
        // 4th full round with the dense 11x11 layer of the partial-round block merged into its linear step: lane 0 is the
        // MDS row (+ a_0, the first partial S-box's constant), lanes 1.. are rows of E = D0 . MDS[1.., :] (gen_poseidon_fast.py)
        u64 z[12];
#pragma unroll
        for (int i = 0; i < 12; i++) z[i] = sbox7(s[i]);
#pragma nounroll
        for (int r = 0; r < 11; r++) {
            Acc a;
            a.init();
#pragma unroll
            for (int c = 0; c < 12; c++) a.fma_k(PF_E[r * 12 + c], z[c]);
            s[1 + r] = a.reduce();  // straight into the (dead) state: a separate result array costs 34 VGPRs and a wave of occupancy
        }
        s[0] = mds_row0_terms(z, PF_A[0]);
    }
    for (int i = 0; i < 22; i++) {
        u64 s0 = sbox7(s[0]);
        Acc a;
        a.init();
        a.e01 = i < 21 ? PF_A[i + 1] : PF_RC26[0];  // the next S-box's / next full round's constant for lane 0
        a.fma_small(25, s0);
#pragma unroll
        for (int j = 0; j < 11; j++) a.fma_k(PF_WHAT[i * 11 + j], s[1 + j]);
#pragma unroll
        for (int j = 0; j < 11; j++) s[1 + j] = mulr_add_k(PF_V[i * 11 + j], s0, s[1 + j]);
        s[0] = a.reduce();
    }
#pragma unroll
    for (int j = 1; j < 12; j++) s[j] = add_wrap(s[j], PF_RC26[j]);
}
// glf::poseidon with the sparse partial rounds.  In: canonical or not; out: canonical.
GL_HD void poseidon_sparse(u64* s) {
    const unsigned long long* RC = poseidon_rc();
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = add_wrap(s[i], RC[i]);
    for (int r = 0; r < 3; r++) full_round(s, RC + 12 * (r + 1));
    partial_block_sparse(s);
    for (int r = 26; r < 29; r++) full_round(s, RC + 12 * (r + 1));
    full_round(s, nullptr);
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = canon(s[i]);
}

// One absorb-and-permute step of an overwrite-mode sponge (hash_n_to_hash_no_pad) over `width` input words of which the
// words >= `live` are known to be 0: the chunk at word c0 is already in s[0..7] (a chunk of known zeros need not be).  The
// first chunk meets a zero capacity, a whole chunk of known zeros behind it is a zero rate, anything else is general; the
// outputs kept are those the chunk at c0 + 8 leaves standing.  c0, width, live: wave-uniform on the device.
GL_HD u32 sponge_first_kind(int c0, int width, int live) {
    return c0 == 0 ? (u32)FR_ZERO_CAP : (c0 >= live && c0 + 8 <= width) ? (u32)FR_ZERO_RATE : (u32)FR_GENERAL;
}
GL_HD void sponge_permute(u64* s, int c0, int width, int live) {
    permute_known_any<true>(s, sponge_first_kind(c0, width, live), rows_before_chunk(width - (c0 + 8)));
}
// two_to_one(a, b): words 0..7 = a || b, zero capacity, digest out
GL_HD void two_to_one_permute(u64* s) {
    permute_known<FR_ZERO_CAP, ROWS_DIGEST>(s);
}

#if defined(__HIPCC__)
// ---- cooperative form: ONE sponge state spread over 12 lanes of a 16-lane group (lane i holds word i; lanes 12..15 are
// idle and must hold 0).  Same permutation, same constants; the linear layers gather the other words with cross-lane
// reads (ds_bpermute) and the partial rounds' dot product is a 4-step butterfly sum.  4.3 k VALU instructions per lane
// instead of 15.5 k: this is for the Fiat-Shamir chain (k_challenger), where ~110 permutations per proof are strictly
// sequential and a thread-per-sponge kernel leaves a single proof waiting on one lane's instruction stream.
__device__ __forceinline__ u64 shfl64(u64 v, int src_lane) { return (u64)__shfl((unsigned long long)v, src_lane, 64); }
__device__ inline u64 poseidon_coop(u64 w, const u32 i /* lane within the 16-lane group */) {
    const int lane = (int)(threadIdx.x & 63), gbase = lane & ~15;
    const bool live = i < 12;
    const u32 ii = live ? i : 0;  // index clamp for the idle lanes' (unused) constant loads
    const unsigned long long* RC = (const unsigned long long*)gl::D_POSEIDON_RC;
    // circulant MDS row of this lane on the group's words z, plus the next constant
    auto mds = [&](u64 z, u64 rc) -> u64 {
        const u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
        u64 al = (u32)rc, ah = rc >> 32;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            u32 src = i + k;
            src = src >= 12 ? src - 12 : src;  // (i + k) mod 12 for live lanes; idle lanes read some lane of the group, unused
            const u64 x = shfl64(z, gbase + (int)(src & 15));
            const u32 c = C[k] + ((k == 0 && i == 0) ? 8u : 0u);
            al += (x & gl::EPS) * c;
            ah += (x >> 32) * c;
        }
        return fold_al_ah(al, ah);
    };
    w = live ? add_wrap(w, RC[ii]) : 0;
    for (int r = 0; r < 3; r++) w = mds(sbox7(w), live ? RC[12 * (r + 1) + ii] : 0);
    {   // 4th full round with the dense layer merged in (PF_E): lane 0 takes the MDS row, lanes 1..11 a row of E
        const u64 z = sbox7(w);
        const u64 row0 = mds(z, i == 0 ? PF_A[0] : 0);
        const u32 er = (live && i >= 1) ? i - 1 : 0;
        Acc a;
        a.init();
#pragma unroll
        for (int c = 0; c < 12; c++) a.fma(PF_E[er * 12 + c], shfl64(z, gbase + c));
        const u64 rowe = a.reduce();
        w = i == 0 ? row0 : (live ? rowe : 0);
    }
    for (int pr = 0; pr < 22; pr++) {
        const u64 z0 = shfl64(sbox7(w), gbase);  // lane 0's S-box output, to everybody
        const u32 cj = (live && i >= 1) ? pr * 11 + (i - 1) : 0;
        const u64 coef = i == 0 ? 25 : (live ? PF_WHAT[cj] : 0);
        u64 term = canon(mulr(coef, i == 0 ? z0 : w));  // idle lanes: 0
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) term = gl::add(term, shfl64(term, lane ^ d));
        const u64 s0n = gl::add(term, pr < 21 ? PF_A[pr + 1] : PF_RC26[0]);
        const u64 wj = mulr_add((live && i >= 1) ? PF_V[cj] : 0, z0, w);
        w = i == 0 ? s0n : wj;
    }
    if (live && i >= 1) w = add_wrap(w, PF_RC26[ii]);
    for (int r = 26; r < 29; r++) w = mds(sbox7(w), live ? RC[12 * (r + 1) + ii] : 0);
    w = mds(sbox7(w), 0);
    return live ? canon(w) : 0;
}
#endif

}  // namespace glf
