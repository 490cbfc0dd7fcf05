// Scalars of ecGFp5 modulo the group order n (ecgfp5.h GROUP_ORDER, 319 bits), written once for host and device:
//     sc_muladd(a, b, c) = (a b + c) mod n     for arbitrary 320-bit a, b, c,
// five little-endian 64-bit limbs each.  The 640-bit value a b + c is reduced by shift-and-subtract, one bit per step: it runs
// once per signature beside 320 point doublings, so nothing here is tuned.  Plain C++ on 64-bit limbs; the device takes the high
// half of a product from __umul64hi.  Every loop over limbs has constant bounds, so on the device a scalar is five register
// pairs and never an indexed array in memory.
#pragma once
#include "gl.h"

namespace p2 {
namespace ecsc {

typedef gl::u64 u64;

#if defined(__HIP_DEVICE_COMPILE__)
#define ECSC_UNROLL _Pragma("unroll")
#else
#define ECSC_UNROLL
#endif

// limb i of the group order (the value of ecgfp5::GROUP_ORDER; test_schnorr_host.py compares the two)
GL_HD u64 order_limb(int i) {
    return i == 0 ? 0xe80fd996948bffe1ull : i == 1 ? 0xe8885c39d724a09cull : i == 2 ? 0x7fffffe6cfb80639ull : i == 3 ? 0x7ffffff100000016ull : 0x7ffffffd80000007ull;
}
GL_HD void mul_wide(u64 a, u64 b, u64& hi, u64& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (u64)p;
    hi = (u64)(p >> 64);
#endif
}
// a + b + carry-in -> sum, carry-out (0 or 1)
GL_HD u64 adc(u64 a, u64 b, u64& carry) {
    const u64 s = a + b, c1 = s < a;
    const u64 r = s + carry, c2 = r < s;
    carry = c1 | c2;
    return r;
}
// a - b - borrow-in -> difference, borrow-out (0 or 1)
GL_HD u64 sbb(u64 a, u64 b, u64& borrow) {
    const u64 d = a - b, b1 = a < b;
    const u64 r = d - borrow, b2 = d < borrow;
    borrow = b1 | b2;
    return r;
}
GL_HD bool sc_is_zero(const u64 a[5]) { return (a[0] | a[1] | a[2] | a[3] | a[4]) == 0; }
// a < n
GL_HD bool sc_below_order(const u64 a[5]) {
    u64 borrow = 0;
    ECSC_UNROLL
    for (int i = 0; i < 5; i++) (void)sbb(a[i], order_limb(i), borrow);
    return borrow != 0;
}
// r <- 2 r + bit, then r - n if that is not negative: r stays below n (r < n < 2^319, so 2 r + 1 fits in 320 bits)
GL_HD void sc_shift_in(u64 r[5], u64 bit) {
    u64 t[5], d[5], borrow = 0;
    ECSC_UNROLL
    for (int i = 4; i > 0; i--) t[i] = (r[i] << 1) | (r[i - 1] >> 63);
    t[0] = (r[0] << 1) | bit;
    ECSC_UNROLL
    for (int i = 0; i < 5; i++) d[i] = sbb(t[i], order_limb(i), borrow);
    ECSC_UNROLL
    for (int i = 0; i < 5; i++) r[i] = borrow ? t[i] : d[i];
}
// out = (a b + c) mod n; out may alias an input
GL_HD void sc_muladd(const u64 a[5], const u64 b[5], const u64 c[5], u64 out[5]) {
    // t = a b + c < 2^640: schoolbook rows, each a[i] * b + (row of t) with a running high word
    u64 t[10];
    ECSC_UNROLL
    for (int i = 0; i < 5; i++) t[i] = c[i], t[5 + i] = 0;
    ECSC_UNROLL
    for (int i = 0; i < 5; i++) {
        u64 high = 0;
        ECSC_UNROLL
        for (int j = 0; j < 5; j++) {
            u64 hi, lo, carry = 0;
            mul_wide(a[i], b[j], hi, lo);
            lo = adc(lo, high, carry);  // hi <= 2^64 - 2, so hi + carry does not wrap
            hi += carry;
            carry = 0;
            t[i + j] = adc(t[i + j], lo, carry);
            high = hi + carry;
        }
        // rows 0..i-1 left t[i + 5 ..] at zero, and the total stays below 2^(64 (i + 6)): no carry leaves this word
        t[i + 5] = high;
    }
    u64 r[5] = {0, 0, 0, 0, 0};
    ECSC_UNROLL
    for (int l = 9; l >= 0; l--) {
        const u64 w = t[l];
#if defined(__HIP_DEVICE_COMPILE__)
        _Pragma("nounroll")
#endif
        for (int k = 63; k >= 0; k--) sc_shift_in(r, (w >> k) & 1);
    }
    ECSC_UNROLL
    for (int i = 0; i < 5; i++) out[i] = r[i];
}

}  // namespace ecsc
}  // namespace p2
