// AES / AES-GCM gadgets over the CircuitBuilder mirror, one function per reference function, same names.
//
// Mirrors aes-gcm/src/circuit_aes.rs (trait CircuitBuilderAESState :41-174, impl :176-275, LUT builders
// :299-335, byte_xor :350-358) and aes-gcm/src/circuit_gcm.rs (AesGcmTarget::build :49-172, set_targets
// :174-208, gctr_target :212-260, ghash_target :262-289, gf_2_128_mul_target :290-326,
// right_shift_one_target :327-348, inc32_target :350-368, LUTs :392-425).  Const generics <NK,NB,NR,L,TAG>
// become run-time arguments (NB is always 4).  The native (non-circuit) cipher used to produce witness values
// mirrors aes-gcm/src/native_aes.rs and native_gcm.rs.
//
// Not in the reference: GHASH from carry-less multiply tables (gcm_clmul_lo_lut / gcm_clmul_hi_lut, gf_2_128_mul_tables_target,
// ghash_tables_target), which AesGcmTarget::build uses under CircuitBuilder::set_ghash_tables.  Its inputs must be range-checked
// byte targets; the comment above the gadget says why and which targets of AesGcmTarget qualify.
#pragma once
#include <array>

#include "builder.h"

namespace p2 {
namespace aes {

typedef Target ByteTarget;
typedef std::array<std::array<ByteTarget, 4>, 4> StateTarget;
typedef std::array<ByteTarget, 4> WordTarget;

// ---------------------------------------------------------------- constants (aes-gcm/src/constants.rs)
static const uint8_t SBOX[256] = {
#include "aes_sbox.inc"
};
static const uint8_t RCON[11] = {0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
static const size_t TAG_LEN = 128;

// ---------------------------------------------------------------- native cipher (native_aes.rs, native_gcm.rs)
typedef std::array<std::array<uint8_t, 4>, 4> State;

inline uint8_t gf_2_8_mul(uint8_t a, uint8_t b) {
    uint8_t r = 0;
    for (int i = 0; i < 8; i++) {
        if (b & 1) r ^= a;
        uint8_t hb = a & 0x80;
        a <<= 1;
        if (hb) a ^= 0x1b;
        b >>= 1;
    }
    return r;
}
template <class T>
inline std::array<std::array<T, 4>, 4> shift_rows(const std::array<std::array<T, 4>, 4>& s) {
    std::array<std::array<T, 4>, 4> r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[i][j] = s[i][(i + j) % 4];
    return r;
}
template <class T>
inline std::array<T, 4> rot_word(const std::array<T, 4>& w) {
    return {w[1], w[2], w[3], w[0]};
}
inline std::array<uint8_t, 16> flatten_state(const State& s) {
    std::array<uint8_t, 16> r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[i * 4 + j] = s[j][i];
    return r;
}
// expanded key as 4*(NR+1) words
inline std::vector<std::array<uint8_t, 4>> key_expansion(int NK, int NR, const uint8_t* key) {
    std::vector<std::array<uint8_t, 4>> w(4 * (NR + 1));
    for (int i = 0; i < NK; i++)
        for (int j = 0; j < 4; j++) w[i][j] = key[4 * i + j];
    for (int i = NK; i < 4 * (NR + 1); i++) {
        std::array<uint8_t, 4> temp = w[i - 1];
        if (i % NK == 0) {
            temp = rot_word(temp);
            for (auto& b : temp) b = SBOX[b];
            temp[0] ^= RCON[i / NK];
        } else if (NK > 6 && i % NK == 4) {
            for (auto& b : temp) b = SBOX[b];
        }
        for (int j = 0; j < 4; j++) w[i][j] = w[i - NK][j] ^ temp[j];
    }
    return w;
}
inline State encrypt_block(int NR, const uint8_t* input, const std::vector<std::array<uint8_t, 4>>& w) {
    State s;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) s[i][j] = input[i + 4 * j];
    auto add_round_key = [&](int r) {
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) s[i][j] ^= w[4 * r + j][i];
    };
    auto sub_bytes = [&]() {
        for (auto& row : s)
            for (auto& b : row) b = SBOX[b];
    };
    add_round_key(0);
    for (int round = 1; round < NR; round++) {
        sub_bytes();
        s = shift_rows(s);
        State r;
        for (int c = 0; c < 4; c++) {
            r[0][c] = gf_2_8_mul(2, s[0][c]) ^ gf_2_8_mul(3, s[1][c]) ^ s[2][c] ^ s[3][c];
            r[1][c] = s[0][c] ^ gf_2_8_mul(2, s[1][c]) ^ gf_2_8_mul(3, s[2][c]) ^ s[3][c];
            r[2][c] = s[0][c] ^ s[1][c] ^ gf_2_8_mul(2, s[2][c]) ^ gf_2_8_mul(3, s[3][c]);
            r[3][c] = gf_2_8_mul(3, s[0][c]) ^ s[1][c] ^ s[2][c] ^ gf_2_8_mul(2, s[3][c]);
        }
        s = r;
        add_round_key(round);
    }
    sub_bytes();
    s = shift_rows(s);
    add_round_key(NR);
    return s;
}
inline void inc32(uint8_t* b) {
    uint32_t ctr = ((uint32_t)b[12] << 24) | ((uint32_t)b[13] << 16) | ((uint32_t)b[14] << 8) | b[15];
    ctr += 1;
    b[12] = ctr >> 24;
    b[13] = ctr >> 16;
    b[14] = ctr >> 8;
    b[15] = ctr;
}
inline std::vector<uint8_t> gctr(int NR, const std::vector<std::array<uint8_t, 4>>& key, const uint8_t* icb, const uint8_t* x, size_t len) {
    std::vector<uint8_t> y(len);
    uint8_t cb[16];
    memcpy(cb, icb, 16);
    for (size_t off = 0, i = 0; off < len; off += 16, i++) {
        if (i > 0) inc32(cb);
        auto ks = flatten_state(encrypt_block(NR, cb, key));
        size_t l = std::min<size_t>(16, len - off);
        for (size_t j = 0; j < l; j++) y[off + j] = x[off + j] ^ ks[j];
    }
    return y;
}
inline void right_shift_one(uint8_t* block) {
    uint8_t carry = 0;
    for (int i = 0; i < 16; i++) {
        uint8_t nc = block[i] & 1;
        block[i] = (block[i] >> 1) | (carry << 7);
        carry = nc;
    }
}
inline std::array<uint8_t, 16> gf_2_128_mul(const uint8_t* x, const uint8_t* y) {
    std::array<uint8_t, 16> z{};
    uint8_t v[16];
    memcpy(v, y, 16);
    for (int i = 0; i < 128; i++) {
        if ((x[i / 8] >> (7 - (i % 8))) & 1)
            for (int b = 0; b < 16; b++) z[b] ^= v[b];
        uint8_t lsb = v[15] & 1;
        right_shift_one(v);
        if (lsb) v[0] ^= 0xE1;
    }
    return z;
}
inline std::array<uint8_t, 16> ghash(const uint8_t* h, const uint8_t* x, size_t len) {
    std::array<uint8_t, 16> y{};
    for (size_t i = 0; i < len / 16; i++) {
        uint8_t t[16];
        for (int b = 0; b < 16; b++) t[b] = y[b] ^ x[16 * i + b];
        y = gf_2_128_mul(t, h);
    }
    return y;
}
// The tag of (aad, c) under the expanded key w (SP 800-38D section 7.1, steps 4 to 6): GHASH_H over
// aad || 0^v || c || 0^u || [8 aad_len]_64 || [8 len]_64, then GCTR from J0 = nonce || 0^31 || 1.
inline std::array<uint8_t, 16> gcm_tag(int NR, const std::vector<std::array<uint8_t, 4>>& w, const uint8_t* nonce, const uint8_t* aad, size_t aad_len,
                                       const uint8_t* c, size_t len) {
    uint8_t zero[16] = {0};
    auto h = flatten_state(encrypt_block(NR, zero, w));
    uint8_t j0[16] = {0};
    memcpy(j0, nonce, 12);
    j0[15] = 1;
    std::vector<uint8_t> gin;
    gin.reserve(aad_len + len + 48);
    if (aad_len) gin.insert(gin.end(), aad, aad + aad_len);
    gin.resize((aad_len + 15) / 16 * 16, 0);
    if (len) gin.insert(gin.end(), c, c + len);
    gin.resize((gin.size() + 15) / 16 * 16, 0);
    uint64_t alen = (uint64_t)aad_len * 8, clen = (uint64_t)len * 8;
    for (int i = 7; i >= 0; i--) gin.push_back((uint8_t)(alen >> (8 * i)));
    for (int i = 7; i >= 0; i--) gin.push_back((uint8_t)(clen >> (8 * i)));
    auto s = ghash(h.data(), gin.data(), gin.size());
    auto t = gctr(NR, w, j0, s.data(), 16);
    std::array<uint8_t, 16> tag;
    memcpy(tag.data(), t.data(), 16);
    return tag;
}
// the counter mode of the message: GCTR from inc32(J0)
inline std::vector<uint8_t> gcm_ctr(int NR, const std::vector<std::array<uint8_t, 4>>& w, const uint8_t* nonce, const uint8_t* x, size_t len) {
    uint8_t j0i[16] = {0};
    memcpy(j0i, nonce, 12);
    j0i[15] = 1;
    inc32(j0i);
    return gctr(NR, w, j0i, x, len);
}
// native_gcm.rs:16-68 with the additional authenticated data it leaves out (its a = []).  96-bit nonce, 16-byte tag.
inline void gcm_encrypt_aad(int NK, int NR, const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* pt, size_t len,
                            uint8_t* ct, uint8_t* tag) {
    auto w = key_expansion(NK, NR, key);
    auto c = gcm_ctr(NR, w, nonce, pt, len);
    auto t = gcm_tag(NR, w, nonce, aad, aad_len, c.data(), len);
    if (len) memcpy(ct, c.data(), len);
    memcpy(tag, t.data(), 16);
}
// native_gcm.rs:16-68.  Returns (ciphertext, 16-byte tag); no AAD, 96-bit nonce.
inline void gcm_encrypt(int NK, int NR, const uint8_t* key, const uint8_t* nonce, const uint8_t* pt, size_t len, uint8_t* ct, uint8_t* tag) {
    gcm_encrypt_aad(NK, NR, key, nonce, nullptr, 0, pt, len, ct, tag);
}
// Authenticated decryption (SP 800-38D section 7.2; not in the reference): the tag over (aad, ct) is recomputed and all 16 bytes
// compared, without an early exit; the counter mode runs only when they match.  false: pt is zeroed.
inline bool gcm_decrypt(int NK, int NR, const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* ct, size_t len,
                        const uint8_t* tag, uint8_t* pt) {
    auto w = key_expansion(NK, NR, key);
    auto t = gcm_tag(NR, w, nonce, aad, aad_len, ct, len);
    uint8_t diff = 0;
    for (int i = 0; i < 16; i++) diff |= (uint8_t)(t[i] ^ tag[i]);
    if (diff) {
        if (len) memset(pt, 0, len);
        return false;
    }
    auto p = gcm_ctr(NR, w, nonce, ct, len);
    if (len) memcpy(pt, p.data(), len);
    return true;
}

// ---------------------------------------------------------------- LUT builders
inline size_t sbox_lut(CircuitBuilder& b) {  // circuit_aes.rs:299
    std::vector<std::pair<u16, u16>> t(256);
    for (int i = 0; i < 256; i++) t[i] = {(u16)i, (u16)SBOX[i]};
    return b.add_lookup_table_from_pairs(t);
}
inline size_t byte_xor_lut(CircuitBuilder& b) {  // circuit_aes.rs:309
    std::vector<std::pair<u16, u16>> t;
    t.reserve(65536);
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) t.push_back({(u16)((x << 8) + y), (u16)(x ^ y)});
    return b.add_lookup_table_from_pairs(t);
}
inline size_t gf_2_8_mul_lut(CircuitBuilder& b) {  // circuit_aes.rs:321
    std::vector<std::pair<u16, u16>> t;
    t.reserve(65536);
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) t.push_back({(u16)((x << 8) + y), (u16)gf_2_8_mul((uint8_t)x, (uint8_t)y)});
    return b.add_lookup_table_from_pairs(t);
}
inline size_t u8_unit_right_shift_lut(CircuitBuilder& b) {  // circuit_gcm.rs:392
    std::vector<std::pair<u16, u16>> t(256);
    for (int x = 0; x < 256; x++) t[x] = {(u16)x, (u16)(x >> 1)};
    return b.add_lookup_table_from_pairs(t);
}
inline size_t u8_bitref_lut(CircuitBuilder& b) {  // circuit_gcm.rs:407
    std::vector<std::pair<u16, u16>> t;
    for (int x = 0; x < 256; x++)
        for (int i = 0; i < 8; i++) t.push_back({(u16)((x << 3) + i), (u16)((x >> i) & 1)});
    return b.add_lookup_table_from_pairs(t);
}
// Carry-less byte products in GCM's bit order (not in the reference; CircuitBuilder::set_ghash_tables).  Bit i of a GCM block is
// bit 7 - i % 8 of byte i / 8 and the coefficient of x^i, so a byte B stands for the polynomial whose plain-integer form is the
// bit-reversed byte rev8(B).  With c = clmul(rev8(a), rev8(b)), a 15-bit product, the two tables send (a << 8) + b to
// rev8(c & 0xff) and rev8(c >> 8): the product's coefficients of x^0..x^7 and of x^8..x^14 as GCM bytes (the second one's low bit
// is always 0).
inline uint8_t rev8(uint8_t v) {
    v = (uint8_t)((v >> 4) | (v << 4));
    v = (uint8_t)(((v & 0xCC) >> 2) | ((v & 0x33) << 2));
    return (uint8_t)(((v & 0xAA) >> 1) | ((v & 0x55) << 1));
}
inline u16 clmul8(uint8_t a, uint8_t b) {
    u16 r = 0;
    for (int i = 0; i < 8; i++)
        if ((b >> i) & 1) r ^= (u16)((u16)a << i);
    return r;
}
inline size_t gcm_clmul_lut(CircuitBuilder& b, bool high) {
    std::vector<std::pair<u16, u16>> t;
    t.reserve(65536);
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) {
            u16 c = clmul8(rev8((uint8_t)x), rev8((uint8_t)y));
            t.push_back({(u16)((x << 8) + y), (u16)rev8((uint8_t)(high ? c >> 8 : c & 0xff))});
        }
    return b.add_lookup_table_from_pairs(t);
}
inline size_t gcm_clmul_lo_lut(CircuitBuilder& b) { return gcm_clmul_lut(b, false); }
inline size_t gcm_clmul_hi_lut(CircuitBuilder& b) { return gcm_clmul_lut(b, true); }

// ---------------------------------------------------------------- CircuitBuilderAESState (circuit_aes.rs:41-275)
inline ByteTarget add_virtual_byte_target_unsafe(CircuitBuilder& b) { return b.add_virtual_target(); }
inline void assert_byte(CircuitBuilder& b, Target x, size_t u8_table_idx) { b.add_lookup_from_index(x, u8_table_idx); }
inline ByteTarget add_virtual_byte_target(CircuitBuilder& b, size_t u8_table_idx) {
    ByteTarget t = add_virtual_byte_target_unsafe(b);
    assert_byte(b, t, u8_table_idx);
    return t;
}
inline ByteTarget byte_constant(CircuitBuilder& b, uint8_t c) { return b.constant(c); }
inline StateTarget add_virtual_state_target_unsafe(CircuitBuilder& b) {
    StateTarget s;
    for (auto& row : s)
        for (auto& t : row) t = add_virtual_byte_target_unsafe(b);
    return s;
}
inline StateTarget add_virtual_state_target(CircuitBuilder& b, size_t u8_table_idx) {
    StateTarget s;
    for (auto& row : s)
        for (auto& t : row) t = add_virtual_byte_target(b, u8_table_idx);
    return s;
}
inline std::array<ByteTarget, 16> flatten(const StateTarget& s) {  // circuit_aes.rs:28
    std::array<ByteTarget, 16> r;
    for (int i = 0; i < 16; i++) r[i] = s[i % 4][i / 4];
    return r;
}
inline StateTarget from_flat(const std::array<ByteTarget, 16>& f) {  // circuit_aes.rs:32
    StateTarget s;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) s[i][j] = f[j * 4 + i];
    return s;
}
inline ByteTarget byte_xor(CircuitBuilder& b, size_t xor_lut_idx, ByteTarget x, ByteTarget y) {  // :350
    Target idx = b.mul_const_add(1 << 8, x, y);
    return b.add_lookup_from_index(idx, xor_lut_idx);
}
inline ByteTarget gf_2_8_add(CircuitBuilder& b, size_t xor_lut_idx, ByteTarget x, ByteTarget y) { return byte_xor(b, xor_lut_idx, x, y); }
inline ByteTarget gf_2_8_mul_t(CircuitBuilder& b, size_t mul_lut_idx, ByteTarget x, ByteTarget y) {  // :243
    Target idx = b.mul_const_add(1 << 8, x, y);
    return b.add_lookup_from_index(idx, mul_lut_idx);
}
inline WordTarget state_sub_word(CircuitBuilder& b, size_t sbox_lut_idx, const WordTarget& w) {  // :189
    WordTarget r;
    for (int i = 0; i < 4; i++) r[i] = b.add_lookup_from_index(w[i], sbox_lut_idx);
    return r;
}
inline StateTarget state_sub_bytes(CircuitBuilder& b, size_t sbox_lut_idx, const StateTarget& s) {  // :99
    StateTarget r;
    for (int i = 0; i < 4; i++) r[i] = state_sub_word(b, sbox_lut_idx, s[i]);
    return r;
}
inline ByteTarget bytearray_ip4(CircuitBuilder& b, size_t xor_lut, size_t mul_lut, const WordTarget& x, const WordTarget& y) {  // :253
    ByteTarget acc = b.zero();
    for (int i = 0; i < 4; i++) {
        ByteTarget prod = gf_2_8_mul_t(b, mul_lut, x[i], y[i]);
        acc = gf_2_8_add(b, xor_lut, acc, prod);
    }
    return acc;
}
inline StateTarget state_mix_matrix(CircuitBuilder& b) {  // :337
    ByteTarget one = byte_constant(b, 1), two = byte_constant(b, 2), three = byte_constant(b, 3);
    StateTarget m = {{{two, three, one, one}, {one, two, three, one}, {one, one, two, three}, {three, one, one, two}}};
    return m;
}
inline StateTarget state_mix_columns(CircuitBuilder& b, size_t xor_lut, size_t mul_lut, const StateTarget& mix, const StateTarget& s) {  // :109
    StateTarget out_cols;
    for (int i = 0; i < 4; i++) {
        WordTarget col = {s[0][i], s[1][i], s[2][i], s[3][i]};
        for (int m = 0; m < 4; m++) out_cols[i][m] = bytearray_ip4(b, xor_lut, mul_lut, mix[m], col);
    }
    StateTarget r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[i][j] = out_cols[j][i];
    return r;
}
inline StateTarget state_add_round_key(CircuitBuilder& b, size_t xor_lut, const WordTarget* round_key, const StateTarget& s) {  // :124
    StateTarget r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[i][j] = gf_2_8_add(b, xor_lut, s[i][j], round_key[j][i]);
    return r;
}
inline std::vector<WordTarget> key_expansion_t(CircuitBuilder& b, int NK, int NR, size_t xor_lut, size_t sbox_lut_idx, const std::vector<ByteTarget>& key) {  // :197
    std::array<ByteTarget, 11> rcon;
    for (int i = 0; i < 11; i++) rcon[i] = byte_constant(b, RCON[i]);
    std::vector<WordTarget> st(NK);
    for (int i = 0; i < NK; i++)
        for (int j = 0; j < 4; j++) st[i][j] = key[4 * i + j];
    for (int i = NK; i < 4 * (NR + 1); i++) {
        WordTarget offset;
        if (i % NK == 0) {
            WordTarget term = state_sub_word(b, sbox_lut_idx, rot_word(st[i - 1]));
            offset = term;
            offset[0] = gf_2_8_add(b, xor_lut, term[0], rcon[i / NK]);
        } else if (NK > 6 && i % NK == 4) {
            offset = state_sub_word(b, sbox_lut_idx, st[i - 1]);
        } else {
            offset = st[i - 1];
        }
        WordTarget cur;
        for (int j = 0; j < 4; j++) cur[j] = gf_2_8_add(b, xor_lut, st[i - NK][j], offset[j]);
        st.push_back(cur);
    }
    return st;
}
inline StateTarget encrypt_block_t(CircuitBuilder& b, int NR, size_t xor_lut, size_t mul_lut, size_t sbox_lut_idx, const StateTarget& mix,
                                   StateTarget s, const std::vector<WordTarget>& w) {  // :76
    s = state_add_round_key(b, xor_lut, &w[0], s);
    for (int i = 1; i < NR; i++) {
        s = state_sub_bytes(b, sbox_lut_idx, s);
        s = shift_rows(s);
        s = state_mix_columns(b, xor_lut, mul_lut, mix, s);
        s = state_add_round_key(b, xor_lut, &w[4 * i], s);
    }
    s = state_sub_bytes(b, sbox_lut_idx, s);
    s = shift_rows(s);
    return state_add_round_key(b, xor_lut, &w[4 * NR], s);
}
inline ByteTarget zero_byte(CircuitBuilder& b) { return b.zero(); }
inline StateTarget empty_state(CircuitBuilder& b) {
    StateTarget s;
    for (auto& row : s)
        for (auto& t : row) t = b.zero();
    return s;
}

// ---------------------------------------------------------------- GCM (circuit_gcm.rs)
typedef std::array<ByteTarget, 16> BlockTarget;

inline BlockTarget xor_blocks(CircuitBuilder& b, size_t xor_lut, const BlockTarget& b1, const BlockTarget& b2) {  // :370
    BlockTarget r;
    for (int i = 0; i < 16; i++) r[i] = byte_xor(b, xor_lut, b1[i], b2[i]);
    return r;
}
inline ByteTarget u8_unit_right_shift(CircuitBuilder& b, size_t lut, ByteTarget x) { return b.add_lookup_from_index(x, lut); }  // :398
inline BoolTarget u8_bitref(CircuitBuilder& b, size_t lut, ByteTarget x, ByteTarget i) {  // :417
    Target idx = b.mul_const_add(8, x, i);
    return BoolTarget{b.add_lookup_from_index(idx, lut)};
}
inline BlockTarget right_shift_one_target(CircuitBuilder& b, size_t shift_lut, const BlockTarget& v) {  // :327
    BlockTarget r = v;
    Target carry = b.zero();
    for (int i = 0; i < 16; i++) {
        ByteTarget current = v[i];
        ByteTarget shifted = u8_unit_right_shift(b, shift_lut, current);
        Target next_carry = b.mul_const_add(gl::mul(2, gl::P - 1), shifted, current);
        shifted = b.mul_const_add(1 << 7, carry, shifted);
        r[i] = shifted;
        carry = next_carry;
    }
    return r;
}
inline BlockTarget inc32_target(CircuitBuilder& b, const BlockTarget& block) {  // :350
    BlockTarget r = block;
    Target zero = b.zero();
    Target u8_max = b.constant(255);
    Target carry = b.one();
    for (int byte_index = 15; byte_index >= 12; byte_index--) {
        Target a = block[byte_index];
        Target sum = b.add(a, carry);
        BoolTarget a_is_u8_max = b.is_equal(a, u8_max);
        Target carry_out = b.mul(carry, a_is_u8_max.target);
        r[byte_index] = b.select(a_is_u8_max, zero, sum);
        carry = carry_out;
    }
    return r;
}
inline std::vector<ByteTarget> gctr_target(CircuitBuilder& b, int NR, size_t xor_lut, size_t mul_lut, size_t sbox_lut_idx, const StateTarget& mix,
                                           const std::vector<WordTarget>& key, const BlockTarget& icb, const std::vector<ByteTarget>& x) {  // :212
    const size_t L = x.size();
    std::vector<ByteTarget> y = x;
    BlockTarget cb_i = icb;
    ByteTarget zb = zero_byte(b);
    for (size_t off = 0, i = 0; off < L; off += 16, i++) {
        if (i > 0) cb_i = inc32_target(b, cb_i);
        size_t l = std::min<size_t>(16, L - off);
        BlockTarget x_i;
        x_i.fill(zb);
        for (size_t j = 0; j < l; j++) x_i[j] = x[off + j];
        BlockTarget ciph = flatten(encrypt_block_t(b, NR, xor_lut, mul_lut, sbox_lut_idx, mix, from_flat(cb_i), key));
        BlockTarget y_i;
        size_t n_bytes;
        if (l == 16) {
            y_i = xor_blocks(b, xor_lut, x_i, ciph);
            n_bytes = 16;
        } else {
            // last chunk: MSB_{L%16 bytes}(ciph), zero-padded, then xor over the full block (as the reference does)
            BlockTarget m;
            m.fill(zb);
            for (size_t j = 0; j < L % 16; j++) m[j] = ciph[j];
            y_i = xor_blocks(b, xor_lut, x_i, m);
            n_bytes = L % 16;
        }
        for (size_t j = 0; j < n_bytes; j++) y[off + j] = y_i[j];
    }
    return y;
}
inline BlockTarget gf_2_128_mul_target(CircuitBuilder& b, size_t xor_lut, size_t shift_lut, size_t bitref_lut, const BlockTarget& x, const BlockTarget& y) {  // :290
    ByteTarget zero = zero_byte(b);
    ByteTarget r_first = byte_constant(b, 225);
    BlockTarget z;
    z.fill(zero);
    BlockTarget v = y;
    for (int i = 0; i < 128; i++) {
        int byte_index = i / 8, bit_index = 7 - (i % 8);
        ByteTarget bit_idx_target = byte_constant(b, (uint8_t)bit_index);
        BoolTarget xi = u8_bitref(b, bitref_lut, x[byte_index], bit_idx_target);
        for (int k = 0; k < 16; k++) {
            ByteTarget z_xor_v = byte_xor(b, xor_lut, z[k], v[k]);
            z[k] = b.select(xi, z_xor_v, z[k]);
        }
        BoolTarget lsb = u8_bitref(b, bitref_lut, v[15], zero);
        v = right_shift_one_target(b, shift_lut, v);
        ByteTarget v_xor_r = byte_xor(b, xor_lut, v[0], r_first);
        v[0] = b.select(lsb, v_xor_r, v[0]);
    }
    return z;
}
inline BlockTarget ghash_target(CircuitBuilder& b, size_t xor_lut, size_t shift_lut, size_t bitref_lut, const BlockTarget& h, const std::vector<ByteTarget>& x) {  // :262
    if (x.size() % 16 != 0) throw std::runtime_error("ghash input must be a multiple of 16 bytes");
    ByteTarget zb = zero_byte(b);
    BlockTarget y;
    y.fill(zb);
    for (size_t i = 0; i < x.size() / 16; i++) {
        BlockTarget xi;
        for (int k = 0; k < 16; k++) xi[k] = x[16 * i + k];
        BlockTarget y_xi = xor_blocks(b, xor_lut, y, xi);
        y = gf_2_128_mul_target(b, xor_lut, shift_lut, bitref_lut, y_xi, h);
    }
    return y;
}

// ---------------------------------------------------------------- GHASH from carry-less multiply tables (not in the reference)
// The same function as gf_2_128_mul_target / ghash_target in ArithmeticGate and LookupGate rows of another shape: a product in
// GF(2^128) is 16 x 16 byte-by-byte carry-less products, each one entry of gcm_clmul_lo_lut and one of gcm_clmul_hi_lut, summed
// by byte position into a 32-byte unreduced product and folded back with x^128 = 1 + x + x^2 + x^7 (the byte 0xE1, the
// reference's r_first).  Per GHASH block 800 arithmetic ops and 1072 lookups instead of 10 880 and 4 480.
//
// Every input byte must be a range-checked ByteTarget (a lookup output, add_virtual_byte_target, or a byte constant), as for
// byte_xor: a table index x * 256 + y names one pair (x, y) only when both are bytes.  AesGcmTarget's h and ciphertext bytes are
// XOR-table outputs and its padding and length bytes constants, so they qualify.
struct ClmulAccumulator {
    std::array<std::vector<ByteTarget>, 32> early, late;  // per byte position: pieces of products known early / of the one on the chain
};
// x[p] * y[q] for all (p, q): the low byte of each product goes to position p + q, the high byte to p + q + 1
inline void clmul_accumulate(CircuitBuilder& b, size_t lo_lut, size_t hi_lut, const BlockTarget& x, const BlockTarget& y,
                             std::array<std::vector<ByteTarget>, 32>& pos) {
    for (int p = 0; p < 16; p++)
        for (int q = 0; q < 16; q++) {
            Target idx = b.mul_const_add(1 << 8, x[p], y[q]);
            pos[p + q].push_back(b.add_lookup_from_index(idx, lo_lut));
            pos[p + q + 1].push_back(b.add_lookup_from_index(idx, hi_lut));
        }
}
// XOR of v as a balanced pairwise tree, ceil(log2(size)) byte_xors deep: the witness runs level by level, and a running sum of
// the 31 pieces of a middle position would be 30 deep.
inline ByteTarget xor_tree(CircuitBuilder& b, size_t xor_lut, std::vector<ByteTarget> v) {
    if (v.empty()) return zero_byte(b);
    while (v.size() > 1) {
        std::vector<ByteTarget> next;
        next.reserve((v.size() + 1) / 2);
        for (size_t i = 0; i + 1 < v.size(); i += 2) next.push_back(byte_xor(b, xor_lut, v[i], v[i + 1]));
        if (v.size() & 1) next.push_back(v.back());
        v.swap(next);
    }
    return v[0];
}
// The 32 sums, then the reduction: for k = 15 .. 1 and then 0, D[16 + k] * x^128 = D[16 + k] * 0xE1 goes to D[k] (low byte) and
// D[k + 1] (high byte).  k = 15 writes D[16], which k = 0 reads; hence k = 0 last.
inline BlockTarget clmul_fold(CircuitBuilder& b, size_t xor_lut, size_t lo_lut, size_t hi_lut, const ClmulAccumulator& acc) {
    std::array<ByteTarget, 32> d;
    for (int j = 0; j < 32; j++) {
        // the pieces that wait for the chain get a tree of their own, one XOR away from the result
        ByteTarget late = xor_tree(b, xor_lut, acc.late[j]);
        if (acc.early[j].empty()) {
            d[j] = late;
            continue;
        }
        ByteTarget early = xor_tree(b, xor_lut, acc.early[j]);
        d[j] = acc.late[j].empty() ? early : byte_xor(b, xor_lut, late, early);
    }
    ByteTarget r_first = byte_constant(b, 225);
    std::array<std::vector<ByteTarget>, 17> fold;
    auto reduce = [&](int k, ByteTarget top) {
        Target idx = b.mul_const_add(1 << 8, top, r_first);
        fold[k].push_back(b.add_lookup_from_index(idx, lo_lut));
        fold[k + 1].push_back(b.add_lookup_from_index(idx, hi_lut));
    };
    for (int k = 15; k >= 1; k--) reduce(k, d[16 + k]);
    fold[16].insert(fold[16].begin(), d[16]);
    reduce(0, xor_tree(b, xor_lut, fold[16]));
    BlockTarget z;
    for (int k = 0; k < 16; k++) {
        fold[k].insert(fold[k].begin(), d[k]);
        z[k] = xor_tree(b, xor_lut, fold[k]);
    }
    return z;
}
inline BlockTarget gf_2_128_mul_tables_target(CircuitBuilder& b, size_t xor_lut, size_t lo_lut, size_t hi_lut, const BlockTarget& x, const BlockTarget& y) {
    ClmulAccumulator acc;
    clmul_accumulate(b, lo_lut, hi_lut, x, y, acc.late);
    return clmul_fold(b, xor_lut, lo_lut, hi_lut, acc);
}
// GHASH_h(x).  lanes = 1 is the Horner chain y <- (y ^ x_i) * h.  With lanes = k the powers h^2 .. h^k are computed once and the
// blocks taken k at a time, y <- (y ^ x_1) h^k ^ x_2 h^(k-1) ^ .. ^ x_k h, all k products in ONE unreduced accumulator with one
// tree per position and one fold: the chain, which is what bounds witness generation for long inputs, is k times shorter.  A last
// group of r < k blocks uses h^r .. h.
inline BlockTarget ghash_tables_target(CircuitBuilder& b, size_t xor_lut, size_t lo_lut, size_t hi_lut, const BlockTarget& h,
                                       const std::vector<ByteTarget>& x, int lanes) {
    if (x.size() % 16 != 0) throw std::runtime_error("ghash input must be a multiple of 16 bytes");
    if (lanes < 1 || lanes > 16) throw std::runtime_error("ghash_tables: lanes must be 1 to 16");
    const size_t blocks = x.size() / 16;
    std::vector<BlockTarget> pw(2, h);  // pw[i] = h^i, from the two halves of i
    for (size_t i = 2; i <= std::min<size_t>((size_t)lanes, blocks); i++)
        pw.push_back(gf_2_128_mul_tables_target(b, xor_lut, lo_lut, hi_lut, pw[(i + 1) / 2], pw[i / 2]));
    ByteTarget zb = zero_byte(b);
    BlockTarget y;
    y.fill(zb);
    for (size_t g = 0; g < blocks; g += (size_t)lanes) {
        const size_t r = std::min<size_t>((size_t)lanes, blocks - g);
        ClmulAccumulator acc;
        for (size_t j = 0; j < r; j++) {
            BlockTarget xj;
            for (int k = 0; k < 16; k++) xj[k] = x[16 * (g + j) + k];
            if (j == 0) xj = xor_blocks(b, xor_lut, y, xj);
            clmul_accumulate(b, lo_lut, hi_lut, xj, pw[r - j], j == 0 ? acc.late : acc.early);
        }
        y = clmul_fold(b, xor_lut, lo_lut, hi_lut, acc);
    }
    return y;
}

// AesGcmTarget<NK, 4, NR, L, TAG> (circuit_gcm.rs:24-209)
struct AesGcmTarget {
    int NK, NR;
    size_t L;
    bool TAG;
    std::vector<ByteTarget> key, nonce, pt, ct, tag, aad;

    // aad_len > 0 (not in the reference, whose a = []): that many range-checked byte targets of additional authenticated data,
    // created after the tag targets so that aad_len = 0 numbers every target as before, and hashed in front of the ciphertext.
    static AesGcmTarget build(CircuitBuilder& b, int NK, int NR, size_t L, bool TAG, size_t aad_len = 0) {
        if (aad_len && !TAG) throw std::runtime_error("aad needs the tag");
        AesGcmTarget t;
        t.NK = NK;
        t.NR = NR;
        t.L = L;
        t.TAG = TAG;
        size_t sbox = sbox_lut(b), xorl = byte_xor_lut(b), mull = gf_2_8_mul_lut(b);
        for (int i = 0; i < NK * 4; i++) t.key.push_back(add_virtual_byte_target(b, sbox));
        for (int i = 0; i < 12; i++) t.nonce.push_back(add_virtual_byte_target(b, sbox));
        for (size_t i = 0; i < L; i++) t.pt.push_back(add_virtual_byte_target(b, sbox));
        for (size_t i = 0; i < TAG_LEN / 8; i++) t.tag.push_back(add_virtual_byte_target(b, sbox));
        for (size_t i = 0; i < aad_len; i++) t.aad.push_back(add_virtual_byte_target(b, sbox));
        StateTarget mix = state_mix_matrix(b);
        auto expanded_key = key_expansion_t(b, NK, NR, xorl, sbox, t.key);
        StateTarget es = empty_state(b);
        BlockTarget h = flatten(encrypt_block_t(b, NR, xorl, mull, sbox, mix, es, expanded_key));
        ByteTarget zb = zero_byte(b), ob = byte_constant(b, 1);
        BlockTarget j0;
        j0.fill(zb);
        for (int i = 0; i < 12; i++) j0[i] = t.nonce[i];
        j0[15] = ob;
        BlockTarget inc32_j0 = inc32_target(b, j0);
        t.ct = gctr_target(b, NR, xorl, mull, sbox, mix, expanded_key, inc32_j0, t.pt);
        if (!TAG) return t;
        size_t u = (16 - L % 16) % 16, v = (16 - aad_len % 16) % 16;
        uint64_t clen = (uint64_t)L * 8, alen = (uint64_t)aad_len * 8;
        std::vector<ByteTarget> gin(t.aad);
        if (aad_len)
            for (size_t i = 0; i < v; i++) gin.push_back(zb);
        gin.insert(gin.end(), t.ct.begin(), t.ct.end());
        for (size_t i = 0; i < u; i++) gin.push_back(zb);
        for (int i = 7; i >= 0; i--) gin.push_back(byte_constant(b, (uint8_t)(alen >> (8 * i))));
        for (int i = 7; i >= 0; i--) gin.push_back(byte_constant(b, (uint8_t)(clen >> (8 * i))));
        BlockTarget s;
        if (b.ghash_tables()) {
            // the two clmul tables INSTEAD of the shift and bit tables: a table nobody looks into cannot be built
            size_t lol = gcm_clmul_lo_lut(b), hil = gcm_clmul_hi_lut(b);
            s = ghash_tables_target(b, xorl, lol, hil, h, gin, b.ghash_tables());
        } else {
            size_t shl = u8_unit_right_shift_lut(b), brl = u8_bitref_lut(b);
            s = ghash_target(b, xorl, shl, brl, h, gin);
        }
        std::vector<ByteTarget> sv(s.begin(), s.end());
        auto msb_input = gctr_target(b, NR, xorl, mull, sbox, mix, expanded_key, j0, sv);
        for (size_t i = 0; i < TAG_LEN / 8; i++) b.connect(t.tag[i], msb_input[i]);
        return t;
    }
};

}  // namespace aes
}  // namespace p2
