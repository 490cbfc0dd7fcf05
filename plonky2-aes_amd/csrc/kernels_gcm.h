// AES-GCM in GPU batches (aes_gadgets.h has the host twins gcm_encrypt_aad / gcm_decrypt; include/p2aes.h the entry points;
// DESIGN.md section 9k the decomposition and its figures).  32-bit table work, no field arithmetic: the AES rounds read one
// T-table (256 words: the S-box and its MixColumns multiples, the other three tables being its rotations) from LDS, and GHASH
// multiplies by a fixed element through its 4-bit Shoup table (16 entries of 16 bytes), also in LDS.
//
// Three launches per call, over a per-item workspace that k_gcm_setup fills:
//   k_gcm_setup      one thread per item: round keys, H = E_K(0^128), E_K(J0), the nonce as words, the Shoup table of H
//   k_gcm_ctr        one thread per 16-byte block of the message, grid over count x ceil(len / 16)
//   k_gcm_ghash<L>   L = 1: one thread per item, Horner's rule with H; L = 64: one wave per item, lane j folds blocks j, j + 64, ..
//                    with H^64, pays the power of H its last block is owed, and the wave xors its partials together
// Encryption runs ctr then ghash (over the ciphertext it wrote); decryption ghash first, which writes the status, and then ctr,
// which zeroes the rows of rejected items.
//
// A block is two 64-bit halves in GCM's order: hi = bytes 0..7 big-endian, so bit 63 of hi is the coefficient of x^0.
#pragma once
#include <stdint.h>

#include "gl.h"

namespace p2k {
using gl::u32;
using gl::u64;

// ---- the workspace of one item, in 32-bit words; every part starts at a multiple of 16 bytes
GL_HD u32 gcm_ws_rk() { return 0; }                               // 4 (nr + 1) round-key words, a column's byte r in bits 8 r ..
GL_HD u32 gcm_ws_h(int nr) { return 4 * ((u32)nr + 1); }          // H, four words as the cipher leaves them
GL_HD u32 gcm_ws_ej0(int nr) { return gcm_ws_h(nr) + 4; }         // E_K(J0), the same way
GL_HD u32 gcm_ws_nonce(int nr) { return gcm_ws_h(nr) + 8; }       // the nonce's three words and one of padding
GL_HD u32 gcm_ws_table(int nr) { return gcm_ws_h(nr) + 12; }      // Shoup table of H: 16 entries of (hi.hi, hi.lo, lo.hi, lo.lo)
GL_HD u32 gcm_ws_words(int nr) { return gcm_ws_h(nr) + 12 + 64; }

struct Gf128 {
    u64 hi, lo;
};
GL_HD Gf128 gf128_xor(Gf128 a, Gf128 b) { return Gf128{a.hi ^ b.hi, a.lo ^ b.lo}; }
GL_HD u32 gcm_bswap32(u32 v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
GL_HD u32 gcm_rotl(u32 v, int s) { return (v << s) | (v >> (32 - s)); }
// four words as the cipher leaves them (byte k of the block in bits 8 (k % 4) of word k / 4) <-> the two halves
GL_HD Gf128 gf128_from_words(const u32 w[4]) {
    return Gf128{((u64)gcm_bswap32(w[0]) << 32) | gcm_bswap32(w[1]), ((u64)gcm_bswap32(w[2]) << 32) | gcm_bswap32(w[3])};
}
GL_HD void gf128_to_words(Gf128 v, u32 w[4]) {
    w[0] = gcm_bswap32((u32)(v.hi >> 32)), w[1] = gcm_bswap32((u32)v.hi), w[2] = gcm_bswap32((u32)(v.lo >> 32)), w[3] = gcm_bswap32((u32)v.lo);
}
// v x: one shift towards the higher powers, x^128 = 1 + x + x^2 + x^7 folded back in (the host's right_shift_one and 0xE1)
GL_HD Gf128 gf128_mulx(Gf128 v) {
    const u64 carry = 0 - (v.lo & 1);
    return Gf128{(v.hi >> 1) ^ (carry & 0xE100000000000000ull), (v.hi << 63) | (v.lo >> 1)};
}
// The general product, the host's 128-trip bit loop (aes::gf_2_128_mul): once per lane of the wide GHASH, never per block.
GL_HD Gf128 gf128_mul_bits(Gf128 x, Gf128 y) {
    Gf128 z{0, 0}, v = y;
    for (int i = 0; i < 128; i++) {
        const u64 bit = 0 - (((i < 64 ? x.hi : x.lo) >> (63 - (i & 63))) & 1);
        z.hi ^= v.hi & bit, z.lo ^= v.lo & bit;
        v = gf128_mulx(v);
    }
    return z;
}
// The Shoup table of a multiplier m: entry n = n(x) m for the sixteen polynomials of degree below 4, n's bit 3 the coefficient of
// x^0.  Entry n is four words at t[n * stride * 4 + k * stride], k = 0..3: stride 1 is an entry after the other, stride 64 with
// t offset by the thread is one bank per thread whichever entries a wave's threads read.
GL_HD void shoup_build(Gf128 m, u32* t, u32 stride) {
    Gf128 e[16];
    e[0] = Gf128{0, 0};
    e[8] = m;
    e[4] = gf128_mulx(e[8]), e[2] = gf128_mulx(e[4]), e[1] = gf128_mulx(e[2]);
    for (int i = 2; i <= 8; i *= 2)
        for (int j = 1; j < i; j++) e[i + j] = gf128_xor(e[i], e[j]);
    for (int n = 0; n < 16; n++) {
        u32* q = t + (size_t)n * 4 * stride;
        q[0] = (u32)(e[n].hi >> 32), q[stride] = (u32)e[n].hi, q[2 * stride] = (u32)(e[n].lo >> 32), q[3 * stride] = (u32)e[n].lo;
    }
}
GL_HD Gf128 shoup_entry(const u32* t, u32 stride, u32 n) {
    const u32* q = t + (size_t)n * 4 * stride;
    return Gf128{((u64)q[0] << 32) | q[stride], ((u64)q[2 * stride] << 32) | q[3 * stride]};
}
// x m from m's table: x's 32 nibbles from the highest power down, the running product shifted four powers up between them and
// the four coefficients that leave folded back: their polynomial times 0xE1 << 120, which is the carry-less product with 0x1C2
// placed at bit 48 of hi.
GL_HD Gf128 shoup_mul(Gf128 x, const u32* t, u32 stride) {
    Gf128 z = shoup_entry(t, stride, (u32)x.lo & 15);
    for (int k = 1; k < 32; k++) {
        const u32 rem = (u32)z.lo & 15;
        z.lo = (z.hi << 60) | (z.lo >> 4);
        z.hi = (z.hi >> 4) ^ ((u64)((rem << 5) ^ (rem << 10) ^ (rem << 11) ^ (rem << 12)) << 48);
        const u32 n = (u32)((k < 16 ? x.lo >> (4 * k) : x.hi >> (4 * (k - 16))) & 15);
        z = gf128_xor(z, shoup_entry(t, stride, n));
    }
    return z;
}

// ---- AES.  te[x] = (2 S(x), S(x), S(x), 3 S(x)) in bytes 0..3: what MixColumns makes of a row-0 byte; row r takes it rotated
// left by 8 r bits, and S(x) itself is byte 1.
GL_HD u32 aes_te0(u32 sbox_byte) {
    const u32 s = sbox_byte, s2 = ((s << 1) ^ ((s >> 7) * 0x11b)) & 0xff;
    return s2 | (s << 8) | (s << 16) | ((s2 ^ s) << 24);
}
GL_HD u32 aes_sub_word(const u32* te, u32 w) {
    return ((te[w & 0xff] >> 8) & 0xff) | (te[(w >> 8) & 0xff] & 0xff00) | ((te[(w >> 16) & 0xff] << 8) & 0xff0000) | ((te[w >> 24] << 16) & 0xff000000u);
}
// aes::key_expansion: rk[i] is word i, key byte 4 i + j in bits 8 j
GL_HD void aes_expand_key(const u32* te, int nk, int nr, const uint8_t* key, u32* rk) {
    for (int i = 0; i < nk; i++) rk[i] = (u32)key[4 * i] | ((u32)key[4 * i + 1] << 8) | ((u32)key[4 * i + 2] << 16) | ((u32)key[4 * i + 3] << 24);
    u32 rcon = 1;
    for (int i = nk; i < 4 * (nr + 1); i++) {
        u32 t = rk[i - 1];
        if (i % nk == 0) {
            t = aes_sub_word(te, (t >> 8) | (t << 24)) ^ rcon;
            rcon = ((rcon << 1) ^ ((rcon >> 7) * 0x11b)) & 0xff;
        } else if (nk > 6 && i % nk == 4) {
            t = aes_sub_word(te, t);
        }
        rk[i] = rk[i - nk] ^ t;
    }
}
// aes::encrypt_block on the four column words s
GL_HD void aes_encrypt(const u32* te, const u32* rk, int nr, u32 s[4]) {
    for (int c = 0; c < 4; c++) s[c] ^= rk[c];
    for (int r = 1; r < nr; r++) {
        u32 t[4];
#pragma unroll
        for (int c = 0; c < 4; c++)
            t[c] = te[s[c] & 0xff] ^ gcm_rotl(te[(s[(c + 1) & 3] >> 8) & 0xff], 8) ^ gcm_rotl(te[(s[(c + 2) & 3] >> 16) & 0xff], 16) ^
                   gcm_rotl(te[s[(c + 3) & 3] >> 24], 24) ^ rk[4 * r + c];
        for (int c = 0; c < 4; c++) s[c] = t[c];
    }
    u32 t[4];
    for (int c = 0; c < 4; c++)
        t[c] = (((te[s[c] & 0xff] >> 8) & 0xff) | (te[(s[(c + 1) & 3] >> 8) & 0xff] & 0xff00) | ((te[(s[(c + 2) & 3] >> 16) & 0xff] << 8) & 0xff0000) |
                ((te[s[(c + 3) & 3] >> 24] << 16) & 0xff000000u)) ^
               rk[4 * nr + c];
    for (int c = 0; c < 4; c++) s[c] = t[c];
}

#ifdef __HIPCC__
static __device__ const uint8_t GCM_SBOX[256] = {
#include "aes_sbox.inc"
};
// the T-table of a workgroup, any block size; the caller's barrier follows
GL_D void gcm_load_te(u32* te) {
    for (u32 i = threadIdx.x; i < 256; i += blockDim.x) te[i] = aes_te0(GCM_SBOX[i]);
}
GL_D void gcm_load16(const uint8_t* __restrict__ p, u32 avail, bool aligned, u32 w[4]) {
    if (aligned && avail >= 16) {
        const uint4 v = *(const uint4*)p;
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return;
    }
    for (int k = 0; k < 4; k++) w[k] = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++)
        if (k < avail) w[k >> 2] |= (u32)p[k] << (8 * (k & 3));
}
GL_D void gcm_store16(uint8_t* __restrict__ p, u32 avail, bool aligned, const u32 w[4]) {
    if (aligned && avail >= 16) {
        *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (u32 k = 0; k < 16; k++)
        if (k < avail) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

// key [count][4 nk], nonce [count][12] or NULL (then E_K(J0) is zero: the block-cipher test entry), h [count][16] or NULL: given,
// H is taken from it and no key is read (the GHASH test entry).
__global__ __launch_bounds__(64) void k_gcm_setup(const uint8_t* __restrict__ key, int nk, const uint8_t* __restrict__ nonce, const uint8_t* __restrict__ h,
                                                   size_t count, u32* __restrict__ ws) {
    __shared__ u32 te[256];
    gcm_load_te(te);
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int nr = nk + 6;
    u32* w = ws + i * gcm_ws_words(nr);
    u32 hw[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
    if (h) {
        gcm_load16(h + 16 * i, 16, false, hw);
    } else {
        aes_expand_key(te, nk, nr, key + (size_t)4 * nk * i, w + gcm_ws_rk());
        aes_encrypt(te, w + gcm_ws_rk(), nr, hw);
        if (nonce) {
            u32 nw[4];
            gcm_load16(nonce + 12 * i, 12, false, nw);
            for (int k = 0; k < 3; k++) w[gcm_ws_nonce(nr) + k] = e[k] = nw[k];
            w[gcm_ws_nonce(nr) + 3] = 0;
            e[3] = 0x01000000u;  // J0 = nonce || 0^31 || 1
            aes_encrypt(te, w + gcm_ws_rk(), nr, e);
        }
    }
    for (int k = 0; k < 4; k++) w[gcm_ws_h(nr) + k] = hw[k], w[gcm_ws_ej0(nr) + k] = e[k];
    shoup_build(gf128_from_words(hw), w + gcm_ws_table(nr), 1);
}

// out[item][16 b ..] = in[item][16 b ..] ^ E_K(nonce || b + 2), the last block as long as the message; rows `stride` bytes apart.
// ALIGNED: both bases and the stride are multiples of 16, whole blocks move as 128 bits.  gate (decryption) or NULL: an item
// whose gate word is not zero gets zeros.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_gcm_ctr(const u32* __restrict__ ws, int nk, const uint8_t* __restrict__ in, size_t len, size_t stride, size_t count,
                                                  const int* __restrict__ gate, uint8_t* __restrict__ out) {
    __shared__ u32 te[256];
    gcm_load_te(te);
    __syncthreads();
    const size_t blocks = (len + 15) / 16, g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= count * blocks) return;
    const size_t i = g / blocks, b = g % blocks;
    const int nr = nk + 6;
    const u32 avail = (u32)(len - 16 * b < 16 ? len - 16 * b : 16);
    uint8_t* o = out + i * stride + 16 * b;
    u32 s[4] = {0, 0, 0, 0};
    if (!gate || gate[i] == 0) {
        const u32* w = ws + i * gcm_ws_words(nr);
        u32 x[4];
        gcm_load16(in + i * stride + 16 * b, avail, ALIGNED, x);
        for (int k = 0; k < 3; k++) s[k] = w[gcm_ws_nonce(nr) + k];
        s[3] = gcm_bswap32((u32)b + 2);
        aes_encrypt(te, w + gcm_ws_rk(), nr, s);
        for (int k = 0; k < 4; k++) s[k] ^= x[k];
    }
    gcm_store16(o, avail, ALIGNED, s);
}

// What GHASH reads for an item: aad || 0^v || c || 0^u || [8 aad_len]_64 || [8 len]_64; raw: c alone, whole blocks (the test entry).
struct GhashIn {
    const uint8_t* aad;
    const uint8_t* c;
    size_t aad_len, len, stride;  // c rows are `stride` bytes apart, aad rows aad_len
    bool raw, aligned;            // aligned: c's base and stride are multiples of 16
};
GL_D size_t ghash_blocks(const GhashIn& in) { return in.raw ? in.len / 16 : (in.aad_len + 15) / 16 + (in.len + 15) / 16 + 1; }
GL_D Gf128 ghash_block(const GhashIn& in, size_t i, size_t b) {
    const size_t na = in.raw ? 0 : (in.aad_len + 15) / 16, nc = (in.len + 15) / 16;
    u32 w[4];
    if (b < na) {
        const size_t left = in.aad_len - 16 * b;
        gcm_load16(in.aad + i * in.aad_len + 16 * b, (u32)(left < 16 ? left : 16), false, w);
    } else if (b < na + nc) {
        const size_t left = in.len - 16 * (b - na);
        gcm_load16(in.c + i * in.stride + 16 * (b - na), (u32)(left < 16 ? left : 16), in.aligned, w);
    } else {
        return Gf128{(u64)in.aad_len * 8, (u64)in.len * 8};
    }
    return gf128_from_words(w);
}
// the end of an item: raw, out = the hash; else out = hash ^ E_K(J0) is the tag, written (given == NULL) or compared with given
GL_D void ghash_finish(const GhashIn& in, size_t i, Gf128 y, const u32* __restrict__ w, int nr, const uint8_t* __restrict__ given, uint8_t* __restrict__ out,
                       int* __restrict__ status) {
    u32 t[4];
    gf128_to_words(y, t);
    if (!in.raw)
        for (int k = 0; k < 4; k++) t[k] ^= w[gcm_ws_ej0(nr) + k];
    if (given) {
        u32 g[4], diff = 0;
        gcm_load16(given + 16 * i, 16, false, g);
        for (int k = 0; k < 4; k++) diff |= g[k] ^ t[k];
        status[i] = diff ? 1 : 0;
        return;
    }
    gcm_store16(out + 16 * i, 16, false, t);
    if (status) status[i] = 0;
}

template <int LANES>
__global__ __launch_bounds__(64) void k_gcm_ghash(const u32* __restrict__ ws, int nk, GhashIn in, size_t count, const uint8_t* __restrict__ given,
                                                   uint8_t* __restrict__ out, int* __restrict__ status);

// One thread per item.  Its table sits in LDS as [entry][word][thread]: a wave's threads read 64 consecutive words whichever
// entries they want, so no read conflicts.
template <>
__global__ __launch_bounds__(64) void k_gcm_ghash<1>(const u32* __restrict__ ws, int nk, GhashIn in, size_t count, const uint8_t* __restrict__ given,
                                                      uint8_t* __restrict__ out, int* __restrict__ status) {
    __shared__ u32 table[64 * 64];
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int nr = nk + 6;
    const u32* w = ws + i * gcm_ws_words(nr);
    u32* t = table + threadIdx.x;
    for (int k = 0; k < 64; k++) t[64 * k] = w[gcm_ws_table(nr) + k];
    const size_t n = ghash_blocks(in);
    Gf128 y{0, 0};
    for (size_t b = 0; b < n; b++) y = shoup_mul(gf128_xor(y, ghash_block(in, i, b)), t, 64);
    ghash_finish(in, i, y, w, nr, given, out, status);
}

// One wave per item.  The powers H^1 .. H^64 come from six doubling steps, each a table product by H^s for the lanes s .. 2 s - 1;
// lane j holds H^(j + 1).  The last of them, H^64, is the multiplier of every lane's Horner chain.
template <>
__global__ __launch_bounds__(64) void k_gcm_ghash<64>(const u32* __restrict__ ws, int nk, GhashIn in, size_t count, const uint8_t* __restrict__ given,
                                                       uint8_t* __restrict__ out, int* __restrict__ status) {
    __shared__ u32 table[64];
    __shared__ u32 pw[64 * 4];  // lane j's power H^(j + 1), as table entries are
    const size_t i = blockIdx.x;
    const u32 j = threadIdx.x;
    const int nr = nk + 6;
    const u32* w = ws + i * gcm_ws_words(nr);
    table[j] = w[gcm_ws_table(nr) + j];
    Gf128 p = shoup_entry(w + gcm_ws_table(nr), 1, 8);  // entry 8 is the multiplier itself: H
    for (u32 s = 1; s < 64; s *= 2) {
        // here `table` is H^s's and lanes below s hold their final power
        if (j < s) pw[4 * j] = (u32)(p.hi >> 32), pw[4 * j + 1] = (u32)p.hi, pw[4 * j + 2] = (u32)(p.lo >> 32), pw[4 * j + 3] = (u32)p.lo;
        __syncthreads();
        if (j >= s && j < 2 * s) p = shoup_mul(shoup_entry(pw, 1, j - s), table, 1);  // H^(j + 1) = H^(j + 1 - s) H^s
        __syncthreads();
        if (j == 2 * s - 1) shoup_build(p, table, 1);  // H^(2 s)
        __syncthreads();
    }
    pw[4 * j] = (u32)(p.hi >> 32), pw[4 * j + 1] = (u32)p.hi, pw[4 * j + 2] = (u32)(p.lo >> 32), pw[4 * j + 3] = (u32)p.lo;
    __syncthreads();
    const size_t n = ghash_blocks(in);
    Gf128 y{0, 0};
    if (j < n) {
        size_t b = j;
        y = ghash_block(in, i, b);
        for (b += 64; b < n; b += 64) y = gf128_xor(shoup_mul(y, table, 1), ghash_block(in, i, b));
        // b - 64 was this lane's last block, and block k of n is owed H^(n - k)
        y = gf128_mul_bits(y, shoup_entry(pw, 1, (u32)(n - (b - 64)) - 1));
    }
    u32 v[4] = {(u32)(y.hi >> 32), (u32)y.hi, (u32)(y.lo >> 32), (u32)y.lo};
    for (int m = 32; m >= 1; m >>= 1)
        for (int k = 0; k < 4; k++) v[k] ^= (u32)__shfl_xor((int)v[k], m, 64);
    if (j == 0) ghash_finish(in, i, Gf128{((u64)v[0] << 32) | v[1], ((u64)v[2] << 32) | v[3]}, w, nr, given, out, status);
}

// test entry: out[i] = E_key[i](in[i]), one thread per block
__global__ __launch_bounds__(64) void k_aes_encrypt_blocks(const u32* __restrict__ ws, int nk, const uint8_t* __restrict__ in, size_t count, uint8_t* __restrict__ out) {
    __shared__ u32 te[256];
    gcm_load_te(te);
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int nr = nk + 6;
    u32 s[4];
    gcm_load16(in + 16 * i, 16, false, s);
    aes_encrypt(te, ws + i * gcm_ws_words(nr) + gcm_ws_rk(), nr, s);
    gcm_store16(out + 16 * i, 16, false, s);
}

// out[i stride_words + j] = bytes[i byte_stride + j], j < row_bytes: a byte row as the ByteTarget segment of a value-matrix row
__global__ __launch_bounds__(256) void k_bytes_to_words(const uint8_t* __restrict__ bytes, size_t row_bytes, size_t byte_stride, size_t count, u64* __restrict__ out,
                                                         size_t stride_words) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= count * row_bytes) return;
    const size_t i = g / row_bytes, j = g % row_bytes;
    out[i * stride_words + j] = bytes[i * byte_stride + j];
}
#endif  // __HIPCC__

}  // namespace p2k
