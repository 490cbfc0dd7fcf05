// The tree hasher of KeccakGoldilocksConfig (upstream plonky2 hash/keccak.rs, KeccakHash<25>, as recalled), defined once for the
// host verifier, the host compressor and the device kernels (kernels_keccak.h).
//
//   hash_no_pad(words)  = first 25 bytes of Keccak-256 (original padding 0x01 .. 0x80, rate 136 bytes = 17 words) over the words
//                         as 8-byte little-endian values
//   two_to_one(l, r)    = first 25 bytes of Keccak-256 over l's 25 bytes || r's 25 bytes (one permutation)
//
// A 25-byte digest is carried as upstream's BytesHash<25>::to_vec form: four field elements holding bytes 0-6, 7-13, 14-20 and
// 21-24, little-endian (each below 2^56, the last below 2^32), so a hash stays four words everywhere a Poseidon hash is four
// words.  two_to_one reads only the low 7 (4) bytes of each word: a verifier must reject a word outside its range (in_range)
// or one proof would have many accepted encodings.
//
// The same permutation serves keccak256(bytes) on the host: plonky2 tags every LookupGate / LookupTableGate with the Keccak-256
// of its table and the hash is part of the gate's id(), which builder.h needs to sort the gate types as upstream does.
#pragma once
#include <string.h>

#include <array>
#include <utility>
#include <vector>

#include "gl.h"

namespace p2 {
namespace kc {
using gl::u32;
using gl::u64;

static const u32 RATE_WORDS = 17;
#define P2_KECCAK_RC                                                                                                                    \
    {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull, \
     0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull, \
     0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, \
     0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull}
static const u64 RC_HOST[24] = P2_KECCAK_RC;
#if defined(__HIPCC__)
static __constant__ u64 RC_DEV[24] = P2_KECCAK_RC;
#endif
#undef P2_KECCAK_RC

GL_HD u64 round_constant(int r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return RC_DEV[r];
#else
    return RC_HOST[r];
#endif
}

// rotation by a compile-time amount; on the device two v_alignbit_b32 per 64-bit lane
template <int R>
GL_HD u64 rotl(u64 v) {
    if (R == 0) return v;
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = (u32)v, hi = (u32)(v >> 32);
    if (R == 32) return ((u64)lo << 32) | hi;
    const u32 a = R < 32 ? hi : lo, b = R < 32 ? lo : hi;  // the rotation by R mod 32 of (a:b)
    const u32 s = 32 - (R & 31);
    return ((u64)__builtin_amdgcn_alignbit(a, b, s) << 32) | __builtin_amdgcn_alignbit(b, a, s);
#else
    return (v << (R & 63)) | (v >> ((64 - R) & 63));
#endif
}

// rho offset of lane x + 5 y
constexpr int rho_offset(int i) {
    const int t[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return t[i];
}

// theta's column parities applied, then rho and pi: lane I = x + 5 y goes to y + 5 ((2 x + 3 y) mod 5)
template <int I>
GL_HD void rho_pi(const u64* s, const u64* d, u64* b) {
    constexpr int x = I % 5, y = I / 5;
    b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl<rho_offset(I)>(s[I] ^ d[x]);
}
template <int... I>
GL_HD void rho_pi_all(const u64* s, const u64* d, u64* b, std::integer_sequence<int, I...>) {
    const int unused[] = {(rho_pi<I>(s, d, b), 0)...};
    (void)unused;
}

GL_HD void keccak_round(u64* s, u64 rc) {
    u64 c[5], d[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rotl<1>(c[(x + 1) % 5]);
    rho_pi_all(s, d, b, std::make_integer_sequence<int, 25>());
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) s[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    s[0] ^= rc;
}

// Keccak-f[1600].  The round loop stays a loop on the device: one round is ~300 32-bit instructions, 24 of them unrolled would
// be 7 k instructions per call site for nothing (the round constant is a scalar load either way).
GL_HD void permute(u64* s) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < 24; r++) keccak_round(s, round_constant(r));
}

// the first 25 bytes of the state as four words of 7, 7, 7 and 4 bytes
GL_HD void pack_digest(const u64* s, u64* out) {
    const u64 M56 = (1ull << 56) - 1;
    out[0] = s[0] & M56;
    out[1] = ((s[0] >> 56) | (s[1] << 8)) & M56;
    out[2] = ((s[1] >> 48) | (s[2] << 16)) & M56;
    out[3] = ((s[2] >> 40) | (s[3] << 24)) & 0xFFFFFFFFull;
}
GL_HD bool in_range(const u64* h) { return ((h[0] | h[1] | h[2]) >> 56) == 0 && (h[3] >> 32) == 0; }

// word `c` of the padded message of `n` words in `blocks` rate blocks: 0x01 right behind the message, 0x80 in the last byte
GL_HD u64 pad_word(u64 w, u32 c, u32 n, u32 blocks) {
    if (c == n) w ^= 0x01;
    if (c == RATE_WORDS * blocks - 1) w ^= 0x80ull << 56;
    return w;
}

GL_HD void hash_no_pad(const u64* in, u32 n, u64* out) {
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
    const u32 blocks = n / RATE_WORDS + 1;  // n = 0 mod 17: a block of padding alone
    for (u32 b = 0; b < blocks; b++) {
#pragma unroll
        for (u32 k = 0; k < RATE_WORDS; k++) {
            const u32 c = RATE_WORDS * b + k;
            s[k] ^= pad_word(c < n ? in[c] : 0, c, n, blocks);
        }
        permute(s);
    }
    pack_digest(s, out);
}

// l and r in range (in_range): their 50 bytes are lanes 0 .. 6.25 of one block
GL_HD void two_to_one(const u64* l, const u64* r, u64* out) {
    u64 s[25];
    s[0] = l[0] | (l[1] << 56);
    s[1] = (l[1] >> 8) | (l[2] << 48);
    s[2] = (l[2] >> 16) | (l[3] << 40);
    s[3] = (l[3] >> 24) | (r[0] << 8);
    s[4] = r[1] | (r[2] << 56);
    s[5] = (r[2] >> 8) | (r[3] << 48);
    s[6] = (r[3] >> 16) | (0x01ull << 16);
#pragma unroll
    for (int i = 7; i < 25; i++) s[i] = 0;
    s[16] = 0x80ull << 56;
    permute(s);
    pack_digest(s, out);
}

// Keccak-256 of a byte string (host; lanes are little-endian words of the message, as everywhere above)
static inline std::array<uint8_t, 32> keccak256(const uint8_t* data, size_t len) {
    const size_t RATE = 8 * RATE_WORDS;
    std::vector<uint8_t> msg(data, data + len);
    msg.push_back(0x01);
    msg.resize((msg.size() + RATE - 1) / RATE * RATE, 0);
    msg.back() |= 0x80;
    u64 s[25] = {0};
    for (size_t off = 0; off < msg.size(); off += RATE) {
        for (size_t i = 0; i < RATE_WORDS; i++) {
            u64 w;
            memcpy(&w, &msg[off + 8 * i], 8);
            s[i] ^= w;
        }
        permute(s);
    }
    std::array<uint8_t, 32> out;
    memcpy(out.data(), s, 32);
    return out;
}

}  // namespace kc
}  // namespace p2
