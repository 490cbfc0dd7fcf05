// The Poseidon sponge cipher in GPU batches (poseidon_cipher.h has the scheme and the host twins; include/p2aes.h the entry
// points).  One thread per message, 64 threads per block; the whole cost is Poseidon: one hash_state is
// hash_n_to_m_no_pad(20 words, 20) from a fresh state, three absorbing permutations and two that squeeze, per three Fq elements.
// So the sponge step runs on the block-form permutation with what the tree kernels' sponge already leaves out
// (glf::permute_known_any): the S-boxes of the zero capacity in front of the first chunk, and the last round's MDS rows of
// outputs that the next chunk overwrites or that nobody reads.  Every value stays canonical, so outputs are the host's word for
// word.  A thread walks its own row of msg / ct, 15 words per five permutations: these loads do not coalesce and are left so.
#pragma once
#include "poseidon_fast.h"

namespace p2k {
using gl::u32;
using gl::u64;

// pcipher::hash_state on s = (s0 | s1 | s2 | s3), 20 canonical words in, 20 out.  The five permutations are trips of ONE loop, so
// a kernel holds one copy of the permutation; which words move between s and the sponge state is a uniform switch on the trip,
// and every index is a constant.  (A switch, not an if / else-if chain: with the chain the device build returned wrong words
// h[16..20) while the host build of the same text was right -- DESIGN.md section 9j.)  Overwrite mode: the chunk at word 8
// overwrites words 0..7, the four-word chunk at word 16 words 0..3, and each absorbing permutation computes only the rows its
// successor's chunk leaves standing.  The two
// permutations that feed another one and are read themselves (the third and fourth) compute all rows, the fifth rows 0..3.
// `last` (uniform): the caller reads s1 = h[5..10) only.  Then the fourth permutation computes rows 0..1, the fifth is not run,
// and the other fifteen words of s are left as they were.
GL_HD void pcipher_hash_state(u64 s[20], bool last) {
    u64 st[12];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = s[i];
#pragma unroll
    for (int i = 8; i < 12; i++) st[i] = 0;  // never read: FR_ZERO_CAP
    const int trips = last ? 4 : 5;
#pragma nounroll
    for (int p = 0; p < trips; p++) {
        const u32 kind = p == 0 ? (u32)glf::FR_ZERO_CAP : (u32)glf::FR_GENERAL;
        const u32 rows = p == 0 ? glf::rows_before_chunk(20 - 8) : p == 1 ? glf::rows_before_chunk(20 - 16) : p == 2 ? (u32)glf::ROWS_ALL
                         : p == 3 ? (last ? 0x003u : (u32)glf::ROWS_ALL) : (u32)glf::ROWS_DIGEST;
        glf::permute_known_any<true>(st, kind, rows);
        switch (p) {
        case 0:
#pragma unroll
            for (int i = 0; i < 8; i++) st[i] = s[8 + i];
            break;
        case 1:
#pragma unroll
            for (int i = 0; i < 4; i++) st[i] = s[16 + i];
            break;
        case 2:
            if (last) {
#pragma unroll
                for (int i = 5; i < 8; i++) s[i] = st[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) s[i] = st[i];
            }
            break;
        case 3:
            if (last) {
                s[8] = st[0], s[9] = st[1];
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) s[8 + i] = st[i];
            }
            break;
        default:
#pragma unroll
            for (int i = 0; i < 4; i++) s[16 + i] = st[i];
            break;
        }
    }
}

#if defined(__HIPCC__) && !defined(P2_PCIPHER_SPONGE_ONLY)  // capi_host.cpp takes the sponge step alone: the kernels live in prover_gpu.hip
// the cipher's opening state: s = [0, ks.x, ks.u, (nonce0, nonce1, l, 0, 0)]; false: a word of ks or nonce is not below p
GL_D bool pcipher_init(u64 s[20], const u64* __restrict__ ks, const u64* __restrict__ nonce, u32 l) {
    bool ok = true;
#pragma unroll
    for (int w = 0; w < 5; w++) s[w] = 0;
#pragma unroll
    for (int w = 0; w < 10; w++) s[5 + w] = ks[w], ok &= ks[w] < gl::P;
    s[15] = nonce[0], s[16] = nonce[1], s[17] = l, s[18] = 0, s[19] = 0;
    return ok & (nonce[0] < gl::P) & (nonce[1] < gl::P);
}
GL_D void pcipher_zero_row(u64* __restrict__ o, u32 n) {
#pragma nounroll
    for (u32 w = 0; w < n; w++) o[w] = 0;
}

// ct[i] = encrypt(ks[i], msg[i], nonce[i]) (lib.rs:41): the message padded with zeros to blocks of three, per block hash_state,
// s[1..3] += m, ct = s[1..3]; then the closing hash_state's s[1] as the tag.  Rows: ks 10 words, nonce 2, msg 5 l,
// ct 5 (3 blocks + 1).  status 0, or 2 (row zeroed) for a word of ks, nonce or msg not below p.
__global__ __launch_bounds__(64) void k_pcipher_encrypt(const u64* __restrict__ ks, const u64* __restrict__ nonce, const u64* __restrict__ msg, u32 l, size_t count,
                                                        u64* __restrict__ ct, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u32 blocks = (l + 2) / 3, ct_words = 15 * blocks + 5;
    const u64* m = msg + i * (size_t)(5 * l);
    u64* c = ct + i * (size_t)ct_words;
    u64 s[20];
    bool ok = pcipher_init(s, ks + 10 * i, nonce + 2 * i, l);
#pragma nounroll
    for (u32 b = 0; ok; b++) {
        const bool last = b == blocks;
        pcipher_hash_state(s, last);
        if (last) break;
        const u32 n = min(15u, 5 * l - 15 * b);  // the words of this block that the message has
#pragma unroll
        for (u32 w = 0; w < 15; w++) {
            const u64 v = w < n ? m[15 * b + w] : 0;
            ok &= v < gl::P;
            s[5 + w] = gl::add(s[5 + w], v);
            c[15 * b + w] = s[5 + w];
        }
    }
    if (ok) {
#pragma unroll
        for (u32 w = 0; w < 5; w++) c[15 * blocks + w] = s[5 + w];
    } else {
        pcipher_zero_row(c, ct_words);
    }
    status[i] = ok ? 0 : 2;
}

// msg[i] = decrypt(ks[i], ct[i], nonce[i], l) (lib.rs:75): per block hash_state, m = ct - s[1..3], s[1..3] = ct; the padding
// elements m[l..) must be zero, which the reference asserts only when l > 3; the closing hash_state's s[1] must equal the tag.
// Rows as k_pcipher_encrypt's; msg has 5 l words.  status 0; 1 (row zeroed) where the reference's asserts fail; 2 (row zeroed)
// for a word of ks, nonce or ct not below p.
__global__ __launch_bounds__(64) void k_pcipher_decrypt(const u64* __restrict__ ks, const u64* __restrict__ nonce, const u64* __restrict__ ct, u32 l, size_t count,
                                                        u64* __restrict__ msg, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u32 blocks = (l + 2) / 3, ct_words = 15 * blocks + 5;
    const u64* c = ct + i * (size_t)ct_words;
    u64* m = msg + i * (size_t)(5 * l);
    u64 s[20];
    bool ok = pcipher_init(s, ks + 10 * i, nonce + 2 * i, l);
    u64 pad = 0;  // the OR of the padding words
#pragma nounroll
    for (u32 b = 0; ok; b++) {
        const bool last = b == blocks;
        pcipher_hash_state(s, last);
        if (last) break;
        const u32 n = min(15u, 5 * l - 15 * b);
#pragma unroll
        for (u32 w = 0; w < 15; w++) {
            const u64 v = c[15 * b + w];
            ok &= v < gl::P;
            const u64 d = gl::sub(v, s[5 + w]);
            s[5 + w] = v;
            if (w < n)
                m[15 * b + w] = d;
            else
                pad |= d;
        }
    }
    bool good = l <= 3 || pad == 0;
    if (ok) {
#pragma unroll
        for (u32 w = 0; w < 5; w++) {
            const u64 t = c[15 * blocks + w];
            ok &= t < gl::P;
            good &= t == s[5 + w];
        }
    }
    const int st = !ok ? 2 : good ? 0 : 1;
    if (st) pcipher_zero_row(m, 5 * l);
    status[i] = st;
}
#endif

}  // namespace p2k
