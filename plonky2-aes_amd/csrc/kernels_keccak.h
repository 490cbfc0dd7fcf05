// HIP kernels of the Keccak configuration (Config::hasher == HASHER_KECCAK; keccak_hash.h defines the hasher), each launched in
// place of a Poseidon kernel.  The prover's tree kernels and the range check are kernels of their own: the Poseidon ones are
// hand-scheduled around their sponge and share nothing with a 25-lane state.  The path walk of the batched verifier and the
// tree reconstruction of the compressor are the bodies of kernels_verify.h / kernels_compress.h instantiated with the
// KeccakTree policy below.  The code generation of the Poseidon kernels is pinned by tests/test_codegen.py and
// tests/test_public_inputs_host.py, which select kernels by name fragments: none of the fragments may occur in a kernel name
// below, so the two instantiations are non-template kernels with names of their own.
//
// One thread = one sponge: 25 lanes = 50 VGPRs of state, a round is 32-bit logic throughout (xor, v_bfi_b32 for chi,
// v_alignbit_b32 for rho), the round loop is not unrolled.  All stores are vector stores; the round constants come from
// __constant__ memory.
#pragma once
#include "kernels_compress.h"
#include "keccak_hash.h"

namespace p2k {
namespace kc = p2::kc;

// ------------------------------------------------------------------------------------------- prover: trees
// Leaf digests of a column-major batch (the job of k_hash_leaves): digest[leaf] = hash_no_pad(row `leaf` of `cols` columns),
// columns >= active_cols known-zero and never loaded.  17 words per permutation, the pad bits folded into the last block.
__global__ __launch_bounds__(256) void k_kc_leaves(const u64* __restrict__ data, int cols, int active_cols, size_t col_stride, size_t batch_stride,
                                                   size_t num_leaves, u64* __restrict__ digests, size_t dig_batch_stride) {
    const size_t leaf = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (leaf >= num_leaves) return;
    const u64* d = data + (size_t)blockIdx.y * batch_stride + leaf;
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
    const u32 n = (u32)cols, blocks = n / kc::RATE_WORDS + 1;
    for (u32 b = 0; b < blocks; b++) {
        u64 w[kc::RATE_WORDS];
#pragma unroll
        for (u32 k = 0; k < kc::RATE_WORDS; k++) {  // the loads of a block issue together, in front of the first xor
            const u32 c = kc::RATE_WORDS * b + k;
            w[k] = (c < (u32)active_cols && c < n) ? d[(size_t)k * col_stride] : 0;
        }
#pragma unroll
        for (u32 k = 0; k < kc::RATE_WORDS; k++) s[k] ^= kc::pad_word(w[k], kc::RATE_WORDS * b + k, n, blocks);
        d += kc::RATE_WORDS * col_stride;
        kc::permute(s);
    }
    u64 h[4];
    kc::pack_digest(s, h);
    u64* out = digests + (size_t)blockIdx.y * dig_batch_stride + leaf * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = h[i];
}

// FRI commit-phase leaves (the job of k_hash_fri_leaves): leaf t = `arity` consecutive extension values, flattened (c0, c1);
// arity 16 is 32 words, two permutations.
__global__ __launch_bounds__(256) void k_kc_fri_leaves(const u64* __restrict__ vals, size_t len, size_t batch_stride, int arity, u64* __restrict__ digests,
                                                       size_t dig_batch_stride) {
    const size_t leaf = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (leaf >= len / arity) return;
    const u64* v = vals + (size_t)blockIdx.y * batch_stride + leaf * arity;
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
    const u32 n = 2 * (u32)arity, blocks = n / kc::RATE_WORDS + 1;
    for (u32 b = 0; b < blocks; b++) {
#pragma unroll
        for (u32 k = 0; k < kc::RATE_WORDS; k++) {
            const u32 e = kc::RATE_WORDS * b + k;
            s[k] ^= kc::pad_word(e < n ? v[(size_t)(e & 1) * len + (e >> 1)] : 0, e, n, blocks);
        }
        kc::permute(s);
    }
    u64 h[4];
    kc::pack_digest(s, h);
    u64* out = digests + (size_t)blockIdx.y * dig_batch_stride + leaf * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = h[i];
}

// One Merkle level (the job of k_merkle_level): parent[i] = two_to_one(child[2i], child[2i+1]).
__global__ __launch_bounds__(256) void k_kc_level(const u64* __restrict__ child, u64* __restrict__ parent, size_t num_parents, size_t batch_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_parents) return;
    const u64* c = child + (size_t)blockIdx.y * batch_stride + 8 * i;
    u64 in[8], h[4];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = c[k];
    kc::two_to_one(in, in + 4, h);
    u64* o = parent + (size_t)blockIdx.y * batch_stride + 4 * i;
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = h[k];
}

// ------------------------------------------------------------------------------------------- verifier
// The range check of a Keccak proof's hash words: hash_idx[i] is the word index of hash i (the caps first, then every sibling).
// A word outside its range is a NON_CANONICAL verdict, with the precedence canonicality has (k_vfy_finish).
__global__ __launch_bounds__(256) void k_kcv_range(VerifyArgs a, const u32* __restrict__ hash_idx, u32 count) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (i >= count) return;
    if (!kc::in_range(a.words + (size_t)p * a.W + hash_idx[i])) atomicOr(&a.flags[p], (u32)VF_NONCANON);
}

// The tree hasher as the path walks use it: the members of PoseidonTree (kernels_verify.h)
struct KeccakTree {
    static __device__ __forceinline__ void hash_or_noop(const u64* in, u32 len, u64* out) { kc::hash_no_pad(in, len, out); }
    static __device__ __forceinline__ void compress(u64* cur, const u64* sib, bool right) {
        u64 lr[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            lr[i] = right ? sib[i] : cur[i];
            lr[4 + i] = right ? cur[i] : sib[i];
        }
        kc::two_to_one(lr, lr + 4, cur);
    }
    static __device__ __forceinline__ bool valid(const u64* h) { return kc::in_range(h); }
};

// k_vfy_queries and k_cmp_merkle with the Keccak hasher
__global__ __launch_bounds__(64) void k_kcv_queries(VerifyArgs a) { vfy_queries<KeccakTree>(a); }
__global__ __launch_bounds__(CMP_MAXQ) void k_kcc_merkle(CmpArgs a) { cmp_merkle<KeccakTree>(a); }

}  // namespace p2k
