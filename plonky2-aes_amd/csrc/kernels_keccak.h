// HIP kernels of the Keccak configuration (Config::hasher == HASHER_KECCAK; keccak_hash.h defines the hasher): the Merkle trees
// of the prover, the path walk of the batched verifier and the tree reconstruction of the compressor.  Each is the Keccak
// sibling of a Poseidon kernel and is launched in its place; the Poseidon kernels are untouched (their code generation is
// pinned by tests/test_codegen.py and tests/test_public_inputs_host.py, which select kernels by name fragments -- none of the
// fragments occurs in a name below).
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

__device__ __forceinline__ bool kcv_merkle(const u64* leaf, u32 width, u32 index, const u64* cap, u32 cap_n, const u64* sib, u32 depth) {
    u64 cur[4];
    kc::hash_no_pad(leaf, width, cur);
    for (u32 l = 0; l < depth; l++) {
        const u64* s = sib + 4 * (size_t)l;
        const bool right = index & 1;
        u64 lr[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            lr[i] = right ? s[i] : cur[i];
            lr[4 + i] = right ? cur[i] : s[i];
        }
        kc::two_to_one(lr, lr + 4, cur);
        index >>= 1;
    }
    const u64* c = cap + 4 * (size_t)(index & (cap_n - 1));
    return index < cap_n && cur[0] == c[0] && cur[1] == c[1] && cur[2] == c[2] && cur[3] == c[3];
}

// k_vfy_queries with the Keccak path walk: same slots, same checks, same failure keys.
__global__ __launch_bounds__(64) void k_kcv_queries(VerifyArgs a) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, slot = blockIdx.y, slots = gridDim.y;
    if (t >= a.batch * a.num_queries) return;
    const u32 p = t / a.num_queries, q = t % a.num_queries;
    const u64* w = a.words + (size_t)p * a.W;
    const u64* ch = a.chal + (size_t)p * CH_WORDS;
    const u64* vq = a.vq + (size_t)p * VQ_WORDS;
    const u64* qw = w + a.q_off + (size_t)q * a.q_stride;
    const u32 cap_n = 1u << a.cap_height;
    const u32 x_index = (u32)(ch[CH_QUERY + q] & (((u64)1 << a.lde_bits) - 1));
    const u32 key = (q * slots + slot) << 1;
    const u64 *leaf = nullptr, *cap = nullptr, *sib = nullptr;
    u32 width = 0, index = 0, depth = 0, mkey = key;
    if (slot < 4) {
        cap = slot == 0 ? a.vd : w + (size_t)(slot - 1) * a.cap_words;
        leaf = qw + a.init_eval_off[slot], width = a.init_width[slot], index = x_index, sib = qw + a.init_sib_off[slot], depth = a.init_depth;
    } else {
        const u64 subgroup_x0 = gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity((int)a.lde_bits), gl::bitrev(x_index, (int)a.lde_bits)));
        const u32 k = slot - 4;
        const E2 expect = vfy_expected(a, w, qw, k, x_index, subgroup_x0, ch, vq);
        if (k == a.num_rounds) {
            const u64 sx = gl::exp_pow2(subgroup_x0, (int)(VFY_ARITY_BITS * a.num_rounds));
            E2 fe = gl::e2(0);
            for (u32 i = a.final_len; i-- > 0;) fe = gl::add(gl::mul(fe, sx), vfy_e2(w, a.final_off + 2 * i));
            if (!gl::eq(fe, expect)) atomicMin(&a.qfail[p], key);
            return;
        }
        const u32 xk = x_index >> (VFY_ARITY_BITS * k), within = xk & (VFY_ARITY - 1);
        leaf = qw + a.step_eval_off[k];
        if (!gl::eq(vfy_e2(leaf, 2 * within), expect)) {
            atomicMin(&a.qfail[p], key);
            return;
        }
        cap = w + a.fri_caps_off + (size_t)k * a.cap_words, width = 2 * VFY_ARITY, index = xk >> VFY_ARITY_BITS;
        sib = qw + a.step_sib_off[k], depth = a.step_depth[k], mkey = key | 1;
    }
    if (!kcv_merkle(leaf, width, index, cap, cap_n, sib, depth)) atomicMin(&a.qfail[p], mkey);
}

// ------------------------------------------------------------------------------------------- compressed proofs
// k_cmp_merkle with the Keccak hasher; a stored sibling outside its range is NON_CANONICAL like one that is not below p.
__global__ __launch_bounds__(CMP_MAXQ) void k_kcc_merkle(CmpArgs a) {
    __shared__ u32 s_node[CMP_MAXQ], s_mask[CMP_MAXQ];
    __shared__ u64 s_cur[CMP_MAXQ][4], s_sib[CMP_MAXQ][4];
    const VerifyArgs& v = a.v;
    const u32 p = blockIdx.x, slot = blockIdx.y, q = threadIdx.x, Q = v.num_queries;
    const CmpPlan& pl = a.plan[p];
    if (pl.len == 0) return;  // (uniform over the workgroup)
    const bool mine = q < Q;
    const u32 t = slot < 4 ? 0 : slot - 3, depth = cmp_depth(v, t);
    u64* qw = v.words + (size_t)p * v.W + v.q_off + (size_t)(mine ? q : 0) * v.q_stride;
    u64* sib_out = qw + (slot < 4 ? v.init_sib_off[slot] : v.step_sib_off[slot - 4]);
    const u32 mask = mine ? pl.mask[t][q] : 0;
    const u32 leaf = mine ? pl.idx[q] >> cmp_shift(t) : 0xFFFFFFFFu;
    const uint8_t* stored = a.cproofs + (size_t)p * v.proof_bytes + (mine ? pl.off[t][q] + cmp_sib_at(a, slot, __popc(mask)) : 0);
    u64 cur[4];
    if (slot < 4) kc::hash_no_pad(qw + v.init_eval_off[slot], v.init_width[slot], cur);
    else kc::hash_no_pad(qw + v.step_eval_off[slot - 4], 2 * VFY_ARITY, cur);
    s_mask[q] = mask;
    for (u32 l = 0; l < depth; l++) {
        const u32 node = leaf >> l;
        s_node[q] = mine ? node : 0xFFFFFFFFu;
        for (int i = 0; i < 4; i++) s_cur[q][i] = cur[i];
        if ((mask >> l) & 1) {
            const uint8_t* b = stored + 32 * __popc(mask & ((1u << l) - 1));
            u64 y[4];
            for (int i = 0; i < 4; i++) {
                y[i] = vfy_ld_bytes(b + 8 * i);
                s_sib[q][i] = y[i];
            }
            if (!kc::in_range(y)) atomicOr(&v.flags[p], (u32)VF_NONCANON);
        }
        __syncthreads();
        u64 sb[4] = {0, 0, 0, 0};
        if (mine) {
            if ((mask >> l) & 1) {
                for (int i = 0; i < 4; i++) sb[i] = s_sib[q][i];
            } else {
                u32 from = CMP_MAXQ;
                bool on_path = false;
                for (u32 e = 0; e < Q && from == CMP_MAXQ; e++)
                    if (s_node[e] == (node ^ 1)) from = e, on_path = true;
                for (u32 e = 0; e < q && from == CMP_MAXQ; e++)
                    if (s_node[e] == node && ((s_mask[e] >> l) & 1)) from = e;
                if (from < CMP_MAXQ)
                    for (int i = 0; i < 4; i++) sb[i] = on_path ? s_cur[from][i] : s_sib[from][i];
            }
            for (int i = 0; i < 4; i++) sib_out[4 * l + i] = sb[i];
            u64 lr[8];
            const bool right = node & 1;
            for (int i = 0; i < 4; i++) {
                lr[i] = right ? sb[i] : cur[i];
                lr[4 + i] = right ? cur[i] : sb[i];
            }
            kc::two_to_one(lr, lr + 4, cur);
        }
        __syncthreads();
    }
}

}  // namespace p2k
