// Batched leaf updates of a stand-alone Merkle tree (p2_merkle_tree_update*, include/p2aes.h; the definition is the sequential
// loop mt::host_update, merkle_host.h).  The k writes apply IN ORDER, and item j may ask for the path siblings it saw and the cap
// entry it left.  One after the other that is k * depth dependent permutations; here every level is one launch of independent ones.
//
//   k_mu_leaves      thread per item: status (0, 1 the index names no leaf, 2 a word not below p; any other than 0 raises the
//                    call's flag, behind which every later kernel returns without writing), key (index << 32) | j, v0[j] = the
//                    leaf's digest.  The keys are then sorted (rocPRIM radix sort, launched by the host code): A_0.
//   fast path (no trace): the sorted keys are grouped by index >> l at EVERY level l.
//   k_mu_fast_leaf   the last item of each leaf's group writes its digest to level 0: the last write wins.
//   k_mu_fast_level  the thread at the last position of a node's group rehashes the node from its two children, in place: every
//                    dirty node once, nothing else.
//   traced path: A_l is the items sorted by (index >> l, time); v_l[p] the digest of node index >> l as item A_l[p] left it.
//   k_mu_gather      thread per (item, level): the STORED sibling, what tree.prove gave before the call, into the trace row.
//   k_mu_step        thread per position p of A_l, item j in node N.  Two binary searches find the segment of the sibling node
//                    N ^ 1 and the rank r of time j in it: the sibling as of time j is v_l of that segment's entry r - 1 (written
//                    over the gathered one), or with r = 0 the stored digest, which the trace row already holds.  The parent's
//                    version v_{l+1} = two_to_one(ordered by bit l) goes to (start of the parent's range) + (own rank) + r: a
//                    merge by time of the two child segments, so A_{l+1} is sorted by (index >> (l + 1), time).  Because the
//                    gather has read every stored digest a step could want, steps never read the digest levels and the final
//                    version of a node (the last entry of its segment) is written back by the step that reads it as input; the
//                    last step also writes the cap and root_after.  v and A ping-pong between two buffers.
//   k_mu_roots       depth 0 only (the leaf digest is the cap entry): root_after[j] = v0[j].
// Hashes are counted per call: a wave-level sum, then one atomic add per wave (mu_count).  Hashing is the path walks' own
// (PoseidonTree::hash_or_noop, kernels_verify.h) and the tree levels' (glf::two_to_one_permute, k_merkle_level's).
#pragma once
#include "kernels_merkle.h"

namespace p2k {

// first word of node `node` of level l (merkle_build's layout, level_off in prover_gpu.hip)
__device__ __forceinline__ size_t mu_off(u32 bits, u32 l, u64 node) { return 4 * (((size_t)2 << bits) - ((size_t)2 << (bits - l))) + 4 * node; }
// Every thread of the block calls this (none has returned): lane 0 of each wave adds the wave's number of hashes.
__device__ __forceinline__ void mu_count(bool hashed, u64* counter) {
    const u64 m = __ballot(hashed);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(m));
}
// the first q in [lo, hi) whose node at level l is at least `node` (A_l is sorted by node first), or hi
__device__ __forceinline__ size_t mu_lower(const u64* a, size_t lo, size_t hi, u32 l, u64 node) {
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (((a[mid] >> 32) >> l) < node) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the first q in [lo, hi), one node's segment (sorted by time), whose time is at least `time`, or hi
__device__ __forceinline__ size_t mu_rank(const u64* a, size_t lo, size_t hi, u32 time) {
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((u32)a[mid] < time) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mu_leaves(const u64* __restrict__ indices, const u64* __restrict__ leaves, u32 leaf_len, u32 bits, size_t k, u64* __restrict__ keys,
                                                   u64* __restrict__ v0, int* __restrict__ status, u32* __restrict__ flag) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const u64 index = indices[j];
    const u64* leaf = leaves + j * leaf_len;
    int st = 0;
    if (index >> bits) st = 1;
    else {
        bool canonical = true;
        for (u32 w = 0; w < leaf_len; w++) canonical &= leaf[w] < gl::P;
        if (!canonical) st = 2;
    }
    status[j] = st;
    if (st) {
        atomicOr(flag, 1u);
        return;
    }
    keys[j] = (index << 32) | j;
    u64 h[4];
    PoseidonTree::hash_or_noop(leaf, leaf_len, h);
#pragma unroll
    for (int w = 0; w < 4; w++) v0[4 * j + w] = h[w];
}

__global__ __launch_bounds__(256) void k_mu_fast_leaf(const u64* __restrict__ keys, const u64* __restrict__ v0, size_t k, u64* __restrict__ dig, const u32* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= k || *flag) return;
    const u64 key = keys[p];
    if (p + 1 < k && (keys[p + 1] >> 32) == (key >> 32)) return;
    const u64* v = v0 + 4 * (size_t)(u32)key;
    u64* o = dig + 4 * (key >> 32);
#pragma unroll
    for (int w = 0; w < 4; w++) o[w] = v[w];
}

// level l >= 1 of the fast path: child = level l - 1, parent = level l of the digests
__global__ __launch_bounds__(256) void k_mu_fast_level(const u64* __restrict__ keys, size_t k, u32 l, const u64* __restrict__ child, u64* __restrict__ parent,
                                                       const u32* __restrict__ flag, u64* __restrict__ counter) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool last = p < k && !*flag;
    u64 node = 0;
    if (last) {
        node = (keys[p] >> 32) >> l;
        last = p + 1 == k || ((keys[p + 1] >> 32) >> l) != node;
    }
    if (last) {
        u64 st[12];
        const u64* c = child + 8 * node;
#pragma unroll
        for (int w = 0; w < 8; w++) st[w] = c[w];
#pragma unroll
        for (int w = 8; w < 12; w++) st[w] = 0;
        glf::two_to_one_permute(st);
        u64* o = parent + 4 * node;
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = st[w];
    }
    mu_count(last, counter);
}

// k_mt_paths' gather behind the call's flag: indices are known to be leaves here, and nothing may be written after a bad item
__global__ __launch_bounds__(256) void k_mu_gather(const u64* __restrict__ dig, u32 bits, u32 depth, const u64* __restrict__ indices, size_t k, u64* __restrict__ siblings,
                                                   size_t sib_stride, const u32* __restrict__ flag) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * depth || *flag) return;
    const size_t j = t / depth;
    const u32 l = (u32)(t - j * depth);
    const u64* s = dig + mu_off(bits, l, (indices[j] >> l) ^ 1);
    u64* o = siblings + j * sib_stride + 4 * l;
#pragma unroll
    for (int w = 0; w < 4; w++) o[w] = s[w];
}

// Step l of the traced path (see the head of the file).  by_time: v_in is v0, indexed by the items' times (l = 0); else by
// position in a_in.  last: l + 1 == depth, the parents are cap entries.
__global__ __launch_bounds__(256) void k_mu_step(const u64* __restrict__ a_in, const u64* __restrict__ v_in, size_t k, u32 l, u32 by_time, u32 last, u64* __restrict__ a_out,
                                                 u64* __restrict__ v_out, u64* __restrict__ dig, u32 bits, u64* siblings, size_t sib_stride, u64* root_after,
                                                 size_t root_stride, const u32* __restrict__ flag, u64* __restrict__ counter) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < k && !*flag;
    if (active) {
        const u64 key = a_in[p];
        const u32 j = (u32)key;
        const u64 node = (key >> 32) >> l, even = node & ~(u64)1;
        const bool right = node & 1;
        const size_t b0 = mu_lower(a_in, 0, k, l, even), b1 = mu_lower(a_in, b0, k, l, even + 1), b2 = mu_lower(a_in, b1, k, l, even + 2);
        const size_t own_lo = right ? b1 : b0, own_hi = right ? b2 : b1, sib_lo = right ? b0 : b1, sib_hi = right ? b1 : b2;
        const size_t r = mu_rank(a_in, sib_lo, sib_hi, j) - sib_lo;
        u64 own[4], sib[4];
        u64* row = siblings + (size_t)j * sib_stride + 4 * l;
        if (r) {
            const size_t q = sib_lo + r - 1;
            const u64* s = v_in + 4 * (by_time ? (size_t)(u32)a_in[q] : q);
#pragma unroll
            for (int w = 0; w < 4; w++) row[w] = sib[w] = s[w];
        } else {
#pragma unroll
            for (int w = 0; w < 4; w++) sib[w] = row[w];
        }
        const u64* v = v_in + 4 * (by_time ? (size_t)j : p);
#pragma unroll
        for (int w = 0; w < 4; w++) own[w] = v[w];
        if (p + 1 == own_hi) {  // the node's final version
            u64* o = dig + mu_off(bits, l, node);
#pragma unroll
            for (int w = 0; w < 4; w++) o[w] = own[w];
        }
        u64 st[12];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            st[w] = right ? sib[w] : own[w];
            st[4 + w] = right ? own[w] : sib[w];
            st[8 + w] = 0;
        }
        glf::two_to_one_permute(st);
        const size_t np = b0 + (p - own_lo) + r;
        a_out[np] = key;
        u64* vo = v_out + 4 * np;
#pragma unroll
        for (int w = 0; w < 4; w++) vo[w] = st[w];
        if (last) {
            if (root_after) {
                u64* o = root_after + (size_t)j * root_stride;
#pragma unroll
                for (int w = 0; w < 4; w++) o[w] = st[w];
            }
            if (np + 1 == b2) {
                u64* o = dig + mu_off(bits, l + 1, node >> 1);
#pragma unroll
                for (int w = 0; w < 4; w++) o[w] = st[w];
            }
        }
    }
    mu_count(active, counter);
}

__global__ __launch_bounds__(256) void k_mu_roots(const u64* __restrict__ v0, size_t k, u64* __restrict__ root_after, size_t root_stride, const u32* __restrict__ flag) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k || *flag) return;
#pragma unroll
    for (int w = 0; w < 4; w++) root_after[j * root_stride + w] = v0[4 * j + w];
}

}  // namespace p2k
