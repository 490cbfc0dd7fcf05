// Sparse keyed Merkle trees on the device (p2_merkle_map_*, include/p2aes.h; the definition is mt::HostMap, merkle_host.h): the
// complete tree of depth D over N << 2^D sorted entries, of which only the non-empty nodes exist.  Level l keeps the ascending
// ids (key >> l) of its n_l non-empty nodes and their digests; every other node of the level is E_l.
//
// Build (mm_build in prover_gpu.hip launches it; keys sorted by rocPRIM's radix sort over D bits in between):
//   k_mm_check    thread per entry: the key below 2^D and p, the value words below p; the lowest bad (entry, kind) by atomicMin.
//   k_mm_diff     thread per sorted entry i: b_i = the highest bit in which key i differs from key i - 1 (b_0 = 64); equal
//                 neighbours are a duplicate.  Entry i starts a node of every level l <= b_i, so the 65-bin histogram of b gives
//                 every level's size n_l = #{i : b_i >= l} in one read-back.  The entries are then sorted by 64 - b (stable): O.
//                 The entries with b == l are O[n_{l+1} .. n_l), ascending: group_l.
//   k_mm_gather   thread per (entry, word): the values into key order.
//   k_mm_leaves   thread per entry: the leaf digest, and the entry's place in level 1.
//   k_mm_level    thread per PARENT r of level l + 1: every launched lane hashes, and every non-empty node is hashed once.  The
//                 lane reads the parent's first entry e and the rank c of its first child from the arrays the launch below
//                 filled, takes child c + 1 as the second child if its id has the same parent, an E_l for the missing side,
//                 and hashes.  Then it places itself in level l + 2 if b_e >= l + 2: its rank there is r - #{group_{l+1} < e},
//                 because rank_{l+2}(e) = #{j < e : b_j >= l + 2} = rank_{l+1}(e) - #{j < e : b_j == l + 1} -- one binary search
//                 of a static array, no scan and no round trip per level.  (e, r) ping-pong between two buffers.
//   k_mm_cap      thread per cap entry: the digest of node c of level D - h, or E_{D-h}.
// Lookups: k_mm_get, a thread per (query, level) that searches the level's ids for (key >> l) ^ 1, and one more thread per query
// for presence and value.  The searching lanes diverge; they do not hash.  k_mm_verify: a thread per proof, vfy_merkle_walk.
// Hashing: glf::two_to_one_permute for the levels (k_merkle_level's), PoseidonTree's sponge for leaves and path checks.
#pragma once
#include "kernels_merkle_update.h"

namespace p2k {

// What a lookup needs of one level: n ascending ids and their digests
struct MapLevel {
    const u64* ids;
    const u64* dig;
    size_t n;
};
// kinds of a bad entry, mt::MapBad
#define MM_BAD_KEY 0u
#define MM_BAD_WORD 1u
#define MM_BAD_DUPLICATE 2u

__device__ __forceinline__ bool mm_key_ok(u64 key, u32 key_bits) { return key < gl::P && (key_bits == 64 || (key >> key_bits) == 0); }
// hash_or_noop(value | 1) without the concatenation: word value_len of the input is the constant one
__device__ __forceinline__ void mm_leaf_digest(const u64* value, u32 value_len, u64* out) {
    const u32 len = value_len + 1;
    if (len <= 4) {
#pragma unroll
        for (u32 i = 0; i < 4; i++) out[i] = i < value_len ? value[i] : (i == value_len ? 1 : 0);
        return;
    }
    u64 st[12];
#pragma unroll
    for (int i = 0; i < 12; i++) st[i] = 0;
    for (u32 off = 0; off < len; off += 8) {
#pragma unroll
        for (u32 i = 0; i < 8; i++)
            if (off + i < len) st[i] = off + i < value_len ? value[off + i] : 1;
        glf::poseidon_sparse(st);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = st[i];
}
// the first q in [0, n) with a[q] >= x, or n
template <class T>
__device__ __forceinline__ size_t mm_lower(const T* a, size_t n, T x) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mm_check(const u64* __restrict__ keys, const u64* __restrict__ values, size_t n, u32 key_bits, u32 value_len,
                                                  u32* __restrict__ pos, unsigned long long* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pos[i] = (u32)i;
    if (!mm_key_ok(keys[i], key_bits)) {
        atomicMin(bad, 4ull * i + MM_BAD_KEY);
        return;
    }
    bool canonical = true;
    for (u32 w = 0; w < value_len; w++) canonical &= values[i * value_len + w] < gl::P;
    if (!canonical) atomicMin(bad, 4ull * i + MM_BAD_WORD);
}

// hist: 65 bins.  bkey[i] = 64 - b_i (the second sort's key), idx[i] = i (its value).
__global__ __launch_bounds__(256) void k_mm_diff(const u64* __restrict__ skeys, const u32* __restrict__ spos, size_t n, u32* __restrict__ bkey, u32* __restrict__ idx,
                                                 u32* __restrict__ hist, unsigned long long* __restrict__ bad) {
    __shared__ u32 h[65];
    if (threadIdx.x < 65) h[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        u32 b = 64;
        if (i) {
            const u64 x = skeys[i] ^ skeys[i - 1];
            if (x == 0) {
                atomicMin(bad, 4ull * spos[i] + MM_BAD_DUPLICATE);  // the sort is stable: entry spos[i] came after spos[i - 1]
                b = 0;
            } else {
                b = 63 - (u32)__clzll((long long)x);
            }
        }
        bkey[i] = 64 - b;
        idx[i] = (u32)i;
        atomicAdd(&h[b], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 65 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_mm_gather(const u64* __restrict__ values, const u32* __restrict__ spos, size_t n, u32 value_len, u64* __restrict__ svals) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * value_len) return;
    const size_t i = t / value_len;
    svals[t] = values[(size_t)spos[i] * value_len + (t - i * value_len)];
}

// The place of node r (first entry e) of level l in level l + 1, if it starts a node there: see the head of the file.
// group = O + n_{l+1}, the cnt entries with b == l.
__device__ __forceinline__ void mm_place(u32 l, u32 r, u32 e, const u32* __restrict__ bkey, const u32* __restrict__ group, size_t cnt, u32* __restrict__ ent_out,
                                         u32* __restrict__ child_out) {
    if (64 - bkey[e] < l + 1) return;
    const size_t up = r - mm_lower(group, cnt, e);
    ent_out[up] = e;
    child_out[up] = r;
}

__global__ __launch_bounds__(256) void k_mm_leaves(const u64* __restrict__ svals, size_t n, u32 value_len, u64* __restrict__ dig0, u32 place, const u32* __restrict__ bkey,
                                                   const u32* __restrict__ group, size_t cnt, u32* __restrict__ ent_out, u32* __restrict__ child_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 h[4];
    mm_leaf_digest(svals + i * value_len, value_len, h);
#pragma unroll
    for (int w = 0; w < 4; w++) dig0[4 * i + w] = h[w];
    if (place) mm_place(0, (u32)i, (u32)i, bkey, group, cnt, ent_out, child_out);
}

// Level l (n_c nodes: ids_c, dig_c) -> level l + 1 (n_p nodes).  ent_in / child_in: the first entry of parent r and the rank of its
// first child.  empty: E_l.  place: this is not the last level, so the parents place themselves in level l + 2 (group: the
// entries with b == l + 1).
__global__ __launch_bounds__(256) void k_mm_level(u32 l, const u64* __restrict__ ids_c, const u64* __restrict__ dig_c, size_t n_c, const u32* __restrict__ ent_in,
                                                  const u32* __restrict__ child_in, size_t n_p, const u64* __restrict__ empty, u64* __restrict__ ids_p,
                                                  u64* __restrict__ dig_p, u32 place, const u32* __restrict__ bkey, const u32* __restrict__ group, size_t cnt,
                                                  u32* __restrict__ ent_out, u32* __restrict__ child_out, u64* __restrict__ counter) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = r < n_p;
    if (active) {
        const u32 e = ent_in[r];
        const size_t c = child_in[r];
        const u64 id = ids_c[c];
        const bool right = id & 1;
        const bool two = !right && c + 1 < n_c && (ids_c[c + 1] >> 1) == (id >> 1);
        const u64* own = dig_c + 4 * c;
        const u64* other = two ? own + 4 : empty;
        u64 st[12];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const u64 a = own[w], b = other[w];
            st[w] = right ? b : a;
            st[4 + w] = right ? a : b;
            st[8 + w] = 0;
        }
        glf::two_to_one_permute(st);
        ids_p[r] = id >> 1;
#pragma unroll
        for (int w = 0; w < 4; w++) dig_p[4 * r + w] = st[w];
        if (place) mm_place(l + 1, (u32)r, e, bkey, group, cnt, ent_out, child_out);
    }
    mu_count(active, counter);
}

__global__ __launch_bounds__(256) void k_mm_cap(const u64* __restrict__ ids, const u64* __restrict__ dig, size_t n, const u64* __restrict__ empty, u32 cap_n,
                                                u64* __restrict__ cap) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cap_n) return;
    const size_t q = mm_lower(ids, n, (u64)c);
    const u64* s = q < n && ids[q] == c ? dig + 4 * q : empty;
#pragma unroll
    for (int w = 0; w < 4; w++) cap[4 * c + w] = s[w];
}

// k_mm_get: thread (query j, slot s).  s < depth: the sibling of level s to out[j * stride + sib_off + 4 s ..]; s == depth:
// status[j] (0, or 2 for a key that is not below 2^key_bits and p), present and the value (zeros when absent).  A row with
// status 2 is left untouched.  levels: depth + 1 records; empties: [65][4].
__global__ __launch_bounds__(256) void k_mm_get(const MapLevel* __restrict__ levels, const u64* __restrict__ svals, const u64* __restrict__ empties, u32 key_bits, u32 depth,
                                                u32 value_len, const u64* __restrict__ qkeys, size_t nq, u64* __restrict__ out, size_t stride, size_t present_off,
                                                size_t value_off, size_t sib_off, int* __restrict__ status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq * (depth + 1)) return;
    const size_t j = t / (depth + 1);
    const u32 s = (u32)(t - j * (depth + 1));
    const u64 key = qkeys[j];
    const bool ok = mm_key_ok(key, key_bits);
    if (s == depth && status) status[j] = ok ? 0 : 2;
    if (!ok) return;
    u64* row = out + j * stride;
    if (s == depth) {
        const MapLevel L = levels[0];
        const size_t q = mm_lower(L.ids, L.n, key);
        const bool present = q < L.n && L.ids[q] == key;
        row[present_off] = present;
        for (u32 w = 0; w < value_len; w++) row[value_off + w] = present ? svals[q * value_len + w] : 0;
        return;
    }
    const MapLevel L = levels[s];
    const u64 want = (key >> s) ^ 1;
    const size_t q = mm_lower(L.ids, L.n, want);
    const u64* d = q < L.n && L.ids[q] == want ? L.dig + 4 * q : empties + 4 * s;
    u64* o = row + sib_off + 4 * (size_t)s;
#pragma unroll
    for (int w = 0; w < 4; w++) o[w] = d[w];
}

// k_mm_verify: one thread per proof.  0 the walk reaches cap entry key >> depth, 1 it does not, 2 malformed: the key not below
// 2^key_bits and p, `present` neither 0 nor 1, or a value, sibling or cap word not below p (mt::host_map_verify).
__global__ __launch_bounds__(64) void k_mm_verify(const u64* __restrict__ keys, u32 key_bits, const u64* __restrict__ present, const u64* __restrict__ values, u32 value_len,
                                                  const u64* __restrict__ siblings, const u64* __restrict__ cap, u32 cap_height, size_t n, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 depth = key_bits - cap_height, cap_n = 1u << cap_height;
    const u64* value = values + i * value_len;
    const u64* sib = siblings + i * 4 * (size_t)depth;
    const u64 key = keys[i], flag = present[i];
    bool ok = mm_key_ok(key, key_bits) && flag <= 1;
    for (u32 w = 0; w < value_len; w++) ok &= value[w] < gl::P;
    for (u32 w = 0; w < 4 * depth; w++) ok &= sib[w] < gl::P;
    for (u32 w = 0; w < 4 * cap_n; w++) ok &= cap[w] < gl::P;
    if (!ok) {
        status[i] = 2;
        return;
    }
    u64 cur[4] = {0, 0, 0, 0};
    if (flag) mm_leaf_digest(value, value_len, cur);
    status[i] = vfy_merkle_walk<PoseidonTree, u64>(cur, key, cap, cap_n, sib, depth) ? 0 : 1;
}

}  // namespace p2k
