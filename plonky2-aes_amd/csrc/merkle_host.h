// Stand-alone Poseidon Merkle trees on the host (plonky2 hash/merkle_tree.rs MerkleTree::new, prove; merkle_proofs.rs
// verify_merkle_proof_to_cap): the shape rules both halves of the C ABI share, and the host twin of the device tree
// (p2_native_merkle_*) built on the verifier's hashing (verifier.h h_hash_or_noop, h_two_to_one, verify_merkle_to_cap).
// Leaves are row-major [num_leaves][leaf_len] canonical words.  Only caps and paths are interface: level l holds the
// 2^(bits - l) digests of that level in index order, which is not upstream's in-memory order.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "verifier.h"

namespace p2 {
namespace mt {

// num_leaves a power of two >= 1, cap_height <= log2(num_leaves), leaf_len >= 1; throws with the reason otherwise.  Returns log2(num_leaves).
inline u32 check_shape(size_t num_leaves, size_t leaf_len, int cap_height) {
    u32 bits = 0;
    while (bits < 63 && ((size_t)1 << bits) < num_leaves) bits++;
    if (num_leaves == 0 || ((size_t)1 << bits) != num_leaves) throw std::runtime_error("num_leaves must be a power of two, at least 1");
    if (cap_height < 0 || (u32)cap_height > bits) throw std::runtime_error("cap_height must be between 0 and log2(num_leaves)");
    if (leaf_len == 0) throw std::runtime_error("leaf_len must be at least 1");
    if (leaf_len > ((size_t)1 << 20) || bits > 32) throw std::runtime_error("tree too large: at most 2^32 leaves of at most 2^20 words");
    return bits;
}
// the first word >= p of `count` words, or count
inline size_t first_non_canonical(const u64* w, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (w[i] >= gl::P) return i;
    return count;
}

struct HostTree {
    u32 bits, cap_height;
    std::vector<std::vector<Hash4>> levels;  // [0 .. bits - cap_height]: leaf digests first, the cap last
    HostTree(const u64* leaves, size_t num_leaves, size_t leaf_len, int cap_h) {
        bits = check_shape(num_leaves, leaf_len, cap_h);
        cap_height = (u32)cap_h;
        if (!leaves) throw std::runtime_error("null leaves");
        size_t bad = first_non_canonical(leaves, num_leaves * leaf_len);
        if (bad != num_leaves * leaf_len) throw std::runtime_error("word " + std::to_string(bad % leaf_len) + " of leaf " + std::to_string(bad / leaf_len) + " is not below p");
        levels.resize(bits - cap_height + 1);
        levels[0].resize(num_leaves);
        for (size_t i = 0; i < num_leaves; i++) levels[0][i] = h_hash_or_noop(leaves + i * leaf_len, leaf_len, HASHER_POSEIDON);
        for (u32 l = 1; l <= bits - cap_height; l++) {
            levels[l].resize(num_leaves >> l);
            for (size_t i = 0; i < levels[l].size(); i++) levels[l][i] = h_two_to_one(levels[l - 1][2 * i], levels[l - 1][2 * i + 1], HASHER_POSEIDON);
        }
    }
};

// The first item of an update that cannot be applied, as a message, or "" (p2_native_merkle_update, p2_merkle_tree_update): the
// index is looked at before the words.  An update with such an item changes nothing.
inline std::string first_bad_item(const u64* indices, const u64* leaves, size_t k, size_t num_leaves, size_t leaf_len) {
    for (size_t j = 0; j < k; j++) {
        if (indices[j] >= num_leaves) return "leaf index " + std::to_string(indices[j]) + " (entry " + std::to_string(j) + ") is not below num_leaves";
        const size_t bad = first_non_canonical(leaves + j * leaf_len, leaf_len);
        if (bad != leaf_len) return "word " + std::to_string(bad) + " of the leaf of entry " + std::to_string(j) + " is not below p";
    }
    return "";
}
// MerkleTree.update_batch as it is DEFINED: the k writes one after the other, item j on the tree left by the items before it
// (duplicates are legal, the last write wins).  Before its write item j records the siblings of its path (siblings [k][depth][4],
// the lowest level first: tree.prove(indices[j]) at that moment), after it cap entry indices[j] >> depth (root_after [k][4]);
// either may be null.  depth + 1 hashes of the verifier's per item; the device does the same in k * depth independent ones.
inline void host_update(HostTree& t, size_t leaf_len, const u64* indices, const u64* leaves, size_t k, u64* siblings, u64* root_after) {
    const u32 depth = t.bits - t.cap_height;
    for (size_t j = 0; j < k; j++) {
        size_t n = indices[j];
        if (siblings)
            for (u32 l = 0; l < depth; l++) memcpy(siblings + 4 * (j * depth + l), t.levels[l][(n >> l) ^ 1].e, 32);
        t.levels[0][n] = h_hash_or_noop(leaves + j * leaf_len, leaf_len, HASHER_POSEIDON);
        for (u32 l = 0; l < depth; l++, n >>= 1) t.levels[l + 1][n >> 1] = h_two_to_one(t.levels[l][n & ~(size_t)1], t.levels[l][n | 1], HASHER_POSEIDON);
        if (root_after) memcpy(root_after + 4 * j, t.levels[depth][n].e, 32);
    }
}

// One path: 0 accepted, 1 rejected, 2 a word (leaf, sibling or cap) that is not below p
inline int host_verify(const u64* leaf, size_t leaf_len, size_t index, const u64* siblings, size_t depth, const u64* cap, u32 cap_height) {
    const size_t cap_n = (size_t)1 << cap_height;
    if (first_non_canonical(leaf, leaf_len) != leaf_len || first_non_canonical(siblings, 4 * depth) != 4 * depth || first_non_canonical(cap, 4 * cap_n) != 4 * cap_n)
        return 2;
    std::vector<Hash4> c(cap_n), s(depth);
    if (cap_n) memcpy(c.data(), cap, 32 * cap_n);
    if (depth) memcpy(s.data(), siblings, 32 * depth);
    return verify_merkle_to_cap(leaf, leaf_len, index, c, s, HASHER_POSEIDON) ? 0 : 1;
}

}  // namespace mt
}  // namespace p2
