// Stand-alone Poseidon Merkle trees on the host (plonky2 hash/merkle_tree.rs MerkleTree::new, prove; merkle_proofs.rs
// verify_merkle_proof_to_cap): the shape rules both halves of the C ABI share, and the host twin of the device tree
// (p2_native_merkle_*) built on the verifier's hashing (verifier.h h_hash_or_noop, h_two_to_one, verify_merkle_to_cap).
// Leaves are row-major [num_leaves][leaf_len] canonical words.  Only caps and paths are interface: level l holds the
// 2^(bits - l) digests of that level in index order, which is not upstream's in-memory order.
#pragma once
#include <algorithm>
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

// ---- sparse keyed trees: MerkleMap(key_bits = D, value_len = V, cap_height = h) (p2_native_merkle_map_*, p2_merkle_map_*;
// include/p2aes.h has the definition).  The complete tree of depth D with the entry of key k at leaf k: an occupied leaf is
// hash_or_noop(value | 1), an empty one 0^4, an empty subtree of height l is E_l = two_to_one(E_{l-1}, E_{l-1}).  This is the
// definition in code: it works on the sorted entries, a node without entries is an E_l, and 2^D nodes never exist.
static const u32 MAP_MAX_VALUE_LEN = 134;
inline void map_check_shape(int key_bits, int cap_height, size_t value_len) {
    if (key_bits < 1 || key_bits > 64) throw std::runtime_error("key_bits must be 1 to 64");
    if (cap_height < 0 || cap_height > 16 || cap_height > key_bits) throw std::runtime_error("cap_height must be between 0 and min(key_bits, 16)");
    if (value_len > MAP_MAX_VALUE_LEN) throw std::runtime_error("value_len must be at most 134");
}
inline bool map_key_ok(u64 key, u32 key_bits) { return key < gl::P && (key_bits == 64 || (key >> key_bits) == 0); }
inline u64 map_shr(u64 key, u32 s) { return s >= 64 ? 0 : key >> s; }
// What the device reports for a bad entry: the kinds in the order they are looked at within one entry
enum MapBad { MAP_BAD_KEY = 0, MAP_BAD_WORD = 1, MAP_BAD_DUPLICATE = 2 };
inline std::string map_bad_message(size_t entry, int kind) {
    const std::string e = "entry " + std::to_string(entry);
    if (kind == MAP_BAD_KEY) return "the key of " + e + " is not below 2^key_bits and p";
    if (kind == MAP_BAD_WORD) return "a value word of " + e + " is not below p";
    return "the key of " + e + " is a duplicate of an earlier entry's";
}
inline void map_empty_digests(Hash4 (&E)[65]) {
    E[0] = Hash4{{0, 0, 0, 0}};
    for (u32 l = 1; l <= 64; l++) E[l] = h_two_to_one(E[l - 1], E[l - 1], HASHER_POSEIDON);
}
// hash_or_noop(value | 1)
inline Hash4 map_leaf_digest(const u64* value, size_t value_len) {
    std::vector<u64> w(value, value + value_len);
    w.push_back(1);
    return h_hash_or_noop(w.data(), w.size(), HASHER_POSEIDON);
}

struct HostMap {
    u32 D, h, V;
    std::vector<u64> keys;    // ascending
    std::vector<size_t> pos;  // keys[i] is entry pos[i] of the caller's
    std::vector<Hash4> leaf;  // leaf digests in key order
    Hash4 E[65];
    // the first entry that cannot be taken names itself in the exception: the lowest entry index, its key before its words
    // before a duplicate
    HostMap(const u64* in_keys, const u64* values, size_t n, size_t value_len, int key_bits, int cap_height) {
        map_check_shape(key_bits, cap_height, value_len);
        D = (u32)key_bits, h = (u32)cap_height, V = (u32)value_len;
        if (n && (!in_keys || (V && !values))) throw std::runtime_error("null argument");
        pos.resize(n);
        for (size_t i = 0; i < n; i++) pos[i] = i;
        std::stable_sort(pos.begin(), pos.end(), [&](size_t a, size_t b) { return in_keys[a] < in_keys[b]; });
        size_t bad = n;
        int kind = 0;
        auto note = [&](size_t entry, int k) {
            if (entry < bad || (entry == bad && k < kind)) bad = entry, kind = k;
        };
        for (size_t i = 0; i < n; i++) {
            if (!map_key_ok(in_keys[i], D)) note(i, MAP_BAD_KEY);
            else if (first_non_canonical(values + i * V, V) != V) note(i, MAP_BAD_WORD);
        }
        for (size_t i = 1; i < n; i++)
            if (in_keys[pos[i]] == in_keys[pos[i - 1]]) note(pos[i], MAP_BAD_DUPLICATE);
        if (bad != n) throw std::runtime_error(map_bad_message(bad, kind));
        map_empty_digests(E);
        keys.resize(n), leaf.resize(n);
        for (size_t i = 0; i < n; i++) keys[i] = in_keys[pos[i]], leaf[i] = map_leaf_digest(values + pos[i] * V, V);
    }
    u32 depth() const { return D - h; }
    // entries [lo, hi) are those below node `id` of level l
    void range(u32 l, u64 id, size_t* lo, size_t* hi) const {
        *lo = std::lower_bound(keys.begin(), keys.end(), id, [&](u64 k, u64 v) { return map_shr(k, l) < v; }) - keys.begin();
        *hi = std::upper_bound(keys.begin(), keys.end(), id, [&](u64 v, u64 k) { return v < map_shr(k, l); }) - keys.begin();
    }
    // the digest of the node of level l above entries [lo, hi): one hash per non-empty node
    Hash4 node(u32 l, size_t lo, size_t hi) const {
        if (lo == hi) return E[l];
        if (l == 0) return leaf[lo];
        size_t mid = lo;
        while (mid < hi && !((keys[mid] >> (l - 1)) & 1)) mid++;
        return h_two_to_one(node(l - 1, lo, mid), node(l - 1, mid, hi), HASHER_POSEIDON);
    }
    Hash4 node_at(u32 l, u64 id) const {
        size_t lo, hi;
        range(l, id, &lo, &hi);
        return node(l, lo, hi);
    }
    void cap(u64* out) const {
        for (u64 c = 0; c < ((u64)1 << h); c++) memcpy(out + 4 * c, node_at(depth(), c).e, 32);
    }
    // -1: no such entry
    ptrdiff_t find(u64 key) const {
        auto it = std::lower_bound(keys.begin(), keys.end(), key);
        return it != keys.end() && *it == key ? it - keys.begin() : -1;
    }
    // top down from the key's cap entry: every subtree beside the path is hashed once
    void siblings(u64 key, u64* out) const {
        size_t lo, hi;
        range(depth(), map_shr(key, depth()), &lo, &hi);
        for (u32 l = depth(); l-- > 0;) {
            size_t mid = lo;
            while (mid < hi && !((keys[mid] >> l) & 1)) mid++;
            const bool right = (key >> l) & 1;
            const Hash4 s = right ? node(l, lo, mid) : node(l, mid, hi);
            memcpy(out + 4 * l, s.e, 32);
            if (right) lo = mid;
            else hi = mid;
        }
    }
};

// One proof: 0 the walk reaches cap entry key >> depth, 1 it does not, 2 malformed (a key not below 2^key_bits and p, a word not
// below p, `present` other than 0 or 1).  The shape is checked by the caller (map_check_shape).
inline int host_map_verify(u64 key, u32 key_bits, u64 present, const u64* value, size_t value_len, const u64* siblings, const u64* cap, u32 cap_height) {
    const u32 depth = key_bits - cap_height;
    const size_t cap_n = (size_t)1 << cap_height;
    if (!map_key_ok(key, key_bits) || present > 1 || first_non_canonical(value, value_len) != value_len || first_non_canonical(siblings, 4 * (size_t)depth) != 4 * (size_t)depth ||
        first_non_canonical(cap, 4 * cap_n) != 4 * cap_n)
        return 2;
    Hash4 cur = present ? map_leaf_digest(value, value_len) : Hash4{{0, 0, 0, 0}};
    for (u32 l = 0; l < depth; l++) {
        Hash4 s;
        memcpy(s.e, siblings + 4 * l, 32);
        cur = ((key >> l) & 1) ? h_two_to_one(s, cur, HASHER_POSEIDON) : h_two_to_one(cur, s, HASHER_POSEIDON);
    }
    return memcmp(cur.e, cap + 4 * map_shr(key, depth), 32) == 0 ? 0 : 1;
}

}  // namespace mt
}  // namespace p2
