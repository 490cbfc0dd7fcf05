"""A sparse keyed Merkle tree in Python over tests/merkle_ref.py's hash_or_noop and the CPU oracle's two_to_one (liboracle.so,
not the library under test): MerkleMap(key_bits = D, value_len = V, cap_height = h) as include/p2aes.h defines it.  Only the
non-empty nodes are computed: level l is the ascending ids key >> l of the sorted keys and their digests, one batched
two_to_one per level with E_l for a missing child; every other node is an entry of the E_l table."""
import numpy as np

import merkle_ref

P = merkle_ref.P


def _two_to_one(left, right):
    return merkle_ref._two_to_one(np.array(left, dtype=np.uint64), np.array(right, dtype=np.uint64))


def empty_digests(n=65):
    out = [[0, 0, 0, 0]]
    while len(out) < n:
        out.append([int(w) for w in _two_to_one(out[-1], out[-1])])
    return out


E = empty_digests()


def leaf_digest(value):
    return merkle_ref.hash_or_noop(list(value) + [1])


class Map:
    """entries: {key: value words}.  levels[l] = (ids, digests) of the non-empty nodes for l = 0 .. D - h."""

    def __init__(self, entries, key_bits, cap_height=0, value_len=None):
        self.entries = {int(k): [int(w) for w in v] for k, v in entries.items()}
        self.V = value_len if value_len is not None else (len(next(iter(self.entries.values()))) if self.entries else 0)
        assert all(len(v) == self.V for v in self.entries.values())
        self.D, self.h, self.depth = key_bits, cap_height, key_bits - cap_height
        assert all(0 <= k < min(1 << key_bits, P) for k in self.entries)
        keys = sorted(self.entries)
        ids = np.array(keys, dtype=np.uint64)
        dig = np.array([leaf_digest(self.entries[k]) for k in keys], dtype=np.uint64).reshape(len(keys), 4)
        self.levels = [(ids, dig)]
        for l in range(self.depth):
            up, rank = np.unique(ids >> np.uint64(1), return_inverse=True)
            left = np.tile(np.array(E[l], dtype=np.uint64), (len(up), 1))
            right = left.copy()
            odd = (ids & np.uint64(1)).astype(bool)
            left[rank[~odd]] = dig[~odd]
            right[rank[odd]] = dig[odd]
            ids, dig = up, (_two_to_one(left, right).reshape(len(up), 4) if len(up) else np.zeros((0, 4), dtype=np.uint64))
            self.levels.append((ids, dig))

    def node(self, l, node_id):
        ids, dig = self.levels[l]
        q = int(np.searchsorted(ids, np.uint64(node_id)))
        return [int(w) for w in dig[q]] if q < len(ids) and int(ids[q]) == node_id else list(E[l])

    @property
    def cap(self):
        return [self.node(self.depth, c) for c in range(1 << self.h)]

    def proof(self, key):
        """(present, value, siblings)"""
        value = self.entries.get(key)
        return (int(value is not None), list(value) if value is not None else [0] * self.V, [self.node(l, (key >> l) ^ 1) for l in range(self.depth)])

    @property
    def hashes(self):
        """the non-empty nodes above the leaves: 1 + #{i >= 1 : msb(k_i ^ k_{i-1}) >= l} summed over l = 1 .. D - h"""
        keys = sorted(self.entries)
        if not keys:
            return 0
        msb = [(a ^ b).bit_length() - 1 for a, b in zip(keys, keys[1:])]
        total = sum(1 + sum(1 for m in msb if m >= l) for l in range(1, self.depth + 1))
        assert total == sum(len(ids) for ids, _ in self.levels[1:])
        return total

    def changed(self, key, value):
        """the map with `value` at `key`, or without the key for value = None"""
        entries = dict(self.entries)
        if value is None:
            del entries[key]
        else:
            entries[key] = list(value)
        return Map(entries, self.D, self.h, self.V)


def walk(key, proof, cap_hashes, depth):
    """True iff the proof's start digest climbs over its siblings, the bits of `key` as swap bits, to cap entry key >> depth"""
    present, value, siblings = proof
    cur = leaf_digest(value) if present else [0, 0, 0, 0]
    assert len(siblings) == depth
    for l, s in enumerate(siblings):
        left, right = (s, cur) if (key >> l) & 1 else (cur, s)
        cur = [int(w) for w in _two_to_one(left, right)]
    return cur == [int(w) for w in cap_hashes[key >> depth]]
