"""A Merkle tree in Python over the CPU oracle's Poseidon (proof_ref.poseidon_hasher: liboracle.so, not the library under
test): hash_or_noop, the levels, the cap, a path and the walk back to the cap, as plonky2's MerkleTree::new / prove /
verify_merkle_proof_to_cap define them.  Leaves are lists of field elements of one length."""
import numpy as np

import proof_ref

P = proof_ref.P
_hash_no_pad, _two_to_one = proof_ref.poseidon_hasher()


def hash_or_noop(leaf):
    leaf = [int(w) for w in leaf]
    return leaf + [0] * (4 - len(leaf)) if len(leaf) <= 4 else [int(w) for w in _hash_no_pad(np.array(leaf, dtype=np.uint64))]


def levels(leaves, cap_height=0):
    """[leaf digests, ..., the cap]: level l holds the 2^(bits - l) nodes in index order"""
    out = [[hash_or_noop(leaf) for leaf in leaves]]
    while len(out[-1]) > 1 << cap_height:
        prev = np.array(out[-1], dtype=np.uint64)
        out.append([[int(w) for w in h] for h in _two_to_one(prev[0::2], prev[1::2])])
    return out


def cap(lv):
    return lv[-1]


def path(lv, index):
    return [lv[l][(index >> l) ^ 1] for l in range(len(lv) - 1)]


def walk(leaf, index, siblings, cap_hashes):
    """True iff the leaf at `index` climbs through `siblings` to its entry of the cap"""
    cur = hash_or_noop(leaf)
    for s in siblings:
        l, r = (s, cur) if index & 1 else (cur, s)
        cur = [int(w) for w in _two_to_one(np.array(l, dtype=np.uint64), np.array(r, dtype=np.uint64))]
        index >>= 1
    return index < len(cap_hashes) and cur == [int(w) for w in cap_hashes[index]]
