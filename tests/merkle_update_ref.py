"""Ordered leaf updates of a Merkle tree as a sequential Python model on tests/merkle_ref.py (the CPU oracle's Poseidon, not the
library under test): one item at a time on merkle_ref.levels(...), with merkle_ref.path(...) recorded before each item and
the cap entry after it.  Also what each device path must hash: the fast path every changed node once, the traced path every
version of every node on every item's path.  Shared by the update tests: the item lists and the update circuit."""
import functools

import numpy as np

import merkle_cases as mc
import merkle_ref

P = merkle_ref.P
SHAPES = ((1, 0), (2, 0), (2, 1), (8, 0), (8, 1), (8, 3))   # (num_leaves, cap_height): depth 0 with and without a level, depths 1 to 3
LEAF_LENS = (1, 4, 5, 8, 9)                                 # hash_or_noop's boundary and the first sponge-block boundary


def _two_to_one(left, right):
    return [int(w) for w in merkle_ref._two_to_one(np.array(left, dtype=np.uint64), np.array(right, dtype=np.uint64))]


class Update:
    """The tree `leaves` (cap height cap_height) after the items [(index, leaf)] applied in order.
    siblings[j]: merkle_ref.path of item j's index before item j; roots_after[j]: its cap entry after item j; caps: the k + 1 caps;
    leaves, levels: the final tree."""

    def __init__(self, leaves, cap_height, items):
        self.leaves = [list(leaf) for leaf in leaves]
        self.levels = [[list(h) for h in level] for level in merkle_ref.levels(leaves, cap_height)]
        depth = self.depth = len(self.levels) - 1
        self.siblings, self.roots_after, self.caps = [], [], [[list(h) for h in self.levels[depth]]]
        for index, leaf in items:
            self.siblings.append([list(h) for h in merkle_ref.path(self.levels, index)])
            self.leaves[index] = list(leaf)
            self.levels[0][index] = merkle_ref.hash_or_noop(leaf)
            for l in range(depth):
                n = index >> (l + 1)
                self.levels[l + 1][n] = _two_to_one(self.levels[l][2 * n], self.levels[l][2 * n + 1])
            self.roots_after.append(list(self.levels[depth][index >> depth]))
            self.caps.append([list(h) for h in self.levels[depth]])

    @property
    def cap(self):
        return self.levels[self.depth]

    def path(self, index):
        return merkle_ref.path(self.levels, index)


def fast_hashes(indices, depth):
    """two_to_one calls of an update without a trace: the distinct (l, index >> l) for l = 1 .. depth"""
    return len({(l, i >> l) for i in indices for l in range(1, depth + 1)})


def traced_hashes(indices, depth):
    return len(indices) * depth


def new_leaf(leaf_len, tag):
    """a canonical leaf that depends on `tag`; the extremes p - 1 and 0 are in it"""
    words = [(0x9E3779B97F4A7C15 * (tag + 1) * (w + 1) + tag) % P for w in range(leaf_len)]
    words[0] = P - 1 - tag
    if leaf_len > 1:
        words[-1] = 0
    return words


def item_lists(num_leaves, leaf_len):
    """{label: [(index, leaf)]}: one item; [i, i ^ 1] and [i ^ 1, i] (the sibling that changed earlier in the same batch); one
    leaf written three times; all leaves in reverse order; nothing"""
    i = num_leaves - 1
    out = {"one item": [(i // 2, new_leaf(leaf_len, 1))], "one leaf three times": [(i, new_leaf(leaf_len, t)) for t in (2, 3, 4)],
           "all leaves in reverse": [(n, new_leaf(leaf_len, 10 + n)) for n in reversed(range(num_leaves))], "k = 0": []}
    if num_leaves > 1:
        out["i then i ^ 1"] = [(i, new_leaf(leaf_len, 5)), (i ^ 1, new_leaf(leaf_len, 6))]
        out["i ^ 1 then i"] = [(i ^ 1, new_leaf(leaf_len, 7)), (i, new_leaf(leaf_len, 8))]
    return out


@functools.lru_cache(maxsize=None)
def case(num_leaves, cap_height, leaf_len, label):
    """(the leaves before, the items, the model after them), computed once"""
    lv, _ = mc.ref(num_leaves, leaf_len)
    items = item_lists(num_leaves, leaf_len)[label]
    return lv, items, Update(lv, cap_height, items)


LABELS = tuple(item_lists(8, 1))


def check_tree(tree, model):
    """cap and every path of `tree` are the model's"""
    n = len(model.leaves)
    assert tree.cap == model.cap
    assert tree.prove_batch(range(n)) == [model.path(i) for i in range(n)]


class UpdateCircuit:
    """old_leaf at the index under old_cap, new_leaf there under new_cap; both caps are public inputs"""

    def __init__(self, pkg, depth, cap_height, leaf_len, public=True, **kw):
        b = pkg.CircuitBuilder(**kw)
        self.old_leaf, self.new_leaf = b.add_virtual_target_arr(leaf_len), b.add_virtual_target_arr(leaf_len)
        self.bits = b.add_virtual_target_arr(depth + cap_height)
        self.old_cap = b.add_virtual_cap(cap_height)
        self.sibs = [b.add_virtual_hash() for _ in range(depth)]
        self.new_cap = b.merkle_update_to_cap(self.old_leaf, self.new_leaf, self.bits, self.old_cap, self.sibs)
        self.claimed = b.add_virtual_cap(cap_height)
        for x, y in zip(self.new_cap, self.claimed):
            b.connect_hashes(x, y)
        if public:
            b.register_public_inputs([t for h in self.old_cap + self.claimed for t in h])
        self.pkg, self.depth, self.cap_height = pkg, depth, cap_height
        self.data = b.build()

    def witness(self, old_leaf, new_leaf, index, siblings, old_cap, new_cap):
        pw = self.pkg.PartialWitness()
        pw.set_target_arr(self.old_leaf, old_leaf)
        pw.set_target_arr(self.new_leaf, new_leaf)
        pw.set_cap_target(self.old_cap, old_cap)
        pw.set_cap_target(self.claimed, new_cap)
        pw.set_merkle_proof_target((self.bits, self.sibs), index, siblings)
        return pw.map
