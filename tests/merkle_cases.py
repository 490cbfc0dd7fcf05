"""Shared by the Merkle tests: deterministic leaves, reference trees (tests/merkle_ref.py, computed once per shape), the
tampered-path set and the membership circuit."""
import functools
import random

import merkle_ref

P = merkle_ref.P
LEAF_LENS = (1, 4, 5, 8, 9, 16, 17)      # hash_or_noop's boundary (4 | 5) and the sponge-block boundaries (8 | 9, 16 | 17)


def leaves(num_leaves, leaf_len, seed=0):
    """[num_leaves][leaf_len] canonical words; the extremes 0 and p - 1 are among them"""
    r = random.Random(1000 * leaf_len + num_leaves + 7 * seed)
    rows = [[r.randrange(P) for _ in range(leaf_len)] for _ in range(num_leaves)]
    rows[0][0], rows[-1][-1] = P - 1, 0
    return rows


@functools.lru_cache(maxsize=None)
def ref(num_leaves, leaf_len, seed=0):
    """(leaves, levels down to the root): the cap of height h is levels[len(levels) - 1 - h]"""
    lv = leaves(num_leaves, leaf_len, seed)
    return lv, merkle_ref.levels(lv, 0)


def ref_cap(levels, cap_height):
    return levels[len(levels) - 1 - cap_height]


def ref_path(levels, cap_height, index):
    return merkle_ref.path(levels[: len(levels) - cap_height], index)


def tampered(lv, levels, cap_height, index):
    """[(label, leaf, index, siblings, cap, status the reference gives)]: the honest path, then one change each -- a leaf word,
    a sibling word, an index bit (a path bit and, with a cap above the root, a cap bit), a cap word, an index past the tree --
    and one word = p in the leaf, a sibling and the cap."""
    leaf, sibs, cap = list(lv[index]), [list(h) for h in ref_path(levels, cap_height, index)], [list(h) for h in ref_cap(levels, cap_height)]
    depth = len(sibs)
    out = [("honest", leaf, index, sibs, cap)]

    def changed(rows, i, j, v=None):
        rows = [list(r) for r in rows]
        rows[i][j] = (rows[i][j] + 1) % P if v is None else v
        return rows

    out.append(("leaf word", changed([leaf], 0, len(leaf) - 1)[0], index, sibs, cap))
    out.append(("cap word", leaf, index, sibs, changed(cap, index >> depth, 2)))
    out.append(("index past the tree", leaf, index + len(lv), sibs, cap))
    out.append(("cap word = p", leaf, index, sibs, changed(cap, len(cap) - 1, 3, P)))
    out.append(("leaf word = p", changed([leaf], 0, 0, P)[0], index, sibs, cap))
    if depth:
        out.append(("sibling word", leaf, index, changed(sibs, depth // 2, 1), cap))
        out.append(("path bit", leaf, index ^ 1, sibs, cap))
        out.append(("sibling word = p", leaf, index, changed(sibs, depth - 1, 0, P), cap))
    if cap_height:
        out.append(("cap bit", leaf, index ^ (1 << depth), sibs, cap))
    res = []
    for label, lf, ix, sb, cp in out:
        words = lf + [w for h in sb for w in h] + [w for h in cp for w in h]
        want = 2 if any(w >= P for w in words) else (0 if merkle_ref.walk(lf, ix, sb, cp) else 1)
        assert (want == 0) == (label == "honest"), label
        res.append((label, lf, ix, sb, cp, want))
    return res


class Membership:
    """leaf (leaf_len targets) is the leaf at the index spelled by `bits` of a tree with cap `cap` (set by the witness)"""

    def __init__(self, pkg, depth, cap_height, leaf_len, builder=None, **kw):
        b = builder or pkg.CircuitBuilder(**kw)
        self.leaf = b.add_virtual_target_arr(leaf_len)
        self.bits = b.add_virtual_target_arr(depth + cap_height)
        self.cap = b.add_virtual_cap(cap_height)
        self.sibs = [b.add_virtual_hash() for _ in range(depth)]
        b.verify_merkle_proof_to_cap(self.leaf, self.bits, self.cap, self.sibs)
        self.pkg, self.depth, self.cap_height = pkg, depth, cap_height
        self.data = None if builder else b.build()

    def targets(self):
        """every target a witness sets, leaf | bits | cap | siblings"""
        return self.leaf + self.bits + [t for h in self.cap for t in h] + [t for h in self.sibs for t in h]

    def witness(self, leaf, index, siblings, cap):
        pw = self.pkg.PartialWitness()
        pw.set_target_arr(self.leaf, leaf)
        pw.set_cap_target(self.cap, cap)
        pw.set_merkle_proof_target((self.bits, self.sibs), index, siblings)
        return pw.map

    def honest(self, lv, levels, index):
        return self.witness(lv[index], index, ref_path(levels, self.cap_height, index), ref_cap(levels, self.cap_height))
