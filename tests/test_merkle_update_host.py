"""Ordered leaf updates on the host: p2_native_merkle_update (MerkleTree(device=None).update_batch), the sequential loop that
DEFINES an update, against tests/merkle_update_ref.py, a Python model over the CPU oracle's Poseidon.  Everything compared is a
field element or a return code: exact."""
import ctypes as C

import pytest

import merkle_cases as mc
import merkle_update_ref as mu

P = mu.P


@pytest.mark.parametrize("label", mu.LABELS)
@pytest.mark.parametrize("leaf_len", mu.LEAF_LENS)
@pytest.mark.parametrize("shape", mu.SHAPES, ids=["%dx%d" % s for s in mu.SHAPES])
def test_the_host_twin_equals_the_model(pkg, shape, leaf_len, label):
    num_leaves, cap_height = shape
    if label not in mu.item_lists(num_leaves, leaf_len):
        return                                            # a tree of one leaf has no i ^ 1
    lv, items, model = mu.case(num_leaves, cap_height, leaf_len, label)
    for trace in (False, True):
        tree = pkg.MerkleTree(lv, cap_height, device=None)
        cap0 = tree.cap
        got = tree.update_batch([i for i, _ in items], [leaf for _, leaf in items], trace=trace)
        mu.check_tree(tree, model)
        if not trace:
            assert got is None
            continue
        assert got.siblings == model.siblings and got.roots_after == model.roots_after
        assert got.caps(cap0) == model.caps and len(got.caps(cap0)) == len(items) + 1
        assert all(len(s) == tree.depth for s in got.siblings)
    # the trace is the witness of a membership proof: the old leaf under cap j, the new one under cap j + 1
    leaves = [list(leaf) for leaf in lv]
    for j, (i, leaf) in enumerate(items):
        assert pkg.merkle.verify(leaves[i], i, model.siblings[j], model.caps[j], device=None) == 0
        assert pkg.merkle.verify(leaf, i, model.siblings[j], model.caps[j + 1], device=None) == 0
        leaves[i] = leaf


def test_update_is_update_batch_of_one(pkg):
    lv, items, model = mu.case(8, 1, 5, "one item")
    tree = pkg.MerkleTree(lv, 1, device=None)
    assert tree.update(items[0][0], items[0][1]) is None
    mu.check_tree(tree, model)


@pytest.mark.parametrize("shape", ((8, 1), (8, 3), (1, 0)), ids=("8x1", "8x3", "1x0"))
def test_a_bad_item_changes_nothing(pkg, shape):
    """an index equal to num_leaves and a word equal to p, each behind a good item: P2_ERR_INVALID, the entry named, cap and
    every path as they were"""
    num_leaves, cap_height = shape
    lv, levels = mc.ref(num_leaves, 5)
    before = mu.Update(lv, cap_height, [])
    good = mu.new_leaf(5, 1)
    word_p = list(good)
    word_p[3] = P
    for items, message in (([(0, good), (num_leaves, good)], "entry 1"), ([(0, good), (num_leaves - 1, word_p)], "word 3 of the leaf of entry 1")):
        tree = pkg.MerkleTree(lv, cap_height, device=None)
        for trace in (False, True):
            with pytest.raises(pkg.P2Error, match=message):
                tree.update_batch([i for i, _ in items], [leaf for _, leaf in items], trace=trace)
            mu.check_tree(tree, before)


def test_argument_and_shape_errors(pkg):
    L = pkg.lib()
    u64 = C.c_uint64
    words, idx, out = (u64 * 64)(*range(64)), (u64 * 4)(0, 1, 2, 3), (u64 * 64)()
    for num_leaves, leaf_len, cap_height in ((0, 4, 0), (3, 4, 0), (4, 0, 0), (4, 4, 3), (4, 4, -1)):
        assert L.p2_native_merkle_update(words, num_leaves, leaf_len, cap_height, idx, words, 1, out, out) == 1, (num_leaves, leaf_len, cap_height)
        assert L.p2_last_error()
    assert L.p2_native_merkle_update(None, 4, 4, 0, idx, words, 1, out, out) == 1
    assert L.p2_native_merkle_update(words, 4, 4, 0, None, words, 1, out, out) == 1
    assert L.p2_native_merkle_update(words, 4, 4, 0, idx, None, 1, out, out) == 1
    assert list(words) == list(range(64))
    assert L.p2_native_merkle_update(words, 4, 4, 0, None, None, 0, None, None) == 0      # k = 0
    assert L.p2_native_merkle_update(words, 4, 4, 0, idx, (u64 * 16)(*range(100, 116)), 4, None, None) == 0      # no trace asked for
    assert list(words[:16]) == list(range(100, 116))
    # the device entry points refuse what they can before they need a device
    assert L.p2_merkle_tree_update(None, idx, words, 1, out, out) == 1
    assert L.p2_merkle_tree_update_device(None, None, None, 1, None, 0, None, 0, None, None) == 1
    assert L.p2_merkle_tree_last_update_hashes(None, out) == 1
    tree = pkg.MerkleTree([[1, 2], [3, 4]], device=None)
    for call in (lambda: tree.update_batch([0, 1], [[1, 2]]), lambda: tree.update_batch([0], [[1, 2, 3]]), lambda: tree.update_batch([0, 1], [[1, 2], [3]]),
                 lambda: tree.update_batch([-1], [[1, 2]]), lambda: tree.update_batch_device(0, 0, 1, 0, 0, 0, 0, 0), lambda: tree.last_update_hashes):
        with pytest.raises(pkg.P2Error):
            call()
    assert tree.cap == pkg.MerkleTree([[1, 2], [3, 4]], device=None).cap


def test_the_new_entry_points_are_declared(pkg):
    L = pkg.lib()
    for f in ("p2_native_merkle_update", "p2_merkle_tree_update", "p2_merkle_tree_update_device", "p2_merkle_tree_last_update_hashes",
              "p2_builder_merkle_update_to_cap", "p2_builder_merkle_update"):
        assert f in L._p2_signatures and hasattr(L, f), f
