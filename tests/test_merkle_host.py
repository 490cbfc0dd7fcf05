"""Stand-alone Poseidon Merkle trees on the host (p2_native_merkle_cap / _prove / _verify through MerkleTree(device=None) and
merkle.verify(device=None)) against tests/merkle_ref.py, whose hash is the CPU oracle's.  Everything compared is a field
element or a status code: exact."""
import ctypes as C

import pytest

import merkle_cases as mc
import merkle_ref

P = mc.P
SHAPES = ((1, 0), (2, 0), (2, 1), (8, 0), (8, 2), (8, 3))


@pytest.mark.parametrize("leaf_len", mc.LEAF_LENS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_caps_and_every_path_equal_the_reference(pkg, leaf_len, shape):
    num_leaves, cap_height = shape
    lv, levels = mc.ref(num_leaves, leaf_len)
    tree = pkg.MerkleTree(lv, cap_height, device=None)
    cap = tree.cap
    assert cap == mc.ref_cap(levels, cap_height) and len(cap) == 1 << cap_height
    paths = tree.prove_batch(range(num_leaves))
    assert paths == [mc.ref_path(levels, cap_height, i) for i in range(num_leaves)]
    assert all(len(p) == tree.depth for p in paths)
    assert pkg.merkle.verify_batch(lv, range(num_leaves), paths, cap, device=None) == [0] * num_leaves
    assert all(merkle_ref.walk(lv[i], i, paths[i], cap) for i in range(num_leaves))
    assert tree.prove(num_leaves - 1) == paths[-1]


@pytest.mark.parametrize("leaf_len", mc.LEAF_LENS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_tampered_paths_get_the_reference_statuses(pkg, leaf_len, shape):
    num_leaves, cap_height = shape
    lv, levels = mc.ref(num_leaves, leaf_len)
    cases = mc.tampered(lv, levels, cap_height, num_leaves - 1) + mc.tampered(lv, levels, cap_height, 0)[1:]
    got = [pkg.merkle.verify(lf, ix, sb, cp, device=None) for _, lf, ix, sb, cp, _ in cases]
    assert got == [c[5] for c in cases], [c[0] for c in cases]
    assert {0, 1, 2} == set(got)


def test_bad_shapes_are_invalid(pkg):
    L = pkg.lib()
    u64 = C.c_uint64
    words, out = (u64 * 64)(*range(64)), (u64 * 64)()
    for num_leaves, leaf_len, cap_height in ((0, 4, 0), (3, 4, 0), (6, 4, 1), (4, 0, 0), (4, 4, 3), (4, 4, -1), (1, 4, 1)):
        assert L.p2_native_merkle_cap(words, num_leaves, leaf_len, cap_height, out) == 1, (num_leaves, leaf_len, cap_height)
        assert L.p2_last_error()
        assert L.p2_native_merkle_prove(words, num_leaves, leaf_len, cap_height, 0, out) == 1
    assert L.p2_native_merkle_cap(None, 4, 4, 0, out) == 1
    assert L.p2_native_merkle_prove(words, 4, 4, 0, 4, out) == 1 and b"index" in L.p2_last_error()
    words[9] = P                                          # word 1 of leaf 2
    assert L.p2_native_merkle_cap(words, 4, 4, 0, out) == 1 and b"word 1 of leaf 2" in L.p2_last_error()
    st = C.c_int(7)
    for leaf_len, depth, cap_height in ((0, 2, 0), (4, 33, 0), (4, 2, 17), (4, 30, 3), (4, 2, -1)):
        assert L.p2_native_merkle_verify(words, leaf_len, 0, out, depth, out, cap_height, C.byref(st)) == 1
    assert st.value == 7
    with pytest.raises(pkg.P2Error):
        pkg.MerkleTree([[1, 2], [3]], device=None)
    with pytest.raises(pkg.P2Error):
        pkg.MerkleTree([[1], [2], [3]], device=None)
    with pytest.raises(pkg.P2Error):
        pkg.MerkleTree([[1], [P]], device=None)
    with pytest.raises(pkg.P2Error):
        pkg.MerkleTree([[1], [2]], cap_height=2, device=None)
    with pytest.raises(pkg.P2Error):
        pkg.MerkleTree([[1], [2]], device=None).prove(2)


def test_device_entry_points_check_shapes_before_they_need_a_device(pkg):
    """the same rules in the device forms: P2_ERR_INVALID comes before any HIP call"""
    L = pkg.lib()
    u64 = C.c_uint64
    words, h = (u64 * 64)(*range(64)), C.c_void_p()
    for num_leaves, leaf_len, cap_height in ((0, 4, 0), (3, 4, 0), (4, 0, 0), (4, 4, 3), (1 << 50, 4, 0)):
        assert L.p2_merkle_tree_new(words, num_leaves, leaf_len, cap_height, 0, C.byref(h)) == 1 and not h.value
        assert L.p2_merkle_tree_new_device(words, num_leaves, leaf_len, cap_height, 0, None, C.byref(h)) == 1 and not h.value
    words[5] = P
    assert L.p2_merkle_tree_new(words, 4, 4, 0, 0, C.byref(h)) == 1 and b"word 1 of leaf 1" in L.p2_last_error()
    assert L.p2_merkle_tree_cap(None, words, 4) == 1 and L.p2_merkle_tree_prove_batch(None, words, 1, words) == 1
    st = (C.c_int * 1)()
    assert L.p2_merkle_verify_batch(words, 4, words, words, 30, words, 3, 1, st, 0) == 1
    L.p2_merkle_tree_free(None)


def test_the_new_entry_points_are_declared(pkg):
    L = pkg.lib()
    for f in ("p2_native_merkle_cap", "p2_native_merkle_prove", "p2_native_merkle_verify", "p2_merkle_tree_new", "p2_merkle_tree_new_device",
              "p2_merkle_tree_free", "p2_merkle_tree_cap", "p2_merkle_tree_prove_batch", "p2_merkle_tree_prove_batch_device", "p2_merkle_verify_batch",
              "p2_merkle_verify_batch_device", "p2_builder_permute_swapped", "p2_builder_hash_or_noop", "p2_builder_add_virtual_hash",
              "p2_builder_add_virtual_cap", "p2_builder_connect_hashes", "p2_builder_verify_merkle_proof_to_cap", "p2_builder_verify_merkle_proof"):
        assert f in L._p2_signatures and hasattr(L, f), f
