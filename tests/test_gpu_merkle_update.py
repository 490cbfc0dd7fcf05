"""Ordered leaf updates of a device tree (p2_merkle_tree_update, _update_device; kernels_merkle_update.h) against
tests/merkle_update_ref.py, a sequential Python model over the CPU oracle's Poseidon: cap, every path, the trace (the siblings each
item saw, the cap entry it left) and the number of two_to_one calls -- every changed node once without a trace, k * depth with
it, so that neither a design that rehashes shared ancestors per item nor one that skips versions passes.
Shapes: the six smallest trees (no level, one level, a cap above the root, depth 3) with the leaf lengths at hash_or_noop's
boundary (4 | 5) and the sponge-block boundary (8 | 9), each with the item lists of the host test; 4096 leaves under a cap of
16 with 5000 random items (20 workgroups, the last of 136 threads; duplicates guaranteed) and with 1000 items inside one
64-leaf subtree (segments of hundreds of versions per node, one cap entry).  Then the update circuit: four chained proofs with
the siblings written by the tree straight into the prover's value matrix.  Everything compared is exact."""
import ctypes as C
import functools
import random

import pytest

import merkle_cases as mc
import merkle_update_ref as mu
from test_gpu_merkle import D2H, Device

pytestmark = pytest.mark.gpu

P = mu.P
FILL = 0xF00D000000000000


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


def split(items):
    return [i for i, _ in items], [leaf for _, leaf in items]


class DeviceUpdate:
    """one update_batch_device call on buffers of its own: uploaded by the constructor, enqueued by launch, read back by result"""

    def __init__(self, dev, tree, items, trace, stride=None, col=0):
        idx, leaves = split(items)
        self.dev, self.tree, self.trace, self.k, self.col = dev, tree, trace, len(items), col
        self.stride = 4 * tree.depth if stride is None else stride
        self.d_idx, self.d_leaves = dev.put(idx), dev.put([w for leaf in leaves for w in leaf])
        self.d_st = dev.put([0x7777777777777777] * ((self.k + 1) // 2))
        self.fill = [FILL + i for i in range(max(self.k * self.stride, 1))]
        self.d_sib, self.d_root = dev.put(self.fill), dev.put([FILL] * (4 * self.k))

    def launch(self, stream=None):
        self.tree.update_batch_device(self.d_idx.value, self.d_leaves.value, self.k, self.d_sib.value + 8 * self.col if self.trace else None, self.stride,
                                      self.d_root.value if self.trace else None, 4, self.d_st.value, stream=stream)
        return self

    def result(self):
        """(statuses, siblings per item, roots per item, (the whole sibling matrix, what it held before))"""
        dev, k, d, stride, col = self.dev, self.k, self.tree.depth, self.stride, self.col
        mat = dev.get(self.d_sib, len(self.fill))
        sibs = [[mat[j * stride + col + 4 * l:j * stride + col + 4 * l + 4] for l in range(d)] for j in range(k)]
        roots = dev.get(self.d_root, 4 * k)
        return dev.get(self.d_st, k, C.c_int), sibs, [roots[4 * j:4 * j + 4] for j in range(k)], (mat, self.fill)


def device_update(dev, tree, items, trace, stride=None, col=0):
    u = DeviceUpdate(dev, tree, items, trace, stride, col).launch()
    assert dev.H.hipStreamSynchronize(None) == 0
    return u.result()


# ------------------------------------------------------------------ the small lists, both forms, trace off and on
@pytest.mark.parametrize("leaf_len", mu.LEAF_LENS)
@pytest.mark.parametrize("shape", mu.SHAPES, ids=["%dx%d" % s for s in mu.SHAPES])
def test_host_pointer_form_equals_the_model(gpu, shape, leaf_len):
    num_leaves, cap_height = shape
    for label in mu.item_lists(num_leaves, leaf_len):
        lv, items, model = mu.case(num_leaves, cap_height, leaf_len, label)
        idx, leaves = split(items)
        for trace in (False, True):
            tree = gpu.MerkleTree(lv, cap_height)
            cap0 = tree.cap
            got = tree.update_batch(idx, leaves, trace=trace)
            mu.check_tree(tree, model)
            want = mu.traced_hashes(idx, tree.depth) if trace else mu.fast_hashes(idx, tree.depth)
            assert tree.last_update_hashes == want, (label, trace)
            if trace:
                assert got.siblings == model.siblings and got.roots_after == model.roots_after and got.caps(cap0) == model.caps, label
            else:
                assert got is None


@pytest.mark.parametrize("leaf_len", (5, 8))
@pytest.mark.parametrize("shape", mu.SHAPES, ids=["%dx%d" % s for s in mu.SHAPES])
def test_device_pointer_form_equals_the_model(gpu, dev, shape, leaf_len):
    num_leaves, cap_height = shape
    for label in mu.item_lists(num_leaves, leaf_len):
        lv, items, model = mu.case(num_leaves, cap_height, leaf_len, label)
        for trace in (False, True):
            tree = gpu.MerkleTree(lv, cap_height)
            if not items:
                tree.update_batch_device(None, None, 0, None, 0, None, 0, None)      # k = 0: nothing is looked at
                mu.check_tree(tree, model)
                continue
            st, sibs, roots, (mat, fill) = device_update(dev, tree, items, trace)
            assert st == [0] * len(items)
            mu.check_tree(tree, model)
            assert tree.last_update_hashes == (mu.traced_hashes if trace else mu.fast_hashes)(split(items)[0], tree.depth), (label, trace)
            if trace:
                assert sibs == model.siblings and roots == model.roots_after, label
            else:
                assert mat == fill and roots == [[FILL] * 4] * len(items)


def test_update_of_one_and_a_second_update_on_the_same_handle(gpu):
    """update is update_batch of one; a later, larger update grows the handle's scratch block and starts from the tree the first left"""
    lv, items, model = mu.case(8, 1, 5, "all leaves in reverse")
    tree = gpu.MerkleTree(lv, 1)
    assert tree.last_update_hashes == 0
    assert tree.update(items[0][0], items[0][1]) is None and tree.last_update_hashes == 2
    got = tree.update_batch(*split(items[1:]), trace=True)
    mu.check_tree(tree, model)
    assert got.siblings == model.siblings[1:] and got.roots_after == model.roots_after[1:] and tree.last_update_hashes == 7 * 2


# ------------------------------------------------------------------ several workgroups, duplicates, long segments
BIG = (4096, 4, 5)


@functools.lru_cache(maxsize=None)
def big_case(kind):
    num_leaves, cap_height, leaf_len = BIG
    r = random.Random(11 if kind == "random" else 12)
    lv, _ = mc.ref(num_leaves, leaf_len)
    if kind == "random":
        idx = [r.randrange(num_leaves) for _ in range(5000)]
    else:
        idx = [37 * 64 + r.randrange(64) for _ in range(1000)]
    items = [(i, [r.randrange(P) for _ in range(leaf_len)]) for i in idx]
    assert len(set(idx)) < len(idx) and len(idx) % 256
    return lv, items, mu.Update(lv, cap_height, items)


@pytest.mark.parametrize("trace", (False, True), ids=("fast", "traced"))
@pytest.mark.parametrize("kind", ("random", "one subtree"))
def test_many_items(gpu, kind, trace):
    num_leaves, cap_height, leaf_len = BIG
    lv, items, model = big_case(kind)
    idx, leaves = split(items)
    tree = gpu.MerkleTree(lv, cap_height)
    cap0 = tree.cap
    got = tree.update_batch(idx, leaves, trace=trace)
    mu.check_tree(tree, model)
    fresh = gpu.MerkleTree(model.leaves, cap_height)
    assert tree.cap == fresh.cap and tree.prove_batch(range(num_leaves)) == fresh.prove_batch(range(num_leaves))
    assert tree.last_update_hashes == (mu.traced_hashes if trace else mu.fast_hashes)(idx, tree.depth)
    if trace:
        assert got.siblings == model.siblings
        assert got.roots_after == model.roots_after and got.caps(cap0)[-1] == model.cap


# ------------------------------------------------------------------ strides, bad items, ordering
def test_a_strided_trace_lands_in_its_columns(gpu, dev):
    num_leaves, cap_height, leaf_len, stride, col = 8, 1, 9, 23, 7
    lv, items, model = mu.case(num_leaves, cap_height, leaf_len, "all leaves in reverse")
    tree = gpu.MerkleTree(lv, cap_height)
    assert col + 4 * tree.depth < stride
    st, sibs, roots, (mat, fill) = device_update(dev, tree, items, True, stride=stride, col=col)
    want = list(fill)
    for j in range(len(items)):
        want[j * stride + col:j * stride + col + 4 * tree.depth] = [w for h in model.siblings[j] for w in h]
    assert mat == want and roots == model.roots_after and st == [0] * len(items)
    mu.check_tree(tree, model)
    d = dev.put([0] * 64)
    with pytest.raises(gpu.P2Error):
        tree.update_batch_device(d.value, d.value, 2, d.value, 4 * tree.depth - 1, d.value, 4, d.value)
    with pytest.raises(gpu.P2Error):
        tree.update_batch_device(d.value, d.value, 2, d.value, 4 * tree.depth, d.value, 3, d.value)
    with pytest.raises(gpu.P2Error):
        tree.update_batch_device(d.value, d.value, 2, d.value, 4 * tree.depth, d.value, 4, None)
    mu.check_tree(tree, model)


@pytest.mark.parametrize("trace", (False, True), ids=("fast", "traced"))
def test_a_bad_item_leaves_the_tree_bit_for_bit(gpu, dev, trace):
    num_leaves, cap_height, leaf_len = 512, 1, 5
    lv, _ = mc.ref(num_leaves, leaf_len)
    before = mu.Update(lv, cap_height, [])
    good = mu.new_leaf(leaf_len, 3)
    word_p = list(good)
    word_p[4] = P
    items = [(i, mu.new_leaf(leaf_len, i)) for i in range(300)]        # two workgroups: the bad items sit in the second
    items[270] = (num_leaves, good)
    items[280] = (5, word_p)
    items[290] = (1 << 40, word_p)                                     # both: the index is looked at first
    items[299] = ((1 << 64) - 1, good)
    tree = gpu.MerkleTree(lv, cap_height)
    tree.update_batch(*split(items[:8]))
    assert tree.last_update_hashes > 0
    after8 = mu.Update(lv, cap_height, items[:8])
    st, sibs, roots, (mat, fill) = device_update(dev, tree, items, trace)
    assert st == [{270: 1, 280: 2, 290: 1, 299: 1}.get(j, 0) for j in range(300)]
    mu.check_tree(tree, after8)
    assert mat == fill and roots == [[FILL] * 4] * 300 and tree.last_update_hashes == 0
    for part, message in ((items[:271], "entry 270"), (items[271:281], "word 4 of the leaf of entry 9")):
        with pytest.raises(gpu.P2Error, match=message):
            tree.update_batch(*split(part), trace=trace)
    mu.check_tree(tree, after8)
    assert before.cap != after8.cap


def test_two_updates_on_two_streams_are_ordered_by_the_handle(gpu, dev):
    """the second update starts from what the first left although nothing else orders the two streams; the cap read waits for both"""
    num_leaves, cap_height, leaf_len = 512, 1, 5
    lv, _ = mc.ref(num_leaves, leaf_len)
    r = random.Random(21)
    items = [(r.randrange(64), [r.randrange(P) for _ in range(leaf_len)]) for _ in range(1200)]   # 64 leaves: every later item overwrites an earlier one
    model = mu.Update(lv, cap_height, items)
    tree = gpu.MerkleTree(lv, cap_height)
    first, second = DeviceUpdate(dev, tree, items[:600], True), DeviceUpdate(dev, tree, items[600:], True)   # uploads done: nothing but the handle orders the launches
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert dev.H.hipStreamCreateWithFlags(C.byref(s), C.c_uint(1)) == 0        # hipStreamNonBlocking: no implicit ordering through the null stream
    try:
        first.launch(streams[0])
        second.launch(streams[1])
        assert dev.H.hipStreamSynchronize(streams[1]) == 0
        mu.check_tree(tree, model)
        assert dev.H.hipStreamSynchronize(streams[0]) == 0
        for u, lo in ((first, 0), (second, 600)):
            st, sibs, roots, _ = u.result()
            assert st == [0] * 600 and sibs == model.siblings[lo:lo + 600] and roots == model.roots_after[lo:lo + 600]
    finally:
        for s in streams:
            dev.H.hipStreamSynchronize(s)
            dev.H.hipStreamDestroy(s)


# ------------------------------------------------------------------ the update circuit: device witness and proofs against the oracle
def test_proofs_of_a_chain_over_every_index_are_the_oracles(gpu, orc):
    """depth 3 under a cap of two, the 16 leaves written once each in one traced batch: item j takes cap j to cap j + 1, and every
    level sees both swap values on both walks.  (Without public inputs: the oracle proves such circuits only.)"""
    depth, cap_height, leaf_len = 3, 1, 5
    c = mu.UpdateCircuit(gpu, depth, cap_height, leaf_len, public=False)
    lv, _ = mc.ref(16, leaf_len)
    items = [((7 * j + 3) % 16, mu.new_leaf(leaf_len, 60 + j)) for j in range(16)]
    tree = gpu.MerkleTree(lv, cap_height)
    cap0 = tree.cap
    trace = tree.update_batch(*split(items), trace=True)
    caps = trace.caps(cap0)
    assert caps[-1] == tree.cap
    maps = [c.witness(lv[i], leaf, i, trace.siblings[j], caps[j], caps[j + 1]) for j, (i, leaf) in enumerate(items)]
    proofs, st = c.data.prove_batch(maps)
    assert st == [0] * 16
    oc = orc.OracleCircuit(c.data.blob)
    assert c.data.verifier_data() == oc.verifier_data()
    for j in (0, 5, 10, 15):
        st_o, want = oc.prove(maps[j])
        assert st_o == 0 and proofs[j] == want, "proof %d differs from the oracle's" % j
    assert c.data.verify_batch(proofs) == [gpu.VERIFY_OK] * 16
    for p in proofs[:2]:
        c.data.verify(p)
    assert [gpu.host_witness(c.data.blob, m)[1] for m in maps] == [0] * 16


# ------------------------------------------------------------------ end to end: four proofs, proof j takes cap j to cap j + 1
def test_chained_update_proofs_with_siblings_from_the_device(gpu, dev):
    depth, cap_height, leaf_len, B = 3, 1, 5, 4
    num_leaves = 1 << (depth + cap_height)
    c = mu.UpdateCircuit(gpu, depth, cap_height, leaf_len)
    data = c.data
    assert data.num_public_inputs == 16
    lv, _ = mc.ref(num_leaves, leaf_len, seed=4)
    idx = [6, 7, 9, 6]                                    # 7 sees the 6 of item 0 as its sibling; item 3 replaces item 0's leaf
    items = [(i, mu.new_leaf(leaf_len, 40 + j)) for j, i in enumerate(idx)]
    model = mu.Update(lv, cap_height, items)
    old_leaves = [lv[6], lv[7], lv[9], items[0][1]]
    tree = gpu.MerkleTree(lv, cap_height)
    stale = tree.prove(7)
    assert tree.cap == model.caps[0] and stale != model.siblings[1]

    sib_t = [t for h in c.sibs for t in h]
    targets = c.old_leaf + c.new_leaf + c.bits + [t for h in c.old_cap + c.claimed for t in h] + sib_t
    col, n_t = len(targets) - len(sib_t), len(targets)
    rows = []
    for j, (i, leaf) in enumerate(items):
        rows += (list(old_leaves[j]) + list(leaf) + [(i >> b) & 1 for b in range(depth + cap_height)] + [w for h in model.caps[j] + model.caps[j + 1] for w in h] +
                 [gpu.VALUE_UNSET] * len(sib_t))
    pb = data.proof_bytes
    d_vals, d_idx, d_leaves = dev.put(rows), dev.put(idx), dev.put([w for _, leaf in items for w in leaf])
    d_roots, d_ust, d_proofs, d_pst = dev.alloc(32 * B), dev.alloc(4 * B), dev.alloc(B * pb), dev.alloc(4 * B)
    s = C.c_void_p()
    assert dev.H.hipStreamCreate(C.byref(s)) == 0
    try:
        tree.update_batch_device(d_idx.value, d_leaves.value, B, d_vals.value + 8 * col, n_t, d_roots.value, 4, d_ust.value, stream=s)
        data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    finally:
        dev.H.hipStreamSynchronize(s)
        dev.H.hipStreamDestroy(s)
    assert dev.get(d_ust, B, C.c_int) == [0] * B and dev.get(d_pst, B, C.c_int) == [0] * B
    mat = dev.get(d_vals, B * n_t)
    for j in range(B):
        assert mat[j * n_t + col:(j + 1) * n_t] == [w for h in model.siblings[j] for w in h]
    roots = dev.get(d_roots, 4 * B)
    assert [roots[4 * j:4 * j + 4] for j in range(B)] == model.roots_after
    mu.check_tree(tree, model)
    assert tree.last_update_hashes == B * depth
    host = C.create_string_buffer(B * pb)
    assert dev.H.hipMemcpy(host, d_proofs, B * pb, D2H) == 0
    proofs = [host.raw[j * pb:(j + 1) * pb] for j in range(B)]
    for j, p in enumerate(proofs):
        data.verify(p)
        assert data.public_inputs(p) == [w for h in model.caps[j] + model.caps[j + 1] for w in h]
        assert j == 0 or data.public_inputs(p)[:8] == data.public_inputs(proofs[j - 1])[8:]      # the chain: cap j out of proof j - 1, into proof j
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * B
    cproofs, st = data.compress_batch(proofs)
    assert st == [gpu.VERIFY_OK] * B and all(len(cp) < pb for cp in cproofs)
    assert data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * B
    # the path of leaf 7 as it was BEFORE item 0 is no witness of item 1
    w = c.witness(old_leaves[1], items[1][1], 7, stale, model.caps[1], model.caps[2])
    _, st = data.prove_batch([w, c.witness(old_leaves[1], items[1][1], 7, model.siblings[1], model.caps[1], model.caps[2])])
    assert st == [1, 0]
