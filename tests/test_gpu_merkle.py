"""Stand-alone Merkle trees and the membership gadget on the GPU.

Trees: k_mt_transpose (row-major leaves to the column-major layout of k_hash_leaves), the leaf and level kernels, k_mt_paths
and k_mt_verify against tests/merkle_ref.py, a Python tree over the CPU oracle's Poseidon; the host twin path for path.
Shapes: the leaf lengths at the hash_or_noop boundary (4 | 5) and the sponge-block boundaries (8 | 9, 16 | 17) plus 135 (17
blocks, the last of 7 words; five 32-column transpose tiles, the last of 7 columns); 1 and 2 leaves (no level, one level; a
transpose tile of one and two rows), 256 and 512 (one and two workgroups of the leaf kernel), 4096 (three launched levels and
both fused-top kernels under a root; eight fused levels under a cap of 16).
Circuits: the depth-3, cap-height-1 membership circuit at all 16 indices -- swap = 0 and swap = 1 on every level, the first
time that wire is not the constant zero -- device witness against the host twin, proofs byte for byte against the CPU
oracle, both verifiers on honest proofs and on a flipped swap opening; and membership plus hashed ElGamal in one circuit with
the paths written by the tree straight into the prover's value matrix.  Everything compared is exact."""
import ctypes as C
import random

import pytest

import merkle_cases as mc
import proof_ref as R
import test_gpu_proof_replay as replay
from test_gpu_witness import _hip, twin_check

pytestmark = pytest.mark.gpu

P = mc.P
H2D, D2H = 1, 2
LEAF_LENS = mc.LEAF_LENS + (135,)
NUM_LEAVES = (1, 2, 256, 512, 4096)
CAP_HEIGHTS = (0, 4)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def index_set(num_leaves):
    """0, the last leaf, both sides of every edge between two workgroups of the leaf kernel (256 leaves: also an edge between two
    32-row transpose tiles), and a few inside"""
    idx = {0, num_leaves - 1, num_leaves // 2, num_leaves // 3}
    for edge in range(256, num_leaves, 256):
        idx |= {edge - 1, edge}
    return sorted(idx)


class Device:
    """device buffers for one test, freed at its end"""

    def __init__(self):
        self.H, self.bufs = _hip(), []

    def alloc(self, nbytes):
        b = C.c_void_p()
        assert self.H.hipMalloc(C.byref(b), max(nbytes, 8)) == 0
        self.bufs.append(b)
        return b

    def put(self, words):
        arr = (C.c_uint64 * max(len(words), 1))(*words)
        b = self.alloc(C.sizeof(arr))
        assert self.H.hipMemcpy(b, arr, C.sizeof(arr), H2D) == 0
        return b

    def get(self, b, count, ctype=C.c_uint64):
        out = (ctype * max(count, 1))()
        assert self.H.hipMemcpy(out, b, C.sizeof(ctype) * count, D2H) == 0
        return list(out[:count])

    def free(self):
        for b in self.bufs:
            self.H.hipFree(b)
        self.bufs = []


@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


# ------------------------------------------------------------------ build and openings against the reference
@pytest.mark.parametrize("num_leaves", NUM_LEAVES)
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_caps_and_paths_equal_the_reference(gpu, leaf_len, num_leaves):
    lv, levels = mc.ref(num_leaves, leaf_len)
    idx = index_set(num_leaves)
    for cap_height in CAP_HEIGHTS:
        if (1 << cap_height) > num_leaves:
            continue
        tree = gpu.MerkleTree(lv, cap_height)
        assert tree.cap == mc.ref_cap(levels, cap_height), cap_height
        assert tree.prove_batch(idx) == [mc.ref_path(levels, cap_height, i) for i in idx], cap_height
        assert tree.prove(idx[-1]) == mc.ref_path(levels, cap_height, idx[-1])


@pytest.mark.parametrize("leaf_len,num_leaves,cap_height", ((5, 512, 4), (135, 256, 0), (3, 2, 1), (9, 1, 0)))
def test_host_pointer_and_device_pointer_forms_agree(gpu, dev, leaf_len, num_leaves, cap_height):
    lv, levels = mc.ref(num_leaves, leaf_len)
    host_tree = gpu.MerkleTree(lv, cap_height)
    d_leaves = dev.put([w for leaf in lv for w in leaf])
    tree = gpu.MerkleTree.from_device(d_leaves.value, num_leaves, leaf_len, cap_height)
    assert tree.cap == host_tree.cap == mc.ref_cap(levels, cap_height)
    idx = index_set(num_leaves)
    assert tree.prove_batch(idx) == host_tree.prove_batch(idx)
    d_idx, d_out, d_st = dev.put(idx), dev.alloc(32 * len(idx) * max(tree.depth, 1)), dev.alloc(4 * len(idx))
    tree.prove_batch_device(d_idx.value, len(idx), d_out.value, 4 * tree.depth, d_st.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    flat = dev.get(d_out, 4 * tree.depth * len(idx))
    assert flat == [w for path in host_tree.prove_batch(idx) for h in path for w in h]
    assert dev.get(d_st, len(idx), C.c_int) == [0] * len(idx)


def test_strided_openings_and_indices_out_of_range(gpu, dev):
    """paths land at their columns of a wider matrix, the words between them stay, an index past the tree is status 1 and its
    row stays"""
    num_leaves, leaf_len, cap_height, stride, col = 512, 9, 4, 37, 11
    lv, levels = mc.ref(num_leaves, leaf_len)
    tree = gpu.MerkleTree(lv, cap_height)
    depth = tree.depth
    assert depth == 5 and col + 4 * depth < stride
    idx = [511, num_leaves, 255, 256, 1 << 40, 0, (1 << 64) - 1]
    fill = [0xF00D000000000000 + i for i in range(stride * len(idx))]
    d_idx, d_mat, d_st = dev.put(idx), dev.put(fill), dev.put([0x7777777777777777] * len(idx))
    tree.prove_batch_device(d_idx.value, len(idx), d_mat.value + 8 * col, stride, d_st.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    got, want = dev.get(d_mat, len(fill)), list(fill)
    for k, i in enumerate(idx):
        if i < num_leaves:
            want[k * stride + col:k * stride + col + 4 * depth] = [w for h in mc.ref_path(levels, cap_height, i) for w in h]
    assert got == want
    assert dev.get(d_st, len(idx), C.c_int) == [int(i >= num_leaves) for i in idx]
    with pytest.raises(gpu.P2Error):
        tree.prove_batch([0, num_leaves])
    with pytest.raises(gpu.P2Error):
        tree.prove_batch_device(d_idx.value, len(idx), d_mat.value, 4 * depth - 1, d_st.value)


# ------------------------------------------------------------------ verification
def test_every_honest_path_of_the_512_leaf_tree_is_accepted(gpu):
    lv, levels = mc.ref(512, 9)
    tree = gpu.MerkleTree(lv, 4)
    paths = tree.prove_batch(range(512))
    assert gpu.merkle.verify_batch(lv, range(512), paths, tree.cap) == [0] * 512


@pytest.mark.parametrize("leaf_len", mc.LEAF_LENS)
def test_tampered_paths_get_the_host_twins_statuses(gpu, leaf_len):
    for num_leaves, cap_height in ((1, 0), (2, 0), (2, 1), (8, 0), (8, 2), (8, 3)):
        lv, levels = mc.ref(num_leaves, leaf_len)
        cases = mc.tampered(lv, levels, cap_height, num_leaves - 1) + mc.tampered(lv, levels, cap_height, 0)[1:]
        by_cap = {}
        for c in cases:   # one call per cap: the batch form takes one
            by_cap.setdefault(tuple(map(tuple, c[4])), []).append(c)
        for cap, group in by_cap.items():
            args = ([c[1] for c in group], [c[2] for c in group], [c[3] for c in group], [list(h) for h in cap])
            got = gpu.merkle.verify_batch(*args)
            assert got == gpu.merkle.verify_batch(*args, device=None) == [c[5] for c in group], (num_leaves, cap_height, [c[0] for c in group])


def test_verify_batch_device_form(gpu, dev):
    lv, levels = mc.ref(512, 17)
    tree = gpu.MerkleTree(lv, 4)
    idx = index_set(512)
    paths = tree.prove_batch(idx)
    paths[2][3][1] ^= 1
    d = [dev.put([w for i in idx for w in lv[i]]), dev.put(idx), dev.put([w for p in paths for h in p for w in h]), dev.put([w for h in tree.cap for w in h])]
    d_st = dev.alloc(4 * len(idx))
    gpu.merkle.verify_batch_device(d[0].value, 17, d[1].value, d[2].value, tree.depth, d[3].value, 4, len(idx), d_st.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    assert dev.get(d_st, len(idx), C.c_int) == [int(k == 2) for k in range(len(idx))]


# ------------------------------------------------------------------ the membership circuit: swap = 1 through every layer
DEPTH, CAP_HEIGHT, LEAF_LEN = 3, 1, 5


@pytest.fixture(scope="module")
def member(gpu):
    m = mc.Membership(gpu, DEPTH, CAP_HEIGHT, LEAF_LEN)
    lv, levels = mc.ref(16, LEAF_LEN)
    maps = [m.honest(lv, levels, i) for i in range(16)]
    proofs, st = m.data.prove_batch(maps)
    assert st == [0] * 16
    return m, lv, levels, maps, proofs


def test_device_witness_equals_the_host_twin(gpu, member):
    m, lv, levels, maps, _ = member
    wrong = {c[0]: m.witness(c[1], c[2], c[3], c[4]) for c in mc.tampered(lv, levels, CAP_HEIGHT, 10) if c[5] == 1 and c[2] < 16}
    missing = dict(maps[3])
    del missing[m.sibs[2][1]]
    cases = [maps[5], wrong["sibling word"], maps[10], missing, wrong["path bit"], wrong["cap bit"], wrong["leaf word"], maps[15]]
    swap_and_digest = [(1 << 63) | (row << 8) | col for row in range(1, 1 + DEPTH) for col in (24, 12, 13, 14, 15)]   # PoseidonGate rows of the walk
    outs = swap_and_digest + m.targets()
    assert twin_check(gpu, m.data, cases, outs, (1, 3, 8), (1, len(outs))) == [0, 1, 0, 2, 1, 1, 1, 0]
    assert [m.data.explain(c) for c in cases] == [gpu.host_witness(m.data.blob, c)[2] for c in cases]


def test_proofs_are_the_oracles_at_every_index(gpu, orc, member):
    m, lv, levels, maps, proofs = member
    oc = orc.OracleCircuit(m.data.blob)
    assert m.data.verifier_data() == oc.verifier_data()
    for i, (w, proof) in enumerate(zip(maps, proofs)):
        st, want = oc.prove(w)
        assert st == 0 and proof == want, "index %d" % i


def test_both_verifiers_accept_the_honest_proofs(gpu, member):
    m, lv, levels, maps, proofs = member
    for p in proofs:
        m.data.verify(p)
    assert m.data.verify_batch(proofs) == [gpu.VERIFY_OK] * 16


def test_both_verifiers_reject_a_flipped_swap_opening_alike(gpu, member):
    m, lv, levels, maps, proofs = member
    off, nbytes, kind = R.sections(m.data.info)["open_wires"]
    assert kind == "words" and nbytes == 16 * m.data.info["num_wires"]
    data, L, vd = m.data, gpu.lib(), m.data.verifier_data()
    bufs, rows = [], []
    for index in (6, 9):                                  # every level: swap = 0 in one, 1 in the other
        t = R.replay_transcript(data.info, vd, proofs[index], [0, 0, 0, 0])
        b = bytearray(proofs[index])
        b[off + 16 * 24] ^= 1                             # the swap wire's opening at zeta, first coordinate
        bufs += [proofs[index], bytes(b)]
        rows += [t["betas"] + t["gammas"] + [0] * 8 + t["alphas"] + list(t["zeta"])] * 2
    # whole proofs: the openings enter the transcript, so a flipped one fails at the first check behind them in the verifiers'
    # order, the proof-of-work response -- on the host and on the device alike
    codes = [gpu.VERIFY_REASONS[replay.host_reason(gpu, data, b)] for b in bufs]
    assert codes[0] == codes[2] == gpu.VERIFY_OK and gpu.VERIFY_OK not in (codes[1], codes[3])
    assert data.verify_batch(bufs) == codes
    # the vanishing identity alone, under the challenges of the honest proof: both verifiers' evaluators, both swap values
    verdicts = []
    for b, row in zip(bufs, rows):
        terms, n, sides, verdict = (C.c_uint64 * 2048)(), C.c_size_t(), (C.c_uint64 * 8)(), C.c_int(-1)
        assert L.p2_vanishing_terms(data.blob, len(data.blob), b, len(b), (C.c_uint64 * 16)(*row), (C.c_uint64 * 4)(), terms, 1024, C.byref(n), sides,
                                    C.byref(verdict)) == 0, L.p2_last_error()
        verdicts.append(verdict.value)
    assert verdicts == [gpu.VERIFY_OK, gpu.VERIFY_VANISHING] * 2
    flags = (C.c_uint32 * 4)(*([0xFFFFFFFF] * 4))
    assert L.p2_gpu_vanishing_flags(data.gpu(), 4, b"".join(bufs), (C.c_uint64 * 64)(*[w for r in rows for w in r]), (C.c_uint64 * 16)(), flags) == 0
    assert list(flags) == [0, 16, 0, 16]


# ------------------------------------------------------------------ end to end: this ciphertext encrypts a member of the set
def test_membership_and_hashed_elgamal_with_paths_from_the_device(gpu, dev):
    E = gpu.ecgfp5
    depth, cap_height, B = 4, 1, 4
    num_leaves = 1 << (depth + cap_height)
    b = gpu.CircuitBuilder(ec_gate=True)
    m = mc.Membership(gpu, depth, cap_height, 5, builder=b)
    pk_t, nonce_t = b.add_virtual_point_target(), b.add_virtual_biguint320_target()
    c0_t, ct_t = b.hashed_elgamal_encrypt(pk_t, nonce_t, m.leaf)
    b.register_public_inputs([t for h in m.cap for t in h] + c0_t + ct_t)
    data = b.build()
    assert data.info["degree_bits"] == 10 and data.num_public_inputs == 8 + 15

    lv, levels = mc.ref(num_leaves, 5, seed=3)
    tree = gpu.MerkleTree(lv, cap_height)
    cap = tree.cap
    assert cap == mc.ref_cap(levels, cap_height)
    r = random.Random(5)
    idx = [0, 31, 13, 18]
    pk = gpu.ECGFP5SecretKey.rand(77).public_key()
    nonces = [E.random_scalar(100 + k) for k in range(B)]
    sib_t = [t for h in m.sibs for t in h]
    targets = m.leaf + m.bits + [t for h in m.cap for t in h] + pk_t + nonce_t + sib_t
    col, n_t = len(targets) - len(sib_t), len(targets)
    rows = []
    for k, i in enumerate(idx):
        leaf = lv[i] if k != 2 else [r.randrange(P) for _ in range(5)]   # witness 2: a leaf that is not the committed one
        rows += (list(leaf) + [(i >> j) & 1 for j in range(depth + cap_height)] + [w for h in cap for w in h] + list(pk[0]) + list(pk[1]) +
                 [(nonces[k] >> j) & 1 for j in range(320)] + [gpu.VALUE_UNSET] * len(sib_t))
    pb = data.proof_bytes
    d_vals, d_idx, d_mst, d_proofs, d_pst = dev.put(rows), dev.put(idx), dev.alloc(4 * B), dev.alloc(B * pb), dev.alloc(4 * B)
    s = C.c_void_p()
    assert dev.H.hipStreamCreate(C.byref(s)) == 0
    try:
        tree.prove_batch_device(d_idx.value, B, d_vals.value + 8 * col, n_t, d_mst.value, stream=s)
        data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    finally:
        dev.H.hipStreamSynchronize(s)
        dev.H.hipStreamDestroy(s)
    assert dev.get(d_mst, B, C.c_int) == [0] * B and dev.get(d_pst, B, C.c_int) == [0, 0, 1, 0]
    mat = dev.get(d_vals, B * n_t)
    for k, i in enumerate(idx):
        assert mat[k * n_t + col:(k + 1) * n_t] == [w for h in mc.ref_path(levels, cap_height, i) for w in h]
    host = C.create_string_buffer(B * pb)
    assert dev.H.hipMemcpy(host, d_proofs, B * pb, D2H) == 0
    proofs = [host.raw[k * pb:(k + 1) * pb] for k in range(B)]
    good = [p for k, p in enumerate(proofs) if k != 2]
    assert proofs[2] == bytes(pb)
    for k, p in zip((0, 1, 3), good):
        data.verify(p)
        c0, ct = E.hashed_elgamal_encrypt(pk, nonces[k], tuple(lv[idx[k]]))
        assert data.public_inputs(p) == [w for h in cap for w in h] + list(c0[0]) + list(c0[1]) + list(ct)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK, gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_OK]
    cproofs, st = data.compress_batch(good)
    assert st == [gpu.VERIFY_OK] * 3 and all(len(c) < pb for c in cproofs)
    assert data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * 3
    data.verify_compressed(cproofs[0])
    hasher, vd = R.memoised(R.poseidon_hasher()), data.verifier_data()
    assert R.replay(data.info, vd, good[2], hasher, blob=data.blob) is None
    for p in good[:2]:
        assert R.replay(data.info, vd, p, hasher) is None
