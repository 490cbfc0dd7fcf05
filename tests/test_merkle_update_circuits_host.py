"""merkle_update_to_cap in circuits, on the host: a depth-3 tree with a cap of two, every leaf index, witnesses from the host
twin's trace (MerkleTree(device=None).update_batch(..., trace=True)) through p2_host_witness, the CPU oracle and p2_verify -- no
device.  The 16 items of one batch chain: item j takes cap j to cap j + 1.  (The CPU has no prover but the oracle; the byte for
byte comparison of the library's proofs with the oracle's is in tests/test_gpu_merkle_update.py.)"""
import hashlib
import json
import os

import pytest

import circuits
import merkle_cases as mc
import merkle_update_ref as mu
import pi_circuits

P = mu.P
DEPTH, CAP_HEIGHT, LEAF_LEN = 3, 1, 5
NUM_LEAVES = 1 << (DEPTH + CAP_HEIGHT)
ORDER = [(7 * j + 3) % NUM_LEAVES for j in range(NUM_LEAVES)]     # every index once, neighbours apart
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "permute_blobs.json")


@pytest.fixture(scope="module")
def chain(pkg):
    """(circuit, the leaves before, items, the host twin's trace, its caps, the witness of every item)"""
    c = mu.UpdateCircuit(pkg, DEPTH, CAP_HEIGHT, LEAF_LEN, public=False)    # the oracle proves circuits without public inputs
    lv, _ = mc.ref(NUM_LEAVES, LEAF_LEN)
    items = [(i, mu.new_leaf(LEAF_LEN, 20 + i)) for i in ORDER]
    tree = pkg.MerkleTree(lv, CAP_HEIGHT, device=None)
    cap0 = tree.cap
    trace = tree.update_batch([i for i, _ in items], [leaf for _, leaf in items], trace=True)
    caps = trace.caps(cap0)
    model = mu.Update(lv, CAP_HEIGHT, items)
    assert (trace.siblings, caps) == (model.siblings, model.caps)
    maps = [c.witness(lv[i], leaf, i, trace.siblings[j], caps[j], caps[j + 1]) for j, (i, leaf) in enumerate(items)]
    return c, lv, items, trace, caps, maps


def host(pkg, data, m):
    vals, st, f = pkg.host_witness(data.blob, m, ())
    assert f.status == st and (f.kind == "NONE") == (st == 0), f
    return st, f


def test_circuits_without_the_gadget_compile_to_the_blobs_they_compiled_to(pkg):
    want = json.load(open(GOLDEN))
    got = {"poseidon_encrypt_L3": circuits.poseidon_encrypt(pkg, 3, [1])[0].blob, "feistel_poseidon_32": circuits.feistel_poseidon(pkg, [1])[0].blob,
           "public_inputs_small_k9": pi_circuits.small(pkg, 9)[0].blob}
    assert {k: hashlib.sha256(v).hexdigest() for k, v in got.items()} == want


def test_gate_and_op_counts(pkg):
    """two leaf digests and two PoseidonGate rows per level; per cap height h >= 1: verify_merkle_proof_to_cap's h assert_bool and
    8 (2^h - 1) mux ops, then 2 (2^h - 1) - 1 demux ops (the first indicator is the top bit itself) and 4 * 2^h selects of two ops; a root needs no arithmetic at all"""
    for depth, h in ((0, 0), (3, 0), (3, 1), (2, 3)):
        b = pkg.CircuitBuilder()
        old, new, bits = b.add_virtual_target_arr(LEAF_LEN), b.add_virtual_target_arr(LEAF_LEN), b.add_virtual_target_arr(depth + h)
        cap, sibs = b.add_virtual_cap(h), [b.add_virtual_hash() for _ in range(depth)]
        out = b.merkle_update_to_cap(old, new, bits, cap, sibs)
        assert len(out) == 1 << h and all(len(x) == 4 for x in out)
        ops = h + 8 * ((1 << h) - 1) + (2 * ((1 << h) - 1) - 1 + 8 * (1 << h) if h else 0)
        assert b.num_gates() == 2 + 2 * depth + (ops + 19) // 20, (depth, h)
    b = pkg.CircuitBuilder()
    old, new, bits, root, sibs = b.add_virtual_target_arr(3), b.add_virtual_target_arr(3), b.add_virtual_target_arr(2), b.add_virtual_hash(), [b.add_virtual_hash() for _ in range(2)]
    assert len(b.merkle_update(old, new, bits, root, sibs)) == 4 and b.num_gates() == 4      # short leaves are their own digests


@pytest.mark.parametrize("j", range(NUM_LEAVES))
def test_the_host_interpreter_accepts_every_item_of_the_chain(pkg, chain, j):
    c, lv, items, trace, caps, maps = chain
    assert host(pkg, c.data, maps[j])[0] == 0


@pytest.mark.parametrize("j", (0, 5, 10, 15))
def test_wrong_transitions_are_generator_conflicts(pkg, chain, j):
    c, lv, items, trace, caps, maps = chain
    i, leaf = items[j]
    sibs = [list(h) for h in trace.siblings[j]]
    sibs[1][2] = (sibs[1][2] + 1) % P
    wrong_cap = [list(h) for h in caps[j + 1]]
    wrong_cap[(i >> DEPTH) ^ 1][0] ^= 1                    # the entry the update does NOT touch
    wrong_root = [list(h) for h in caps[j + 1]]
    wrong_root[i >> DEPTH][3] ^= 1                        # the entry it does
    stale_leaf = list(lv[i])
    stale_leaf[-1] = (stale_leaf[-1] + 1) % P
    wrong = {"a wrong new_cap entry (untouched side)": c.witness(lv[i], leaf, i, trace.siblings[j], caps[j], wrong_cap),
             "a wrong new_cap entry (the new root)": c.witness(lv[i], leaf, i, trace.siblings[j], caps[j], wrong_root),
             "a wrong sibling": c.witness(lv[i], leaf, i, sibs, caps[j], caps[j + 1]),
             "an old leaf that is not the committed one": c.witness(stale_leaf, leaf, i, trace.siblings[j], caps[j], caps[j + 1]),
             "the cap before the previous item": c.witness(lv[i], leaf, i, trace.siblings[j], caps[j - 1] if j else caps[2], caps[j + 1])}
    for label, w in wrong.items():
        st, f = host(pkg, c.data, w)
        assert (st, f.kind) == (1, "GENERATOR_CONFLICT"), label


def test_a_cap_index_bit_of_two_is_refused(pkg, chain):
    """with both old cap entries equal the mux gives the entry whatever the bit, and with the claimed cap set to what the demux
    makes of a bit of 2 (indicators -1 and 2) every other constraint holds: only assert_bool refuses"""
    c, lv, items, trace, caps, maps = chain
    j = ORDER.index(9)
    i, leaf = items[j]
    assert i >> DEPTH == 1
    e, root = caps[j][1], caps[j + 1][1]
    w = c.witness(lv[i], leaf, i, trace.siblings[j], [e, e], [e, root])
    assert host(pkg, c.data, w)[0] == 0
    select = lambda b, x, y: [(b * xi - (b * yi - yi)) % P for xi, yi in zip(x, y)]   # noqa: E731
    for bit, want in ((1, 0), (0, 0), (2, 1), (P - 1, 1)):
        ind = [(1 - bit) % P, bit]
        w = c.witness(lv[i], leaf, i, trace.siblings[j], [e, e], [select(ind[0], root, e), select(ind[1], root, e)])
        w[c.bits[DEPTH]] = bit
        st, f = host(pkg, c.data, w)
        assert st == want and (f.kind == "GENERATOR_CONFLICT") == bool(want), (bit, f)


def test_length_mismatches_are_invalid(pkg):
    b = pkg.CircuitBuilder()
    old, new, bits, cap, sibs = b.add_virtual_target_arr(5), b.add_virtual_target_arr(5), b.add_virtual_target_arr(4), b.add_virtual_cap(1), [b.add_virtual_hash() for _ in range(3)]
    gates = b.num_gates()
    L, u64 = pkg.lib(), __import__("ctypes").c_uint64
    arr = lambda ts: (u64 * len(ts))(*ts)                   # noqa: E731
    flat = lambda hs: arr([t for h in hs for t in h])     # noqa: E731
    out = (u64 * 8)()
    for n_bits, cap_height, n_sib, leaf_len in ((3, 1, 3, 5), (4, 1, 2, 5), (4, 0, 3, 5), (4, 1, 3, 0), (4, 17, 3, 5), (4, -1, 3, 5)):
        assert L.p2_builder_merkle_update_to_cap(b._h, arr(old), arr(new), leaf_len, arr(bits), n_bits, flat(cap), cap_height, flat(sibs), n_sib, out) == 1, (n_bits, cap_height, n_sib)
        assert L.p2_last_error()
    assert L.p2_builder_merkle_update(b._h, arr(old), arr(new), 5, arr(bits), 4, arr(cap[0]), flat(sibs), 3, out) == 1
    for call in (lambda: b.merkle_update_to_cap(old, new[:4], bits, cap, sibs), lambda: b.merkle_update_to_cap(old, new, bits, cap + cap[:1], sibs),
                 lambda: b.merkle_update_to_cap(old, new, bits, cap, sibs + [sibs[0][:3]]), lambda: b.merkle_update(old, new, bits, cap[0], sibs)):
        with pytest.raises(pkg.P2Error):
            call()
    assert b.num_gates() == gates                         # a refused call adds nothing
    b.merkle_update(old, new, bits[:3], cap[0], sibs)     # the builder is still usable
    b.build()


def test_the_oracle_proves_the_chain_and_the_host_verifier_accepts(pkg, orc, chain):
    """the first item and those that write leaves 6 = 0110 and 9 = 1001: every level sees swap = 0 and swap = 1 on both walks"""
    c, lv, items, trace, caps, maps = chain
    oc = orc.OracleCircuit(c.data.blob)
    vd = oc.verifier_data()
    js = sorted({ORDER.index(6), ORDER.index(9), 0})
    for j in js:
        st, proof = oc.prove(maps[j])
        assert st == 0 and len(proof) == c.data.proof_bytes
        c.data.verify(proof, vd)
        if j == js[0]:
            assert oc.prove(maps[j])[1] == proof          # deterministic: the GPU test compares the library's proofs with these byte for byte
            bad = bytearray(proof)
            bad[len(bad) // 2] ^= 1
            with pytest.raises(pkg.P2Error):
                c.data.verify(bytes(bad), vd)
    wrong = dict(maps[js[-1]])
    wrong[c.sibs[1][0]] ^= 1
    assert oc.prove(wrong)[0] == 1
