"""Merkle membership in circuits, on the host: permute_swapped, hash_or_noop, add_virtual_hash / _cap, connect_hashes and
verify_merkle_proof_to_cap through p2_host_witness, the CPU oracle and p2_verify -- no device.  The gadget is the first
producer of PoseidonGate rows whose swap wire is not the constant zero: the 16 indices of the depth-3, cap-height-1 tree put
both swap values on every level.  Paths and caps come from tests/merkle_ref.py (the oracle's hash)."""
import hashlib
import json
import os

import pytest

import circuits
import merkle_cases as mc
import pi_circuits

P = mc.P
DEPTH, CAP_HEIGHT, LEAF_LEN = 3, 1, 5
NUM_LEAVES = 1 << (DEPTH + CAP_HEIGHT)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "permute_blobs.json")


@pytest.fixture(scope="module")
def member(pkg):
    return mc.Membership(pkg, DEPTH, CAP_HEIGHT, LEAF_LEN), mc.ref(NUM_LEAVES, LEAF_LEN)


def host(pkg, data, m, outs=()):
    vals, st, f = pkg.host_witness(data.blob, m, outs)
    assert f.status == st and (f.kind == "NONE") == (st == 0), f
    return vals, st, f


def test_circuits_that_use_permute_compile_to_the_blobs_they_compiled_to(pkg):
    """tests/golden/permute_blobs.json: SHA-256 of the blobs as the builder made them when permute had no swap argument"""
    want = json.load(open(GOLDEN))
    got = {"poseidon_encrypt_L3": circuits.poseidon_encrypt(pkg, 3, [1])[0].blob, "feistel_poseidon_32": circuits.feistel_poseidon(pkg, [1])[0].blob,
           "public_inputs_small_k9": pi_circuits.small(pkg, 9)[0].blob}
    assert {k: hashlib.sha256(v).hexdigest() for k, v in got.items()} == want


def test_permute_swapped_with_zero_is_permute(pkg):
    """hash_n_to_m_no_pad's row and the same row through permute_swapped(.., zero()): one blob"""
    def build(swapped):
        b = pkg.CircuitBuilder()
        xs = b.add_virtual_target_arr(8)
        if swapped:
            b.permute_swapped(xs + [b.zero()] * 4, b.zero())
        else:
            b.hash_n_to_m_no_pad(xs, 4)
        return b.build().blob
    assert build(True) == build(False)


def test_permute_swapped_exchanges_the_first_two_quarters(pkg):
    b = pkg.CircuitBuilder()
    xs, swap = b.add_virtual_target_arr(12), b.add_virtual_target()
    out = b.permute_swapped(xs, swap)
    data = b.build()
    vals = [(i + 1) * 0x0123456789ABCDEF % P for i in range(12)]
    plain = pkg.poseidon_native.hash_n_to_m_no_pad  # (rate 8: not the tool for a 12-word state; the sponge of 8 words with a zero capacity is)
    vals[8:] = [0, 0, 0, 0]
    for s in (0, 1):
        got, st, _ = host(pkg, data, dict(zip(xs + [swap], vals + [s])), out[:8])
        v = vals[4:8] + vals[:4] if s else vals[:8]
        assert st == 0 and got == plain(v, 8)
    assert host(pkg, data, dict(zip(xs + [swap], vals + [2])))[1] == 0   # the generator takes any swap; the gate's constraint refuses it at proving time


def test_hash_or_noop_pads_short_leaves_and_hashes_long_ones(pkg):
    for n in (1, 4, 5, 9):
        b = pkg.CircuitBuilder()
        xs = b.add_virtual_target_arr(n)
        gates = b.num_gates()
        h = b.hash_or_noop(xs)
        assert b.num_gates() - gates == (0 if n <= 4 else (n + 7) // 8)
        y = b.add_virtual_hash()
        b.connect_hashes(h, y)
        data = b.build()
        vals = [P - 1 - i for i in range(n)]
        got, st, _ = host(pkg, data, dict(zip(xs, vals)), y)
        assert st == 0 and got == (vals + [0] * (4 - n) if n <= 4 else pkg.poseidon_native.hash_n_to_m_no_pad(vals, 4))


def test_gate_and_op_counts(pkg):
    """per level one PoseidonGate row; per cap height h: h assert_bool ops and (2^h - 1) * 4 selects of two ops each"""
    for depth, h in ((0, 0), (3, 0), (3, 1), (2, 3)):
        b = pkg.CircuitBuilder()
        mc.Membership(pkg, depth, h, LEAF_LEN, builder=b)
        ops = h + 8 * ((1 << h) - 1)
        assert b.num_gates() == 1 + depth + (ops + 19) // 20, (depth, h)


@pytest.mark.parametrize("index", range(NUM_LEAVES))
def test_the_honest_path_is_accepted_at_every_index(pkg, member, index):
    m, (lv, levels) = member
    assert host(pkg, m.data, m.honest(lv, levels, index))[1] == 0


@pytest.mark.parametrize("index", (0, 5, 10, 15))
def test_wrong_paths_are_generator_conflicts(pkg, member, index):
    m, (lv, levels) = member
    wrong = {}
    for label, lf, ix, sb, cp, want in mc.tampered(lv, levels, CAP_HEIGHT, index):
        if want == 1 and ix < NUM_LEAVES:
            wrong[label] = m.witness(lf, ix, sb, cp)
    assert set(wrong) == {"leaf word", "cap word", "sibling word", "path bit", "cap bit"}
    for label, w in wrong.items():
        _, st, f = host(pkg, m.data, w)
        assert (st, f.kind) == (1, "GENERATOR_CONFLICT"), label


def test_a_cap_index_bit_of_two_is_refused(pkg, member):
    """with both cap entries equal the mux gives the entry whatever the bit (2 x - (2 x - x) = x): only assert_bool stands
    between a bit of 2 and an accepted witness"""
    m, (lv, levels) = member
    cap = mc.ref_cap(levels, CAP_HEIGHT)
    w = m.witness(lv[9], 9, mc.ref_path(levels, CAP_HEIGHT, 9), [cap[1], cap[1]])
    assert host(pkg, m.data, w)[1] == 0
    for bit, want in ((0, 0), (2, 1), (P - 1, 1)):
        w[m.bits[DEPTH]] = bit
        _, st, f = host(pkg, m.data, w)
        assert st == want and (f.kind == "GENERATOR_CONFLICT") == bool(want), (bit, f)


def test_length_mismatches_are_invalid(pkg):
    b = pkg.CircuitBuilder()
    leaf, bits, cap, sibs = b.add_virtual_target_arr(5), b.add_virtual_target_arr(4), b.add_virtual_cap(1), [b.add_virtual_hash() for _ in range(3)]
    for call in (lambda: b.verify_merkle_proof_to_cap(leaf, bits[:3], cap, sibs), lambda: b.verify_merkle_proof_to_cap(leaf, bits, cap, sibs[:2]),
                 lambda: b.verify_merkle_proof_to_cap(leaf, bits, cap + cap[:1], sibs), lambda: b.verify_merkle_proof_to_cap([], bits, cap, sibs),
                 lambda: b.verify_merkle_proof(leaf, bits, cap[0], sibs), lambda: b.add_virtual_cap(17), lambda: b.permute_swapped(leaf, bits[0])):
        with pytest.raises(pkg.P2Error):
            call()
    b.verify_merkle_proof(leaf, bits[:3], cap[0], sibs)   # the builder is still usable
    b.build()


def test_the_oracle_proves_the_blob_and_the_host_verifier_accepts(pkg, orc, member):
    """indices 6 = 0110 and 9 = 1001: every level sees swap = 0 in one proof and swap = 1 in the other"""
    m, (lv, levels) = member
    oc = orc.OracleCircuit(m.data.blob)
    vd = oc.verifier_data()
    for index in (6, 9):
        st, proof = oc.prove(m.honest(lv, levels, index))
        assert st == 0 and len(proof) == m.data.proof_bytes
        m.data.verify(proof, vd)
    wrong = m.honest(lv, levels, 6)
    wrong[m.sibs[1][0]] ^= 1
    assert oc.prove(wrong)[0] == 1
