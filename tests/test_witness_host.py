"""Witness outputs and fault diagnosis on the host (CPU): p2_host_witness, the sequential twin of the device's witness run
and the check function the device kernels share with it (csrc/witness_check.h).

Three kinds of evidence:
  * against the CPU oracle (which runs the same compiled op program): statuses, and every routed wire read back as an out-target;
  * against values that do not come from the op program at all: the Python value of every node of a random circuit built here,
    the AES-GCM known answers of tests/golden/aes_kat.json, the native ElGamal / poseidon-cipher results -- with ONLY the
    inputs set, so the circuit has to compute what it is asked for;
  * the fault record for each way a witness can fail, and the interface rules of include/p2aes.h.
All comparisons are of field elements, bytes and status codes: exact."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import blob_reader
import circuits
import device_build as device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "aes_kat.json")))
WIRE = 1 << 63


def wire(row, col):
    return WIRE | (row << 8) | col


class FullBlob(blob_reader.Blob):
    """blob_reader.Blob read on to the witness program: num_slots, ops, level offsets, vt_slot, wire_slot [80][n]."""

    def __init__(self, data):
        super().__init__(data)
        self.num_slots = self.u32()
        self.ops = self.arr("<u1", 40).reshape(-1, 40)
        self.level_offsets = self.arr("<u4")
        self.vt_slot = self.arr("<i4")
        self.wire_slot = self.arr("<i4").reshape(80, self.n)


def wired_targets(blob):
    """Every routed wire with a slot, column-major like the oracle's wire matrix: (targets, flat indices col * n + row)."""
    fb = FullBlob(blob)
    idx = np.flatnonzero(fb.wire_slot.reshape(-1) >= 0)
    cols, rows = idx // fb.n, idx % fb.n
    return [wire(int(r), int(c)) for r, c in zip(rows, cols)], idx, fb


def kind_matches_status(f):
    return {"NONE": 0, "NOT_SET": 2}.get(f.kind, 1) == f.status


def check_against_oracle(pkg, orc, data, pws, break_one=True):
    """Statuses equal the oracle's on the honest witnesses and on two broken ones; every wired slot equals the oracle's matrix."""
    oc = orc.OracleCircuit(data.blob)
    targets, idx, fb = wired_targets(data.blob)
    for k in (0, len(idx) // 2, len(idx) - 1):   # the blob's table is the oracle's
        assert oc.wire_slot(int(idx[k] // fb.n), int(idx[k] % fb.n)) == fb.wire_slot.reshape(-1)[idx[k]]
    cases = [dict(pw.map) for pw in pws]
    if break_one:
        m = dict(pws[0].map)
        last = list(m)[-1]
        wrong = dict(m)
        wrong[last] = (m[last] + 1) % 256 if m[last] < 256 else (m[last] + 1) % P   # stays a byte where the target is one
        missing = dict(m)
        del missing[list(m)[0]]
        cases += [wrong, missing]
    seen = set()
    for m in cases:
        st_o, wires_o = oc.generate_witness(m, 135 << fb.degree_bits)
        vals, st_h, f = pkg.host_witness(data.blob, m, targets)
        assert st_h == st_o
        assert kind_matches_status(f), f
        seen.add(st_h)
        if st_o == 0:
            assert np.array_equal(np.array(vals, dtype=np.uint64), np.array(wires_o, dtype=np.uint64)[idx])
    return seen


# ------------------------------------------------------------------ host twin against the oracle
def test_small_circuits_against_the_oracle(pkg, orc):
    assert check_against_oracle(pkg, orc, *circuits.assert_byte(pkg, [0, 77, 255]), break_one=False) == {0}
    data, _ = circuits.assert_byte(pkg, [0])
    oc = orc.OracleCircuit(data.blob)
    t = list(circuits.assert_byte(pkg, [0])[1][0].map)[0]
    for m in ({t: 256}, {}):   # not a byte: the range check's lookup misses; nothing set: the lookup never runs
        assert pkg.host_witness(data.blob, m)[1] == oc.generate_witness(m, 135 << data.info["degree_bits"])[0] != 0
    assert check_against_oracle(pkg, orc, *circuits.gf_2_8_add(pkg, [(1, 2), (255, 255), (0x57, 0x83)])) == {0, 1, 2}
    assert check_against_oracle(pkg, orc, *circuits.arithmetic_only(pkg, [(3, 5, 7, 64), (P - 1, P - 2, 5, 1), (2, 3, 4, 34)])) == {0, 1, 2}


def test_aes_circuits_against_the_oracle(pkg, orc):
    key, block = bytes(range(16)), bytes(range(16, 32))
    assert check_against_oracle(pkg, orc, *circuits.encrypt_block(pkg, key, block)) == {0, 1, 2}
    data, pws, _ = circuits.encrypt(pkg, 4, 13, True)
    assert check_against_oracle(pkg, orc, data, pws) == {0, 1, 2}


def test_poseidon_circuits_against_the_oracle(pkg, orc):
    data, pws, _, _ = circuits.poseidon_encrypt(pkg, 3, [1, 2])
    assert check_against_oracle(pkg, orc, data, pws) == {0, 1, 2}
    assert check_against_oracle(pkg, orc, *circuits.feistel_poseidon(pkg, [5])) == {0, 1, 2}


@pytest.mark.parametrize("seed", range(8))
def test_random_circuits_against_the_oracle(pkg, orc, seed):
    data, pws = circuits.random_circuit(pkg, orc, seed)
    assert 0 in check_against_oracle(pkg, orc, data, pws)


@pytest.fixture(scope="module")
def elgamal(pkg):
    return circuits.ecgfp5_elgamal(pkg, [7])


def test_elgamal_against_the_oracle(pkg, orc, elgamal):
    data, pws, _, _ = elgamal
    assert check_against_oracle(pkg, orc, data, pws) == {0, 1, 2}


# ------------------------------------------------------------------ independent values
def _aes_sbox():
    """The AES S-box from its definition: inverse in GF(2^8) mod x^8 + x^4 + x^3 + x + 1, then the affine map."""
    def mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a = (a << 1) ^ (0x11B if a & 0x80 else 0)
            b >>= 1
        return r
    box = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if mul(x, y) == 1), 0)
        box.append(inv ^ (inv << 1 | inv >> 7) & 0xFF ^ (inv << 2 | inv >> 6) & 0xFF ^ (inv << 3 | inv >> 5) & 0xFF ^ (inv << 4 | inv >> 4) & 0xFF ^ 0x63)
    return box


SBOX = _aes_sbox()


def node_circuit(pkg, seed, n_ops=60):
    """A random circuit over the builder's vocabulary (add, sub, mul, mul_const_add, is_equal + select, S-box lookups, connect of
    two computed values, in-circuit Poseidon sponges) that keeps the Python value of EVERY node.  Returns (data, inputs as
    target -> value, nodes as [(target, value)])."""
    r = random.Random(1000 + seed)
    b = pkg.CircuitBuilder()
    lut = b.sbox_lut()
    nodes, inputs = [], {}
    for i in range(r.randrange(3, 7)):
        byte = i % 2 == 0
        t = b.add_virtual_byte_target(lut) if byte else b.add_virtual_target()
        v = r.randrange(256) if byte else r.choice([0, 1, P - 1, r.randrange(P)])
        nodes.append((t, v))
        inputs[t] = v
    for c in (0, 1, 255, P - 3):
        nodes.append((b.constant(c), c))
    for _ in range(n_ops):
        kind = r.choice(["add", "sub", "mul", "mca", "select", "sbox", "connect", "hash"])
        (x, xv), (y, yv), (z, zv) = (r.choice(nodes) for _ in range(3))
        if kind == "add":
            nodes.append((b.add(x, y), (xv + yv) % P))
        elif kind == "sub":
            nodes.append((b.sub(x, y), (xv - yv) % P))
        elif kind == "mul":
            nodes.append((b.mul(x, y), xv * yv % P))
        elif kind == "mca":
            k = r.choice([3, 1 << 32, P - 1, r.randrange(P)])
            nodes.append((b.mul_const_add(k, x, y), (k * xv + yv) % P))
        elif kind == "select":
            e = b.is_equal(x, y)
            nodes.append((e, int(xv == yv)))
            nodes.append((b.select(e, z, x), zv if xv == yv else xv))
        elif kind == "sbox":
            t, v = r.choice([nd for nd in nodes if nd[1] < 256])
            nodes.append((b.add_lookup_from_index(t, lut), SBOX[v]))
        elif kind == "connect":
            t1, t2 = b.add(x, y), b.add(y, x)
            if t1 != t2:
                b.connect(t1, t2)
            nodes += [(t1, (xv + yv) % P), (t2, (xv + yv) % P)]
        else:
            ins = [r.choice(nodes) for _ in range(r.randrange(1, 11))]
            m = r.randrange(1, 10)
            outs = b.hash_n_to_m_no_pad([t for t, _ in ins], m)
            nodes += list(zip(outs, pkg.poseidon_native.hash_n_to_m_no_pad([v for _, v in ins], m)))
    return b.build(), inputs, nodes


@pytest.mark.parametrize("seed", range(8))
def test_every_node_of_a_random_circuit_reads_back_as_its_python_value(pkg, seed):
    data, inputs, nodes = node_circuit(pkg, seed)
    vals, st, f = pkg.host_witness(data.blob, inputs, [t for t, _ in nodes])
    assert st == 0 and f.kind == "NONE"
    assert vals == [v for _, v in nodes]


_GCM = {}


def gcm_circuit(pkg, nk, L, tag):
    if (nk, L, tag) not in _GCM:
        b = pkg.CircuitBuilder()
        t = pkg.AesGcmTarget.build(b, nk, nk + 6, L, tag)
        _GCM[nk, L, tag] = (b.build(), t)
    return _GCM[nk, L, tag]


def gcm_inputs(t, key, iv, pt, tag_zero):
    m = dict(zip(t.key + t.nonce + t.pt, bytes(key) + bytes(iv) + bytes(pt)))
    if tag_zero:
        m.update({x: 0 for x in t.tag})   # TAG = false: the tag targets exist, are range-checked and nothing computes them
    return m


GCM_VECTORS = [v for v in GOLD["cavp_gcm128"] + GOLD["derived_by_pinned_oracle"] if v["pt"]]


@pytest.mark.parametrize("i", range(len(GCM_VECTORS)))
def test_aes_gcm_known_answers_are_computed_from_the_inputs_alone(pkg, i):
    v = GCM_VECTORS[i]
    key, iv, pt = bytes.fromhex(v["key"]), bytes.fromhex(v["iv"]), bytes.fromhex(v["pt"])
    with_tag = i % 2 == 0   # both builds of the target over the vectors
    data, t = gcm_circuit(pkg, len(key) // 4, len(pt), with_tag)
    vals, st, f = pkg.host_witness(data.blob, gcm_inputs(t, key, iv, pt, not with_tag), t.ct + t.tag)
    assert st == 0 and f.kind == "NONE"
    assert bytes(vals[: len(pt)]).hex() == v["ct"]
    assert bytes(vals[len(pt):]).hex() == (v["tag"] if with_tag else "00" * 16)


def flat(point):
    return list(point[0]) + list(point[1])


def test_elgamal_pair_is_computed_from_the_inputs_alone(pkg, elgamal):
    data, pws, (pk_t, nonce_t, msg_t, ct_t), cases = elgamal
    _, pk, msg, nonce, ct = cases[0]
    m = dict(zip(pk_t + msg_t + nonce_t, flat(pk) + flat(msg) + [(nonce >> i) & 1 for i in range(320)]))
    vals, st, f = pkg.host_witness(data.blob, m, ct_t[0] + ct_t[1])
    assert st == 0 and f.kind == "NONE"
    assert vals == flat(ct[0]) + flat(ct[1]) == flat(pkg.ecgfp5.elgamal_encrypt(pk, nonce, msg)[0]) + flat(pkg.ecgfp5.elgamal_encrypt(pk, nonce, msg)[1])


def test_hashed_elgamal_and_public_key_are_computed_from_the_inputs_alone(pkg):
    data, _, (pk_t, nonce_t, msg_t, ct_t), cases = circuits.ecgfp5_hashed_elgamal(pkg, [3])
    _, pk, msg, nonce, ct = cases[0]
    m = dict(zip(pk_t + msg_t + nonce_t, flat(pk) + list(msg) + [(nonce >> i) & 1 for i in range(320)]))
    vals, st, _ = pkg.host_witness(data.blob, m, ct_t[0] + ct_t[1])
    assert st == 0 and vals == flat(ct[0]) + list(ct[1])
    data, _, (sk_t, pk_t), cases = circuits.ecgfp5_public_key(pkg, [4])
    sk, pk = cases[0]
    vals, st, _ = pkg.host_witness(data.blob, dict(zip(sk_t, [(sk.value >> i) & 1 for i in range(320)])), pk_t)
    assert st == 0 and vals == flat(pk) == flat(pkg.ecgfp5.mul(sk.value, pkg.ecgfp5.generator()))


def test_poseidon_cipher_text_is_computed_from_the_inputs_alone(pkg):
    data, _, t, cases = circuits.poseidon_encrypt(pkg, 3, [11, 12])
    for ks, msg, nonce, ct in cases:
        m = dict(zip(t.ks + t.m + t.nonce, [v for fq in ks for v in fq] + [v for fq in msg for v in fq] + list(nonce)))
        vals, st, f = pkg.host_witness(data.blob, m, t.ct)
        assert st == 0 and f.kind == "NONE"
        assert vals == [v for fq in pkg.poseidon_native.encrypt(ks, msg, nonce) for v in fq] == [v for fq in ct for v in fq]


# ------------------------------------------------------------------ faults
KAT13 = GOLD["derived_by_pinned_oracle"][0]   # AES-128, 13 bytes: test_encrypt's inputs


@pytest.fixture(scope="module")
def gcm13(pkg):
    data, t = gcm_circuit(pkg, 4, 13, True)
    key, iv, pt = (bytes.fromhex(KAT13[k]) for k in ("key", "iv", "pt"))
    honest = gcm_inputs(t, key, iv, pt, False)
    honest.update(zip(t.ct + t.tag, bytes.fromhex(KAT13["ct"]) + bytes.fromhex(KAT13["tag"])))
    return data, t, honest


def explain(pkg, data, m):
    _, st, f = pkg.host_witness(data.blob, m)
    assert f.status == st and kind_matches_status(f), f
    return f


def test_fault_none(pkg, gcm13):
    data, t, honest = gcm13
    f = explain(pkg, data, honest)
    assert (f.kind, f.status, f.op_kind, f.input_index, f.target, f.gate_row) == ("NONE", 0, None, None, None, None)


def test_fault_input_not_canonical(pkg, gcm13):
    data, t, honest = gcm13
    m = dict(honest)
    m[t.nonce[4]] = P + 3
    f = explain(pkg, data, m)
    assert (f.kind, f.status, f.input_index, f.found, f.target) == ("INPUT_NOT_CANONICAL", 1, list(m).index(t.nonce[4]), P + 3, t.nonce[4])
    m[t.key[1]] = P   # an earlier entry: the lowest index wins
    assert explain(pkg, data, m).input_index == list(m).index(t.key[1])


def test_fault_input_conflict(pkg):
    b = pkg.CircuitBuilder()
    x, y, z = (b.add_virtual_target() for _ in range(3))
    b.connect(x, y)
    out = b.add(b.mul(x, y), z)
    data = b.build()
    assert pkg.host_witness(data.blob, {x: 5, y: 5, z: 1}, [out])[:2] == ([26], 0)
    f = explain(pkg, data, {z: 1, x: 5, y: 6})
    assert (f.kind, f.status, f.input_index, f.computed, f.found, f.target) == ("INPUT_CONFLICT", 1, 2, 5, 6, min(x, y))


def test_fault_lookup_miss(pkg, gcm13):
    data, t, honest = gcm13
    m = dict(honest)
    m[t.key[7]] = 256
    f = explain(pkg, data, m)
    assert (f.kind, f.status, f.op_kind, f.found, f.input_index, f.target) == ("LOOKUP_MISS", 1, "LOOKUP", 256, list(m).index(t.key[7]), t.key[7])
    assert f.gate_row is not None


def test_fault_generator_conflict_names_the_wrong_ciphertext_byte(pkg, gcm13):
    data, t, honest = gcm13
    m = dict(honest)
    right = bytes.fromhex(KAT13["ct"])[5]
    m[t.ct[5]] = right ^ 0x40
    f = explain(pkg, data, m)
    assert (f.kind, f.status, f.input_index, f.computed, f.found, f.target) == ("GENERATOR_CONFLICT", 1, list(m).index(t.ct[5]), right, right ^ 0x40, t.ct[5])
    assert f.op_kind in pkg.OP_KINDS and f.gate_row is not None


def test_fault_not_set_names_the_missing_plaintext_byte(pkg, gcm13):
    data, t, honest = gcm13
    m = dict(honest)
    del m[t.pt[3]]
    f = explain(pkg, data, m)
    assert (f.kind, f.status, f.target, f.input_index, f.op_kind) == ("NOT_SET", 2, t.pt[3], None, None)
    del m[t.key[0]]   # two missing: the lowest target
    assert explain(pkg, data, m).target == min(t.pt[3], t.key[0])


def test_fault_not_set_names_the_tag_of_a_target_built_without_tag(pkg):
    v = GOLD["derived_by_pinned_oracle"][1]
    key, iv, pt = (bytes.fromhex(v[k]) for k in ("key", "iv", "pt"))
    data, t = gcm_circuit(pkg, 4, 17, False)
    m = dict(zip(t.key + t.nonce + t.pt, key + iv + pt))   # what a caller who wants the ciphertext would set
    vals, st, f = pkg.host_witness(data.blob, m, t.ct)
    assert (f.kind, st, f.target) == ("NOT_SET", 2, t.tag[0]) and kind_matches_status(f)
    assert bytes(vals).hex() == v["ct"]   # computed all the same
    m.update({x: 0 for x in t.tag})
    assert pkg.host_witness(data.blob, m, t.ct)[:2] == (list(bytes.fromhex(v["ct"])), 0)


def test_two_faults_report_the_first_in_order(pkg, gcm13):
    data, t, honest = gcm13
    wrong_ct = dict(honest)
    wrong_ct[t.ct[5]] ^= 1
    m = dict(wrong_ct)
    del m[t.pt[3]]   # a conflict and a missing input: the conflict (status 1)
    f = explain(pkg, data, m)
    assert (f.kind, f.target) == ("GENERATOR_CONFLICT", t.ct[5])
    m = dict(wrong_ct)
    m[t.key[9]] = 300   # a lookup miss and a conflict: the generator that comes first in the blob's op order
    f = explain(pkg, data, m)
    assert (f.kind, f.found) == ("LOOKUP_MISS", 300)
    m[t.tag[15]] = P + 1   # and a non-canonical value: before both
    assert explain(pkg, data, m).kind == "INPUT_NOT_CANONICAL"


# ------------------------------------------------------------------ interface
def test_out_targets_outside_the_circuit_are_invalid(pkg, gcm13):
    data, t, honest = gcm13
    fb = FullBlob(data.blob)
    col, row = (int(x) for x in np.argwhere(fb.wire_slot < 0)[0])
    for bad in (len(fb.vt_slot), len(fb.vt_slot) + 12345, wire(row, col), wire(fb.n, 0), wire(0, 80)):
        with pytest.raises(pkg.P2Error, match="output target is not a target of this circuit"):
            pkg.host_witness(data.blob, honest, [t.ct[0], bad])
    with pytest.raises(pkg.P2Error, match="input target is not a target of this circuit"):
        pkg.host_witness(data.blob, {len(fb.vt_slot): 1})


def test_no_outputs_and_duplicate_outputs(pkg, gcm13):
    data, t, honest = gcm13
    assert pkg.host_witness(data.blob, honest, [])[:2] == ([], 0)
    ct = list(bytes.fromhex(KAT13["ct"]))
    vals, st, _ = pkg.host_witness(data.blob, honest, [t.ct[2], t.ct[2], t.ct[0], t.ct[2]], explain=False)
    assert (vals, st) == ([ct[2], ct[2], ct[0], ct[2]], 0)
    # a routed wire reads the slot it shares with a virtual target
    targets, idx, fb = wired_targets(data.blob)
    slot = fb.vt_slot[t.ct[4]]
    k = int(np.flatnonzero(fb.wire_slot.reshape(-1)[idx] == slot)[0])
    assert pkg.host_witness(data.blob, honest, [targets[k], t.ct[4]])[0] == [ct[4], ct[4]]
    # an unset target reads as VALUE_UNSET
    m = dict(honest)
    del m[t.pt[3]]
    assert pkg.host_witness(data.blob, m, [t.pt[3], t.pt[2]])[0] == [pkg.VALUE_UNSET, honest[t.pt[2]]]


def test_null_handles_and_no_device_are_errors_not_crashes(pkg):
    L = pkg.lib()
    want = 1 if L.p2_gpu_device_count() > 0 else 2   # P2_ERR_INVALID for a null handle; P2_ERR_NO_DEVICE where there can be none
    st, vals, out1 = (C.c_int * 1)(), (C.c_uint64 * 1)(), (C.c_uint64 * 1)(0)
    a, keep = pkg.api._assignment({0: 1})
    assert L.p2_witness_batch(None, 1, C.byref(a), out1, 1, vals, st) == want
    assert L.p2_witness_batch_device(None, 1, out1, 1, None, out1, 1, None, None, None) == want
    assert L.p2_prove_batch_outputs(None, 1, C.byref(a), out1, 1, vals, None, st) == want
    assert L.p2_prove_batch_outputs_device(None, 1, out1, 1, None, out1, 1, None, None, None, None) == want
    assert L.p2_witness_explain(None, C.byref(a), st, None) == want
    assert L.p2_last_error()
    if want == 2:
        assert not L.p2_circuit_load(b"", 0, 0) and b"no HIP device" in L.p2_last_error()
    assert L.p2_host_witness(None, 0, C.byref(a), None, 0, None, st, None) == 1
    assert L.p2_host_witness(b"P2AESCIR", 8, C.byref(a), None, 0, None, st, None) == 1   # a truncated blob


def test_fault_kinds_agree_with_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "p2aes.h")).read()
    kinds = {name: int(v) for name, v in re.findall(r"P2_FAULT_(\w+) = (\d+)", header)}
    assert kinds == {name: i for i, name in enumerate(pkg.FAULT_KINDS)}
    circuit_h = open(os.path.join(ROOT, "plonky2-aes_amd", "csrc", "circuit.h")).read()
    ops = {name: int(v) for name, v in re.findall(r"^\s+OP_(\w+) = (\d+),", circuit_h, flags=re.M)}
    assert ops == {name: i for i, name in enumerate(pkg.OP_KINDS)}
    assert "#define P2_VALUE_UNSET UINT64_MAX" in header and pkg.VALUE_UNSET == 2**64 - 1
    assert not pkg.lib()._p2_missing


@pytest.mark.parametrize("fragment", ["k_gather_slots", "k_witness_wired_unset", "k_witness_check", "k_witness_report"])
def test_new_kernels_use_no_scratch(fragment):
    remarks = device.cross_compile()[0]
    found = [v for name, v in remarks.items() if fragment in name]
    assert found, fragment
    for k in found:
        assert k["ScratchSize"] == 0, k
