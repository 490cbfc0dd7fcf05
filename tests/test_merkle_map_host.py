"""MerkleMap on the host: the reference (tests/merkle_map_ref.py) checked in its own right, the host twin
(pkg.MerkleMap(device=None), p2_native_merkle_map_*) against it on every subset of the small key spaces and on the D = 64 keys,
its refusals and verify statuses, and the four gadgets on a D = 3, h = 1 map through p2_host_witness, the CPU oracle and
p2_verify -- no device."""
import ctypes as C
import itertools

import pytest

import merkle_map_cases as mc
import merkle_map_ref as ref
import merkle_ref

P = ref.P
P2_ERR_INVALID = 1                       # include/p2aes.h


# ---- the reference itself
def test_reference_dense_map_is_the_dense_tree():
    for value_len in mc.VALUE_LENS:
        for h in (0, 2):
            m = mc.model(tuple(range(16)), 4, h, value_len)
            lv = merkle_ref.levels([mc.value_of(k, value_len) + [1] for k in range(16)], h)
            assert m.cap == merkle_ref.cap(lv)
            assert all(m.proof(k)[2] == merkle_ref.path(lv, k) for k in range(16))
            assert m.hashes == 16 - (1 << h)


def test_reference_empty_map_and_walk():
    for D, h in ((1, 0), (1, 1), (3, 1), (64, 0), (64, 4)):
        m = ref.Map({}, D, h, 2)
        assert m.cap == [ref.E[D - h]] * (1 << h) and m.hashes == 0
        for key in (0, 1, min(1 << D, P) - 1):
            assert m.proof(key) == (0, [0, 0], ref.E[:D - h]) and ref.walk(key, m.proof(key), m.cap, D - h)
    m = mc.model(tuple(mc.KEYS_64), 64, 4, 3)
    for key in mc.KEYS_64 + [2, P - 2]:
        assert ref.walk(key, m.proof(key), m.cap, 60)
        bad = m.proof(key)
        assert not ref.walk(key, (1 - bad[0], bad[1], bad[2]), m.cap, 60)


# ---- the host twin against the reference
@pytest.mark.parametrize("value_len", mc.VALUE_LENS)
@pytest.mark.parametrize("key_bits", (1, 2, 3))
def test_twin_on_every_subset(pkg, key_bits, value_len):
    space = range(1 << key_bits)
    for r in range(len(space) + 1):
        for keys in itertools.combinations(space, r):
            for h in range(min(key_bits, 2) + 1):
                m = mc.model(keys, key_bits, h, value_len)
                shuffled = list(reversed(keys[1:])) + list(keys[:1])          # the twin sorts
                mm = pkg.MerkleMap(shuffled, [m.entries[k] for k in shuffled], key_bits, h, device=None, value_len=value_len)
                mc.check_map(mm, m, list(space))


@pytest.mark.parametrize("h", (0, 4))
def test_twin_on_the_64_bit_keys(pkg, h):
    m = mc.model(tuple(mc.KEYS_64), 64, h, 4)
    keys, values = mc.entries(m)
    mm = pkg.MerkleMap(keys, values, 64, h, device=None)
    queries = mc.KEYS_64 + [2, P - 2, (1 << 63) - 1, 0x1234567890ABCDE2, 0x4FEDCBA987654321]
    mc.check_map(mm, m, queries)
    assert all(ref.walk(k, p, mm.cap, 64 - h) for k, p in zip(queries, mm.get_batch(queries)))
    assert pkg.merkle_map.verify_batch(queries, 64, mm.get_batch(queries), mm.cap, device=None) == [0] * len(queries)


def test_twin_refusals_name_the_entry(pkg):
    good = lambda D, h, V: pkg.MerkleMap([1, 0], [[5] * V] * 2, D, h, device=None)   # noqa: E731
    good(64, 0, 2), good(1, 1, 0), good(16, 16, 134)
    cases = [(([3, P], [[1], [2]], 64, 0), "entry 1"), (([3, 5, 1 << 8], [[1], [2], [3]], 8, 0), "entry 2"), (([7, 3, 9, 3], [[1]] * 4, 8, 2), "entry 3"),
             (([7, 3], [[1, 2], [P, 0]], 8, 0), "entry 1"), (([7, 7, 1 << 9], [[1]] * 3, 8, 0), "entry 1"), (([1 << 9, 7, 7], [[1]] * 3, 8, 0), "entry 0"),
             (([1], [[1]], 0, 0), "key_bits"), (([1], [[1]], 65, 0), "key_bits"), (([1], [[1]], 3, 4), "cap_height"), (([1], [[1]], 20, 17), "cap_height"),
             (([1], [[1] * 135], 8, 0), "value_len")]
    for args, word in cases:
        with pytest.raises(pkg.P2Error, match=word):
            pkg.MerkleMap(*args, device=None)
    L = pkg.lib()
    out = (C.c_uint64 * 4)()
    assert L.p2_native_merkle_map_cap((C.c_uint64 * 2)(3, 3), (C.c_uint64 * 2)(1, 2), 2, 1, 8, 0, out) == P2_ERR_INVALID and b"duplicate" in L.p2_last_error()
    mm = good(8, 0, 1)
    with pytest.raises(pkg.P2Error):
        mm.get(1 << 8)


@pytest.mark.parametrize("key_bits,h,key", ((3, 1, 5), (3, 1, 4), (64, 4, 0x1234567890ABCDE0), (64, 4, 0x1234567890ABCDE2)))
def test_twin_verify_statuses(pkg, key_bits, h, key):
    keys = (1, 5, 6) if key_bits == 3 else tuple(mc.KEYS_64)
    m = mc.model(keys, key_bits, h, 4)
    for label, k, proof, cap, want in mc.tampered(m, key):
        assert pkg.merkle_map.verify(k, key_bits, proof, cap, device=None) == want, label
    L = pkg.lib()
    st, w = C.c_int(), (C.c_uint64 * 16)()
    for D, hh, V in ((0, 0, 1), (65, 0, 1), (3, 4, 1), (20, 17, 1), (8, 0, 135)):
        assert L.p2_native_merkle_map_verify(0, D, 0, w, V, w, w, hh, C.byref(st)) == P2_ERR_INVALID


# ---- the gadgets: a D = 3, h = 1 map of three entries
D, H, V = 3, 1, 4
KEYS = (1, 5, 6)


@pytest.fixture(scope="module")
def m3():
    return mc.model(KEYS, D, H, V)


@pytest.fixture(scope="module")
def circuits_(pkg):
    return {kind: mc.MapCircuit(pkg, kind, D, H, V, public=False) for kind in ("lookup", "update", "insert", "remove")}


def host(pkg, data, w):
    vals, st, f = pkg.host_witness(data.blob, w, ())
    assert f.status == st and (f.kind == "NONE") == (st == 0), f
    return st, f.kind


def test_the_host_map_agrees_and_gate_counts(pkg, m3, circuits_):
    keys, values = mc.entries(m3)
    mc.check_map(pkg.MerkleMap(keys, values, D, H, device=None), m3, list(range(8)))
    # rows: digests of one row each (5 words), one or two rows per level; ops per the header: 9 + h + 8 (2^h - 1) = 18 for lookup, ...
    mux, demux = H + 8 * ((1 << H) - 1), 2 * ((1 << H) - 1) - 1 + 8 * (1 << H)
    rows = {"lookup": 1 + (D - H), "update": 2 + 2 * (D - H), "insert": 1 + 2 * (D - H), "remove": 1 + 2 * (D - H)}
    ops = {"lookup": 9 + mux, "update": 18 + mux + demux, "insert": mux + demux, "remove": mux + demux}
    for kind, c in circuits_.items():
        assert c.gates <= rows[kind] + (ops[kind] + 19) // 20 + 1, kind          # the ops spread over at most one more gate by their constants
        assert c.gates >= rows[kind] + 1, kind


def test_lookup_at_all_eight_keys(pkg, m3, circuits_):
    c = circuits_["lookup"]
    for key in range(8):
        proof = m3.proof(key)
        assert proof[0] == (key in KEYS)
        assert host(pkg, c.data, c.witness(key, proof, m3.cap))[0] == 0, key


def test_insert_remove_and_replace(pkg, m3, circuits_):
    for key in range(8):
        proof = m3.proof(key)
        if key in KEYS:
            gone = m3.changed(key, None)
            assert host(pkg, circuits_["remove"].data, circuits_["remove"].witness(key, proof, m3.cap, new_cap=gone.cap))[0] == 0, key
            new = mc.value_of(key, V, tag=3)
            other = m3.changed(key, new)
            c = circuits_["update"]
            assert host(pkg, c.data, c.witness(key, proof, m3.cap, (1, new), other.cap))[0] == 0, key
            assert host(pkg, c.data, c.witness(key, proof, m3.cap, (0, new), gone.cap))[0] == 0, key          # update as remove
            assert host(pkg, c.data, c.witness(key, proof, m3.cap, (1, new), gone.cap)) == (1, "GENERATOR_CONFLICT"), key
            assert host(pkg, circuits_["insert"].data, circuits_["insert"].witness(key, (0, new, proof[2]), m3.cap, new_cap=other.cap)) == (1, "GENERATOR_CONFLICT")
        else:
            new = mc.value_of(key, V)
            more = m3.changed(key, new)
            assert more.proof(key)[2] == proof[2]                             # the proof before the change serves the transition
            c = circuits_["insert"]
            assert host(pkg, c.data, c.witness(key, (0, new, proof[2]), m3.cap, new_cap=more.cap))[0] == 0, key
            c = circuits_["update"]
            assert host(pkg, c.data, c.witness(key, proof, m3.cap, (1, new), more.cap))[0] == 0, key          # update as insert
            assert host(pkg, c.data, c.witness(key, proof, m3.cap, (0, new), m3.cap))[0] == 0, key            # absent stays absent
            assert host(pkg, circuits_["remove"].data, circuits_["remove"].witness(key, (1, new, proof[2]), m3.cap, new_cap=m3.cap)) == (1, "GENERATOR_CONFLICT")


def test_wrong_witnesses_are_generator_conflicts(pkg, m3, circuits_):
    c = circuits_["lookup"]
    for key in (5, 4):
        for label, k, proof, cap, want in mc.tampered(m3, key):
            if want == 2 or label.startswith("a key of"):
                continue                                                  # not field elements / not D bits: no witness to set
            assert host(pkg, c.data, c.witness(k, proof, cap)) == ((1, "GENERATOR_CONFLICT") if want else (0, "NONE")), (key, label)
    stale = m3.changed(6, None)                                           # key 5's proof from before key 6 left
    assert host(pkg, c.data, c.witness(5, m3.proof(5), stale.cap)) == (1, "GENERATOR_CONFLICT")
    assert host(pkg, c.data, c.witness(5, stale.proof(5), stale.cap))[0] == 0


def test_a_flag_of_two_is_refused(pkg, m3, circuits_):
    """a cap built so that the walk from 2 * digest checks: every constraint but assert_bool(present) holds"""
    c = circuits_["lookup"]
    key = 5
    present, value, sibs = m3.proof(key)
    for flag, want in ((1, 0), (0, 0), (2, 1), (P - 1, 1)):
        cur = [flag * w % P for w in ref.leaf_digest(value)]
        for l, s in enumerate(sibs):
            cur = [int(w) for w in ref._two_to_one(*((s, cur) if (key >> l) & 1 else (cur, s)))]
        cap = [list(h) for h in m3.cap]
        cap[key >> (D - H)] = cur
        w = c.witness(key, (1, value, sibs), cap)
        w[c.present] = flag
        st, kind = host(pkg, c.data, w)
        assert st == want and (kind == "GENERATOR_CONFLICT") == bool(want), flag


def test_length_mismatches_add_nothing(pkg):
    b = pkg.CircuitBuilder()
    bits, cap, sibs, value, new = b.add_virtual_target_arr(3), b.add_virtual_cap(1), [b.add_virtual_hash() for _ in range(2)], b.add_virtual_target_arr(4), b.add_virtual_target_arr(4)
    present, new_present = b.add_virtual_target(), b.add_virtual_target()
    gates = b.num_gates()
    L, u64 = pkg.lib(), C.c_uint64
    arr = lambda ts: (u64 * max(len(ts), 1))(*ts)               # noqa: E731
    flat = lambda hs: arr([t for h in hs for t in h])         # noqa: E731
    out = (u64 * 8)()
    big = arr(list(range(140)))
    for n_bits, h, n_sib, v_len in ((2, 1, 2, 4), (3, 1, 1, 4), (3, 0, 2, 4), (3, 17, 2, 4), (3, -1, 2, 4), (0, 0, 0, 4), (3, 1, 2, 135)):
        v = big if v_len > 4 else arr(value)
        assert L.p2_builder_merkle_map_lookup_to_cap(b._h, arr(bits), n_bits, v, v_len, present, flat(cap), h, flat(sibs), n_sib) == P2_ERR_INVALID, (n_bits, h, n_sib)
        assert L.p2_builder_merkle_map_update_to_cap(b._h, arr(bits), n_bits, present, v, new_present, v, v_len, flat(cap), h, flat(sibs), n_sib, out) == P2_ERR_INVALID
        assert L.p2_builder_merkle_map_insert_to_cap(b._h, arr(bits), n_bits, v, v_len, flat(cap), h, flat(sibs), n_sib, out) == P2_ERR_INVALID
        assert L.p2_builder_merkle_map_remove_to_cap(b._h, arr(bits), n_bits, v, v_len, flat(cap), h, flat(sibs), n_sib, out) == P2_ERR_INVALID
        assert L.p2_last_error()
    assert L.p2_builder_merkle_map_lookup(b._h, arr(bits), 3, arr(value), 4, present, arr(cap[0]), flat(sibs), 2) == P2_ERR_INVALID
    assert L.p2_builder_merkle_map_insert(b._h, arr(bits), 3, arr(value), 4, arr(cap[0]), flat(sibs), 2, out) == P2_ERR_INVALID
    for call in (lambda: b.merkle_map_update_to_cap(bits, present, value, new_present, new[:3], cap, sibs), lambda: b.merkle_map_lookup_to_cap(bits, value, present, cap + cap[:1], sibs),
                 lambda: b.merkle_map_insert_to_cap(bits, value, cap, sibs + [sibs[0][:3]]), lambda: b.merkle_map_remove(bits, value, cap[0], sibs)):
        with pytest.raises(pkg.P2Error):
            call()
    assert b.num_gates() == gates                              # a refused call adds nothing
    b.merkle_map_lookup(bits[:2], value, present, cap[0], sibs)  # the builder is still usable
    b.merkle_map_update(bits[:2], present, value, new_present, new, cap[0], sibs)
    b.build()


def test_the_oracle_proves_and_the_host_verifier_accepts(pkg, orc, m3, circuits_):
    """a lookup of a present and of an absent key with one circuit, and an insert: keys 5 = 101 and 2 = 010 see swap = 0 and 1"""
    more = m3.changed(2, mc.value_of(2, V))
    runs = [("lookup", circuits_["lookup"].witness(5, m3.proof(5), m3.cap)), ("lookup", circuits_["lookup"].witness(2, m3.proof(2), m3.cap)),
            ("insert", circuits_["insert"].witness(2, (0, mc.value_of(2, V), m3.proof(2)[2]), m3.cap, new_cap=more.cap))]
    for kind, w in runs:
        c = circuits_[kind]
        oc = orc.OracleCircuit(c.data.blob)
        st, proof = oc.prove(w)
        assert st == 0 and len(proof) == c.data.proof_bytes
        c.data.verify(proof, oc.verifier_data())
        bad = bytearray(proof)
        bad[len(bad) // 2] ^= 1
        with pytest.raises(pkg.P2Error):
            c.data.verify(bytes(bad), oc.verifier_data())
    wrong = dict(runs[0][1])
    wrong[circuits_["lookup"].present] = 0
    assert orc.OracleCircuit(circuits_["lookup"].data.blob).prove(wrong)[0] == 1
