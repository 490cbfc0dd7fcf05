"""The Poseidon cipher on the CPU: the sponge step the kernels run (p2_host_pcipher_hash_state, the host build of
p2k::pcipher_hash_state) against tests/pcipher_ref.py word for word; the single-item twins and the device=None batches against
the reference at l = 0..7 and 129; the refusal of a ciphertext that is not 3 k + 1 elements; the two gadgets and the
sealed-message circuit through the host witness generator; and the circuit sizes DESIGN.md section 9j records."""
import ctypes as C
import random

import pytest

import elgamal_cases as ecs
import elgamal_ref as eref
import pcipher_cases as cs
import pcipher_ref as ref
import sponge_ref

P = ref.P
P2_ERR_INVALID = 1                       # include/p2aes.h
LENGTHS = tuple(range(8)) + (129,)
# (rows, degree_bits) read from the builder: decrypt alone at L = 3 and 129, the sealed circuit at L = 3 with the gate and without
DECRYPT_SIZES = {3: (11, 4), 129: (253, 8)}
SEALED_SIZES = {True: (697, 10), False: (14814, 14)}


def hash_state_lib(pkg, words, last):
    out = (C.c_uint64 * 20)()
    assert pkg.lib().p2_host_pcipher_hash_state((C.c_uint64 * 20)(*words), last, out) == 0
    return list(out)


def sponge_inputs():
    r = random.Random(cs.SEED + 1)
    base = [r.randrange(P) for _ in range(20)]
    states = [base[:i] + [x] + base[i + 1:] for i in range(20) for x in sponge_ref.EXTREMES]
    states += [[x] * 20 for x in sponge_ref.EXTREMES]
    return states + [[r.randrange(P) for _ in range(20)] for _ in range(200)]


@pytest.fixture(scope="module")
def sponge_want(orc):
    ins = sponge_inputs()
    return ins, [ref.hash_n_to_m_no_pad(s, 20) for s in ins]


@pytest.mark.parametrize("last", (0, 1))
def test_sponge_step_equals_the_plain_sponge(pkg, sponge_want, last):
    ins, want = sponge_want
    for s, h in zip(ins, want):
        got = hash_state_lib(pkg, s, last)
        if last:
            assert got[5:10] == h[5:10] and got[:5] == [0] * 5 and got[10:] == [0] * 10, s
        else:
            assert got == h, s


def test_sponge_step_refuses_a_word_not_below_p(pkg):
    out = (C.c_uint64 * 20)()
    assert pkg.lib().p2_host_pcipher_hash_state((C.c_uint64 * 20)(*([0] * 19 + [P])), 0, out) != 0


@pytest.fixture(scope="module")
def cipher_want(orc):
    """per length four items and the reference's ciphertexts"""
    return {l: [(it, ref.encrypt(*it[:1], it[2], it[1])) for it in cs.items(4, l)] for l in LENGTHS}


@pytest.mark.parametrize("l", LENGTHS)
def test_twins_and_host_batches_equal_the_reference(pkg, cipher_want, l):
    pn = pkg.poseidon_native
    its = [it for it, _ in cipher_want[l]]
    want = [ct for _, ct in cipher_want[l]]
    assert all(len(ct) == ref.pad3(l) + 1 for ct in want)
    for (ks, nonce, msg), ct in zip(its, want):
        assert pn.encrypt(list(ks), msg, list(nonce)) == ct
        assert pn.decrypt(list(ks), ct, list(nonce), l) == msg == ref.decrypt(ks, ct, nonce, l)
    kss, nonces, msgs = [i[0] for i in its], [i[1] for i in its], [i[2] for i in its]
    assert pn.encrypt_batch(kss, nonces, msgs, device=None) == (want, [0] * 4)
    assert pn.decrypt_batch(kss, nonces, want, l, device=None) == (msgs, [0] * 4)


@pytest.mark.parametrize("l", (4, 5, 6, 1, 2))
def test_host_batch_statuses(pkg, orc, l):
    rows = cs.directed_decrypt(l)
    msgs, st = pkg.poseidon_native.decrypt_batch([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], l, device=None)
    assert st == [r[4] for r in rows]
    assert msgs == [r[5] if r[5] is not None else [ref.ZERO] * l for r in rows]


def test_host_batch_refuses_what_the_kernels_refuse(pkg):
    pn = pkg.poseidon_native
    ks, nonce, msg = cs.items(1, 2)[0]
    cts, st = pn.encrypt_batch([ks, ks], [nonce, nonce], [msg, cs.with_word(msg, 1, 4, P)], device=None)
    assert st == [0, 2] and cts[1] == [ref.ZERO] * 4 and cts[0] != cts[1]
    with pytest.raises(pkg.P2Error):
        pn.encrypt_batch([ks], [nonce], [[ref.ZERO] * 3073], device=None)
    with pytest.raises(pkg.P2Error):
        pn.encrypt_batch([ks, ks], [nonce], [msg, msg], device=None)


@pytest.mark.parametrize("n_ct", (3, 5, 0, 2))
def test_decrypt_refuses_a_ciphertext_that_is_not_3k_plus_1(pkg, n_ct):
    """pcipher::decrypt would write past its message there; the reference panics"""
    lib = pkg.lib()
    u64 = C.c_uint64
    msg = (u64 * 40)(*([7] * 40))
    rc = lib.p2_native_poseidon_decrypt((u64 * 10)(), (u64 * 40)(), n_ct, (u64 * 2)(), 0, msg)
    assert rc == P2_ERR_INVALID and "3 k + 1" in lib.p2_last_error().decode()
    assert list(msg) == [7] * 40
    with pytest.raises(pkg.P2Error):
        pkg.poseidon_native.decrypt([ref.ZERO, ref.ZERO], [ref.ZERO] * max(n_ct, 1), [0, 0], 0)


# ------------------------------------------------------------------ gadgets
def cipher_circuit(pkg, L, decrypt):
    b = pkg.CircuitBuilder()
    ks, nonce = b.add_virtual_target_arr(10), b.add_virtual_target_arr(2)
    rows = b.add_virtual_target_arr(5 * (L + 1 if decrypt else L))
    out = (b.poseidon_decrypt if decrypt else b.poseidon_encrypt)(ks, nonce, rows)
    gates = b.num_gates()
    return b.build(), ks, nonce, rows, out, gates


def cipher_witness(pkg, c, ks, nonce, rows):
    pw = pkg.PartialWitness()
    pw.set_target_arr(c[1], list(ks[0]) + list(ks[1]))
    pw.set_target_arr(c[2], list(nonce))
    pw.set_target_arr(c[3], cs.flat(rows))
    return pw.map


@pytest.mark.parametrize("L", (3, 6))
def test_gadgets_against_the_reference(pkg, orc, L):
    ks, nonce, msg = cs.items(1, L, seed=cs.SEED + 5)[0]
    ct = ref.encrypt(ks, msg, nonce)
    enc, dec = cipher_circuit(pkg, L, False), cipher_circuit(pkg, L, True)
    assert len(enc[4]) == 5 * (L + 1) and len(dec[4]) == 5 * L
    vals, st, f = pkg.host_witness(enc[0].blob, cipher_witness(pkg, enc, ks, nonce, msg), enc[4])
    assert st == 0 and f.kind == "NONE" and vals == cs.flat(ct)
    vals, st, f = pkg.host_witness(dec[0].blob, cipher_witness(pkg, dec, ks, nonce, ct), dec[4])
    assert st == 0 and f.kind == "NONE" and vals == cs.flat(msg)
    tag_targets = dec[3][5 * L:]
    for j in range(5):
        bad = cs.with_word(ct, L, j, (ct[L][j] + 1) % P)
        _, st, f = pkg.host_witness(dec[0].blob, cipher_witness(pkg, dec, ks, nonce, bad))
        assert st == 1 and f.kind == "GENERATOR_CONFLICT" and f.target == tag_targets[j], (j, f)


def test_build_is_the_gadget_on_fresh_targets(pkg):
    """PoseidonEncryptTarget::build allocates its targets and runs poseidon_encrypt: the same gates as the gadget on targets made
    in build's order"""
    L = 3
    b = pkg.CircuitBuilder()
    pkg.PoseidonEncryptTarget.build(b, L)
    b2 = pkg.CircuitBuilder()
    b2.zero()
    ks, m, nonce = b2.add_virtual_target_arr(10), b2.add_virtual_target_arr(5 * L), b2.add_virtual_target_arr(2)
    b2.poseidon_encrypt(ks, nonce, m)
    assert b.build().blob == b2.build().blob


def test_gadget_arguments(pkg):
    b = pkg.CircuitBuilder()
    ks, nonce = b.add_virtual_target_arr(10), b.add_virtual_target_arr(2)
    for bad in (lambda: b.poseidon_encrypt(ks, nonce, b.add_virtual_target_arr(20)), lambda: b.poseidon_decrypt(ks, nonce, b.add_virtual_target_arr(15)),
                lambda: b.poseidon_decrypt(ks[:9], nonce, b.add_virtual_target_arr(20)), lambda: b.poseidon_decrypt(ks, nonce, [])):
        with pytest.raises(pkg.P2Error):
            bad()
    assert pkg.lib().p2_builder_poseidon_encrypt(b._h, (C.c_uint64 * 10)(), (C.c_uint64 * 2)(), (C.c_uint64 * 20)(), 4, (C.c_uint64 * 25)()) != 0
    assert len(b.poseidon_encrypt(ks, nonce, [])) == 5 and len(b.poseidon_decrypt(ks, nonce, b.add_virtual_target_arr(5))) == 0


@pytest.fixture(scope="module")
def sealed(pkg):
    return {gate: cs.SealedCircuit(pkg, gate) for gate in (True, False)}


@pytest.fixture(scope="module")
def sealed_case(orc):
    """one sealed message from the references: R = r G, ks = r pk = sk R"""
    sk, r = ecs.RAND_SK, ecs.RAND_K
    pk, R = eref.g_mul_gen(sk), eref.g_mul_gen(r)
    ks = eref.g_mul(r, pk)
    assert ks == eref.g_mul(sk, R)
    _, nonce, msg = cs.items(1, 3, seed=cs.SEED + 6)[0]
    return sk, pk, R, nonce, ref.encrypt(ks, msg, nonce), msg


@pytest.mark.parametrize("gate", (True, False))
def test_sealed_circuit(pkg, sealed, sealed_case, gate):
    sk, pk, R, nonce, ct, msg = sealed_case
    c = sealed[gate]
    vals, st, f = pkg.host_witness(c.data.blob, c.witness(sk, pk, R, nonce, ct), c.out)
    assert st == 0 and f.kind == "NONE" and vals == cs.flat(msg)
    # a flipped key bit is refused at connect(public_key(sk), pk)
    _, st, f = pkg.host_witness(c.data.blob, c.witness(sk ^ 1, pk, R, nonce, ct))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT" and f.target in c.pk + c.derived_pk, f
    # with its own public key the other key passes the tie and fails at the tag
    _, st, f = pkg.host_witness(c.data.blob, c.witness(sk ^ 1, eref.g_mul_gen(sk ^ 1), R, nonce, ct))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT" and f.target in c.ct[15:], f


@pytest.mark.parametrize("L", (3, 129))
def test_decrypt_sizes(pkg, L):
    dec, enc_b = cipher_circuit(pkg, L, True), pkg.CircuitBuilder()
    pkg.PoseidonEncryptTarget.build(enc_b, L)
    enc = enc_b.build()
    print("poseidon_decrypt L = %d: %d rows, degree_bits %d; PoseidonEncryptTarget degree_bits %d" % (L, dec[5], dec[0].info["degree_bits"], enc.info["degree_bits"]))
    assert (dec[5], dec[0].info["degree_bits"]) == DECRYPT_SIZES[L]
    assert dec[0].info["degree_bits"] == enc.info["degree_bits"]


@pytest.mark.parametrize("gate", (True, False))
def test_sealed_sizes(sealed, gate):
    c = sealed[gate]
    print("sealed circuit L = 3, ec_gate %s: %d rows, degree_bits %d" % (gate, c.gates, c.data.info["degree_bits"]))
    assert (c.gates, c.data.info["degree_bits"]) == SEALED_SIZES[gate]
    assert c.data.num_public_inputs == 10 + 10 + 2 + 20
