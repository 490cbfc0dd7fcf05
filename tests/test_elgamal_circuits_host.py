"""The decryption gadgets (CPU): neg_point, elgamal_decrypt and hashed_elgamal_decrypt through the host witness generator, with
the step gate and without, against tests/elgamal_ref.py (the oracle's curve, the CPU oracle's Poseidon).  The circuit of
elgamal_cases.DecryptCircuit is the one the sizes of DESIGN.md section 9i were taken from: public_key tied to pk, multiply_point, a
negation, add_point, with pk, c0, c1 and msg public."""
import pytest

import elgamal_cases as cs
import elgamal_ref as ref

ec, P, N = ref.ec, ref.P, ref.N
# rows and degree_bits of the plain decryption circuit; the 5 % is for the count and kind of public inputs a test registers
SIZES = {True: (712, 10), False: (14820, 14)}


@pytest.fixture(scope="module")
def plain(pkg):
    return {gate: cs.DecryptCircuit(pkg, gate) for gate in (True, False)}


@pytest.fixture(scope="module")
def hashed(pkg):
    return {gate: cs.DecryptCircuit(pkg, gate, hashed=True) for gate in (True, False)}


@pytest.fixture(scope="module")
def case():
    """one ciphertext of each cipher under one key, from the reference, and the key with bit 0 flipped"""
    sk, other = cs.RAND_SK, cs.RAND_SK ^ 1
    pk = ref.g_mul_gen(sk)
    msg, m5 = ref.g_mul_gen(cs.RAND_M), cs.message5(2)
    c0, c1 = ref.elgamal_encrypt(pk, cs.RAND_K, msg)
    _, ct = ref.hashed_elgamal_encrypt(pk, cs.RAND_K, m5)
    assert ref.elgamal_decrypt(sk, c0, c1) == msg and ref.hashed_elgamal_decrypt(sk, c0, ct) == m5
    return sk, other, pk, ref.g_mul_gen(other), c0, c1, msg, ct, m5


@pytest.mark.parametrize("gate", (True, False))
def test_sizes(plain, hashed, gate):
    rows, bits = SIZES[gate]
    c = plain[gate]
    print("ec_gate %s: %d rows, degree_bits %d; hashed %d rows" % (gate, c.gates, c.data.info["degree_bits"], hashed[gate].gates))
    assert c.data.info["degree_bits"] == bits == hashed[gate].data.info["degree_bits"]
    assert abs(c.gates - rows) <= 0.05 * rows
    assert c.data.num_public_inputs == 40 and hashed[gate].data.num_public_inputs == 30


@pytest.mark.parametrize("gate", (True, False))
def test_plain_decryption(pkg, plain, case, gate):
    sk, other, pk, other_pk, c0, c1, msg, _, _ = case
    c = plain[gate]
    vals, st, f = pkg.host_witness(c.data.blob, c.witness(sk, pk, c0, c1), c.out)
    assert st == 0 and f.kind == "NONE" and vals == cs.flat_point(msg)
    # the message as an input too: the same witness, and a wrong message conflicts with what the gadget computes
    assert pkg.host_witness(c.data.blob, c.witness(sk, pk, c0, c1, msg), c.out)[:2] == (cs.flat_point(msg), 0)
    _, st, f = pkg.host_witness(c.data.blob, c.witness(sk, pk, c0, c1, ec.generator()))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT"
    # a flipped key bit, with its own public key: another message, the reference's for that key
    vals, st, _ = pkg.host_witness(c.data.blob, c.witness(other, other_pk, c0, c1), c.out)
    assert st == 0 and vals == cs.flat_point(ref.elgamal_decrypt(other, c0, c1)) != cs.flat_point(msg)
    # connect(public_key(sk), pk) refuses a key that is not pk's, and the fault names a target of the tie
    _, st, f = pkg.host_witness(c.data.blob, c.witness(other, pk, c0, c1))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT" and f.target in c.pk + c.derived_pk, f
    assert "%#x" % f.target in str(f)


@pytest.mark.parametrize("gate", (True, False))
def test_hashed_decryption(pkg, hashed, case, gate):
    sk, other, pk, other_pk, c0, _, _, ct, m5 = case
    c = hashed[gate]
    vals, st, f = pkg.host_witness(c.data.blob, c.witness(sk, pk, c0, ct), c.out)
    assert st == 0 and f.kind == "NONE" and tuple(vals) == m5
    vals, st, _ = pkg.host_witness(c.data.blob, c.witness(other, other_pk, c0, ct), c.out)
    assert st == 0 and tuple(vals) == ref.hashed_elgamal_decrypt(other, c0, ct) != m5
    _, st, f = pkg.host_witness(c.data.blob, c.witness(other, pk, c0, ct))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT" and f.target in c.pk + c.derived_pk, f


def test_neg_point(pkg):
    b = pkg.CircuitBuilder()
    p = b.add_virtual_target_arr(10)
    q = b.neg_point(p)
    assert q[:5] == p[:5] and not set(q[5:]) & set(p)
    data = b.build()
    for pt in (ec.generator(), ec.NEUTRAL, ref.g_mul_gen(cs.RAND_M)):
        pw = pkg.PartialWitness()
        pw.set_target_arr(p, cs.flat_point(pt))
        vals, st, _ = pkg.host_witness(data.blob, pw, q)
        assert st == 0 and vals == cs.flat_point(ec.g_neg(pt))
    with pytest.raises(pkg.P2Error):
        b2 = pkg.CircuitBuilder()
        b2.neg_point(b2.add_virtual_target_arr(9))


def test_gadget_arguments(pkg):
    b = pkg.CircuitBuilder()
    sk, c0 = b.add_secret_key(), b.add_virtual_target_arr(10)
    with pytest.raises(pkg.P2Error):
        b.elgamal_decrypt(sk[:319], c0, c0)
    with pytest.raises(pkg.P2Error):
        b.elgamal_decrypt(sk, c0, c0[:5])
    with pytest.raises(pkg.P2Error):
        b.hashed_elgamal_decrypt(sk, c0, c0)
