"""Schnorr signatures on ecGFp5, on the host: (a b + c) mod n against Python integers, p2_schnorr_sign word for word against
tests/schnorr_ref.py (the oracle's curve and hash), p2_schnorr_verify on the reference's signatures and on every tampering class
of schnorr_cases.tampered.  No device."""
import ctypes as C

import pytest

import schnorr_cases as sc
import schnorr_ref as ref

ec, P, N = ref.ec, ref.P, ref.N


def test_the_two_spellings_of_the_group_order_agree(pkg):
    """ecgfp5_scalar.h spells n limb by limb: n - 1 + 1 = 0 and 1 * n + 0 = 0 under it, and the value is ecgfp5.h's"""
    E = pkg.ecgfp5
    assert E.group_order() == N
    assert E.scalar_muladd(1, N - 1, 1) == 0 and E.scalar_muladd(1, N, 0) == 0 and E.scalar_muladd(1, N + 1, 0) == 1


def test_scalar_muladd_against_python_integers(pkg):
    for a, b, c in sc.muladd_triples():
        assert pkg.ecgfp5.scalar_muladd(a, b, c) == (a * b + c) % N, (hex(a), hex(b), hex(c))
    for a in sc.DIRECTED:
        for b in sc.DIRECTED:
            assert pkg.ecgfp5.scalar_muladd(a, b, sc.DIRECTED[(a + b) % len(sc.DIRECTED)]) == (a * b + sc.DIRECTED[(a + b) % len(sc.DIRECTED)]) % N


def test_challenge_is_the_oracles_sponge(pkg):
    r, pk = ref.g_mul_gen(sc.RAND_K), ref.g_mul_gen(sc.RAND_SK)
    for n in sc.MSG_LENS + (29, 1024):
        m = sc.message(n)
        assert pkg.schnorr.challenge(r, pk, m) == ref.challenge(r, pk, m), n
    with pytest.raises(pkg.P2Error):
        pkg.schnorr.challenge(r, pk, [0] * 1025)


@pytest.mark.parametrize("msg_len", sc.MSG_LENS)
def test_sign_equals_the_reference_word_for_word(pkg, msg_len):
    m = sc.message(msg_len)
    for sk in (1, 2, N - 1, sc.RAND_SK):
        for k in (1, 2, N - 1, sc.RAND_K):
            assert pkg.schnorr.sign(sk, m, k) == ref.sign(sk, m, k), (sk, k)


def test_sign_batch_host_twin_gives_keys_and_statuses(pkg):
    sks, ks = [1, sc.RAND_SK, 0, N, sc.RAND_SK, 2], [sc.RAND_K, 2, 1, 1, 0, N]
    msgs = [sc.message(5, i) for i in range(6)]
    sigs, pks, st = pkg.schnorr.sign_batch(sks, msgs, ks, device=None)
    assert st == [0, 0, 2, 2, 2, 2]
    for i in range(6):
        if st[i] == 0:
            assert sigs[i] == ref.sign(sks[i], msgs[i], ks[i]) and pks[i] == ref.g_mul_gen(sks[i])
        else:
            assert sigs[i] == (0, (0, 0, 0, 0)) and pks[i] == ec.NEUTRAL
    assert pkg.schnorr.sign_batch([1], [[P]], [1], device=None)[2] == [2]


def test_sign_refuses_bad_nonces_and_keys(pkg):
    m = sc.message(3)
    for sk, k in ((sc.RAND_SK, 0), (sc.RAND_SK, N), (sc.RAND_SK, N + 1), (sc.RAND_SK, sc.M320), (0, sc.RAND_K), (N, sc.RAND_K)):
        with pytest.raises(pkg.P2Error):
            pkg.schnorr.sign(sk, m, k)
    with pytest.raises(pkg.P2Error):
        pkg.schnorr.sign(sc.RAND_SK, [P], sc.RAND_K)
    with pytest.raises(pkg.P2Error):
        pkg.schnorr.sign(sc.RAND_SK, [0] * 1025, sc.RAND_K)
    # a drawn nonce: signatures differ, both verify
    a, b = pkg.schnorr.sign(sc.RAND_SK, m), pkg.schnorr.sign(sc.RAND_SK, m)
    pk = ref.g_mul_gen(sc.RAND_SK)
    assert a != b and pkg.schnorr.verify(pk, m, a) == pkg.schnorr.verify(pk, m, b) == 0


@pytest.mark.parametrize("msg_len", sc.MSG_LENS)
def test_verify_accepts_the_references_signatures(pkg, msg_len):
    m = sc.message(msg_len)
    for sk, k in ((1, 1), (2, N - 1), (N - 1, 2), (sc.RAND_SK, sc.RAND_K), (sc.RAND_SK, 0), (N - 1, 0)):
        assert pkg.schnorr.verify(ref.g_mul_gen(sk), m, ref.sign(sk, m, k)) == 0, (sk, k)


def test_the_k0_signature_is_what_the_issue_says(pkg):
    m = sc.message(5)
    pk = ref.g_mul_gen(sc.RAND_SK)
    s, e = sc.k0_signature(sc.RAND_SK, m)
    assert e == ref.challenge(ec.NEUTRAL, pk, m) and s == ref.e_int(e) * sc.RAND_SK % N
    assert pkg.schnorr.verify(pk, m, (s, e)) == 0 == ref.verify(pk, m, (s, e))


@pytest.mark.parametrize("msg_len", (0, 5, 12))
def test_tampered_signatures_get_their_statuses(pkg, msg_len):
    m = sc.message(msg_len)
    pk, other = ref.g_mul_gen(sc.RAND_SK), ref.g_mul_gen(2)
    cases = sc.tampered(pk, m, ref.sign(sc.RAND_SK, m, sc.RAND_K), other)
    labels = {c[0] for c in cases}
    assert {"s bit", "e word 0 bit", "e word 3 bit", "other key", "s = n", "s + n", "pk off the curve", "pk outside the group", "pk neutral",
            "e word 0 not canonical", "pk.x word not canonical"} <= labels and (not m or "msg word bit" in labels)
    got = pkg.schnorr.verify_batch([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], device=None)
    assert got == [c[4] for c in cases], [c[0] for c, g in zip(cases, got) if g != c[4]]


def test_the_reference_verifier_agrees_on_a_sample(pkg):
    """the constructed statuses against schnorr_ref.verify itself (two oracle multiplications each)"""
    m = sc.message(5)
    pk = ref.g_mul_gen(sc.RAND_SK)
    cases = sc.tampered(pk, m, ref.sign(sc.RAND_SK, m, sc.RAND_K), ref.g_mul_gen(2))
    for c in [c for c in cases if c[0] in ("honest", "s bit", "e word 2 bit", "msg word bit", "s + n", "pk outside the group")]:
        assert ref.verify(c[1], c[2], c[3]) == c[4], c[0]


def test_mul_batch_host_twin(pkg):
    g = ref.ec.generator()
    outs, st = pkg.ecgfp5.mul_batch([sc.RAND_K, 0, 5], [g, g, sc.point_outside_the_group()], device=None)
    assert st == [0, 0, 2] and outs[:2] == [ref.g_mul_gen(sc.RAND_K), ec.NEUTRAL]


def test_message_length_limit_of_the_c_calls(pkg):
    L = pkg.lib()
    st = C.c_int(-1)
    big = (C.c_uint64 * 1025)()
    pk = (C.c_uint64 * 10)(*ec.as_fields(ref.g_mul_gen(2)))
    sig = (C.c_uint64 * 9)()
    assert L.p2_schnorr_verify(pk, big, 1025, sig, C.byref(st)) != 0 and st.value == -1
    assert L.p2_schnorr_verify(pk, big, 1024, sig, C.byref(st)) == 0 and st.value == 1
