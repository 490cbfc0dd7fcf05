"""The host twins of the ElGamal batch kernels (CPU): p2_ecgfp5_encode_binary_padded and the device=None loops of api.ecgfp5
against tests/elgamal_ref.py, which calls nothing of the library -- the oracle's textbook curve and the CPU oracle's Poseidon.
Everything compared is exact.  The reference costs 0.14 s per multiplication, so it sees a dozen items; the GPU tests then hold
the kernels to these twins on the larger counts."""
import random

import pytest

import elgamal_cases as cs
import elgamal_ref as ref

ec, P, N = ref.ec, ref.P, ref.N


@pytest.fixture(scope="module")
def E(pkg):
    return pkg.ecgfp5


def test_the_square_test_agrees_with_decompress():
    """elgamal_ref.decodes (one square test) and the oracle's decompress say the same of random words, of u = 0 and of G's u"""
    r = random.Random(cs.SEED + 2)
    ws = [tuple(r.randrange(P) for _ in range(5)) for _ in range(12)] + [ec.ZERO, ec.generator()[1]]
    got = [ref.decompress(w) is not None for w in ws]
    assert got == [ref.decodes(w) for w in ws] and True in got[:12] and False in got[:12]
    assert ref.decompress(ec.ZERO) == ec.NEUTRAL and ref.decompress(ec.generator()[1]) == ec.generator()


def test_decompress_twin_against_the_reference(E):
    r = random.Random(cs.SEED + 3)
    ws = [tuple(r.randrange(P) for _ in range(5)) for _ in range(10)] + [ec.ZERO, ec.generator()[1], (P, 0, 0, 0, 0), ec.generator()[1][:4] + (cs.M64,)]
    pts, st = E.decompress_batch(ws, device=None)
    want = [None if any(v >= P for v in w) else ref.decompress(w) for w in ws]
    assert st == [2 if any(v >= P for v in w) else 1 if g is None else 0 for w, g in zip(ws, want)]
    assert sorted(set(st)) == [0, 1, 2]
    assert pts == [g or ec.NEUTRAL for g in want]


def test_encode_binary_padded_against_the_reference(E):
    """same point and same attempt number: limbs zero, all ones and random with the first decodable attempt number 1, a middle
    one, 16 and none; a pad word of 2^32 - 1 is skipped over a non-zero limb and tried over a zero limb"""
    cases = cs.encode_directed()
    want = [ref.encode_padded(limbs, pads) for _, limbs, pads, _ in cases]
    assert [w[1] for w in want] == [c[3] for c in cases]                     # the reference takes the attempt built in
    pts, used, st = E.encode_binary_batch([ref.int_of(c[1]) for c in cases], [c[2] for c in cases], device=None)
    assert used == [w[1] for w in want]
    assert st == [1 if w[0] is None else 0 for w in want] and st.count(1) == 3
    assert pts == [w[0] or ec.NEUTRAL for w in want]
    assert all(ec.in_group(p) for p in pts)


def test_a_pad_list_that_never_decodes_is_an_error(E, pkg):
    import ctypes as C
    label, limbs, pads, first = cs.encode_directed()[3]
    assert first == cs.ATTEMPTS and ref.encode_padded(limbs, pads) == (None, cs.ATTEMPTS)
    out, used = (C.c_uint64 * 10)(*([7] * 10)), C.c_uint32(99)
    flat = (C.c_uint32 * (5 * cs.ATTEMPTS))(*[v for row in pads for v in row])
    rc = pkg.lib().p2_ecgfp5_encode_binary_padded((C.c_uint32 * 5)(*limbs), flat, cs.ATTEMPTS, out, C.byref(used))
    assert rc != 0 and used.value == cs.ATTEMPTS and list(out) == [7] * 10
    assert "no attempt" in pkg.lib().p2_last_error().decode()
    # a list of one row that decodes is no error
    ok = cs.encode_directed()[0]
    flat = (C.c_uint32 * 5)(*ok[2][0])
    assert pkg.lib().p2_ecgfp5_encode_binary_padded((C.c_uint32 * 5)(*ok[1]), flat, 1, out, C.byref(used)) == 0 and used.value == 0
    assert (tuple(out[0:5]), tuple(out[5:10])) == ref.encode_padded(ok[1], ok[2])[0]


def test_undirected_items_decode_within_the_cap_and_decode_inverts_encode(E):
    """The reference finds a point within 16 attempts for every item of the fixed seed -- asserted before the library is touched
    -- and takes the attempt the library takes; decode_binary of the point is the message."""
    items = cs.undirected(12)
    firsts = [ref.first_attempt(limbs, pads) for limbs, pads in items]
    assert max(firsts) < cs.ATTEMPTS
    want = [ref.encode_padded(limbs, pads) for limbs, pads in items]
    assert [w[1] for w in want] == firsts
    xs = [ref.int_of(limbs) for limbs, _ in items]
    pts, used, st = E.encode_binary_batch(xs, [pads for _, pads in items], device=None)
    assert (pts, used, st) == ([w[0] for w in want], firsts, [0] * 12)
    assert E.decode_binary_batch(pts) == xs == [E.decode_binary(p) for p in pts]
    assert [ref.decode(p) for p in pts] == [limbs for limbs, _ in items]


def test_encode_arguments(E, pkg):
    limbs, pads = cs.undirected(1)[0]
    for bad in ([], pads * 17):
        with pytest.raises(pkg.P2Error):
            E.encode_binary_batch([1], [bad], device=None)
    with pytest.raises(pkg.P2Error):
        E.encode_binary_batch([1 << 160], [pads], device=None)
    with pytest.raises(pkg.P2Error):
        E.encode_binary_batch([1], [[[1 << 32] * 5]], device=None)
    with pytest.raises(pkg.P2Error):
        E.encode_binary_batch([1, 2], [pads], device=None)
    assert E.encode_binary_batch([], [], device=None) == ([], [], [])


def test_plain_cipher_twins_against_the_reference(E):
    pk = ref.g_mul_gen(cs.RAND_SK)
    msgs = cs.good_points()
    nonces = [cs.RAND_K, 0, 1]
    c0s, c1s, st = E.elgamal_encrypt_batch([pk] * 3, nonces, msgs, device=None)
    assert st == [0] * 3
    want = [ref.elgamal_encrypt(pk, k, m) for k, m in zip(nonces, msgs)]
    assert list(zip(c0s, c1s)) == want
    assert (c0s[1], c1s[1]) == (ec.NEUTRAL, msgs[1])                          # nonce 0
    back, st = E.elgamal_decrypt_batch([cs.RAND_SK] * 3, c0s, c1s, device=None)
    assert st == [0] * 3 and back == msgs == [ref.elgamal_decrypt(cs.RAND_SK, a, b) for a, b in want]


def test_hashed_cipher_twins_against_the_reference(E):
    pk = ref.g_mul_gen(cs.RAND_SK)
    msgs = [cs.message5(0), (0,) * 5, (P - 1,) * 5]
    nonces = [cs.RAND_K, 0, 1]
    c0s, cts, st = E.hashed_elgamal_encrypt_batch([pk] * 3, nonces, msgs, device=None)
    assert st == [0] * 3
    want = [ref.hashed_elgamal_encrypt(pk, k, m) for k, m in zip(nonces, msgs)]
    assert list(zip(c0s, cts)) == want
    back, st = E.hashed_elgamal_decrypt_batch([cs.RAND_SK] * 3, c0s, cts, device=None)
    assert st == [0] * 3 and back == msgs == [ref.hashed_elgamal_decrypt(cs.RAND_SK, a, c) for a, c in want]


def test_malformed_rows_of_the_twins(E):
    """a scalar not below n, a word not below p, a point outside the group or off the curve: status 2 and zeroed rows; the
    neutral is inside"""
    g, pk = ec.generator(), ref.g_mul_gen(2)
    bad = [p for _, p in cs.bad_points()]
    n = len(bad)
    c0s, c1s, st = E.elgamal_encrypt_batch(bad + [pk] * n + [pk, ec.NEUTRAL], [1] * (2 * n) + [N, 1], [g] * n + bad + [g, ec.NEUTRAL], device=None)
    assert st == [2] * (2 * n + 1) + [0]
    assert c0s[:-1] == c1s[:-1] == [ec.NEUTRAL] * (2 * n + 1) and (c0s[-1], c1s[-1]) == (g, ec.NEUTRAL)
    msgs, st = E.elgamal_decrypt_batch([1] * (2 * n) + [N, cs.M320, N - 1], bad + [g] * n + [g] * 3, [g] * n + bad + [g] * 3, device=None)
    assert st == [2] * (2 * n + 2) + [0] and msgs == [ec.NEUTRAL] * (2 * n + 2) + [ref.g_mul_gen(2)]
    m5 = cs.message5(1)
    c0s, cts, st = E.hashed_elgamal_encrypt_batch(bad + [pk] * 3, [1] * n + [N, 1, 1], [m5] * (n + 1) + [m5[:4] + (P,), (cs.M64,) + m5[1:]], device=None)
    assert st == [2] * (n + 3) and c0s == [ec.NEUTRAL] * (n + 3) and cts == [(0,) * 5] * (n + 3)
    msgs, st = E.hashed_elgamal_decrypt_batch([1] * n + [N, 1], bad + [g, g], [m5] * (n + 1) + [m5[:2] + (P,) + m5[3:]], device=None)
    assert st == [2] * (n + 2) and msgs == [(0,) * 5] * (n + 2)
