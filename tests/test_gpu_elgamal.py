"""ElGamal on ecGFp5 in GPU batches, and decryption inside a circuit, on the GPU.

Kernels: k_ec_decompress_batch, k_ec_encode_binary, k_elgamal_encrypt / _decrypt, k_hashed_elgamal_encrypt / _decrypt and
k_ec_scalar_bits.  Each is held to tests/elgamal_ref.py (the oracle's curve in textbook affine arithmetic, the CPU oracle's
Poseidon; nothing of the library) on a directed dozen, and to the host twins at counts 1, 63, 64, 65 (one block, its last lane,
the first lane of a second) and 257 (five blocks, the last of one item).  Expected statuses come by construction.
Circuits: one pipeline with no host round trip -- encode, encrypt and bits on the device, assembled on the device into the value
matrix of the step-gate ElGamal circuit, proven, decrypted on the device; four proofs of the decryption circuit through both
verifiers, compression and the replay of tests/proof_ref.py, a wrong key, and one proof without the gate.
Everything compared is exact."""
import ctypes as C
import random

import pytest

import ec_circuits
import elgamal_cases as cs
import elgamal_ref as ref
import proof_ref as R
from test_gpu_merkle import Device
from test_gpu_schnorr import Stream

pytestmark = pytest.mark.gpu

ec, P, N = ref.ec, ref.P, ref.N
COUNTS = (1, 63, 64, 65, 257)
D2D = 3
flat_point, words5 = cs.flat_point, cs.words5
ZERO5 = (0,) * 5


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture(scope="module")
def E(gpu):
    return gpu.ecgfp5


@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


def put32(dev, words):
    arr = (C.c_uint32 * max(len(words), 1))(*words)
    b = dev.alloc(C.sizeof(arr))
    assert dev.H.hipMemcpy(b, arr, C.sizeof(arr), 1) == 0
    return b


def at(buf, words):
    return C.c_void_p(buf.value + 8 * words)


# ------------------------------------------------------------------ decompress
def test_decompress_directed_against_the_reference(E):
    r = random.Random(cs.SEED + 10)
    g = ec.generator()
    ws = [ec.ZERO, g[1], ec.f_neg(g[1]), (P, 0, 0, 0, 0), g[1][:4] + (cs.M64,)] + [tuple(r.randrange(P) for _ in range(5)) for _ in range(7)]
    want = [None if any(v >= P for v in w) else ref.decompress(w) for w in ws]
    want_st = [2 if any(v >= P for v in w) else 1 if p is None else 0 for w, p in zip(ws, want)]
    assert want[:3] == [ec.NEUTRAL, g, ec.g_neg(g)] and sorted(set(want_st)) == [0, 1, 2]
    pts, st = E.decompress_batch(ws)
    assert st == want_st and pts == [p or ec.NEUTRAL for p in want]


def test_decompress_counts_against_the_host_twin(E):
    r = random.Random(cs.SEED + 11)
    ws = [tuple(r.randrange(P) for _ in range(5)) for _ in range(257)]
    ws[0], ws[62], ws[63] = ec.ZERO, (0, 0, P, 0, 0), ec.generator()[1]
    ws[64], ws[256] = (cs.M64,) * 5, ws[5][:4] + (P + 1,)
    want = E.decompress_batch(ws, device=None)
    assert want[1][0] == 0 and [want[1][i] for i in (62, 64, 256)] == [2, 2, 2] and want[1].count(1) > 64 and want[1].count(0) > 64
    for count in COUNTS:
        assert E.decompress_batch(ws[:count]) == (want[0][:count], want[1][:count]), count


# ------------------------------------------------------------------ encode_binary
def encode_items():
    """257 items: the directed ones (first decodable attempt 1, a middle one, 16, none; skipped and tried pad words) spread over
    the block edges, undirected ones from the fixed seed elsewhere"""
    directed = cs.encode_directed()
    items = cs.undirected(257)
    where = [0, 1, 62, 63, 64, 65, 66, 127, 128, 129, 200, 254, 255, 256]
    assert len(where) == len(directed)
    for i, d in zip(where, directed):
        items[i] = (d[1], d[2])
    return items, dict(zip(where, directed))


def test_encode_binary_against_the_reference_and_the_host_twin(E):
    items, directed = encode_items()
    # the reference, before the library is touched: every undirected item decodes within the cap, the directed ones where built
    firsts = [ref.first_attempt(limbs, pads) for limbs, pads in items]
    assert all((firsts[i] == directed[i][3]) if i in directed else firsts[i] < cs.ATTEMPTS for i in range(257))
    assert {firsts[i] for i in directed} == {0, 1, 2, 7, 15, 16}
    xs, pads = [ref.int_of(limbs) for limbs, _ in items], [p for _, p in items]
    want = E.encode_binary_batch(xs, pads, device=None)
    assert want[1] == firsts and want[2] == [1 if f == cs.ATTEMPTS else 0 for f in firsts]
    for count in COUNTS:
        pts, used, st = E.encode_binary_batch(xs[:count], pads[:count])
        assert (pts, used, st) == (want[0][:count], firsts[:count], want[2][:count]), count
    # the points are the reference's on the directed items and a few others
    for i in sorted(directed)[:10] + [2, 3]:
        assert want[0][i] == (ref.encode_padded(*items[i])[0] or ec.NEUTRAL), i
    good = [i for i in range(257) if want[2][i] == 0]
    assert E.decode_binary_batch([want[0][i] for i in good]) == [xs[i] for i in good]


def test_encode_limits(gpu, E):
    limbs, pads = cs.undirected(1)[0]
    for bad in ([], pads * 17):
        with pytest.raises(gpu.P2Error):
            E.encode_binary_batch([1], [bad])
    assert E.encode_binary_batch([], []) == ([], [], []) and E.decompress_batch([]) == ([], [])
    # one attempt: the kernel's loop of one
    first = ref.first_attempt(limbs, pads)
    pts, used, st = E.encode_binary_batch([ref.int_of(limbs)] * 2, [[pads[first]], [pads[first]][:1]])
    assert (used, st) == ([0, 0], [0, 0]) and pts[0] == pts[1] == ref.encode_padded(limbs, pads)[0]


# ------------------------------------------------------------------ the plain cipher
def plain_dozen():
    """[(pk, nonce, msg, status)]: scalars 0, 1, 2, n - 1 and n; G, a random point and the neutral as key and message; words not
    below p, a point outside the group, one off the curve"""
    g, pk, rnd = ec.generator(), ref.g_mul_gen(cs.RAND_SK), ref.g_mul_gen(cs.RAND_M)
    bad = dict(cs.bad_points())
    return [(pk, 0, g, 0), (pk, 1, rnd, 0), (pk, 2, ec.NEUTRAL, 0), (pk, N - 1, g, 0), (pk, N, g, 2), (pk, cs.RAND_K, rnd, 0), (ec.NEUTRAL, cs.RAND_K, g, 0),
            (g, 2, ref.g_mul_gen(2), 0), (bad["word = p"], 1, g, 2), (pk, 1, bad["outside the group"], 2), (bad["off the curve"], 1, g, 2), (pk, cs.M320, g, 2),
            (pk, 1, bad["word = 2^64 - 1"], 2)]


def test_plain_cipher_directed_against_the_reference(E):
    items = plain_dozen()
    want = [ref.elgamal_encrypt(pk, k, m) if st == 0 else (ec.NEUTRAL, ec.NEUTRAL) for pk, k, m, st in items]
    c0s, c1s, st = E.elgamal_encrypt_batch([i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
    assert st == [i[3] for i in items] and list(zip(c0s, c1s)) == want
    assert (c0s[0], c1s[0]) == (ec.NEUTRAL, items[0][2])                       # nonce 0: c0 neutral, c1 the message
    # decryption: the first eight under the key they were made for; then sk 0, 1, 2, n - 1 and n, and points outside the group
    g, rnd = ec.generator(), ref.g_mul_gen(cs.RAND_M)
    bad = dict(cs.bad_points())
    dec = [(cs.RAND_SK, c0s[i], c1s[i], 0) for i in (0, 1, 2, 3, 5)] + [(1, c0s[7], c1s[7], 0)]     # item 7 was made for G, the key of 1
    dec += [(0, g, rnd, 0), (1, g, rnd, 0), (2, rnd, g, 0), (N - 1, g, ec.NEUTRAL, 0), (N, g, rnd, 2), (1, bad["outside the group"], g, 2),
            (1, g, bad["off the curve"], 2), (1, bad["word = p"], g, 2)]
    msgs, st = E.elgamal_decrypt_batch([d[0] for d in dec], [d[1] for d in dec], [d[2] for d in dec])
    assert st == [d[3] for d in dec]
    assert msgs == [ref.elgamal_decrypt(sk, a, b) if s == 0 else ec.NEUTRAL for sk, a, b, s in dec]
    assert msgs[:6] == [items[i][2] for i in (0, 1, 2, 3, 5, 7)]               # round trips


def cipher_inputs(E):
    """257 items for the count tests: three keys, random nonces, messages over G, a random point, the neutral and 2 G; malformed
    rows at the block edges"""
    r = random.Random(cs.SEED + 12)
    sk_pool = [cs.RAND_SK, 2, 1]
    pk_pool = [ref.g_mul_gen(sk) for sk in sk_pool]
    msg_pool = cs.good_points() + [ref.g_mul_gen(2)]
    sks, pks = [sk_pool[i % 3] for i in range(257)], [pk_pool[i % 3] for i in range(257)]
    nonces, msgs = [r.randrange(N) for _ in range(257)], [msg_pool[i % 4] for i in range(257)]
    nonces[1], nonces[2] = 0, N - 1
    bad = dict(cs.bad_points())
    wrong = {0: ("nonce", N), 5: ("pk", bad["outside the group"]), 63: ("msg", bad["word = p"]), 64: ("pk", bad["off the curve"]), 65: ("nonce", cs.M320),
             130: ("msg", bad["x = 0, u != 0"]), 255: ("pk", bad["x != 0, u = 0"]), 256: ("msg", bad["word = 2^64 - 1"])}
    for i, (what, v) in wrong.items():
        {"nonce": nonces, "pk": pks, "msg": msgs}[what][i] = v
    return sks, pks, nonces, msgs, wrong


def test_plain_cipher_counts_against_the_host_twin(E):
    sks, pks, nonces, msgs, wrong = cipher_inputs(E)
    want = E.elgamal_encrypt_batch(pks, nonces, msgs, device=None)
    assert want[2] == [2 if i in wrong else 0 for i in range(257)]
    for count in COUNTS:
        assert E.elgamal_encrypt_batch(pks[:count], nonces[:count], msgs[:count]) == tuple(w[:count] for w in want), count
    # decryption of what came out: a zeroed row is (neutral, neutral), which decrypts to the neutral; a key not below n is malformed
    sks[7], sks[64] = N, cs.M320
    back = E.elgamal_decrypt_batch(sks, want[0], want[1], device=None)
    assert back[1] == [2 if i in (7, 64) else 0 for i in range(257)]
    assert all(back[0][i] == (ec.NEUTRAL if i in wrong or i in (7, 64) else msgs[i]) for i in range(257))
    for count in COUNTS:
        assert E.elgamal_decrypt_batch(sks[:count], want[0][:count], want[1][:count]) == (back[0][:count], back[1][:count]), count


# ------------------------------------------------------------------ the hashed cipher
def test_hashed_cipher_directed_against_the_reference(E):
    g, pk = ec.generator(), ref.g_mul_gen(cs.RAND_SK)
    bad = dict(cs.bad_points())
    m = [cs.message5(i) for i in range(4)]
    items = [(pk, 0, m[0], 0), (pk, 1, ZERO5, 0), (pk, 2, (P - 1,) * 5, 0), (pk, N - 1, m[1], 0), (pk, N, m[1], 2), (pk, cs.RAND_K, m[2], 0),
             (ec.NEUTRAL, cs.RAND_K, m[3], 0), (g, 2, m[3], 0), (bad["word = p"], 1, m[0], 2), (bad["outside the group"], 1, m[0], 2),
             (bad["off the curve"], 1, m[0], 2), (pk, 1, m[0][:4] + (P,), 2), (pk, 1, (cs.M64,) + m[0][1:], 2)]
    want = [ref.hashed_elgamal_encrypt(p, k, w) if st == 0 else (ec.NEUTRAL, ZERO5) for p, k, w, st in items]
    c0s, cts, st = E.hashed_elgamal_encrypt_batch([i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
    assert st == [i[3] for i in items] and list(zip(c0s, cts)) == want
    dec = [(cs.RAND_SK, c0s[i], cts[i], 0) for i in (0, 1, 2, 3, 5)] + [(1, c0s[7], cts[7], 0)]
    dec += [(0, g, m[0], 0), (1, g, m[1], 0), (N - 1, g, m[2], 0), (N, g, m[0], 2), (1, bad["outside the group"], m[0], 2), (1, g, m[0][:2] + (P,) + m[0][3:], 2),
            (1, bad["word = 2^64 - 1"], m[0], 2)]
    msgs, st = E.hashed_elgamal_decrypt_batch([d[0] for d in dec], [d[1] for d in dec], [d[2] for d in dec])
    assert st == [d[3] for d in dec]
    assert msgs == [ref.hashed_elgamal_decrypt(sk, a, c) if s == 0 else ZERO5 for sk, a, c, s in dec]
    assert msgs[:6] == [items[i][2] for i in (0, 1, 2, 3, 5, 7)]


def test_hashed_cipher_counts_against_the_host_twin(E):
    sks, pks, nonces, _, wrong = cipher_inputs(E)
    wrong = {i: w for i, w in wrong.items() if w[0] != "msg"}
    msgs = [cs.message5(i) for i in range(257)]
    msgs[63], msgs[256] = msgs[63][:4] + (P,), (cs.M64,) + msgs[256][1:]
    wrong.update({63: None, 256: None})
    want = E.hashed_elgamal_encrypt_batch(pks, nonces, msgs, device=None)
    assert want[2] == [2 if i in wrong else 0 for i in range(257)]
    for count in COUNTS:
        assert E.hashed_elgamal_encrypt_batch(pks[:count], nonces[:count], msgs[:count]) == tuple(w[:count] for w in want), count
    sks[7] = N
    cts = list(want[1])
    cts[66] = cts[66][:4] + (P,)
    back = E.hashed_elgamal_decrypt_batch(sks, want[0], cts, device=None)
    assert back[1] == [2 if i in (7, 66) else 0 for i in range(257)]
    assert all(back[0][i] == msgs[i] for i in range(257) if i not in wrong and i not in (7, 66))
    for count in COUNTS:
        assert E.hashed_elgamal_decrypt_batch(sks[:count], want[0][:count], cts[:count]) == (back[0][:count], back[1][:count]), count


# ------------------------------------------------------------------ device-pointer forms, on a stream of their own
def test_device_pointer_forms_agree_with_the_host_pointer_forms(gpu, E, dev):
    n = 65
    items = cs.undirected(n, seed=cs.SEED + 13)
    xs, pads = [ref.int_of(limbs) for limbs, _ in items], [p for _, p in items]
    r = random.Random(cs.SEED + 14)
    sks = [r.randrange(1, N) for _ in range(n)]
    nonces = [r.randrange(N) for _ in range(n)]
    nonces[7] = N
    pks, pst = E.mul_batch(sks, [ec.generator()] * n)
    m5 = [cs.message5(200 + i) for i in range(n)]
    pts, used, est = E.encode_binary_batch(xs, pads)
    assert est == [0] * n and pst == [0] * n
    c0s, c1s, cst = E.elgamal_encrypt_batch(pks, nonces, pts)
    back, dst = E.elgamal_decrypt_batch(sks, c0s, c1s)
    h0s, cts, hst = E.hashed_elgamal_encrypt_batch(pks, nonces, m5)
    hback, hdst = E.hashed_elgamal_decrypt_batch(sks, h0s, cts)
    assert cst == hst == [2 if i == 7 else 0 for i in range(n)] and dst == hdst == [0] * n
    assert back == [ec.NEUTRAL if i == 7 else pts[i] for i in range(n)] and [hback[i] for i in range(n) if i != 7] == [m5[i] for i in range(n) if i != 7]
    wpts, wst = E.decompress_batch([p[1] for p in pts])
    assert wpts == pts and wst == [0] * n

    d_limbs, d_pad = put32(dev, [v for limbs, _ in items for v in limbs]), put32(dev, [v for p in pads for row in p for v in row])
    d_sk, d_k, d_pk = dev.put([w for k in sks for w in words5(k)]), dev.put([w for k in nonces for w in words5(k)]), dev.put([w for p in pks for w in flat_point(p)])
    d_m5 = dev.put([w for m in m5 for w in m])
    d_pts, d_used, d_c0, d_c1, d_back, d_h0, d_ct, d_hback, d_w = (dev.alloc(80 * n), dev.alloc(4 * n), dev.alloc(80 * n), dev.alloc(80 * n), dev.alloc(80 * n), dev.alloc(80 * n),
                                                                 dev.alloc(40 * n), dev.alloc(40 * n), dev.alloc(80 * n))
    d_st = [dev.alloc(4 * n) for _ in range(6)]
    with Stream(dev) as s:
        E.encode_binary_batch_device(d_limbs.value, d_pad.value, cs.ATTEMPTS, n, d_pts.value, d_used.value, d_st[0].value, stream=s)
        E.elgamal_encrypt_batch_device(d_pk.value, d_k.value, d_pts.value, n, d_c0.value, d_c1.value, d_st[1].value, stream=s)   # reads what encode wrote
        E.elgamal_decrypt_batch_device(d_sk.value, d_c0.value, d_c1.value, n, d_back.value, d_st[2].value, stream=s)
        E.hashed_elgamal_encrypt_batch_device(d_pk.value, d_k.value, d_m5.value, n, d_h0.value, d_ct.value, d_st[3].value, stream=s)
        E.hashed_elgamal_decrypt_batch_device(d_sk.value, d_h0.value, d_ct.value, n, d_hback.value, d_st[4].value, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    assert dev.get(d_pts, 10 * n) == [w for p in pts for w in flat_point(p)] and dev.get(d_used, n, C.c_uint32) == used
    assert dev.get(d_c0, 10 * n) == [w for p in c0s for w in flat_point(p)] and dev.get(d_c1, 10 * n) == [w for p in c1s for w in flat_point(p)]
    assert dev.get(d_back, 10 * n) == [w for p in back for w in flat_point(p)]
    assert dev.get(d_h0, 10 * n) == [w for p in h0s for w in flat_point(p)] and dev.get(d_ct, 5 * n) == [w for c in cts for w in c]
    assert dev.get(d_hback, 5 * n) == [w for m in hback for w in m]
    assert [dev.get(b, n, C.c_int) for b in d_st[:5]] == [est, cst, dst, hst, hdst]
    # decompress of the u halves of what encode wrote, from a buffer of compressed points; on the default stream
    d_u = dev.put([w for p in pts for w in p[1]])
    E.decompress_batch_device(d_u.value, n, d_w.value, d_st[5].value)
    assert dev.H.hipStreamSynchronize(None) == 0
    assert dev.get(d_w, 10 * n) == dev.get(d_pts, 10 * n) and dev.get(d_st[5], n, C.c_int) == [0] * n


@pytest.mark.parametrize("stride", (320, 400))
def test_scalar_bits_device(gpu, E, dev, stride):
    n = 65
    r = random.Random(cs.SEED + 15)
    ks = [0, 1, N - 1, N, cs.M320, 1 << 319, 1 << 64, (1 << 64) - 1] + [r.getrandbits(320) for _ in range(n - 8)]
    d_k = dev.put([w for k in ks for w in words5(k)])
    d_out = dev.put([7] * (n * stride))
    with Stream(dev) as s:
        E.scalar_bits_device(d_k.value, n, d_out.value, stride, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    got = dev.get(d_out, n * stride)
    assert got == [v for k in ks for v in [(k >> j) & 1 for j in range(320)] + [7] * (stride - 320)]
    with pytest.raises(gpu.P2Error):
        E.scalar_bits_device(d_k.value, n, d_out.value, 319)
    E.scalar_bits_device(d_k.value, 0, d_out.value, stride)


# ------------------------------------------------------------------ one pipeline with no host round trip
def test_encode_encrypt_prove_decrypt_without_a_host_round_trip(gpu, E, dev):
    """Messages and keys go up once.  encode_binary, elgamal_encrypt and scalar_bits run on the device; rows of the value matrix
    of the step-gate ElGamal circuit (tests/ec_circuits.py) are assembled by device-to-device copies on the same stream; the
    prover's ciphertext outputs equal the kernel's c0 | c1; the device decrypts and the host decodes the original limbs."""
    B = 4
    data, _, (pk_t, nonce_t, msg_t, ct_t), _ = ec_circuits.elgamal(gpu, [], ec_gate=True)
    assert data.info["degree_bits"] == 10
    items = cs.undirected(B, seed=cs.SEED + 16)
    assert all(ref.first_attempt(limbs, pads) < cs.ATTEMPTS for limbs, pads in items)
    r = random.Random(cs.SEED + 17)
    sks, nonces = [r.randrange(1, N) for _ in range(B)], [r.randrange(1, N) for _ in range(B)]
    pks, _ = E.mul_batch(sks, [ec.generator()] * B)
    targets = pk_t + msg_t + nonce_t
    n_t, outs = len(targets), ct_t[0] + ct_t[1]
    assert n_t == 340
    d_limbs, d_pad = put32(dev, [v for limbs, _ in items for v in limbs]), put32(dev, [v for _, p in items for row in p for v in row])
    d_sk, d_k, d_pk = dev.put([w for k in sks for w in words5(k)]), dev.put([w for k in nonces for w in words5(k)]), dev.put([w for p in pks for w in flat_point(p)])
    d_msg, d_used, d_c0, d_c1, d_back = dev.alloc(80 * B), dev.alloc(4 * B), dev.alloc(80 * B), dev.alloc(80 * B), dev.alloc(80 * B)
    d_vals, d_out, d_proofs = dev.put([gpu.VALUE_UNSET] * (B * n_t)), dev.alloc(8 * 20 * B), dev.alloc(B * data.proof_bytes)
    d_st = [dev.alloc(4 * B) for _ in range(4)]
    with Stream(dev) as s:
        E.encode_binary_batch_device(d_limbs.value, d_pad.value, cs.ATTEMPTS, B, d_msg.value, d_used.value, d_st[0].value, stream=s)
        E.elgamal_encrypt_batch_device(d_pk.value, d_k.value, d_msg.value, B, d_c0.value, d_c1.value, d_st[1].value, stream=s)
        E.scalar_bits_device(d_k.value, B, at(d_vals, 20).value, n_t, stream=s)
        for i in range(B):
            assert dev.H.hipMemcpyAsync(at(d_vals, n_t * i), at(d_pk, 10 * i), 80, D2D, s) == 0
            assert dev.H.hipMemcpyAsync(at(d_vals, n_t * i + 10), at(d_msg, 10 * i), 80, D2D, s) == 0
        data.prove_batch_outputs_device(targets, d_vals.value, outs, d_out.value, d_proofs.value, d_st[2].value, B, stream=s)
        E.elgamal_decrypt_batch_device(d_sk.value, d_c0.value, d_c1.value, B, d_back.value, d_st[3].value, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    assert [dev.get(b, B, C.c_int) for b in d_st] == [[0] * B] * 4
    c0, c1 = dev.get(d_c0, 10 * B), dev.get(d_c1, 10 * B)
    assert dev.get(d_out, 20 * B) == [w for i in range(B) for w in c0[10 * i:10 * i + 10] + c1[10 * i:10 * i + 10]]
    pb = data.proof_bytes
    host = C.create_string_buffer(B * pb)
    assert dev.H.hipMemcpy(host, d_proofs, B * pb, 2) == 0
    proofs = [host.raw[k * pb:(k + 1) * pb] for k in range(B)]
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * B
    back = dev.get(d_back, 10 * B)
    points = [(tuple(back[10 * i:10 * i + 5]), tuple(back[10 * i + 5:10 * i + 10])) for i in range(B)]
    assert E.decode_binary_batch(points) == [ref.int_of(limbs) for limbs, _ in items]
    assert points == [ref.encode_padded(limbs, pads)[0] for limbs, pads in items]
    # the ciphertext is the reference's for one item (two oracle multiplications)
    assert ref.elgamal_encrypt(pks[0], nonces[0], points[0]) == ((tuple(c0[0:5]), tuple(c0[5:10])), (tuple(c1[0:5]), tuple(c1[5:10])))


# ------------------------------------------------------------------ the decryption circuit
def decrypt_cases(E, count):
    """[(sk, pk, c0, c1, msg)]: ciphertexts from the batch kernel, checked against the reference where it is cheap"""
    sks = [cs.RAND_SK, 2, N - 1, 1][:count]
    pks = [ref.g_mul_gen(sk) for sk in sks]
    msgs = [ref.g_mul_gen(cs.RAND_M), ec.generator(), ec.NEUTRAL, ref.g_mul_gen(2)][:count]
    nonces = [cs.RAND_K, 1, 2, 0][:count]
    c0s, c1s, st = E.elgamal_encrypt_batch(pks, nonces, msgs)
    assert st == [0] * count and (c0s[0], c1s[0]) == ref.elgamal_encrypt(pks[0], nonces[0], msgs[0])
    return list(zip(sks, pks, c0s, c1s, msgs))


@pytest.fixture(scope="module")
def proven(gpu, E):
    c = cs.DecryptCircuit(gpu, True)
    assert c.data.info["degree_bits"] == 10 and c.data.num_public_inputs == 40
    cases = decrypt_cases(E, 4)
    maps = [c.witness(*case) for case in cases]
    sk, pk, c0, c1, msg = cases[0]
    maps.append(c.witness(sk ^ 1, pk, c0, c1))                 # a key that is not pk's: only the tie to pk can object
    proofs, st = c.data.prove_batch(maps)
    return c, cases, maps, proofs, st


def test_four_decryptions_prove_and_a_wrong_key_does_not(gpu, E, proven):
    c, cases, maps, proofs, st = proven
    assert st == [0, 0, 0, 0, 1]
    good = proofs[:4]
    for p, (sk, pk, c0, c1, msg) in zip(good, cases):
        c.data.verify(p)
        assert c.data.public_inputs(p) == flat_point(pk) + flat_point(c0) + flat_point(c1) + flat_point(msg)
    assert c.data.verify_batch(good) == [gpu.VERIFY_OK] * 4
    cproofs, cst = c.data.compress_batch(good)
    assert cst == [gpu.VERIFY_OK] * 4 and all(len(x) < c.data.proof_bytes for x in cproofs)
    assert c.data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * 4
    c.data.verify_compressed(cproofs[1])
    f = c.data.explain(maps[4])
    assert f.kind == "GENERATOR_CONFLICT" and f.target in c.pk + c.derived_pk and f == gpu.host_witness(c.data.blob, maps[4])[2]
    # the native decryption agrees with what was proven, and the witness run computes the message when it is not given
    assert E.elgamal_decrypt_batch([x[0] for x in cases], [x[2] for x in cases], [x[3] for x in cases]) == ([x[4] for x in cases], [0] * 4)
    vals, wst = c.data.generate_witness([c.witness(*x[:4]) for x in cases], c.out)
    assert wst == [0] * 4 and vals == [flat_point(x[4]) for x in cases]


def test_proofs_replay_under_the_reference(gpu, proven):
    c, _, _, proofs, _ = proven
    hasher, vd = R.memoised(R.poseidon_hasher()), c.data.verifier_data()
    assert R.replay(c.data.info, vd, proofs[0], hasher, blob=c.data.blob) is None
    for p in proofs[1:4]:
        assert R.replay(c.data.info, vd, p, hasher) is None


def test_one_proof_without_the_gate(gpu, E):
    """the arithmetic-gate circuit (2^14 rows): the same statement, through both verifiers and the replay"""
    c = cs.DecryptCircuit(gpu, False)
    assert c.data.info["degree_bits"] == 14
    (sk, pk, c0, c1, msg), = decrypt_cases(E, 1)
    proofs, st = c.data.prove_batch([c.witness(sk, pk, c0, c1, msg), c.witness(sk ^ 1, pk, c0, c1, msg)])
    assert st == [0, 1]
    c.data.verify(proofs[0])
    assert c.data.verify_batch(proofs[:1]) == [gpu.VERIFY_OK]
    assert c.data.public_inputs(proofs[0]) == flat_point(pk) + flat_point(c0) + flat_point(c1) + flat_point(msg)
    assert R.replay(c.data.info, c.data.verifier_data(), proofs[0], R.memoised(R.poseidon_hasher())) is None


def test_hashed_decryption_proves(gpu, E):
    c = cs.DecryptCircuit(gpu, True, hashed=True)
    sk, pk, m5 = cs.RAND_SK, ref.g_mul_gen(cs.RAND_SK), cs.message5(3)
    (c0,), (ct,), st = E.hashed_elgamal_encrypt_batch([pk], [cs.RAND_K], [m5])
    assert st == [0] and (c0, ct) == ref.hashed_elgamal_encrypt(pk, cs.RAND_K, m5)
    proofs, st = c.data.prove_batch([c.witness(sk, pk, c0, ct, m5), c.witness(sk, pk, c0, ct, cs.message5(4))])
    assert st == [0, 1]
    c.data.verify(proofs[0])
    assert c.data.verify_batch(proofs[:1]) == [gpu.VERIFY_OK] and c.data.public_inputs(proofs[0]) == flat_point(pk) + flat_point(c0) + list(ct) + list(m5)
