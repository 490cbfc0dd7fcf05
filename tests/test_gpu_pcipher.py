"""The Poseidon cipher in GPU batches, and sealed-message decryption inside a circuit, on the GPU.

Kernels: k_pcipher_encrypt and k_pcipher_decrypt.  Both are held to tests/pcipher_ref.py (lib.rs on the CPU oracle's Poseidon;
nothing of the library) on 12 items at each of l = 0..7 -- all three paddings, both sides of the reference's l > 3 rule -- and to
the host twins at counts 1, 63, 64, 65 (one block, its last lane, the first lane of a second) and 257 for l in 0, 2, 3, 4, 7, and
at count 65 for l = 129.  The directed decryption items (tests/pcipher_cases.py) get the statuses they were built for, with
zeroed rows, untouched neighbours and intact guard words behind every output buffer.
Circuit: four messages sealed on the device, the sealed circuit with the step gate proven with the messages read back from the
witness runs, both verifiers, compression, the replay of tests/proof_ref.py, and a tampered ciphertext that fails witness
generation.  Everything compared is exact."""
import ctypes as C
import random

import pytest

import elgamal_cases as ecs
import elgamal_ref as eref
import pcipher_cases as cs
import pcipher_ref as ref
import proof_ref as R
import schnorr_cases as sc
from test_gpu_merkle import Device
from test_gpu_schnorr import Stream

pytestmark = pytest.mark.gpu

P, N = ref.P, eref.N
COUNTS = (1, 63, 64, 65, 257)
GUARD = 0x5A5AA5A5C3C33C3C
flat = cs.flat


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture(scope="module")
def PN(gpu):
    return gpu.poseidon_native


@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


def split(items):
    return [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]


# ------------------------------------------------------------------ against the reference and the twins
@pytest.mark.parametrize("l", range(8))
def test_both_kernels_equal_the_reference(PN, orc, l):
    kss, nonces, msgs = split(cs.items(12, l))
    want = [ref.encrypt(ks, m, n) for ks, n, m in zip(kss, nonces, msgs)]
    assert all(ref.decrypt(ks, ct, n, l) == m for ks, n, m, ct in zip(kss, nonces, msgs, want))
    assert PN.encrypt_batch(kss, nonces, msgs) == (want, [0] * 12)
    assert PN.decrypt_batch(kss, nonces, want, l) == (msgs, [0] * 12)


@pytest.mark.parametrize("l", (0, 2, 3, 4, 7))
def test_counts_against_the_host_twins(PN, l):
    kss, nonces, msgs = split(cs.items(257, l, seed=cs.SEED + 2))
    msgs[64] = cs.with_word(msgs[64], l - 1, 4, P) if l else msgs[64]          # a malformed row at a block's first lane
    want = PN.encrypt_batch(kss, nonces, msgs, device=None)
    assert want[1] == [2 if (i == 64 and l) else 0 for i in range(257)]
    cts = [list(c) for c in want[0]]
    cts[62] = cs.with_word(cts[62], len(cts[62]) - 1, 0, (cts[62][-1][0] + 1) % P)   # a wrong tag beside a block's last lane
    back = PN.decrypt_batch(kss, nonces, cts, l, device=None)
    assert back[1][62] == 1 and back[0][63] == msgs[63] and back[1].count(0) >= 254
    for count in COUNTS:
        assert PN.encrypt_batch(kss[:count], nonces[:count], msgs[:count]) == (want[0][:count], want[1][:count]), count
        assert PN.decrypt_batch(kss[:count], nonces[:count], cts[:count], l) == (back[0][:count], back[1][:count]), count


def test_the_references_own_length_against_the_host_twins(PN):
    l = 129
    kss, nonces, msgs = split(cs.items(65, l, seed=cs.SEED + 3))
    want = PN.encrypt_batch(kss, nonces, msgs, device=None)
    assert want[1] == [0] * 65 and all(len(c) == 130 for c in want[0])
    assert PN.encrypt_batch(kss, nonces, msgs) == want
    assert PN.decrypt_batch(kss, nonces, want[0], l) == (msgs, [0] * 65) == PN.decrypt_batch(kss, nonces, want[0], l, device=None)


# ------------------------------------------------------------------ directed decryption items
@pytest.mark.parametrize("l", (4, 5, 6, 1, 2))
def test_directed_decryption_items(PN, orc, dev, l):
    rows = cs.directed_decrypt(l)
    n, nct = len(rows), ref.pad3(l) + 1
    want_st = [r[4] for r in rows]
    want_msgs = [r[5] if r[5] is not None else [ref.ZERO] * l for r in rows]
    assert {0, 1, 2} <= set(want_st)
    kss, nonces, cts = [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]
    assert PN.decrypt_batch(kss, nonces, cts, l) == (want_msgs, want_st)
    assert PN.decrypt_batch(kss, nonces, cts, l, device=None) == (want_msgs, want_st)
    # the device-pointer form on buffers with guard words behind them; statuses start as garbage
    d_ks, d_nonce, d_ct = dev.put([w for k in kss for w in flat(k)]), dev.put([w for x in nonces for w in x]), dev.put([w for c in cts for w in flat(c)])
    d_msg, d_st = dev.put([GUARD] * (5 * l * n + 4)), dev.put([GUARD] * ((n + 1) // 2 + 2))
    PN.decrypt_batch_device(d_ks.value, d_nonce.value, d_ct.value, l, n, d_msg.value, d_st.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    assert dev.get(d_msg, 5 * l * n + 4) == [w for m in want_msgs for w in flat(m)] + [GUARD] * 4
    assert dev.get(d_st, n, C.c_int) == want_st
    assert dev.get(d_st, (n + 1) // 2 + 2)[-2:] == [GUARD] * 2


def test_directed_encryption_items(PN, dev):
    l = 4
    kss, nonces, msgs = split(cs.items(6, l, seed=cs.SEED + 4))
    g = (kss[0][0], kss[0][1])
    kss[1] = sc.with_word(g, 0, 2, P)
    kss[2] = sc.with_word(g, 1, 4, cs.M64)
    nonces[3] = (nonces[3][0], P)
    msgs[4] = cs.with_word(msgs[4], 3, 0, cs.M64)
    want_st = [0, 2, 2, 2, 2, 0]
    nct, n = ref.pad3(l) + 1, 6
    cts, st = PN.encrypt_batch(kss, nonces, msgs)
    assert st == want_st and (cts, st) == PN.encrypt_batch(kss, nonces, msgs, device=None)
    assert all((c == [ref.ZERO] * nct) == bool(s) for c, s in zip(cts, st))
    d_ks, d_nonce, d_msg = dev.put([w for k in kss for w in flat(k)]), dev.put([w for x in nonces for w in x]), dev.put([w for m in msgs for w in flat(m)])
    d_ct, d_st = dev.put([GUARD] * (5 * nct * n + 4)), dev.put([GUARD] * 5)
    PN.encrypt_batch_device(d_ks.value, d_nonce.value, d_msg.value, l, n, d_ct.value, d_st.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    assert dev.get(d_ct, 5 * nct * n + 4) == [w for c in cts for w in flat(c)] + [GUARD] * 4
    assert dev.get(d_st, n, C.c_int) == want_st and dev.get(d_st, 5)[-2:] == [GUARD] * 2


# ------------------------------------------------------------------ limits, streams
def test_length_limit_and_empty_batches(gpu, PN):
    lib, u64 = gpu.lib(), C.c_uint64
    one, st = (u64 * 16)(), (C.c_int * 1)()
    assert lib.p2_poseidon_encrypt_batch(one, one, one, 3073, 1, one, st, 0) == 1 and "3072" in lib.p2_last_error().decode()
    assert lib.p2_poseidon_decrypt_batch(one, one, one, 3073, 1, one, st, 0) == 1
    assert lib.p2_poseidon_encrypt_batch_device(None, None, None, 3073, 0, None, None, 0, None) == 1
    assert lib.p2_poseidon_decrypt_batch_device(None, None, None, 3073, 0, None, None, 0, None) == 1
    assert PN.encrypt_batch([], [], []) == ([], []) and PN.decrypt_batch([], [], [], 3) == ([], [])
    with pytest.raises(gpu.P2Error):
        PN.encrypt_batch([cs.items(1, 0)[0][0]], [(0, 0)], [[ref.ZERO] * 3073])


def test_device_forms_on_a_stream_of_their_own(PN, dev):
    l, n = 5, 65
    kss, nonces, msgs = split(cs.items(n, l, seed=cs.SEED + 8))
    cts, st = PN.encrypt_batch(kss, nonces, msgs)
    assert st == [0] * n
    nct = ref.pad3(l) + 1
    d_ks, d_nonce, d_msg = dev.put([w for k in kss for w in flat(k)]), dev.put([w for x in nonces for w in x]), dev.put([w for m in msgs for w in flat(m)])
    d_ct, d_back = dev.alloc(40 * nct * n), dev.alloc(40 * l * n)
    d_st = [dev.alloc(4 * n) for _ in range(2)]
    with Stream(dev) as s:
        PN.encrypt_batch_device(d_ks.value, d_nonce.value, d_msg.value, l, n, d_ct.value, d_st[0].value, stream=s)
        PN.decrypt_batch_device(d_ks.value, d_nonce.value, d_ct.value, l, n, d_back.value, d_st[1].value, stream=s)   # reads what encrypt wrote
        assert dev.H.hipStreamSynchronize(s) == 0
    assert dev.get(d_ct, 5 * nct * n) == [w for c in cts for w in flat(c)]
    assert dev.get(d_back, 5 * l * n) == [w for m in msgs for w in flat(m)]
    assert [dev.get(b, n, C.c_int) for b in d_st] == [[0] * n] * 2


# ------------------------------------------------------------------ sealing
def sealed_inputs():
    r = random.Random(cs.SEED + 9)
    sks = [ecs.RAND_SK, 2, N - 1, r.randrange(1, N)]
    rs = [ecs.RAND_K, 1, r.randrange(1, N), N - 1]
    nonces = [(r.randrange(P), r.randrange(P)) for _ in range(4)]
    msgs = [[cs.fq(r) for _ in range(3)] for _ in range(4)]
    return sks, rs, nonces, msgs


def test_seal_and_open_round_trip(gpu, PN):
    sks, rs, nonces, msgs = sealed_inputs()
    pks, st = gpu.ecgfp5.mul_batch(sks, [eref.ec.generator()] * 4)
    assert st == [0] * 4 and pks[0] == eref.g_mul_gen(sks[0])
    Rs, cts, st = PN.seal_batch(pks, rs, nonces, msgs)
    assert st == [0] * 4 and (Rs, cts, st) == PN.seal_batch(pks, rs, nonces, msgs, device=None)
    assert Rs[0] == eref.g_mul_gen(rs[0]) and cts[0] == ref.encrypt(eref.g_mul(rs[0], pks[0]), msgs[0], nonces[0])
    assert PN.open_batch(sks, Rs, nonces, cts, 3) == (msgs, [0] * 4) == PN.open_batch(sks, Rs, nonces, cts, 3, device=None)
    # another key opens nothing
    assert PN.open_batch([sks[1]] + sks[1:], Rs, nonces, cts, 3) == ([[ref.ZERO] * 3] + msgs[1:], [1, 0, 0, 0])
    # a public key outside the group: status 2, rows zeroed, the others as before
    bad = [pks[0], sc.point_outside_the_group()] + pks[2:]
    for device in (0, None):
        Rs2, cts2, st2 = PN.seal_batch(bad, rs, nonces, msgs, device)
        assert st2 == [0, 2, 0, 0] and cts2[1] == [ref.ZERO] * 4 and Rs2[1] == eref.ec.NEUTRAL
        assert [cts2[i] for i in (0, 2, 3)] == [cts[i] for i in (0, 2, 3)]
    assert PN.open_batch(sks, [Rs[0], sc.point_outside_the_group()] + Rs[2:], nonces, cts, 3)[1] == [0, 2, 0, 0]


# ------------------------------------------------------------------ the sealed circuit
@pytest.fixture(scope="module")
def proven(gpu, PN):
    c = cs.SealedCircuit(gpu, True)
    sks, rs, nonces, msgs = sealed_inputs()
    pks, _ = gpu.ecgfp5.mul_batch(sks, [eref.ec.generator()] * 4)
    Rs, cts, st = PN.seal_batch(pks, rs, nonces, msgs)
    assert st == [0] * 4
    maps = [c.witness(sk, pk, Rp, n, ct) for sk, pk, Rp, n, ct in zip(sks, pks, Rs, nonces, cts)]
    maps.append(c.witness(sks[0], pks[0], Rs[0], nonces[0], cs.with_word(cts[0], 1, 2, (cts[0][1][2] + 1) % P)))   # one tampered ciphertext word
    proofs, st, vals = c.data.prove_batch(maps, outputs=c.out)
    return c, (pks, Rs, nonces, cts, msgs), maps, proofs, st, vals


def test_four_sealed_messages_prove_and_a_tampered_one_does_not(gpu, proven):
    c, (pks, Rs, nonces, cts, msgs), maps, proofs, st, vals = proven
    assert c.data.info["degree_bits"] == 10 and c.data.num_public_inputs == 42
    assert st == [0, 0, 0, 0, 1]
    assert vals[:4] == [flat(m) for m in msgs]
    good = proofs[:4]
    for p, pk, Rp, n, ct in zip(good, pks, Rs, nonces, cts):
        c.data.verify(p)
        assert c.data.public_inputs(p) == ecs.flat_point(pk) + ecs.flat_point(Rp) + list(n) + flat(ct)
    assert c.data.verify_batch(good) == [gpu.VERIFY_OK] * 4
    cproofs, cst = c.data.compress_batch(good)
    assert cst == [gpu.VERIFY_OK] * 4 and all(len(x) < c.data.proof_bytes for x in cproofs)
    assert c.data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * 4
    back, bst = c.data.decompress_batch(cproofs)
    assert bst == [gpu.VERIFY_OK] * 4 and back == good
    f = c.data.explain(maps[4])
    assert f.kind == "GENERATOR_CONFLICT" and f == gpu.host_witness(c.data.blob, maps[4])[2]


def test_one_proof_replays_under_the_reference(gpu, proven):
    c, proofs = proven[0], proven[3]
    assert R.replay(c.data.info, c.data.verifier_data(), proofs[0], R.memoised(R.poseidon_hasher()), blob=c.data.blob) is None
