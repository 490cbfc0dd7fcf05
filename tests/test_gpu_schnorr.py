"""Native ecGFp5 and Schnorr signatures in GPU batches, and the signature circuit on the GPU.

Kernels: k_ec_scalar_muladd, k_ec_mul_batch, k_schnorr_sign and k_schnorr_verify against tests/schnorr_ref.py (the oracle's curve
in textbook affine arithmetic, the CPU oracle's Poseidon) and against the host twins.  Shapes: one thread per item at 64 per
block, so counts 1, 63, 64, 65 (one block, its last lane, the first lane of a second) and 257 (five blocks, the last of one
item); message lengths over the sponge-block boundaries (20 + msg_len crosses 24 and 32).  Expected statuses come by
construction: the reference signs, the case tampers (schnorr_cases.tampered).
Circuit: pk and a 5-word message public, the signature private; four proofs with the step gate through both verifiers,
compression and the replay of tests/proof_ref.py, a tampered fifth witness, the device witness against the host twin and the
reference's R; one proof without the gate through the same checks; and membership of the signed message in a committed set in
one circuit, with signatures and paths written on the proving stream.  (The CPU oracle cannot prove either circuit: it does not
know the bit hints of split_le, witness op LIMB -- as for tests/test_gpu_split.py the replay pins the proofs.)
Everything compared is exact."""
import ctypes as C
import random

import pytest

import proof_ref as R
import schnorr_cases as sc
import schnorr_ref as ref
from test_gpu_merkle import Device
from test_gpu_witness import twin_check

pytestmark = pytest.mark.gpu

ec, P, N = ref.ec, ref.P, ref.N
COUNTS = (1, 63, 64, 65, 257)
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


def words5(k):
    return [(k >> (64 * i)) & sc.M64 for i in range(5)]


def flat_point(p):
    return list(p[0]) + list(p[1])


def sig_words(sig):
    return words5(sig[0]) + list(sig[1])


class Stream:
    def __init__(self, dev):
        self.H, self.s = dev.H, C.c_void_p()
        assert self.H.hipStreamCreate(C.byref(self.s)) == 0

    def __enter__(self):
        return self.s

    def __exit__(self, *exc):
        self.H.hipStreamSynchronize(self.s)
        self.H.hipStreamDestroy(self.s)


# ------------------------------------------------------------------ scalars modulo the group order
@pytest.mark.parametrize("count", (1, 65))
def test_scalar_muladd_on_the_device(gpu, count):
    triples = sc.muladd_triples()
    triples = (triples * (count // len(triples) + 1))[:count] if count > 1 else triples[3:4]
    if count > 1:
        assert len(set(triples)) == len(sc.muladd_triples())   # 65 threads hold every directed triple
    arr = [(C.c_uint64 * (5 * count))(*[w for t in triples for w in words5(t[j])]) for j in range(3)]
    out = (C.c_uint64 * (5 * count))()
    assert gpu.lib().p2_gpu_ecgfp5_scalar_muladd(arr[0], arr[1], arr[2], count, out, 0) == 0, gpu.lib().p2_last_error()
    got = [sum(out[5 * i + j] << (64 * j) for j in range(5)) for i in range(count)]
    assert got == [(a * b + c) % N for a, b, c in triples]
    assert got == [gpu.ecgfp5.scalar_muladd(*t) for t in triples]


def test_scalar_muladd_single_threads_cover_the_directed_set(gpu):
    """count = 1 for every triple would be 61 launches; one launch per position of the directed operands keeps it to four"""
    triples = sc.muladd_triples()
    for t in triples[:4]:
        arr = [(C.c_uint64 * 5)(*words5(t[j])) for j in range(3)]
        out = (C.c_uint64 * 5)()
        assert gpu.lib().p2_gpu_ecgfp5_scalar_muladd(arr[0], arr[1], arr[2], 1, out, 0) == 0
        assert sum(out[j] << (64 * j) for j in range(5)) == (t[0] * t[1] + t[2]) % N


# ------------------------------------------------------------------ scalar multiplication
def test_mul_batch_against_the_oracle(gpu):
    q = ref.g_mul_gen(sc.RAND_SK)
    scalars = [0, 1, 2, N - 1, N, sc.M320, sc.RAND_K]
    ks = [k for k in scalars for _ in range(3)]
    ps = [p for _ in scalars for p in (ec.generator(), q, ec.NEUTRAL)]
    assert len(ks) == 21
    outs, st = gpu.ecgfp5.mul_batch(ks, ps)
    assert st == [0] * 21
    want = [ref.g_mul_gen(k) if p == ec.generator() else ec.NEUTRAL if p == ec.NEUTRAL else ec.g_mul(k, p) for k, p in zip(ks, ps)]
    assert outs == want
    assert outs[3 * 4] == ec.NEUTRAL and outs[3 * 3] == ec.g_neg(ec.generator())   # n G and (n - 1) G


def test_mul_batch_counts_against_the_host_and_points_outside_the_group(gpu):
    r = random.Random(11)
    base = [ec.generator(), ref.g_mul_gen(sc.RAND_SK), ref.g_mul_gen(2), ec.NEUTRAL]
    ks = [r.getrandbits(320) for _ in range(257)]
    ps = [base[i % 4] for i in range(257)]
    bad = {5: sc.point_outside_the_group(), 64: sc.with_word(base[1], 0, 0, (base[1][0][0] + 1) % P), 200: sc.with_word(base[0], 1, 2, sc.M64), 256: (ec.ZERO, base[0][1])}
    for i, p in bad.items():
        ps[i] = p
    want = [ec.NEUTRAL if i in bad else gpu.ecgfp5.mul(k, p) for i, (k, p) in enumerate(zip(ks, ps))]
    for count in COUNTS:
        outs, st = gpu.ecgfp5.mul_batch(ks[:count], ps[:count])
        assert st == [2 if i in bad else 0 for i in range(count)], count
        assert outs == want[:count], count


# ------------------------------------------------------------------ signing
@pytest.mark.parametrize("msg_len", sc.MSG_LENS)
def test_sign_batch_equals_the_reference(gpu, msg_len):
    sks, ks = [sc.RAND_SK, N - 1, 1, 2], [sc.RAND_K, 2, N - 1, sc.RAND_K]
    msgs = [sc.message(msg_len, i) for i in range(4)]
    sigs, pks, st = gpu.schnorr.sign_batch(sks, msgs, ks)
    assert st == [0] * 4
    assert sigs == [ref.sign(sk, m, k) for sk, m, k in zip(sks, msgs, ks)]
    assert pks == [ref.g_mul_gen(sk) for sk in sks]


def test_sign_batch_counts_and_malformed_rows(gpu):
    r = random.Random(12)
    sks, ks = [r.randrange(1, N) for _ in range(257)], [r.randrange(1, N) for _ in range(257)]
    msgs = [sc.message(5, i) for i in range(257)]
    bad = {0: ("sk", 0), 3: ("k", 0), 62: ("sk", N), 63: ("k", N + 1), 64: ("msg", P), 65: ("k", sc.M320), 130: ("msg", sc.M64), 256: ("sk", sc.M320)}
    for i, (what, v) in bad.items():
        if what == "sk":
            sks[i] = v
        elif what == "k":
            ks[i] = v
        else:
            msgs[i] = msgs[i][:4] + [v]
    want = gpu.schnorr.sign_batch(sks, msgs, ks, device=None)
    assert want[2] == [2 if i in bad else 0 for i in range(257)]
    assert all(want[0][i] == (0, (0, 0, 0, 0)) and want[1][i] == ec.NEUTRAL for i in bad)
    for count in COUNTS:
        sigs, pks, st = gpu.schnorr.sign_batch(sks[:count], msgs[:count], ks[:count])
        assert (sigs, pks, st) == (want[0][:count], want[1][:count], want[2][:count]), count
    # every honest row verifies, on the device and on the host
    good = [i for i in range(257) if i not in bad]
    args = ([want[1][i] for i in good], [msgs[i] for i in good], [want[0][i] for i in good])
    assert gpu.schnorr.verify_batch(*args) == [0] * len(good)
    assert gpu.schnorr.verify_batch(*[a[:5] for a in args], device=None) == [0] * 5


# ------------------------------------------------------------------ verification
def verify_cases():
    """257 items: good signatures of three reference key and nonce pairs over varied messages (k G is computed once per pair), every
    tampering class at known positions, the k = 0 signature"""
    pairs = [(sc.RAND_SK, sc.RAND_K), (N - 1, 2), (2, N - 1)]
    other = ref.g_mul_gen(1)
    items = []
    for i in range(257):
        sk, k = pairs[i % 3]
        m = sc.message(5, i)
        items.append(("honest", ref.g_mul_gen(sk), m, ref.sign(sk, m, k), 0))
    classes = sc.tampered(items[0][1], items[0][2], items[0][3], other)[1:]
    for j, pos in enumerate(range(1, 257, 6)):
        _, pk, m, sig, _ = items[pos]
        items[pos] = sc.tampered(pk, m, sig, other)[1 + j % len(classes)]
    assert {c[0] for c in items} >= {c[0] for c in classes} and len(classes) == 19
    items[64] = ("k = 0", items[64][1], items[64][2], sc.k0_signature(pairs[64 % 3][0], items[64][2]), 0)
    items[256] = ("k = 0", items[256][1], items[256][2], sc.k0_signature(pairs[256 % 3][0], items[256][2]), 0)
    return items


def test_verify_batch_statuses(gpu):
    items = verify_cases()
    args = ([c[1] for c in items], [c[2] for c in items], [c[3] for c in items])
    want = [c[4] for c in items]
    assert sorted(set(want)) == [0, 1, 2]
    got = gpu.schnorr.verify_batch(*args)
    assert got == want, [(i, items[i][0], g) for i, g in enumerate(got) if g != want[i]]
    assert gpu.schnorr.verify_batch(*args, device=None) == want
    for count in COUNTS[:4]:
        assert gpu.schnorr.verify_batch(*[a[:count] for a in args]) == want[:count], count


@pytest.mark.parametrize("msg_len", (0, 1, 3, 4, 11, 12, 13))
def test_verify_batch_over_the_message_lengths(gpu, msg_len):
    m = sc.message(msg_len)
    pk, other = ref.g_mul_gen(sc.RAND_SK), ref.g_mul_gen(2)
    cases = sc.tampered(pk, m, ref.sign(sc.RAND_SK, m, sc.RAND_K), other) + [("k = 0", pk, m, sc.k0_signature(sc.RAND_SK, m), 0)]
    assert gpu.schnorr.verify_batch([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]) == [c[4] for c in cases]


def test_limits(gpu):
    pk = ref.g_mul_gen(2)
    with pytest.raises(gpu.P2Error):
        gpu.schnorr.verify_batch([pk], [[0] * 1025], [(1, (0, 0, 0, 0))])
    with pytest.raises(gpu.P2Error):
        gpu.schnorr.sign_batch([1], [[0] * 1025], [1])
    m = sc.message(1024)
    sigs, pks, st = gpu.schnorr.sign_batch([sc.RAND_SK], [m], [sc.RAND_K])
    assert st == [0] and sigs[0] == ref.sign(sc.RAND_SK, m, sc.RAND_K)
    assert gpu.schnorr.verify_batch(pks, [m], sigs) == [0]
    assert gpu.schnorr.verify_batch([], [], []) == [] and gpu.ecgfp5.mul_batch([], []) == ([], [])


# ------------------------------------------------------------------ device-pointer forms, on a stream of their own
def test_device_pointer_forms_agree_with_the_host_pointer_forms(gpu, dev):
    n = 65
    r = random.Random(13)
    sks, ks = [r.randrange(1, N) for _ in range(n)], [r.randrange(1, N) for _ in range(n)]
    ks[7] = 0
    msgs = [sc.message(5, i) for i in range(n)]
    sigs, pks, st = gpu.schnorr.sign_batch(sks, msgs, ks)
    d_sk, d_k, d_msg = dev.put([w for k in sks for w in words5(k)]), dev.put([w for k in ks for w in words5(k)]), dev.put([w for m in msgs for w in m])
    d_sig, d_pk, d_st, d_vst, d_out, d_mst = dev.alloc(72 * n), dev.alloc(80 * n), dev.alloc(4 * n), dev.alloc(4 * n), dev.alloc(80 * n), dev.alloc(4 * n)
    with Stream(dev) as s:
        gpu.schnorr.sign_batch_device(d_sk.value, d_k.value, d_msg.value, 5, n, d_sig.value, d_pk.value, d_st.value, stream=s)
        gpu.schnorr.verify_batch_device(d_pk.value, d_msg.value, 5, d_sig.value, n, d_vst.value, stream=s)   # reads what sign wrote
        gpu.ecgfp5.mul_batch_device(d_k.value, d_pk.value, n, d_out.value, d_mst.value, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    assert dev.get(d_sig, 9 * n) == [w for g in sigs for w in sig_words(g)]
    assert dev.get(d_pk, 10 * n) == [w for p in pks for w in flat_point(p)]
    assert dev.get(d_st, n, C.c_int) == st == [2 if i == 7 else 0 for i in range(n)]
    # row 7 is zeros: the neutral as a key is malformed; the product with it is the neutral
    assert dev.get(d_vst, n, C.c_int) == [2 if i == 7 else 0 for i in range(n)] == gpu.schnorr.verify_batch(pks, msgs, sigs)
    outs, mst = gpu.ecgfp5.mul_batch(ks, pks)
    assert dev.get(d_out, 10 * n) == [w for p in outs for w in flat_point(p)] and dev.get(d_mst, n, C.c_int) == mst == [0] * n
    # without a public-key buffer
    d_sig2, d_st2 = dev.alloc(72 * n), dev.alloc(4 * n)
    gpu.schnorr.sign_batch_device(d_sk.value, d_k.value, d_msg.value, 5, n, d_sig2.value, None, d_st2.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    assert dev.get(d_sig2, 9 * n) == dev.get(d_sig, 9 * n) and dev.get(d_st2, n, C.c_int) == st


# ------------------------------------------------------------------ the circuit
KEYS = (sc.RAND_SK, 2, N - 1, 1)


@pytest.fixture(scope="module")
def proven(gpu):
    c = sc.SignatureCircuit(gpu, 5, True, public=True)
    assert c.data.info["degree_bits"] == 10 and c.data.num_public_inputs == 15
    msgs = [sc.message(5, 40 + i) for i in range(4)]
    pks = [ref.g_mul_gen(sk) for sk in KEYS]
    sigs = [ref.sign(sk, m, sc.RAND_K) for sk, m in zip(KEYS, msgs)]
    maps = [c.witness(pk, m, g) for pk, m, g in zip(pks, msgs, sigs)]
    maps.append(c.witness(pks[0], msgs[0], (sigs[0][0] ^ 4, sigs[0][1])))
    proofs, st = c.data.prove_batch(maps)
    return c, pks, msgs, sigs, maps, proofs, st


def test_four_signatures_prove_and_a_tampered_one_does_not(gpu, proven):
    c, pks, msgs, sigs, maps, proofs, st = proven
    assert st == [0, 0, 0, 0, 1]
    good = proofs[:4]
    for p, pk, m in zip(good, pks, msgs):
        c.data.verify(p)
        assert c.data.public_inputs(p) == flat_point(pk) + m
    assert c.data.verify_batch(good) == [gpu.VERIFY_OK] * 4
    cproofs, cst = c.data.compress_batch(good)
    assert cst == [gpu.VERIFY_OK] * 4 and all(len(x) < c.data.proof_bytes for x in cproofs)
    assert c.data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * 4
    c.data.verify_compressed(cproofs[1])
    # the native verifier agrees with what was proven
    assert gpu.schnorr.verify_batch(pks, msgs, sigs) == [0] * 4


def test_proofs_replay_under_the_reference(gpu, proven):
    c, _, _, _, _, proofs, _ = proven
    hasher, vd = R.memoised(R.poseidon_hasher()), c.data.verifier_data()
    assert R.replay(c.data.info, vd, proofs[0], hasher, blob=c.data.blob) is None
    for p in proofs[1:4]:
        assert R.replay(c.data.info, vd, p, hasher) is None


def test_device_witness_equals_the_host_twin_and_the_references_r(gpu, proven):
    c, pks, msgs, sigs, maps, _, _ = proven
    missing = dict(maps[1])
    del missing[c.sig[1][0]]
    cases = [maps[0], maps[4], maps[2], missing, maps[3]]
    assert twin_check(gpu, c.data, cases, c.r, (1, 5), (1, 10)) == [0, 1, 0, 2, 0]
    vals, st = c.data.generate_witness(maps[:4], c.r)
    assert st == [0] * 4 and vals == [flat_point(ref.g_mul_gen(sc.RAND_K))] * 4
    f = c.data.explain(maps[4])
    assert f.kind == "GENERATOR_CONFLICT" and f.target is not None and f == gpu.host_witness(c.data.blob, maps[4])[2]


def test_one_proof_without_the_gate(gpu):
    """the arithmetic-gate circuit (2^14 rows): the same statement, through both verifiers and the replay"""
    c = sc.SignatureCircuit(gpu, 5, False, public=True)
    assert c.data.info["degree_bits"] == 14
    m = sc.message(5, 40)
    pk, sig = ref.g_mul_gen(sc.RAND_SK), ref.sign(sc.RAND_SK, m, sc.RAND_K)
    proofs, st = c.data.prove_batch([c.witness(pk, m, sig), c.witness(pk, m, (sig[0] ^ 4, sig[1]))])
    assert st == [0, 1]
    c.data.verify(proofs[0])
    assert c.data.verify_batch(proofs[:1]) == [gpu.VERIFY_OK] and c.data.public_inputs(proofs[0]) == flat_point(pk) + m
    assert R.replay(c.data.info, c.data.verifier_data(), proofs[0], R.memoised(R.poseidon_hasher())) is None


def test_signatures_from_the_device_feed_the_prover_on_one_stream(gpu, dev):
    """sign_batch_device and prove_batch_device on one stream of the caller's: keys and challenge words go from the signer's
    buffers into the value matrix as they are; the matrix takes s as bits, which the host spells from the same buffer"""
    c = sc.SignatureCircuit(gpu, 5, True, public=True)
    B = 4
    r = random.Random(14)
    sks, ks = [r.randrange(1, N) for _ in range(B)], [r.randrange(1, N) for _ in range(B)]
    msgs = [sc.message(5, 60 + i) for i in range(B)]
    d_sk, d_k, d_msg = dev.put([w for k in sks for w in words5(k)]), dev.put([w for k in ks for w in words5(k)]), dev.put([w for m in msgs for w in m])
    d_sig, d_pk, d_st = dev.alloc(72 * B), dev.alloc(80 * B), dev.alloc(4 * B)
    targets = c.pk + c.msg + c.sig[1] + c.sig[0]
    pb = c.data.proof_bytes
    d_proofs, d_pst = dev.alloc(B * pb), dev.alloc(4 * B)
    with Stream(dev) as s:
        gpu.schnorr.sign_batch_device(d_sk.value, d_k.value, d_msg.value, 5, B, d_sig.value, d_pk.value, d_st.value, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
        sig, pk = dev.get(d_sig, 9 * B), dev.get(d_pk, 10 * B)
        rows = []
        for i in range(B):
            s_int = sum(sig[9 * i + j] << (64 * j) for j in range(5))
            rows += pk[10 * i:10 * i + 10] + msgs[i] + sig[9 * i + 5:9 * i + 9] + [(s_int >> j) & 1 for j in range(320)]
        d_vals = dev.put(rows)
        c.data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    assert dev.get(d_st, B, C.c_int) == [0] * B and dev.get(d_pst, B, C.c_int) == [0] * B
    host = C.create_string_buffer(B * pb)
    assert dev.H.hipMemcpy(host, d_proofs, B * pb, 2) == 0
    proofs = [host.raw[k * pb:(k + 1) * pb] for k in range(B)]
    assert c.data.verify_batch(proofs) == [gpu.VERIFY_OK] * B
    for i, p in enumerate(proofs):
        assert c.data.public_inputs(p) == pk[10 * i:10 * i + 10] + msgs[i]


def test_a_signed_member_of_a_committed_set(gpu, dev):
    """One 2^10-row circuit: the message is a leaf of a depth-4 tree under a public cap of two, and the holder of the public key
    signed it.  Signatures come from sign_batch_device and paths from the tree, both on the proving stream; the witness whose
    signature is over another leaf gets status 1."""
    import merkle_cases as mc
    depth, cap_height, B = 4, 1, 4
    num_leaves = 1 << (depth + cap_height)
    b = gpu.CircuitBuilder(ec_gate=True)
    m = mc.Membership(gpu, depth, cap_height, 5, builder=b)
    pk_t = b.add_virtual_point_target()
    sig_t = b.add_virtual_schnorr_signature_target()
    b.verify_schnorr_signature(pk_t, m.leaf, sig_t)
    b.register_public_inputs([t for h in m.cap for t in h] + pk_t)
    data = b.build()
    assert data.info["degree_bits"] == 10 and data.num_public_inputs == 8 + 10

    lv, levels = mc.ref(num_leaves, 5, seed=3)
    tree = gpu.MerkleTree(lv, cap_height)
    cap = tree.cap
    assert cap == mc.ref_cap(levels, cap_height)
    idx = [0, 31, 13, 18]
    signed = [lv[i] for i in idx]
    signed[2] = lv[14]                                       # witness 2: a signature over another leaf
    r = random.Random(15)
    sks, ks = [r.randrange(1, N) for _ in range(B)], [r.randrange(1, N) for _ in range(B)]
    d_sk, d_k, d_msg = dev.put([w for k in sks for w in words5(k)]), dev.put([w for k in ks for w in words5(k)]), dev.put([w for leaf in signed for w in leaf])
    d_sig, d_pk, d_sst = dev.alloc(72 * B), dev.alloc(80 * B), dev.alloc(4 * B)
    sib_t = [t for h in m.sibs for t in h]
    targets = m.leaf + m.bits + [t for h in m.cap for t in h] + pk_t + sig_t[1] + sig_t[0] + sib_t
    col, n_t = len(targets) - len(sib_t), len(targets)
    pb = data.proof_bytes
    d_idx, d_mst, d_proofs, d_pst = dev.put(idx), dev.alloc(4 * B), dev.alloc(B * pb), dev.alloc(4 * B)
    with Stream(dev) as s:
        gpu.schnorr.sign_batch_device(d_sk.value, d_k.value, d_msg.value, 5, B, d_sig.value, d_pk.value, d_sst.value, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
        sig, pk = dev.get(d_sig, 9 * B), dev.get(d_pk, 10 * B)
        rows = []
        for k, i in enumerate(idx):
            s_int = sum(sig[9 * k + j] << (64 * j) for j in range(5))
            rows += (list(lv[i]) + [(i >> j) & 1 for j in range(depth + cap_height)] + [w for h in cap for w in h] + pk[10 * k:10 * k + 10] +
                     sig[9 * k + 5:9 * k + 9] + [(s_int >> j) & 1 for j in range(320)] + [gpu.VALUE_UNSET] * len(sib_t))
        d_vals = dev.put(rows)
        tree.prove_batch_device(d_idx.value, B, d_vals.value + 8 * col, n_t, d_mst.value, stream=s)
        data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    assert dev.get(d_sst, B, C.c_int) == [0] * B and dev.get(d_mst, B, C.c_int) == [0] * B and dev.get(d_pst, B, C.c_int) == [0, 0, 1, 0]
    host = C.create_string_buffer(B * pb)
    assert dev.H.hipMemcpy(host, d_proofs, B * pb, 2) == 0
    proofs = [host.raw[k * pb:(k + 1) * pb] for k in range(B)]
    good = [p for k, p in enumerate(proofs) if k != 2]
    for k, p in zip((0, 1, 3), good):
        data.verify(p)
        assert data.public_inputs(p) == [w for h in cap for w in h] + pk[10 * k:10 * k + 10]
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK, gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_OK]
    # the signatures are the reference's: its verifier on one of them (two oracle multiplications)
    s0 = (sum(sig[j] << (64 * j) for j in range(5)), tuple(sig[5:9]))
    assert ref.verify((tuple(pk[0:5]), tuple(pk[5:10])), lv[idx[0]], s0) == 0
    assert R.replay(data.info, data.verifier_data(), good[0], R.memoised(R.poseidon_hasher()), blob=data.blob) is None
