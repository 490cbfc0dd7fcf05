"""GHASH from carry-less multiply tables on the GPU.  The gadget is ArithmeticGate, LookupGate and LookupTableGate rows, which
the CPU oracle follows, so the proofs of the multiplication circuit and of AesGcmTarget built under
CircuitBuilder(ghash_tables=lanes) are held byte for byte to the oracle's, the values the witness run returns to the native
cipher, and the proofs to both verifiers.  The Keccak and public-input builds, which the oracle does not follow, are held to the
proof replay of tests/proof_ref.py the way tests/test_gpu_proof_replay.py does it.

Shapes: one multiplication (2^13 rows: three 2521-row tables), AES-GCM-128 over 13 bytes at lanes = 1 and AES-GCM-256 over 45
bytes at lanes = 2 (four GHASH blocks, two groups), both 2^14 rows -- four 2521-row tables allow nothing smaller.
Everything compared is a byte string, a field element or a status: exact."""
import random

import pytest

import ghash_circuits as K
import proof_ref as R
import test_gpu_proof_replay as replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def oracle_proofs(orc, data, maps):
    oc = orc.OracleCircuit(data.blob)
    assert data.verifier_data() == oc.verifier_data()
    out = []
    for m in maps:
        st, proof = oc.prove(m)
        assert st == 0
        out.append(proof)
    return out


# ------------------------------------------------------------------ 1. one multiplication
@pytest.fixture(scope="module")
def product(gpu):
    data, x_t, y_t, z_t, _ = K.mul(gpu)
    pairs = K.edge_pairs()                                   # zero, all 0xff, two random
    maps = [K.mul_inputs(x_t, y_t, x, y) for x, y in pairs]
    proofs, st, vals = data.prove_batch(maps, outputs=z_t)
    return data, pairs, maps, proofs, st, vals


def test_multiplication_proofs_are_the_oracles(gpu, orc, product):
    data, pairs, maps, proofs, st, vals = product
    assert data.info["degree_bits"] == 13 and st == [0, 0, 0, 0]
    assert [bytes(v) for v in vals] == [gpu.native.gf_2_128_mul(x, y) for x, y in pairs]
    assert proofs == oracle_proofs(orc, data, maps)


def test_multiplication_proofs_pass_both_verifiers(gpu, product):
    data, pairs, maps, proofs, st, vals = product
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 4


def test_a_wrong_product_byte_between_honest_witnesses(gpu, product):
    data, pairs, maps, proofs, st, vals = product
    _, x_t, y_t, z_t, _ = K.mul(gpu)
    wrong = dict(maps[2])
    wrong.update(zip(z_t, vals[2]))
    wrong[z_t[11]] = (vals[2][11] + 1) % 256
    batch = maps[:2] + [wrong] + maps[2:]
    got, st = data.prove_batch(batch)
    twin = gpu.host_witness(data.blob, wrong)
    assert st == [0, 0, twin[1], 0, 0] and twin[1] == 1 and got[2] is None
    assert got[:2] + got[3:] == proofs
    fault = data.explain(wrong)
    assert fault == twin[2] and fault.kind == "GENERATOR_CONFLICT" and fault.target == z_t[11]
    assert (fault.computed, fault.found) == (vals[2][11], (vals[2][11] + 1) % 256)


# ------------------------------------------------------------------ 2. AesGcmTarget with the switch
GCM_CASES = {"aes128_13_lanes1": (4, 13, 1), "aes256_45_lanes2": (8, 45, 2)}


@pytest.fixture(scope="module", params=sorted(GCM_CASES))
def gcm(request, gpu):
    nk, L, lanes = GCM_CASES[request.param]
    data, t = K.gcm(gpu, nk, L, lanes)
    r = random.Random(nk * L)
    cases = [(bytes([42] * (4 * nk)), bytes([111] * 12), bytes([42] * L)),   # circuit_gcm.rs:695 test_encrypt
             tuple(bytes(r.randrange(256) for _ in range(n)) for n in (4 * nk, 12, L))]
    maps = [K.gcm_inputs(t, *c) for c in cases]
    proofs, st, vals = data.prove_batch(maps, outputs=t.ct + t.tag)
    return data, t, cases, maps, proofs, st, vals


def test_gcm_ciphertext_and_tag_are_the_native_ones(gpu, gcm):
    data, t, cases, maps, proofs, st, vals = gcm
    assert data.info["degree_bits"] == 14 and data.info["num_luts"] == 5 and st == [0, 0]
    for v, (key, iv, pt) in zip(vals, cases):
        ct, tag = gpu.native.gcm_encrypt(key, iv, pt)
        assert bytes(v) == ct + tag


def test_gcm_proofs_are_the_oracles_and_pass_both_verifiers(gpu, orc, gcm):
    data, t, cases, maps, proofs, st, vals = gcm
    assert proofs == oracle_proofs(orc, data, maps)
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 2


def test_gcm_flipped_tag_bit_is_refused_at_witness_generation(gpu, gcm):
    data, t, cases, maps, proofs, st, vals = gcm
    honest = dict(maps[1])
    honest.update(zip(t.tag, vals[1][-16:]))
    bad = dict(honest)
    bad[t.tag[3]] ^= 0x10
    assert data.generate_witness([honest, bad, honest], [])[1] == [0, 1, 0]
    got, st = data.prove_batch([bad, honest])
    assert st == [1, 0] and got[0] is None and got[1] == proofs[1]
    assert data.explain(bad) == gpu.host_witness(data.blob, bad)[2]


# ------------------------------------------------------------------ 3. the builds the oracle does not follow
OTHER = {"keccak": dict(hasher="keccak"), "public_inputs": dict(public=True)}


@pytest.fixture(scope="module", params=sorted(OTHER))
def other(request, gpu):
    """AES-GCM-128 over 13 bytes, lanes = 1: three witnesses proved, the last proof and what the device held for it"""
    kw = OTHER[request.param]
    data, t = K.gcm(gpu, 4, 13, 1, **kw)
    r = random.Random(13)
    cases = [tuple(bytes(r.randrange(256) for _ in range(n)) for n in (16, 12, 13)) for _ in range(3)]
    maps = [K.gcm_inputs(t, *c) for c in cases]
    mp = pytest.MonkeyPatch()
    mp.setattr(replay, "_build", lambda pkg_view, name: (gpu.CircuitData(data.blob), maps))
    try:
        p = replay.Proven(gpu, gpu, kw.get("hasher", "poseidon"), "aes_gcm_13_ghash_tables_" + request.param)
    finally:
        mp.undo()
    ct, tag = gpu.native.gcm_encrypt(*cases[-1])
    return request.param, p, list(ct + tag)


def test_other_builds_pass_both_verifiers_and_compress(gpu, other):
    name, p, ct_tag = other
    p.data.verify(p.proof)
    assert p.data.verify_batch([p.proof]) == [gpu.VERIFY_OK]
    assert p.data.public_inputs(p.proof) == (ct_tag if name == "public_inputs" else [])
    assert p.info["num_public_inputs"] == (29 if name == "public_inputs" else 0)
    c = p.data.compress(p.proof)
    assert len(c) < len(p.proof)
    assert p.data.decompress(c) == p.proof
    p.data.verify_compressed(c)
    bad = dict(R.tamper_cases(p.info, p.proof))["open_wires"]
    host_code = gpu.VERIFY_REASONS[replay.host_reason(gpu, p.data, bad)]
    assert p.data.verify_batch([bad, p.proof]) == [host_code, gpu.VERIFY_OK] and host_code != gpu.VERIFY_OK


def test_other_builds_replay(gpu, other):
    name, p, ct_tag = other
    assert R.replay(p.info, p.vd, p.proof, R.memoised(p.hasher)) is None
    replay.test_transcript(p)
    replay.test_caps_and_merkle_paths(p)
    replay.test_wires_leaves(p)
    replay.test_openings(p)
    replay.test_fri(p)
