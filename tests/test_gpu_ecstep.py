"""EcStepGate on the GPU: the device instantiation of the shared constraint evaluator against the Python restatement, the
ECSTEP branch of the witness kernels (k_ecwitness, k_witness_check) against the host twin and ec.g_mul, and proofs of the
ecgfp5 circuits built with the gate -- k_ecstep_post behind k_quotient, k_vfy_ecvanishing -- held to both verifiers,
compression and the proof replay of tests/proof_ref.py (the CPU oracle does not know the gate).  The soundness test proves
rows without a generator from wrong values: a gate nobody evaluates would let them through.

Shapes: 2 and 3 rows (2^2 / 2^3 rows of the circuit), one scalar multiplication (2^9), ElGamal and hashed ElGamal (2^10).
Everything compared is a field element, a byte string or a status code: exact."""
import ctypes as C
import random

import pytest

import ec_circuits as K
import proof_ref as R
import test_gpu_proof_replay as replay
from ec_circuits import ec
from test_gpu_witness import twin_check

pytestmark = pytest.mark.gpu
P = K.P


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


# ------------------------------------------------------------------ 6. the evaluator on the device
@pytest.fixture(scope="module")
def vectors():
    rows = K.vectors()
    return rows, [K.constraints(w) for w in rows]


@pytest.mark.parametrize("count", (1, 63, 64, 65, 257))
def test_device_evaluator_equals_the_restatement(gpu, vectors, count):
    rows, want = vectors
    pick = [i % len(rows) for i in range(count)]
    buf = (C.c_uint64 * (80 * count))(*[v for i in pick for v in rows[i]])
    out = (C.c_uint64 * (40 * count))()
    assert gpu.lib().p2_gpu_ecstep_constraints(buf, count, out, 0) == 0, gpu.lib().p2_last_error()
    for j, i in enumerate(pick):
        assert list(out[40 * j:40 * j + 40]) == want[i], (j, i)


# ------------------------------------------------------------------ 7. device witness against the host twin
def five(honest, wrong, missing):
    """the two failing witnesses between honest ones, in different chunks of two"""
    return [honest[0], wrong, honest[1], missing, honest[2]]


def fresh_handle(gpu, monkeypatch, blob, fuse):
    """a handle whose witness schedule is built under P2AES_WITNESS_FUSE = fuse (None: unset)"""
    if fuse:
        monkeypatch.setenv("P2AES_WITNESS_FUSE", fuse)
    else:
        monkeypatch.delenv("P2AES_WITNESS_FUSE", raising=False)
    data = gpu.CircuitData(blob)
    data.gpu()
    if fuse:
        monkeypatch.delenv("P2AES_WITNESS_FUSE")
    return data


@pytest.mark.parametrize("fuse", (None, "8"))
def test_three_steps_equal_the_host_twin(gpu, monkeypatch, fuse):
    built, bits, base, rows = K.steps_circuit(gpu, 3)
    data = fresh_handle(gpu, monkeypatch, built.blob, fuse)
    r = random.Random(21)
    honest, want = [], []
    for bv in ([1, 0, 1], [0, 1, 1], [1, 1, 0]):
        q = K.random_point(r)
        honest.append(dict(zip(bits + base, bv + list(q[0]) + list(q[1]))))
        want.append([v for mid, out in K.chain(bv, q) for v in K.flat(mid) + K.flat(out)])
    outs = [t for mid, out in rows for t in mid + out]
    wrong, missing = dict(honest[0]), dict(honest[1])
    wrong[rows[1][1][7]] = (want[0][20 + 40 + 7] + 1) % P      # an `out` coefficient of the second row
    del missing[base[3]]                                        # a Q coefficient
    cases = five(honest, wrong, missing)
    assert twin_check(gpu, data, cases, outs, (1, 3, 5), (1, 64, len(outs))) == [0, 1, 0, 2, 0]
    got = [data.explain(m) for m in cases]
    assert got == [gpu.host_witness(data.blob, m)[2] for m in cases]
    assert [f.kind for f in got] == ["NONE", "GENERATOR_CONFLICT", "NONE", "NOT_SET", "NONE"]
    assert got[1].op_kind == "ECSTEP" and got[1].gate_row == (rows[1][1][7] & ~(1 << 63)) >> 8 and got[3].target == base[3]
    vals, st = data.generate_witness(honest, outs)
    assert st == [0, 0, 0] and vals == want


@pytest.mark.parametrize("fuse", (None, "8"))
def test_scalar_multiplication_equals_the_host_twin(gpu, monkeypatch, fuse):
    built, k_t, base_t, res_t = K.multiply_circuit(gpu)
    data = fresh_handle(gpu, monkeypatch, built.blob, fuse)
    r = random.Random(22)
    N = ec.GROUP_ORDER
    honest, want = [], []
    for k, q in ((N - 1, K.random_point(r)), (2**320 - 1, ec.generator()), (r.randrange(N), K.random_point(r))):
        honest.append(dict(zip(k_t + base_t, [(k >> i) & 1 for i in range(320)] + list(q[0]) + list(q[1]))))
        want.append(ec.g_mul(k, q))
    wrong, missing = dict(honest[0]), dict(honest[1])
    wrong[res_t[0]] = (want[0][0][0] + 1) % P
    del missing[base_t[9]]
    cases = five(honest, wrong, missing)
    assert twin_check(gpu, data, cases, res_t, (1, 5), (1, 10)) == [0, 1, 0, 2, 0]
    vals, st = data.generate_witness(honest, res_t)
    assert st == [0, 0, 0] and [(tuple(v[:5]), tuple(v[5:])) for v in vals] == want


# ------------------------------------------------------------------ 8. ElGamal with the gate
@pytest.fixture(scope="module")
def elgamal(gpu):
    data, pws, (pk_t, nonce_t, msg_t, ct_t), cases = K.elgamal(gpu, [1, 2, 3])
    maps = [pw.map for pw in pws]
    proofs, st, vals = data.prove_batch(maps, outputs=ct_t[0] + ct_t[1])
    assert st == [0, 0, 0]
    return data, maps, cases, proofs, vals


def test_elgamal_ciphertexts_are_the_native_ones(gpu, elgamal):
    data, maps, cases, proofs, vals = elgamal
    assert data.info["degree_bits"] <= 11
    for v, (pk, msg, nonce) in zip(vals, cases):
        got = ((tuple(v[0:5]), tuple(v[5:10])), (tuple(v[10:15]), tuple(v[15:20])))
        assert got == tuple(gpu.ecgfp5.elgamal_encrypt(pk, nonce, msg)) == tuple(ec.elgamal_encrypt(pk, nonce, msg))


def test_elgamal_proofs_verify_compress_and_reject_a_flip(gpu, elgamal):
    data, maps, cases, proofs, vals = elgamal
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 3
    bad = dict(R.tamper_cases(data.info, proofs[1]))["open_wires"]
    host_code = gpu.VERIFY_REASONS[replay.host_reason(gpu, data, bad)]
    assert data.verify_batch([bad, proofs[1]]) == [host_code, gpu.VERIFY_OK] and host_code != gpu.VERIFY_OK
    c = data.compress(proofs[2])
    assert len(c) < len(proofs[2])
    data.verify_compressed(c)
    assert data.decompress(c) == proofs[2]


def test_elgamal_proof_replays(gpu, elgamal, monkeypatch):
    data, maps, cases, proofs, vals = elgamal
    monkeypatch.setattr(replay, "_build", lambda pkg_view, name: (gpu.CircuitData(data.blob), maps))
    p = replay.Proven(gpu, gpu, "poseidon", "elgamal_ecstep")
    assert p.proof == proofs[2]
    assert R.replay(p.info, p.vd, p.proof, R.memoised(p.hasher), blob=data.blob) is None
    replay.test_transcript(p)
    replay.test_caps_and_merkle_paths(p)
    replay.test_wires_leaves(p)
    replay.test_openings(p)
    replay.test_fri(p)
    replay.test_vanishing_identity(p)


@pytest.mark.parametrize("kw", ({"hasher": "keccak"}, {"zero_knowledge": True}), ids=("keccak", "zk"))
def test_public_key_under_the_other_configurations(gpu, kw):
    data, pws, (sk_t, pk_t), cases = K.public_key(gpu, [4, 5], **kw)
    proofs, st, vals = data.prove_batch([pw.map for pw in pws], outputs=pk_t)
    assert st == [0, 0]
    assert [(tuple(v[:5]), tuple(v[5:])) for v in vals] == [pk for sk, pk in cases]
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 2


# ------------------------------------------------------------------ 9. Poseidon rows and step rows in one circuit
def test_hashed_elgamal_with_the_gate(gpu):
    data, pws, (pk_t, nonce_t, msg_t, ct_t), cases = K.hashed_elgamal(gpu, [1, 2])
    assert data.info["degree_bits"] <= 11
    proofs, st, vals = data.prove_batch([pw.map for pw in pws], outputs=ct_t[0] + ct_t[1])
    assert st == [0, 0]
    for v, (pk, msg, nonce) in zip(vals, cases):
        c0, ct = gpu.ecgfp5.hashed_elgamal_encrypt(pk, nonce, msg)
        assert (tuple(v[0:5]), tuple(v[5:10])) == tuple(c0) == ec.g_mul(nonce, ec.generator()) and tuple(v[10:15]) == tuple(ct)
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 2


# ------------------------------------------------------------------ 10. soundness: rows without a generator
def test_rows_without_a_generator_are_held_by_the_constraints(gpu):
    data, bits, base, rows = K.steps_circuit(gpu, 2, hinted=False)
    q = K.random_point(random.Random(23))
    bv = [1, 1]
    steps = K.chain(bv, q)
    honest = dict(zip(bits + base, bv + list(q[0]) + list(q[1])))
    for (mid_t, out_t), (mid, out) in zip(rows, steps):
        honest.update(zip(mid_t + out_t, K.flat(mid) + K.flat(out)))
    wrong_mid, wrong_out = dict(honest), dict(honest)
    wrong_mid[rows[0][0][3]] = (honest[rows[0][0][3]] + 1) % P    # a `mid` coefficient of the first row
    wrong_out[rows[1][1][12]] = (honest[rows[1][1][12]] + 1) % P  # an `out` coefficient of the second row
    proofs, st = data.prove_batch([honest])
    assert st == [0]
    data.verify(proofs[0])
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK]
    for m in (wrong_mid, wrong_out):
        assert data.generate_witness([m], [])[1] == [0]           # no generator to disagree
        proofs, st = data.prove_batch([m])
        if st[0] == 0:                                            # then the proof must not verify
            reason = replay.host_reason(gpu, data, proofs[0])
            assert "vanishing" in reason, reason
            assert data.verify_batch(proofs) == [gpu.VERIFY_VANISHING] == [gpu.VERIFY_REASONS[reason]]
