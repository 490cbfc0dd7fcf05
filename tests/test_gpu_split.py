"""Bit and byte decomposition on the GPU: the OP_LIMB branch of k_witness (both CHAINS instantiations, with and without
PoseidonGate rows) against the host twin and against Python's own bits, and proofs of circuits that use the gadgets held to
both verifiers, compression and the proof replay of tests/proof_ref.py (the CPU oracle does not know the op).

Shapes: the five-width split_le circuit and the 1/7/8-byte one (2^5 rows), 40 x 63 bits (2^8 rows; 2520 hints in one level:
a full and a partial trip of the 4 x 512 single-op loop), and the bridge circuit -- Poseidon hash -> 16 key bytes -> AES-128
block, 2^13 rows as every one-block AES circuit.  Everything compared is a field element, a byte or a status code: exact."""
import pytest

import proof_ref as R
import split_circuits as sc
import test_gpu_proof_replay as replay
from test_gpu_witness import twin_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def five(maps, wrong, missing):
    """the two failing witnesses between honest ones, in different chunks of two"""
    return [maps[0], wrong, maps[1], missing, maps[2]]


def explain_equals_the_twin(pkg, data, maps):
    got = [data.explain(m) for m in maps]
    assert got == [pkg.host_witness(data.blob, m)[2] for m in maps]
    return got


# ------------------------------------------------------------------ device against the host twin
def test_split_le_equals_the_host_twin(gpu):
    data, xs, bits, maps, want = sc.split_le(gpu)
    flat = [t for bs in bits for t in bs]
    wrong, missing = dict(maps[3]), dict(maps[4])
    wrong[bits[3][62]] = 1 - ((wrong[xs[3]] >> 62) & 1)   # a bit that loses against its hint
    del missing[xs[1]]
    cases = five(maps, wrong, missing)
    assert twin_check(gpu, data, cases, flat, (1, 3, 5), (1, 64, len(flat))) == [0, 1, 0, 2, 0]
    got = explain_equals_the_twin(gpu, data, cases)
    assert [f.kind for f in got] == ["NONE", "GENERATOR_CONFLICT", "NONE", "NOT_SET", "NONE"]
    assert got[1].op_kind == "LIMB" and got[1].target == bits[3][62] and got[3].target == xs[1]
    vals, st = data.generate_witness(maps, flat)
    assert st == [0] * len(maps) and vals == want


def test_split_bytes_le_equals_the_host_twin(gpu):
    data, xs, parts, maps, want = sc.split_bytes_le(gpu)
    flat = [t for p in parts for t in p]
    wrong, missing = dict(maps[3]), dict(maps[4])
    wrong[xs[1]] = 1 << 56                                # does not fit seven bytes
    del missing[xs[2]]
    cases = five(maps, wrong, missing)
    assert twin_check(gpu, data, cases, flat, (1, 3, 5), (1, len(flat))) == [0, 1, 0, 2, 0]
    got = explain_equals_the_twin(gpu, data, cases)
    assert [f.kind for f in got] == ["NONE", "GENERATOR_CONFLICT", "NONE", "NOT_SET", "NONE"]
    vals, st = data.generate_witness(maps, flat)
    assert st == [0] * len(maps) and vals == want


@pytest.mark.parametrize("n", (1, 62))
def test_is_less_than_on_the_device(gpu, n):
    data, x, y, lt = sc.is_less_than(gpu, n)
    pairs = sc.lt_pairs(n) + [(1 << n, 0)]
    vals, st = data.generate_witness([{x: a, y: c} for a, c in pairs], [lt])
    assert st == [0] * 5 + [1]
    assert [v[0] for v in vals[:5]] == [int(a < c) for a, c in pairs[:5]]


# ------------------------------------------------------------------ a level wider than one trip of the single-op loop
@pytest.mark.parametrize("fuse", (None, "8"))
def test_wide_level(gpu, monkeypatch, fuse):
    blob_data, xs, bits = sc.wide(gpu)
    if fuse:
        monkeypatch.setenv("P2AES_WITNESS_FUSE", fuse)
    else:
        monkeypatch.delenv("P2AES_WITNESS_FUSE", raising=False)
    data = gpu.CircuitData(blob_data.blob)
    data.gpu()                                            # the schedule is built when the handle is loaded
    if fuse:
        monkeypatch.delenv("P2AES_WITNESS_FUSE")
        assert blob_data.witness_schedule(int(fuse))["chains"] > 0   # the Horner sums are what gets chained
    rows = [sc.wide_values(s) for s in range(3)]
    rows[1][17] = 1 << sc.WIDE_BITS                       # one input out of range
    vals, st = data.generate_witness([dict(zip(xs, r)) for r in rows], bits)
    assert st == [0, 1, 0]
    for got, r in zip(vals, rows):
        assert got == [bit for v in r for bit in sc.bits_of(v, sc.WIDE_BITS)]   # the hints are the low bits whatever the sum says


# ------------------------------------------------------------------ the bridge circuit: Poseidon -> bytes -> AES
@pytest.fixture(scope="module")
def bridge(gpu):
    data, secret, block, ct = sc.bridge(gpu)
    maps, want = sc.bridge_cases(gpu, 3)
    proofs, st, vals = data.prove_batch(maps, outputs=ct)
    assert st == [0, 0, 0]
    return data, maps, want, proofs, vals


def test_bridge_ciphertexts_are_the_native_ones(gpu, bridge):
    data, maps, want, proofs, vals = bridge
    assert data.info["degree_bits"] <= 13
    assert [bytes(v) for v in vals] == want and len(set(want)) == 3


def test_bridge_proofs_verify_compress_and_reject_a_flip(gpu, bridge):
    data, maps, want, proofs, vals = bridge
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


def test_bridge_proof_replays(gpu, bridge, monkeypatch):
    """the last proof of the batch against the independent replay, the way test_gpu_proof_replay.py holds the public-input
    circuits: transcript, caps and Merkle paths, wires leaves, openings, FRI"""
    data, maps, want, proofs, vals = bridge
    monkeypatch.setattr(replay, "_build", lambda pkg_view, name: (gpu.CircuitData(data.blob), maps))
    p = replay.Proven(gpu, gpu, "poseidon", "bridge")
    assert p.proof == proofs[2]                           # reading outputs changes no proof byte
    assert R.replay(p.info, p.vd, p.proof, R.memoised(p.hasher)) is None
    replay.test_transcript(p)
    replay.test_caps_and_merkle_paths(p)
    replay.test_wires_leaves(p)
    replay.test_openings(p)
    replay.test_fri(p)


# ------------------------------------------------------------------ the other two configurations
def test_keccak_build_proves_and_verifies(gpu):
    data, xs, bits, maps, want = sc.split_le(gpu, hasher="keccak")
    proofs, st, vals = data.prove_batch(maps[:2], outputs=[t for bs in bits for t in bs])
    assert st == [0, 0] and vals == want[:2] and data.info["hasher"] == "keccak"
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 2


def test_zero_knowledge_build_proves_and_verifies(gpu):
    data, xs, bits, maps, want = sc.split_le(gpu, zero_knowledge=True)
    proofs, st, vals = data.prove_batch(maps[:2], outputs=[t for bs in bits for t in bs])
    assert st == [0, 0] and vals == want[:2] and data.info["zero_knowledge"]
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * 2
