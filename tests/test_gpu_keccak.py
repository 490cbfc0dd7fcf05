"""The Keccak configuration (hasher="keccak") on the GPU.  The CPU oracle hashes with Poseidon and cannot follow, so the trees
are pinned from outside by the Python Keccak / Merkle restatement of tests/keccak_ref.py; the wire matrix is pinned by the
Poseidon build of the same circuit (whose witness the oracle checks elsewhere); here, everything after the wires commitment
is checked by the two verifiers (host and GPU), which must agree verdict for verdict.  Those stages -- transcript, caps, Merkle
paths, openings, FRI -- are pinned from outside by the Python proof replay in tests/test_gpu_proof_replay.py; only the
vanishing identity at zeta is left to the verifiers alone."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import circuits
import keccak_circuits
import keccak_ref
import verify_layout

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
CAP_HEIGHT = 4


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture(scope="module")
def kpkg(gpu):
    return keccak_circuits.KeccakPkg(gpu)


def _u64(data, name, index=0):
    return np.frombuffer(data.debug_read_bytes(name, index), dtype=np.uint64)


def _cap_words(cap):
    return [int(w) for w in np.asarray(cap).reshape(-1)]


def host_reason(pkg, data, proof):
    try:
        data.verify(proof)
        return ""
    except pkg.P2Error as e:
        return str(e).split("verify failed: ", 1)[1]


def host_reason_compressed(pkg, data, cproof):
    try:
        data.verify_compressed(cproof)
        return ""
    except pkg.P2Error as e:
        return str(e).split("verify_compressed failed: ", 1)[1]


# ---------------------------------------------------------------------------------------------- standalone trees
@pytest.mark.parametrize("width", [16, 17, 18, 33, 34, 51, 84, 135, 139])
def test_standalone_tree_caps(gpu, width):
    """p2_gpu_merkle_cap_hasher against the Python Merkle caps; the widths straddle every padding case (width = 16 mod 17 puts
    both pad bits in one word, width = 0 mod 17 needs a block of padding alone)."""
    L = gpu.lib()
    rnd = np.random.default_rng(width)
    for bits in range(5, 13):
        leaves = 1 << bits
        cols = rnd.integers(0, P, size=(width, leaves), dtype=np.uint64)
        flat = np.ascontiguousarray(cols).reshape(-1)
        cap = (C.c_uint64 * (4 << CAP_HEIGHT))()
        rc = L.p2_gpu_merkle_cap_hasher(flat.ctypes.data_as(C.POINTER(C.c_uint64)), width, leaves, CAP_HEIGHT, 1, cap, 0)
        assert rc == 0, L.p2_last_error().decode()
        assert list(cap) == _cap_words(keccak_ref.merkle_cap(cols.T, CAP_HEIGHT)), (width, bits)
    # the Poseidon entry is the hasher-0 form, and Keccak refuses leaves it would not hash
    cap0, cap1 = (C.c_uint64 * 64)(), (C.c_uint64 * 64)()
    assert L.p2_gpu_merkle_cap(flat.ctypes.data_as(C.POINTER(C.c_uint64)), width, leaves, CAP_HEIGHT, cap0, 0) == 0
    assert L.p2_gpu_merkle_cap_hasher(flat.ctypes.data_as(C.POINTER(C.c_uint64)), width, leaves, CAP_HEIGHT, 0, cap1, 0) == 0
    assert list(cap0) == list(cap1) != list(cap)
    assert L.p2_gpu_merkle_cap_hasher(flat.ctypes.data_as(C.POINTER(C.c_uint64)), 3, leaves, CAP_HEIGHT, 1, cap1, 0) != 0


# ---------------------------------------------------------------------------------------------- whole proofs
# pre_cap is recomputed from an LDE of pre_coeffs (p2_gpu_lde, hasher-independent) for circuits of at most 2^14 rows; above
# that (elgamal, 2^15 rows x ~90 columns x 8) the Python side of the comparison holds several GiB of numpy temporaries, so
# elgamal's preprocessed tree is checked through the verifiers only.  The 2^19-row circuit takes no part in the tree checks.
PRE_CAP_MAX_BITS = 14
NAMES = ["aes_block", "aes_gcm_13", "aes_gcm_13_tag", "poseidon_cipher", "elgamal", "zk", "public_inputs"]
_cache = {}


def _proven(gpu, kpkg, name):
    if name not in _cache:
        data, pws = keccak_circuits.build(kpkg, name, 3)
        if data.info["zero_knowledge"]:
            data.set_zk_seed(5)
        proofs, st = data.prove_batch(pws)
        assert st == [0] * len(pws), st
        _cache[name] = (data, pws, proofs)
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_keccak_proofs(gpu, kpkg, name):
    data, pws, proofs = _proven(gpu, kpkg, name)
    info = data.info
    assert info["hasher"] == "keccak"
    n, N = 1 << info["degree_bits"], 8 << info["degree_bits"]
    salt = 4 if info["zero_knowledge"] else 0
    # the wires commitment of the last proof of the batch against the Python tree over the LDE the device holds
    last = len(pws) - 1
    lde = _u64(data, "wires_lde", last)
    want = _cap_words(keccak_ref.merkle_cap_columns(lde, N, info["num_wires"] + salt, CAP_HEIGHT))
    assert [int(w) for w in _u64(data, "wires_cap", last)] == want
    assert list(struct.unpack_from("<64Q", proofs[last], 0)) == want
    del lde
    wires = data.debug_read_bytes("wires", last)
    # the constants | sigmas commitment
    vd = data.verifier_data()
    if info["degree_bits"] <= PRE_CAP_MAX_BITS:
        coeffs = np.ascontiguousarray(_u64(data, "pre_coeffs"))
        ncols = coeffs.size // n
        pre_lde = np.zeros(coeffs.size * 8, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        assert gpu.lib().p2_gpu_lde(coeffs.ctypes.data_as(u64p), ncols, info["degree_bits"], 3, pre_lde.ctypes.data_as(u64p), 0) == 0
        pre_cap = _cap_words(keccak_ref.merkle_cap_columns(pre_lde, N, ncols, CAP_HEIGHT))
        assert [int(w) for w in _u64(data, "pre_cap")] == pre_cap == vd[:64]
        # the circuit digest: the tree hasher over cap || hash_no_pad(padded empty domain separator) || degree_bits
        sep = keccak_ref.hash_no_pad(np.array([1] + [0] * 10 + [1], dtype=np.uint64))
        dig = keccak_ref.hash_no_pad(np.array(pre_cap + _cap_words(sep) + [info["degree_bits"]], dtype=np.uint64))
        assert vd[64:] == _cap_words(dig)
    assert all(w < (1 << 56) for w in vd[0::4] + vd[1::4] + vd[2::4]) and all(w < (1 << 32) for w in vd[3::4])
    # both verifiers accept, the public inputs read back
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * len(proofs)
    if name == "public_inputs":
        vals = keccak_circuits.pi_circuits.aes_gcm(kpkg, L=64, n=3)[2]
        assert [data.public_inputs(p) for p in proofs] == vals
    # the same circuit and witnesses under Poseidon: the same wire matrix, another proof, and neither verifies as the other
    pdata, ppws = keccak_circuits.build(gpu, name, 3)
    if pdata.info["zero_knowledge"]:
        pdata.set_zk_seed(5)
    pproofs, st = pdata.prove_batch(ppws)
    assert st == [0] * len(ppws)
    assert pdata.debug_read_bytes("wires", last) == wires
    assert pdata.proof_bytes == data.proof_bytes and pproofs[last] != proofs[last]
    for d, foreign in ((pdata, proofs[0]), (data, pproofs[0])):
        r = host_reason(gpu, d, foreign)
        assert r != ""
        assert d.verify_batch([foreign]) == [gpu.VERIFY_REASONS[r]]


def test_batch_sizes_and_options_give_the_same_bytes(gpu, kpkg):
    """Batches of 1, 16, 17 and 256, then other chunk / streams options: every proof is a function of its witness alone."""
    pairs = [(i & 255, (7 * i + 3) & 255) for i in range(256)]
    data, pws = circuits.gf_2_8_add(kpkg, pairs)
    full, st = data.prove_batch(pws)
    assert st == [0] * 256 and len(set(full)) == 256
    for b in (1, 16, 17):
        proofs, st = data.prove_batch(pws[:b])
        assert st == [0] * b and proofs == full[:b], b
    for chunk, streams in ((5, 3), (64, 1), (300, 2)):
        data.set_option("chunk", chunk)
        data.set_option("streams", streams)
        proofs, st = data.prove_batch(pws[:40])
        assert st == [0] * 40 and proofs == full[:40], (chunk, streams)
    assert data.verify_batch(full) == [gpu.VERIFY_OK] * 256
    # a fresh handle with small chunks from the start (another workspace shape altogether)
    data2, pws2 = circuits.gf_2_8_add(kpkg, pairs[:20])
    data2.set_option("chunk", 3)
    assert data2.prove_batch(pws2)[0] == full[:20]


# ---------------------------------------------------------------------------------------------- tampering
def _tampers(info, proof, query=3):
    """(label, bytes, expected host reason or None): one change per case."""
    sec = verify_layout.sections(info)
    rounds = info["num_fri_rounds"]

    def flip(name, byte=0, bit=0, at=0):
        b = bytearray(proof)
        b[sec[name][0] + at + byte] ^= 1 << bit
        return bytes(b)

    out = [("cap word", flip("zs_cap", at=8 * 5), None),
           ("leaf word", flip("q%d_init1_leaf" % query, at=8 * 2), "Invalid Merkle proof (initial tree)."),
           ("initial sibling, low byte", flip("q%d_init2_siblings" % query, at=32 * 1), "Invalid Merkle proof (initial tree)."),
           ("initial sibling, top byte", flip("q%d_init2_siblings" % query, at=32 * 1, byte=7), "hash word out of range"),
           ("initial sibling, fourth word", flip("q%d_init0_siblings" % query, at=32 * 2 + 24, byte=4), "hash word out of range"),
           ("cap, top byte", flip("quotient_cap", at=32 * 3 + 8, byte=7), "hash word out of range"),
           ("PoW witness", flip("pow_witness"), "Invalid proof-of-work witness.")]
    if rounds:
        out += [("FRI evaluation", flip("q%d_round0_evals" % query, at=16 * 5), None),
                ("FRI sibling, low byte", flip("q%d_round0_siblings" % query), "Invalid Merkle proof (FRI round)."),
                ("FRI sibling, top byte", flip("q%d_round0_siblings" % query, byte=7, at=16), "hash word out of range"),
                ("FRI cap, fourth word", flip("fri_cap0", at=32 * 7 + 24, byte=5), "hash word out of range")]
    return out


@pytest.mark.parametrize("name", ["aes_gcm_13", "elgamal", "zk"])  # (poseidon_cipher L = 3 is too small to have a FRI round)
def test_tampered_proofs_host_and_gpu_agree(gpu, kpkg, name):
    data, _, proofs = _proven(gpu, kpkg, name)
    cases = _tampers(data.info, proofs[-1])
    batch = [c[1] for c in cases] + [proofs[-1]]
    got = data.verify_batch(batch)
    for (label, bad, expect), code in zip(cases, got):
        r = host_reason(gpu, data, bad)
        assert r != "", label
        if expect is not None:
            assert r == expect, (label, r)
        assert code == gpu.VERIFY_REASONS[r], (label, r, code)
    assert got[-1] == gpu.VERIFY_OK
    assert gpu.VERIFY_REASONS["hash word out of range"] == gpu.VERIFY_NON_CANONICAL


# ---------------------------------------------------------------------------------------------- compressed proofs
@pytest.mark.parametrize("name", ["aes_gcm_13", "elgamal", "zk", "public_inputs"])
def test_compressed_proofs(gpu, kpkg, name):
    data, _, proofs = _proven(gpu, kpkg, name)
    want = [data.compress(p) for p in proofs]
    got, st = data.compress_batch(proofs)
    assert st == [gpu.VERIFY_OK] * len(proofs) and got == want
    assert all(len(c) < data.proof_bytes for c in got)
    assert [data.decompress(c) for c in want] == proofs
    full, st = data.decompress_batch(want)
    assert st == [gpu.VERIFY_OK] * len(proofs) and full == proofs
    assert data.verify_compressed_batch(want) == [gpu.VERIFY_OK] * len(proofs)
    for c in want:
        data.verify_compressed(c)
    # the tampered full proofs: compress agrees (status and bytes), and what compresses gets the same verdict on both sides
    if not data.info["num_public_inputs"]:
        cases = _tampers(data.info, proofs[0])
        cgot, cst = data.compress_batch([c[1] for c in cases])
        tampered_c = []
        for (label, bad, _), c, s in zip(cases, cgot, cst):
            try:
                hc = data.compress(bad)
                assert s == gpu.VERIFY_OK and c == hc, label
                tampered_c.append((label, hc))
            except gpu.P2Error as e:
                r = str(e).split("compress failed: ", 1)[1]
                assert s == gpu.VERIFY_REASONS[r] and c is None, (label, r, s)
        assert any(lbl == "leaf word" for lbl, _ in tampered_c)
        assert not any("top byte" in lbl or "fourth word" in lbl for lbl, _ in tampered_c)  # out of range: refused by compress
        codes = data.verify_compressed_batch([c for _, c in tampered_c])
        for (label, c), code in zip(tampered_c, codes):
            assert code == gpu.VERIFY_REASONS[host_reason_compressed(gpu, data, c)], label
    # bytes of a compressed proof changed in place: verdicts agree, and a stored sibling pushed out of range is seen by both
    rnd = random.Random(11)
    c0 = want[0]
    lo, hi = len(c0) // 4, len(c0) - 8
    batch = []
    for _ in range(96):
        b = bytearray(c0)
        b[rnd.randrange(lo, hi)] ^= 0x40
        batch.append(bytes(b))
    codes = data.verify_compressed_batch(batch)
    reasons = [host_reason_compressed(gpu, data, c) for c in batch]
    assert codes == [gpu.VERIFY_REASONS[r] for r in reasons]
    assert "hash word out of range" in reasons
    dfull, dst = data.decompress_batch(batch[:16])
    for c, f, s in zip(batch[:16], dfull, dst):
        try:
            assert data.decompress(c) == f and s == gpu.VERIFY_OK
        except gpu.P2Error as e:
            assert s == gpu.VERIFY_REASONS[str(e).split("decompress failed: ", 1)[1]]
