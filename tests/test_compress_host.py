"""Compressed proofs on the host (no GPU): p2_proof_compress / p2_proof_decompress / p2_verify_compressed (csrc/compress.h)
against the independent compressor of tests/compress_cases.py, written from the layout of DESIGN.md section 8, on proofs made by
the CPU oracle."""
import ctypes as C
import random
import struct

import pytest

import circuits
import pi_circuits
import verify_layout
from compress_cases import _body_info, _flip, _put, coset_collision, kept_levels, py_compress  # noqa: F401 (the independent compressor)

P = 0xFFFFFFFF00000001


# ------------------------------------------------------------------------------------------------ library wrappers
def _call(pkg, fn, data, vd, inp, cap=None):
    L = pkg.lib()
    out = C.create_string_buffer(cap or data.proof_bytes)
    n = C.c_size_t()
    rc = fn(data.blob, len(data.blob), (C.c_uint64 * len(vd))(*vd), len(vd), bytes(inp), len(inp), out, cap or data.proof_bytes, C.byref(n))
    return rc, (out.raw[:n.value] if rc == 0 else L.p2_last_error().decode())


def compress(pkg, data, vd, proof):
    rc, r = _call(pkg, pkg.lib().p2_proof_compress, data, vd, proof)
    assert rc == 0, r
    return r


def decompress(pkg, data, vd, cproof):
    """(full proof, "") or (None, reason)."""
    rc, r = _call(pkg, pkg.lib().p2_proof_decompress, data, vd, cproof)
    if rc == 0:
        return r, ""
    assert rc == 4, r  # P2_ERR_VERIFY
    return None, r


def reason(pkg, fn, data, vd, proof):
    L = pkg.lib()
    rc = fn(data.blob, len(data.blob), (C.c_uint64 * len(vd))(*vd), len(vd), bytes(proof), len(proof))
    if rc == 0:
        return ""
    assert rc == 4, L.p2_last_error().decode()
    return L.p2_last_error().decode()


def verify_reason(pkg, data, vd, proof):
    return reason(pkg, pkg.lib().p2_verify, data, vd, proof)


def verify_compressed_reason(pkg, data, vd, cproof):
    return reason(pkg, pkg.lib().p2_verify_compressed, data, vd, cproof)


# ------------------------------------------------------------------------------------------------ proofs from the oracle
def _circuit(pkg, name):
    if name == "aes_block":
        data, pws = circuits.encrypt_block(pkg, bytes(range(16)), bytes(range(16, 32)))
        data2, pws2 = circuits.encrypt_block(pkg, bytes([7] * 16), bytes([9] * 16))
        assert data2.blob == data.blob
        return data, pws + pws2
    if name == "lookup_free":
        return circuits.arithmetic_only(pkg, [(3, 5, 7, 15 + 49), (2, 9, 4, 1)])
    if name == "poseidon_gate":
        return circuits.feistel_poseidon(pkg, [1, 2], rounds=8)
    if name == "zk":
        return circuits.zk_gf_2_8_add(pkg, [(1, 2), (0x57, 0x13)])
    if name == "public_inputs":
        data, pws, vals, _ = pi_circuits.small(pkg, 9)
        return data, pws, vals
    raise KeyError(name)


CIRCUITS = ["aes_block", "lookup_free", "poseidon_gate", "zk", "public_inputs"]
_cache = {}


def proven(pkg, orc, name):
    """(data, verifier data, [(full proof, drawn query indices)]) for two witnesses of the named circuit.

    The oracle proves circuits with public inputs as if they had none (it ignores the blob's public-input section): their
    proofs here get the trailer appended, which changes the transcript, so they are well-formed but not honest -- verify()
    rejects them at the vanishing identity -- and their drawn indices are not the oracle's.  (None: the compressor's.)"""
    if name not in _cache:
        data, pws, *vals = _circuit(pkg, name)
        oc = orc.OracleCircuit(data.blob)
        if data.info["zero_knowledge"]:
            oc.set_zk_key([11, 22, 33, 44], 0)
        out = []
        for i, pw in enumerate(pws[:2]):
            st, proof = oc.prove(pw.map, trace=True)
            assert st == 0
            if vals:
                k = data.num_public_inputs
                out.append((proof + struct.pack("<%dQ" % (k + 1), k, *vals[0][i]), None))
            else:
                out.append((proof, oc.trace("query_indices")))
        _cache[name] = (data, oc.verifier_data(), out)
    return _cache[name]


def indices(pkg, data, vd, proof, idx):
    if idx is not None:
        return idx
    c = compress(pkg, data, vd, proof)
    off = verify_layout.sections(_body_info(data.info))["q0_init0_leaf"][0]
    return list(struct.unpack_from("<28I", c, off))


def honest(data):
    return data.num_public_inputs == 0


@pytest.fixture(params=CIRCUITS)
def case(request, pkg, orc):
    return proven(pkg, orc, request.param)


# ------------------------------------------------------------------------------------------------ tests
def test_exports_and_reasons(pkg):
    L = pkg.lib()
    for f in ("p2_proof_compress", "p2_proof_decompress", "p2_verify_compressed", "p2_compress_batch", "p2_decompress_batch",
              "p2_verify_compressed_batch", "p2_compress_batch_device", "p2_decompress_batch_device", "p2_verify_compressed_batch_device"):
        assert f in L._p2_signatures and hasattr(L, f), f
    for r in ("query index out of range", "wrong sibling count in compressed proof", "query indices differ from the transcript"):
        assert pkg.VERIFY_REASONS[r] == pkg.VERIFY_SHAPE


def test_compressor_matches_independent_python(pkg, case):
    data, vd, proofs = case
    for proof, idx in proofs:
        assert (verify_reason(pkg, data, vd, proof) == "") == honest(data)
        want, _ = py_compress(data.info, proof, indices(pkg, data, vd, proof, idx))
        got = compress(pkg, data, vd, proof)
        assert got == want
        assert len(got) < len(proof)


def test_round_trips(pkg, case):
    data, vd, proofs = case
    for proof, _ in proofs:
        c = compress(pkg, data, vd, proof)
        full, err = decompress(pkg, data, vd, c)
        assert err == ""
        # (a proof whose fold checks fail at the dropped evaluations comes back repaired: only honest ones come back as they were)
        assert full == proof or not honest(data)
        assert compress(pkg, data, vd, full) == c


def test_verify_compressed_accepts_honest_proofs(pkg, case):
    data, vd, proofs = case
    for proof, _ in proofs:
        c = compress(pkg, data, vd, proof)
        assert verify_compressed_reason(pkg, data, vd, c) == verify_reason(pkg, data, vd, proof)
        assert verify_compressed_reason(pkg, data, vd, c) == "" or not honest(data)


def test_the_coset_collision_case_is_exercised(pkg, orc):
    """Some proof here has two queries in one coset of its last FRI round at different positions: the later one reads the
    evaluation that the first one leaves out, inferred."""
    hits = []
    for name in CIRCUITS:
        data, vd, proofs = proven(pkg, orc, name)
        for proof, idx in proofs:
            if not honest(data):
                continue
            pair = coset_collision(data.info, idx)
            if pair:
                hits.append(name)
                c = compress(pkg, data, vd, proof)
                assert decompress(pkg, data, vd, c)[0] == proof
                assert verify_compressed_reason(pkg, data, vd, c) == ""
    assert hits


def test_rejections(pkg, orc, case):
    data, vd, proofs = case
    proof, idx = proofs[0]
    idx = indices(pkg, data, vd, proof, idx)
    c, at = py_compress(data.info, proof, idx)
    N = 1 << (data.info["degree_bits"] + 3)

    def rej(bad, want=None):
        r = verify_compressed_reason(pkg, data, vd, bad)
        assert r != "" and r in pkg.VERIFY_REASONS, r
        if want is not None and honest(data):  # (the dishonest proofs fail the PoW check first)
            assert pkg.VERIFY_REASONS[r] == want, r
        full, err = decompress(pkg, data, vd, bad)
        if full is not None:  # decompression succeeded: the verdict is the full proof's
            assert r == verify_reason(pkg, data, vd, full)
        return r

    assert rej(c[:-1]) == "proof truncated"
    assert rej(c[:at["indices"] + 3]) == "proof truncated"
    assert rej(c + b"\0") == "trailing bytes in proof"
    # a sibling-count byte off by one, in the initial trees and in a FRI round
    for key in [k for k in at if k.startswith("init_count_")][:2] + [k for k in at if k.startswith("round_count_")][:2]:
        for d in (1, 255):
            assert rej(_put(c, at[key], bytes([(c[at[key]] + d) & 255]))) == "wrong sibling count in compressed proof"
    # written indices: swapped, wrong, out of range
    ii = at["indices"]
    a, b = next((a, b) for a in range(len(idx)) for b in range(len(idx)) if idx[a] != idx[b])
    sw = list(idx)
    sw[a], sw[b] = sw[b], sw[a]
    rej(_put(c, ii, struct.pack("<%dI" % len(idx), *sw)), pkg.VERIFY_SHAPE)
    wrong = list(idx)
    wrong[3] ^= 1
    rej(_put(c, ii, struct.pack("<%dI" % len(idx), *wrong)), pkg.VERIFY_SHAPE)
    wrong[3] = N
    assert rej(_put(c, ii, struct.pack("<%dI" % len(idx), *wrong))) == "query index out of range"
    # a non-canonical word in each section
    words = {"prefix": 8, "leaf": at["init_leaf_%d_1" % idx.index(min(idx))], "final_poly": at["final_poly"], "pow_witness": at["pow_witness"]}
    evk = next((k for k in at if k.startswith("evals_")), None)
    if evk:
        words["evals"] = at[evk] + 8
    sibk = next((k for k in at if k.startswith("init_sib_")), None)
    if sibk:
        words["init_sibling"] = at[sibk] + 16
    sibr = next((k for k in at if k.startswith("round_sib_")), None)
    if sibr:
        words["round_sibling"] = at[sibr]
    if "pi_values" in at:
        words["pi_value"] = at["pi_values"] + 8
    for name, off in words.items():
        assert rej(_put(c, off, struct.pack("<Q", P + 5))) == "non-canonical field element", name
    # flipped (still canonical) sibling, leaf and evaluation: rejected after decompression, by the full proof's checks
    for name in ("leaf", "evals", "init_sibling", "round_sibling"):
        if name in words:
            off = words[name]
            rej(_put(c, off, _flip(c[off:off + 8])))
    # the proof-of-work witness: POW, ahead of the (then different) drawn indices
    off = at["pow_witness"]
    r = verify_compressed_reason(pkg, data, vd, _put(c, off, _flip(c[off:off + 8])))
    assert r in ("Invalid proof-of-work witness.", "query indices differ from the transcript")


def test_pow_is_reported_before_the_indices(pkg, orc):
    """A PoW witness that fails the PoW check reads as POW, although it also changes the drawn indices."""
    data, vd, proofs = proven(pkg, orc, "lookup_free")
    proof, idx = proofs[0]
    c, at = py_compress(data.info, proof, idx)
    off = at["pow_witness"]
    for v in range(1, 200):
        bad = _put(c, off, struct.pack("<Q", v))
        r = verify_compressed_reason(pkg, data, vd, bad)
        if r == "Invalid proof-of-work witness.":
            assert decompress(pkg, data, vd, bad)[1] == "query indices differ from the transcript"
            return
        assert r == "query indices differ from the transcript"
    pytest.fail("no PoW witness below 200 fails the PoW check")


def test_the_dropped_evaluation_is_repaired_by_inference(pkg, orc):
    """Tampering, in the FULL proof, the evaluation that compression leaves out breaks the full proof's fold check; its
    compressed form does not carry it, and decompression infers the honest value: verify_compressed(c) == verify(decompress(c))."""
    data, vd, proofs = proven(pkg, orc, "aes_block")
    proof, idx = proofs[0]
    S = verify_layout.sections(_body_info(data.info))
    off = S["q0_round0_evals"][0] + 16 * (idx[0] & 15)
    bad = _put(proof, off, _flip(proof[off:off + 8]))
    assert verify_reason(pkg, data, vd, bad) == "FRI fold consistency check failed."
    c = compress(pkg, data, vd, bad)
    assert c == compress(pkg, data, vd, proof)
    full, _ = decompress(pkg, data, vd, c)
    assert full == proof
    assert verify_compressed_reason(pkg, data, vd, c) == verify_reason(pkg, data, vd, full) == ""


def test_compress_rejects_malformed_full_proofs(pkg, orc):
    data, vd, proofs = proven(pkg, orc, "lookup_free")
    proof, _ = proofs[0]
    L = pkg.lib()
    for bad, want in ((proof[:-1], "proof truncated"), (proof + b"\0", "trailing bytes in proof"),
                      (_put(proof, 0, struct.pack("<Q", P)), "non-canonical field element")):
        rc, r = _call(pkg, L.p2_proof_compress, data, vd, bad)
        assert rc == 4 and r == want
    rc, r = _call(pkg, L.p2_proof_compress, data, vd, proof, cap=16)
    assert rc == 1 and "fewer than" in r
    vd_bad = list(vd)
    vd_bad[-1] ^= 1  # another circuit digest: other indices, still a valid compression
    c = compress(pkg, data, vd_bad, proof)
    assert verify_compressed_reason(pkg, data, vd, c) == "query indices differ from the transcript"


def test_mutation_fuzz_never_crashes(pkg, orc):
    rnd = random.Random(7)
    for name in ("lookup_free", "public_inputs"):
        data, vd, proofs = proven(pkg, orc, name)
        proof, idx = proofs[0]
        c = compress(pkg, data, vd, proof)
        for _ in range(150):
            b = bytearray(c)
            kind = rnd.randrange(4)
            if kind == 0:
                for _ in range(rnd.randrange(1, 4)):
                    b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
            elif kind == 1:
                del b[rnd.randrange(len(b)):]
            elif kind == 2:
                b += bytes(rnd.randrange(1, 40))
            else:
                p = rnd.randrange(len(c) - 8)
                b[p:p + 8] = struct.pack("<Q", rnd.choice([0, P - 1, P, 2 ** 64 - 1, rnd.randrange(2 ** 64)]))
            r = verify_compressed_reason(pkg, data, vd, bytes(b))
            assert r in pkg.VERIFY_REASONS, r
            full, err = decompress(pkg, data, vd, bytes(b))
            if full is not None:
                assert r == verify_reason(pkg, data, vd, full)
                assert compress(pkg, data, vd, full) == bytes(b)  # canonical encoding
            else:
                assert err in pkg.VERIFY_REASONS, err
