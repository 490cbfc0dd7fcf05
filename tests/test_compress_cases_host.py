"""The directed compressed-proof cases of tests/compress_cases.py against the host decoder (csrc/compress.h), no GPU.

This file is the reference for the cases' own expectations: every malformed case gets a reason from the set its construction
allows, p2_proof_decompress agrees with p2_verify_compressed the way section 8a relates them, and the index sweeps reach
every branch of the layout code that index_predicates names -- a condition on the inputs, checked from the indices alone.
tests/test_gpu_compress_directed.py runs the same cases on the GPU against the host decoder, which this file holds to the
independent Python compressor.  Proofs come from the CPU oracle."""
import struct

import pytest

import circuits
import compress_cases as CC
import edge_circuits as E
import pi_circuits
import test_compress_host as H
import verify_layout
from test_gpu_degree_ladder import CHAIN_OPS, ROUNDS

# name -> (sweep length, the predicates the sweep and the honest proofs together must show).
# The lengths were found once on the CPU, starting at 64 and to be raised in steps of 64 to at most 512 while a named predicate was
# missing (`python tests/test_compress_cases_host.py` prints, per circuit, the first sweep proof of 512 that shows each).  None
# had to be raised: the last to show are a tree-0 block without siblings at 7 bits (sweep proof 4) and a duplicate index among
# the 2^14 leaves at 11 bits (sweep proof 9, where two in a hundred sets have one: these witnesses were lucky, and a change of
# CHAIN_SEED may need a longer sweep).  The zk circuit (14 bits, three rounds) shows everything but a duplicate within 42.
BASE = ("a", "b", "c", "d")
CIRCUITS = {
    "chain_2": (64, BASE),
    "chain_7": (64, BASE + ("e0", "f0", "g0")),
    "chain_11": (64, BASE + ("e0", "f0", "g0", "e1", "f1", "g1", "h1")),
    "public_inputs": (64, ()),
    "zk": (64, ()),
}
CHAIN_SEED = 900        # witness w of the chain at `bits` rows is seeded CHAIN_SEED + 16 * bits + w, on the CPU and on the GPU


def build(pkg, name, witnesses, hasher="poseidon"):
    """(data, pws) of a circuit of CIRCUITS with `witnesses` witnesses, its shape asserted"""
    if name.startswith("chain_"):
        bits = int(name.split("_")[1])
        data, pws = E.chain(pkg, CHAIN_OPS[bits], [CHAIN_SEED + 16 * bits + w for w in range(witnesses)], hasher=hasher)
        assert data.info["degree_bits"] == bits, data.info
        assert data.info["num_fri_rounds"] == ROUNDS[bits], data.info
        S = verify_layout.sections(data.info)
        assert S["q0_init0_siblings"][1] == 32 * (bits + 3 - 4)
        assert S["final_poly"][1] == 16 * ((1 << bits) >> (4 * ROUNDS[bits]))
        return data, pws
    if name == "public_inputs":
        ws = [(3 + w, 5, 7 * w + 1, 11) for w in range(witnesses)]
        data, pws, vals, _ = pi_circuits.small(pkg, 9, witnesses=ws)
        data.pi_values = vals
        return data, pws
    if name == "zk":
        return circuits.zk_gf_2_8_add(pkg, [(w, 255 - 3 * w) for w in range(witnesses)])
    raise KeyError(name)


_cache = {}


def proven(pkg, orc, name):
    """(data, verifier data, [(full proof, drawn indices or None)]) for two witnesses, as test_compress_host.proven makes them:
    the public-input proofs get their trailer appended and are well-formed but fail the proof-of-work."""
    if name not in _cache:
        data, pws = build(pkg, name, 2)
        oc = orc.OracleCircuit(data.blob)
        if data.info["zero_knowledge"]:
            oc.set_zk_key([11, 22, 33, 44], 0)
        out = []
        for i, pw in enumerate(pws):
            st, proof = oc.prove(pw.map, trace=True)
            assert st == 0
            if data.num_public_inputs:
                k = data.num_public_inputs
                out.append((proof + struct.pack("<%dQ" % (k + 1), k, *data.pi_values[i]), None))
            else:
                out.append((proof, oc.trace("query_indices")))
        _cache[name] = (data, oc.verifier_data(), out)
    return _cache[name]


@pytest.fixture(params=list(CIRCUITS))
def case(request, pkg, orc):
    return (request.param,) + proven(pkg, orc, request.param)


# ------------------------------------------------------------------------------------------------ library wrappers on (buffer, length)
def vc_reason(pkg, data, vd, b):
    buf, n = CC.case_bytes(b)
    L = pkg.lib()
    rc = L.p2_verify_compressed(data.blob, len(data.blob), (H.C.c_uint64 * len(vd))(*vd), len(vd), buf, n)
    if rc == 0:
        return ""
    assert rc == 4, L.p2_last_error().decode()
    return L.p2_last_error().decode()


def decompress(pkg, data, vd, b):
    """(full proof, "") or (None, reason)"""
    buf, n = CC.case_bytes(b)
    L = pkg.lib()
    out = H.C.create_string_buffer(data.proof_bytes)
    got = H.C.c_size_t()
    rc = L.p2_proof_decompress(data.blob, len(data.blob), (H.C.c_uint64 * len(vd))(*vd), len(vd), buf, n, out, data.proof_bytes, H.C.byref(got))
    if rc == 0:
        return out.raw[:got.value], ""
    assert rc == 4, L.p2_last_error().decode()
    return None, L.p2_last_error().decode()


def host_verdicts(pkg, data, vd, b):
    """(verify_compressed's reason, decompress's reason) for one case, held to each other as section 8a relates them
    (test_compress_host.test_rejections' `rej`): what decompresses gets the full proof's verdict; what does not gets the same
    reason from both, but for a failing proof-of-work, which decompression does not check."""
    r = vc_reason(pkg, data, vd, b)
    assert r == "" or r in pkg.VERIFY_REASONS, r
    full, err = decompress(pkg, data, vd, b)
    if full is not None:
        assert r == H.verify_reason(pkg, data, vd, full)
    else:
        assert err == r or (r == CC.POW and err == CC.INDICES), (r, err)
    return r, err


def base_reason(pkg, data, vd, proof):
    return vc_reason(pkg, data, vd, H.compress(pkg, data, vd, proof))


def cases_of(pkg, data, vd, proof, idx):
    return CC.malformed(data.info, proof, idx, base=base_reason(pkg, data, vd, proof) or None,
                        pow_fails=lambda b: vc_reason(pkg, data, vd, b) == CC.POW)


# ------------------------------------------------------------------------------------------------ malformed cases
def test_malformed_cases_get_the_reason_their_construction_allows(pkg, case):
    name, data, vd, proofs = case
    proof, idx = proofs[0]
    idx = H.indices(pkg, data, vd, proof, idx)
    base = base_reason(pkg, data, vd, proof)
    assert (base == "") == (data.num_public_inputs == 0)
    cases = cases_of(pkg, data, vd, proof, idx)
    bad, seen = [], set()
    for label, b, want in cases:
        r, _ = host_verdicts(pkg, data, vd, b)
        seen.add(r)
        if r not in want:
            bad.append((label, r, sorted(want)))
    assert not bad, bad[:10]
    must = {CC.TRUNCATED, CC.TRAILING, CC.INDEX_RANGE, CC.COUNT, CC.NON_CANONICAL, CC.POW}
    if base == "":
        must |= {CC.INDICES, CC.MERKLE_INITIAL} | ({CC.MERKLE_FRI} if data.info["num_fri_rounds"] else set())
    if data.num_public_inputs:
        must.add(CC.PI_COUNT)
    assert must <= seen, must - seen


def test_layout_reason_is_the_host_reason(pkg, case):
    """compress_cases.layout_reason, which decides what the index-table cases expect, against the host on shape-valid and
    shape-invalid bytes of its own kind."""
    name, data, vd, proofs = case
    proof, idx = proofs[0]
    idx = H.indices(pkg, data, vd, proof, idx)
    c, at = CC.py_compress(data.info, proof, idx)
    assert CC.layout_reason(data.info, c, idx) is None
    for b in (c[:-1], c + b"\0", CC._put(c, 0, struct.pack("<Q", CC.P)), CC._put(c, CC.Layout(data.info, c, at).count_offsets()[0], b"\xfe")):
        assert CC.layout_reason(data.info, b, idx) == vc_reason(pkg, data, vd, b)


# ------------------------------------------------------------------------------------------------ index sweeps
def predicates_of(pkg, data, vd, proofs):
    """[(indices the host compressor wrote, predicates)] per proof"""
    out = []
    for p in proofs:
        idx = CC.written_indices(data.info, H.compress(pkg, data, vd, p))
        out.append((idx, CC.index_predicates(idx, data.info)))
    return out


def chosen_sweep(name, info, proof, indices_of):
    """The sweep proofs the GPU tests run: the first eight of the sweep of CIRCUITS[name]'s length plus the first that shows
    each predicate (all of them, not only the required ones).  indices_of(full proof) -> the drawn indices."""
    sweep = CC.index_sweep(proof, info, CIRCUITS[name][0])
    keep, shown = set(range(8)), set()
    for i, p in enumerate(sweep):
        for key, hit in CC.index_predicates(indices_of(p), info).items():
            if hit and key not in shown:
                shown.add(key)
                keep.add(i)
    return [sweep[i] for i in sorted(keep)], shown


def test_index_sweeps(pkg, case):
    name, data, vd, proofs = case
    n, required = CIRCUITS[name]
    sweep = CC.index_sweep(proofs[0][0], data.info, n)
    assert len(sweep) == n and len(set(sweep)) == n
    shown = set()
    for p in [pr for pr, _ in proofs] + sweep:
        c = H.compress(pkg, data, vd, p)
        idx = CC.written_indices(data.info, c)
        assert c == CC.py_compress(data.info, p, idx)[0]
        full, err = decompress(pkg, data, vd, c)
        assert err == ""
        assert H.compress(pkg, data, vd, full) == c
        shown |= {key for key, hit in CC.index_predicates(idx, data.info).items() if hit}
    for (p, drawn), (idx, _) in zip(proofs, predicates_of(pkg, data, vd, [pr for pr, _ in proofs])):
        assert drawn is None or list(drawn) == idx
    assert set(required) <= shown, sorted(set(required) - shown)
    subset, sub_shown = chosen_sweep(name, data.info, proofs[0][0], lambda p: CC.written_indices(data.info, H.compress(pkg, data, vd, p)))
    assert 8 <= len(subset) <= 8 + len(sub_shown) and shown - sub_shown <= set()


def test_the_predicates_on_hand_made_sets():
    """index_predicates itself, on index sets small enough to read: 2^14 leaves, two rounds (tree depths 10, 6, 2)."""
    info = {"degree_bits": 11, "num_fri_rounds": 2}
    far = [0x2000 + 0x155 * k for k in range(28)]     # 28 queries far apart from one another
    none = CC.index_predicates(far, info)
    assert not (none["a"] or none["b"] or none["e0"] or none["e1"] or none["h1"])

    def with_(*head):
        return CC.index_predicates(list(head) + far[len(head):], info)
    assert with_(5, 5)["a"] and not with_(5, 5)["b"]
    assert with_(5, 9, 5)["b"]
    assert with_(0x30, 0x31)["e0"] and not with_(0x30, 0x31)["e1"]
    assert with_(0x300, 0x310)["e1"] and not with_(0x300, 0x310)["e0"] and with_(0x300, 0x310)["h1"]
    assert not with_(0x300, 0x311)["h1"] and with_(0x300, 0x311)["e1"]
    full = CC.index_predicates(list(range(16)) + far[16:], info)
    assert full["c"]                                   # leaves 0..15: every sibling up to level 3 is on a path; above, query 0 keeps them
    assert CC.index_predicates([0] * 28, info)["d"] and CC.index_predicates([0] * 28, info)["g0"] and CC.index_predicates([0] * 28, info)["g1"]
    every = CC.index_predicates([(k & 3) << 4 for k in range(28)], {"degree_bits": 7, "num_fri_rounds": 1})
    assert every["f0"]                                 # round-0 leaves 0, 1, 2, 3 under a two-level tree: nothing to keep


if __name__ == "__main__":   # how the sweep lengths above were found
    import conftest  # noqa: F401
    import __graft_entry__ as g
    import oracle_lib
    pkg_ = g.load_package()
    for name_ in CIRCUITS:
        data_, vd_, proofs_ = proven(pkg_, oracle_lib, name_)
        firsts = {}
        for i, (idx_, pred) in enumerate(predicates_of(pkg_, data_, vd_, CC.index_sweep(proofs_[0][0], data_.info, 512))):
            for key_, hit_ in pred.items():
                if hit_:
                    firsts.setdefault(key_, i)
        print(name_, data_.info["degree_bits"], sorted(firsts.items()))
