"""What gives tests/proof_ref.py its authority (no GPU): on Poseidon circuits without public inputs the CPU oracle is an outside
witness, so the replay must reproduce every transcript value of the oracle's trace, accept the oracle's proofs, reject every
single-bit tamper of the list the GPU tests use, and agree with the host verifier (p2_verify) case by case."""
import ctypes as C
import random

import numpy as np
import pytest

import circuits
import proof_ref

TRACED = ("betas", "gammas", "deltas", "alphas", "zeta", "fri_alpha", "fri_betas", "pow_witness", "query_indices")
VANISHING = "vanishing polynomial identity does not hold at zeta"
CIRCUITS = ["gf_2_8_add", "mix_columns", "zk_gf_2_8_add", "aes_gcm_13"]
_cache = {}


def _circuit(pkg, name):
    if name == "gf_2_8_add":
        return circuits.gf_2_8_add(pkg, [(0x57, 0x13)])
    if name == "mix_columns":
        return circuits.mix_columns(pkg, circuits.random_states(3, 1))
    if name == "zk_gf_2_8_add":
        return circuits.zk_gf_2_8_add(pkg, [(0x57, 0x13)])
    if name == "aes_gcm_13":
        return circuits.encrypt(pkg, 4, 13, False)[:2]
    raise KeyError(name)


def proven(pkg, orc, name):
    """(info, verifier data, proof, oracle trace {name: words}, blob) of the named circuit's first witness, by the oracle"""
    if name not in _cache:
        data, pws = _circuit(pkg, name)
        oc = orc.OracleCircuit(data.blob)
        if data.info["zero_knowledge"]:
            oc.set_zk_key([11, 22, 33, 44], 0)
        st, proof = oc.prove(pws[0].map, trace=True)
        assert st == 0 and len(proof) == data.proof_bytes
        trace = {k: oc.trace(k) for k in TRACED + ("quotient_coeffs",)}
        _cache[name] = (dict(data.info), oc.verifier_data(), proof, trace, data.blob)
    return _cache[name]


def host_reason(pkg, blob, vd, proof):
    L = pkg.lib()
    rc = L.p2_verify(blob, len(blob), (C.c_uint64 * len(vd))(*vd), len(vd), bytes(proof), len(proof))
    if rc == 0:
        return ""
    assert rc == 4, L.p2_last_error().decode()
    return L.p2_last_error().decode()


@pytest.mark.parametrize("name", CIRCUITS)
def test_replay_reproduces_the_oracle_trace(pkg, orc, name):
    info, vd, proof, trace, blob = proven(pkg, orc, name)
    assert info["hasher"] == "poseidon" and info["num_public_inputs"] == 0
    t = proof_ref.replay_transcript(info, vd, proof, [0, 0, 0, 0])
    for k in TRACED:
        assert t[k] == trace[k], "%s differs from the oracle's trace" % k
    assert t["pow_ok"]
    hasher = proof_ref.poseidon_hasher()
    assert proof_ref.check_merkle(info, vd, proof, t["query_indices"], hasher) is None
    assert proof_ref.check_fri(info, proof, t, t["query_indices"]) is None
    assert proof_ref.replay(info, vd, proof, hasher, blob=blob) is None
    assert host_reason(pkg, blob, vd, proof) == ""
    # the other tree hasher does not fit these trees
    assert "Merkle path" in proof_ref.check_merkle(info, vd, proof, t["query_indices"], proof_ref.keccak_hasher())
    # the quotient openings from the oracle's coefficients
    S = proof_ref.sections(info)
    n = 1 << info["degree_bits"]
    assert proof_ref.eval_openings(trace["quotient_coeffs"], n, t["zeta"]) == proof_ref.ext_words(proof, S, "open_quotient")


def test_shapes_cover_rounds_salt_and_lookups(pkg, orc):
    infos = {name: proven(pkg, orc, name)[0] for name in CIRCUITS}
    assert infos["zk_gf_2_8_add"]["zero_knowledge"] and infos["aes_gcm_13"]["num_fri_rounds"] >= 2
    assert all(proof_ref.shape(i)["lookups"] for i in infos.values())


def test_every_tamper_is_rejected_and_the_host_verifier_agrees(pkg, orc):
    """One bit in every section, and for queries 0, 13 and 27 in every leaf, count byte, sibling block and evaluation block;
    then 30 bytes anywhere.  The replay rejects every one; whenever the replay
    rejects so does p2_verify, and whenever p2_verify rejects for anything but the vanishing identity so does the replay."""
    info, vd, proof, trace, blob = proven(pkg, orc, "aes_gcm_13")
    hasher = proof_ref.poseidon_hasher()
    honest = proof_ref.replay_transcript(info, vd, proof, [0, 0, 0, 0])
    cases = proof_ref.tamper_cases(info, proof)
    names = [c[0] for c in cases]
    rounds = info["num_fri_rounds"]
    want = ["wires_cap", "zs_cap", "quotient_cap", "final_poly", "pow_witness"] + ["fri_cap%d" % r for r in range(rounds)]
    want += ["open_" + k for k in proof_ref.BATCH0 + proof_ref.BATCH1]
    for q in proof_ref.TAMPER_QUERIES:
        want += ["q%d_init%d_%s" % (q, o, part) for o in range(4) for part in ("leaf", "count", "siblings")]
        want += ["q%d_round%d_%s" % (q, r, part) for r in range(rounds) for part in ("evals", "count", "siblings")]
    assert sorted(names) == sorted(want)
    rnd = random.Random(7)
    for _ in range(30):
        at = rnd.randrange(len(proof))
        b = bytearray(proof)
        b[at] ^= 1 << rnd.randrange(8)
        cases.append(("byte %d" % at, bytes(b)))
    cases.append(("honest", proof))
    for label, bad in cases:
        verdict = proof_ref.replay(info, vd, bad, hasher)
        host = host_reason(pkg, blob, vd, bad)
        if label == "honest":
            assert verdict is None and host == ""
            continue
        # a check reports (replay() is PoW, then check_merkle, then check_fri), whether or not a transcript value moved too
        assert verdict is not None, label
        if label in ("wires_cap", "open_wires", "fri_cap0", "final_poly"):
            t = proof_ref.replay_transcript(info, vd, bad, [0, 0, 0, 0])
            assert any(t[k] != honest[k] for k in TRACED), label
        if verdict is not None:
            assert host != "", (label, verdict)
        if host not in ("", VANISHING):
            assert verdict is not None, (label, host)


def test_verdicts_name_their_stage(pkg, orc):
    info, vd, proof, trace, blob = proven(pkg, orc, "aes_gcm_13")
    hasher = proof_ref.poseidon_hasher()
    cases = dict(proof_ref.tamper_cases(info, proof))
    t = proof_ref.replay_transcript(info, vd, proof, [0, 0, 0, 0])
    idx = t["query_indices"]
    assert proof_ref.check_merkle(info, vd, cases["q13_init2_leaf"], idx, hasher).startswith("q13_init2:")
    assert proof_ref.check_merkle(info, vd, cases["q27_round1_siblings"], idx, hasher).startswith("q27_round1:")
    assert proof_ref.check_merkle(info, vd, cases["q0_init3_count"], idx, hasher).startswith("q0_init3_count:")
    assert "_init1: Merkle path" in proof_ref.check_merkle(info, vd, cases["wires_cap"], idx, hasher)
    # a leaf value that still hashes to its path cannot be made by a flip; change the opening it is combined with instead
    assert proof_ref.check_fri(info, cases["open_wires"], t, idx).startswith("q0_round0_evals:")
    assert proof_ref.check_fri(info, cases["q13_round1_evals"], t, idx).startswith("q13")
    assert proof_ref.check_fri(info, cases["final_poly"], t, idx).startswith("q0 final_poly:")
    b = bytearray(proof)
    off = proof_ref.sections(info)["open_sigmas"][0]
    b[off:off + 8] = proof_ref.P.to_bytes(8, "little")
    assert proof_ref.check_merkle(info, vd, bytes(b), idx, hasher) == "open_sigmas: word 0 is not below p"
    assert proof_ref.replay(info, vd, cases["pow_witness"], hasher).startswith("pow_witness:")


def test_eval_openings_is_horner(pkg):
    rnd = random.Random(1)
    n, zeta = 32, (rnd.randrange(proof_ref.P), rnd.randrange(proof_ref.P))
    cols = np.array([[rnd.randrange(proof_ref.P) for _ in range(n)] for _ in range(3)], dtype=np.uint64)
    for col, got in zip(cols, proof_ref.eval_openings(cols, n, zeta)):
        acc = (0, 0)
        for c in reversed(col.tolist()):
            acc = proof_ref.xadd(proof_ref.xmul(acc, zeta), (c, 0))
        assert got == acc
