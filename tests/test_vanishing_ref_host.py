"""The vanishing identity at zeta, restated in Python (tests/vanishing_ref.py), against the host verifier's evaluation of it
(p2_vanishing_terms -> verifier.h eval_vanishing) on opening sets that the restatement alone makes valid: term for term, both
sides, and the verdict on every single-coordinate perturbation.  The restatement's own authority comes from an independent
prover: it accepts the CPU oracle's proofs.  No GPU.  Every comparison is between field elements or verdicts, hence exact."""
import pytest

import proof_ref
import vanishing_cases as VC
import vanishing_ref as V

P = proof_ref.P
_sweeps = {}


def swept(pkg, name):
    """(base case, [(case, Python's verdict)]) of the named circuit, once per process"""
    if name not in _sweeps:
        info, blob, circ, data = VC.build(pkg, name)
        base = VC.solved(name, circ, "random", 100)
        _sweeps[name] = (base, [(c, VC.python_verdict(circ, c)) for c in VC.sweep(circ, base)])
    return _sweeps[name]


def test_the_circuits_reach_what_the_table_says(pkg):
    circs = {name: VC.build(pkg, name)[2] for name in VC.NAMES}
    assert circs["arithmetic"].nsel == 1 and not circs["arithmetic"].lookups          # no unused-selector factor, no table
    assert circs["mix_columns"].nsel == 2 and circs["hashed_elgamal"].nsel == 2                  # with the unused-selector factor
    assert len(circs["aes_gcm"].luts) == 3 and len(circs["mix_columns"].luts) >= 1
    assert any(len(t[0]) == 65536 for t in circs["ghash_mul"].luts)
    assert [len(t[0]) for t in circs["small_table"].luts] == [VC.SMALLEST_TABLE]
    assert [len(t[0]) for t in circs["sbox_table"].luts] == [256] and 256 % V.LUT_SLOTS                # a padded last row
    assert V.G_POSEIDON in circs["poseidon_encrypt"].gates and circs["poseidon_encrypt"].nsel == 2
    assert V.G_PUBLIC_INPUT in circs["public_inputs"].gates and VC.build(pkg, "public_inputs")[0]["num_public_inputs"] == 3
    assert V.G_ECSTEP in circs["ec_steps"].gates
    assert {V.G_ECSTEP, V.G_POSEIDON, V.G_ARITHMETIC} <= set(circs["hashed_elgamal"].gates)
    for name in VC.LOOKUP_NAMES:
        assert circs[name].lookups


@pytest.mark.parametrize("fill", ["random", P - 1, 0])
@pytest.mark.parametrize("name", VC.NAMES)
def test_solved_sets_hold_term_for_term(pkg, name, fill):
    info, blob, circ, data = VC.build(pkg, name)
    case = VC.solved(name, circ, fill, 7)
    terms = V.terms(circ, case.o, case.ch, case.pi_hash)
    sides = V.sides(circ, case.o, case.ch, terms, case.pi_hash)
    assert all(l == r for l, r in sides) and VC.python_verdict(circ, case) == V.HOLDS
    verdict, h_terms, h_sides = VC.host(pkg, info, blob, case)
    assert len(h_terms) == len(terms)
    for k, (a, b) in enumerate(zip(h_terms, terms)):
        assert a == b, "term %d of %d" % (k, len(terms))
    assert h_sides == sides and verdict == V.HOLDS


@pytest.mark.parametrize("name", VC.NAMES)
def test_every_opening_sweep(pkg, name):
    """The first coordinate of every element of every open_* section and the second of every seventh: + 1 mod p on a solved
    random set.  Python says whether the identity still holds; the host says the same, case for case."""
    info, blob, circ, data = VC.build(pkg, name)
    base, cases = swept(pkg, name)
    assert len(cases) >= sum(circ.counts.values())
    for case, want in cases:
        assert VC.host(pkg, info, blob, case)[0] == want, case.label
    verdicts = {c.label: v for c, v in cases}
    if V.G_POSEIDON not in circ.gates:
        assert all(verdicts["wires[%d].0 + 1" % w] == V.HOLDS for w in range(80, 135))       # no term reads the advice wires
    assert all(verdicts["quotient[%d].0 + 1" % k] == V.FAILS for k in range(circ.counts["quotient"]))


def test_what_the_circuits_read(pkg):
    """Of the circuits, not of the verifier, from Python alone: hashed ElGamal reads every wire, sigma, Z, partial product and
    quotient element; the EcStep circuits move each of the 40 constraint slots under some perturbation of wires 0..70; the
    lookup circuits read every lookup opening at zeta and, at g zeta, the two per challenge that the protocol reads."""
    verdicts = {c.label: v for c, v in swept(pkg, "hashed_elgamal")[1]}
    circ = VC.build(pkg, "hashed_elgamal")[2]
    for section in ("wires", "sigmas", "zs", "zs_next", "partial_products", "quotient"):
        for e in range(circ.counts[section]):
            assert verdicts["%s[%d].0 + 1" % (section, e)] == V.FAILS, (section, e)
    for name in VC.EC_NAMES:
        circ = VC.build(pkg, name)[2]
        base, cases = swept(pkg, name)
        first = len(V.terms(circ, base.o, base.ch, base.pi_hash)) - circ.ngc
        honest = V.terms(circ, base.o, base.ch, base.pi_hash)[first:first + 40]
        moved = set()
        for case, _ in cases:
            if case.label.startswith("wires[") and case.label.endswith(".0 + 1") and int(case.label[6:case.label.index("]")]) <= 70:
                slots = V.terms(circ, case.o, case.ch, case.pi_hash)[first:first + 40]
                moved |= {k for k in range(40) if slots[k] != honest[k]}
        assert moved == set(range(40)), name
    for name in VC.LOOKUP_NAMES:
        verdicts = {c.label: v for c, v in swept(pkg, name)[1]}
        # at zeta all seven per challenge; at g zeta the identity reads RE (the row transition) and the last partial polynomial
        # (which the first one of this row continues) and no other: the five in between are opened for nothing, upstream too
        for e in range(2 * V.NLP):
            assert verdicts["lookup_zs[%d].0 + 1" % e] == V.FAILS, (name, e)
            read = e % V.NLP in (0, V.NLP - 1)
            assert verdicts["lookup_zs_next[%d].0 + 1" % e] == (V.FAILS if read else V.HOLDS), (name, e)


@pytest.mark.parametrize("name", ["mix_columns", "hashed_elgamal"])
def test_each_challenge_alone(pkg, name):
    info, blob, circ, data = VC.build(pkg, name)
    base = VC.solved(name, circ, "random", 21)
    other = base.copy("alphas[1] + 1")
    other.ch["alphas"][1] = (other.ch["alphas"][1] + 1) % P
    sides = V.sides(circ, other.o, other.ch, None, other.pi_hash)
    assert sides[0][0] == sides[0][1] and sides[1][0] != sides[1][1]
    verdict, _, h_sides = VC.host(pkg, info, blob, other)
    assert h_sides == sides and verdict == V.FAILS == VC.python_verdict(circ, other)


def test_a_zero_factor_in_a_looking_product(pkg):
    """delta's alpha equal to a looking combination (both wires in the base field): one factor of the product is zero, the
    sum of the products that leave one factor out keeps one summand"""
    info, blob, circ, data = VC.build(pkg, "mix_columns")
    for i, slot in ((0, 0), (1, 39), (0, 20)):
        case = VC.solved("mix_columns", circ, "random", 30 + slot)
        case.o["wires"][2 * slot] = (case.o["wires"][2 * slot][0], 0)
        case.o["wires"][2 * slot + 1] = (case.o["wires"][2 * slot + 1][0], 0)
        a = case.ch["deltas"][4 * i]
        case.ch["deltas"][4 * i + 2] = (case.o["wires"][2 * slot][0] + a * case.o["wires"][2 * slot + 1][0]) % P
        V.solve_quotient(circ, case.o, case.ch, case.pi_hash)
        terms = V.terms(circ, case.o, case.ch, case.pi_hash)
        verdict, h_terms, h_sides = VC.host(pkg, info, blob, case)
        assert h_terms == terms and verdict == V.HOLDS and h_sides == V.sides(circ, case.o, case.ch, terms, case.pi_hash)


@pytest.mark.parametrize("name", ["arithmetic", "mix_columns", "hashed_elgamal"])
def test_zeta_in_the_subgroup(pkg, name):
    info, blob, circ, data = VC.build(pkg, name)
    w = proof_ref.root_of_unity(circ.degree_bits)
    for zeta in ([1, 0], [w, 0], [pow(w, circ.n - 1, P), 0]):
        case = VC.solved(name, circ, "random", 5).copy("zeta in the subgroup")
        case.ch["zeta"] = zeta
        assert VC.python_verdict(circ, case) == V.IN_SUBGROUP == VC.host(pkg, info, blob, case)[0]
    case.ch["zeta"] = [w, 1]
    assert VC.python_verdict(circ, case) == V.FAILS == VC.host(pkg, info, blob, case)[0]


def test_the_hook_refuses_what_is_not_a_field_element(pkg):
    info, blob, circ, data = VC.build(pkg, "arithmetic")
    case = VC.solved("arithmetic", circ, "random", 5)
    case.ch["alphas"][0] = P
    with pytest.raises(AssertionError, match="non-canonical"):
        VC.host(pkg, info, blob, case)


# ---------------------------------------------------------------------------------------------- an independent prover
ORACLE_NAMES = ("arithmetic", "small_table", "sbox_table", "poseidon_encrypt")


def _witness(pkg, name):
    import circuits
    if name == "arithmetic":
        return circuits.arithmetic_only(pkg, [(3, 4, 5, 47)])
    if name == "sbox_table":
        return circuits.assert_byte(pkg, [7])
    if name == "poseidon_encrypt":
        return circuits.poseidon_encrypt(pkg, 3, [1])[:2]
    b = pkg.CircuitBuilder()
    lut = b.add_lookup_table_from_pairs([(3, 5)])
    x = b.add_virtual_target()
    b.add_lookup_from_index(x, lut)
    pw = pkg.PartialWitness()
    pw.set_target(x, 3)
    return b.build(), [pw]


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_the_oracles_proofs_satisfy_the_identity(pkg, orc, name):
    data, pws = _witness(pkg, name)
    oc = orc.OracleCircuit(data.blob)
    st, proof = oc.prove(pws[0].map)
    assert st == 0
    info = dict(data.info)
    t = proof_ref.replay_transcript(info, oc.verifier_data(), proof, [0, 0, 0, 0])
    assert V.check_vanishing(info, data.blob, proof, t) is None
    assert proof_ref.replay(info, oc.verifier_data(), proof, proof_ref.poseidon_hasher(), blob=data.blob) is None
    # and not by accepting everything: one opening moved (the transcript kept, as the caller of check_vanishing supplies it)
    S = proof_ref.sections(info)
    for section in ("open_wires", "open_sigmas", "open_zs_next", "open_quotient"):
        b = bytearray(proof)
        b[S[section][0]] ^= 1
        assert "challenge" in V.check_vanishing(info, data.blob, bytes(b), t)


@pytest.mark.parametrize("name", ["gf_2_8_add", "mix_columns", "zk_gf_2_8_add", "aes_gcm_13"])
def test_the_replay_with_a_blob_accepts_the_proof_ref_configurations(pkg, orc, name):
    import test_proof_ref_host
    info, vd, proof, trace, blob = test_proof_ref_host.proven(pkg, orc, name)
    assert proof_ref.replay(info, vd, proof, proof_ref.poseidon_hasher(), blob=blob) is None
    b = bytearray(proof)
    b[proof_ref.sections(info)["open_lookup_zs_next"][0]] ^= 1         # RE at g zeta
    t = proof_ref.replay_transcript(info, vd, proof, [0, 0, 0, 0])
    assert "challenge" in V.check_vanishing(info, blob, bytes(b), t)
