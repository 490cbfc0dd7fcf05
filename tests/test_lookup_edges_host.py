"""The lookup-edge cases of tests/edge_circuits.py on the CPU alone (no GPU): every case that tests/test_gpu_lookup_edges.py
proves on the device is first shown to be a sound reference -- the host witness twin resolves every lookup to the first
matching pair, the CPU oracle proves the three witnesses, and the host verifier and the Python replay (transcript, Merkle
paths, FRI and the vanishing identity with its lookup terms) accept each proof under the oracle's verifier data.  The
refusals: an empty table (at add_lookup_table_from_pairs), a seventh table and an unused table (at build()), and lookup inputs
that are not in the table."""
import os
import sys

import pytest

import edge_circuits as E
import proof_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_builder  # noqa: E402


@pytest.mark.parametrize("name", list(E.LOOKUP_CASES))
def test_case_is_a_sound_reference(pkg, orc, name):
    data, pws, sh, case = E.lookup_case(pkg, name)
    if name in ("scan_1024", "scan_1025"):      # k_lookup_scan's `total`: LookupGate and LookupTableGate rows of the one table
        lu, lut, _, _ = case["rows"][0]
        assert lu + lut == int(name[5:])
    if name == "table_scan":
        assert case["rows"][0][1] == 1025
    oc = orc.OracleCircuit(data.blob)
    vd = oc.verifier_data()
    proofs = []
    for w, pw in enumerate(pws):
        vals, st, fault = pkg.host_witness(data.blob, pw, sh.out_targets())
        assert st == 0 and fault.kind == "NONE"
        assert vals == sh.want_values(w)
        ost, proof = oc.prove(pw.map)
        assert ost == 0 and len(proof) == data.proof_bytes
        E.reference_holds(pkg, data, vd, proof)
        proofs.append(proof)
    assert len(set(proofs)) == 3
    # the flip the GPU tests compare the two verifiers on is one the host verifier and the replay reject
    bad = E.flipped_column_byte(data.info, proofs[-1])
    assert E.host_code(pkg, data, bad, vd) != pkg.VERIFY_OK
    assert proof_ref.replay(dict(data.info), vd, bad, proof_ref.poseidon_hasher(), blob=data.blob) is not None


def test_first_match_wins_on_a_repeated_input(pkg):
    data, pws, sh, case = E.lookup_case(pkg, "sparse_repeated")
    assert sh.want[0] == [[2, 5, 2]]
    assert pkg.host_witness(data.blob, pws[0], sh.out_targets())[0] == [2, 5, 2]


def test_padding_counts(pkg):
    """The two ends of (40 - lookups % 40) % 40 and the steps of the row counts next to them."""
    pad = {name: (E.LU_SLOTS - E.lookup_case(pkg, name)[3]["counts"][0] % E.LU_SLOTS) % E.LU_SLOTS
           for name in ("one", "slots_minus_1", "slots_exact", "slots_plus_1", "two_rows", "two_rows_plus_1")}
    assert pad == {"one": 39, "slots_minus_1": 1, "slots_exact": 0, "slots_plus_1": 39, "two_rows": 0, "two_rows_plus_1": 39}
    rows = {name: E.lookup_case(pkg, name)[3]["rows"][0][:2] for name in pad}
    assert rows == {"one": (1, 1), "slots_minus_1": (1, 1), "slots_exact": (1, 1), "slots_plus_1": (2, 2), "two_rows": (2, 2),
                    "two_rows_plus_1": (3, 3)}


def test_rows_around_the_tables(pkg):
    """The "with rows around" cases have rows of no table before the first LookupGate row and after the last LookupTableGate row."""
    for name, before in (("six_with_rows_around", 100), ("slots_plus_1_with_rows_around", 40)):
        data, _, sh, case = E.lookup_case(pkg, name)
        assert case["rows"][0][2] == sh.gates_before + 1 > before
        assert case["rows"][-1][3] + 2 < 1 << data.info["degree_bits"]


@pytest.mark.parametrize("name", E.VANISHING_CASES)
def test_host_vanishing_identity_on_the_lookup_openings(pkg, name):
    """The host verifier's evaluator (p2_vanishing_terms) against Python's verdict on opening sets Python made valid and on
    their perturbations in the lookup openings and the selectors: several tables, a second table row, 1025 table rows."""
    import vanishing_cases as VC
    data, _, _, _ = E.lookup_case(pkg, name)
    info, circ, cases, want = E.vanishing_lookup_sweep(data)
    for c, w in zip(cases, want):
        assert VC.host(pkg, info, data.blob, c)[0] == w, c.label


# ---------------------------------------------------------------------------------------------- refusals
def test_an_empty_table_is_refused_where_it_is_added(pkg):
    b = pkg.CircuitBuilder()
    with pytest.raises(pkg.P2Error, match="lookup table is empty"):
        b.add_lookup_table_from_pairs([])
    # the C ABI's error value, and the builder is left as it was: the next table is table 0
    L = pkg.lib()
    assert L.p2_builder_add_lookup_table_from_pairs(b._h, None, 0) == (1 << 64) - 1
    assert L.p2_last_error().decode() == "lookup table is empty"
    assert b.add_lookup_table_from_pairs([(3, 5)]) == 0


def test_the_independent_builder_refuses_an_empty_table_too():
    with pytest.raises(ValueError, match="lookup table is empty"):
        oracle_builder.Builder().add_lookup_table_from_pairs([])


@pytest.mark.parametrize("which,message", [("seventh", "too many lookup tables"), ("unused", "LUT is unused")])
def test_refused_at_build(pkg, which, message):
    b = E.build_refusal(pkg, which)
    with pytest.raises(pkg.P2Error, match=message):
        b.build()


@pytest.mark.parametrize("value", E.MISS_VALUES)
def test_a_lookup_input_outside_the_table_faults(pkg, orc, value):
    data, pws, sh = E.miss_circuit(pkg, value)
    oc = orc.OracleCircuit(data.blob)
    vals, st, fault = pkg.host_witness(data.blob, pws[1], sh.out_targets())
    assert st == 1 and vals == [pkg.VALUE_UNSET]
    assert (fault.kind, fault.op_kind, fault.found) == ("LOOKUP_MISS", "LOOKUP", value)
    assert str(value) in str(fault)
    assert oc.prove(pws[1].map) == (1, None)
    for w in (0, 2):
        assert pkg.host_witness(data.blob, pws[w], sh.out_targets())[:2] == (sh.want_values(w), 0)
        assert oc.prove(pws[w].map)[0] == 0
