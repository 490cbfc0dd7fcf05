"""GPU tests (pytest -m gpu) of the lookup argument away from the AES / GCM tables: k_lut_rows, k_lookup_terms, k_lookup_scan,
the lookup branch of k_witness and the lookup views of k_quotient and k_vfy_vanishing, on custom tables at the edges of the
padding count, of the 26 table slots and 40 looking slots of a row, of the 1024 threads of the scan, of the 16-bit entry index
and of the six-table limit (tests/edge_circuits.py LOOKUP_CASES; tests/test_lookup_edges_host.py shows each case a sound
reference on the CPU).  Whole proofs in batches of three, byte for byte against the CPU oracle, then through both verifiers,
the Python replay and the compressor (edge_circuits.gpu_proofs_hold); the looked-up outputs read back from the device against
the first matching pair; refusals against the host witness twin, field for field."""
import ctypes as C

import pytest

import edge_circuits as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return pkg


@pytest.mark.parametrize("name", list(E.LOOKUP_CASES))
def test_lookup_edge(gpu, orc, name):
    data, pws, sh, case = E.lookup_case(gpu, name)
    if name in ("scan_1024", "scan_1025"):      # k_lookup_scan's `total`: per = 1 with every thread live / per = 2, threads 513.. empty
        lu, lut, _, _ = case["rows"][0]
        assert lu + lut == int(name[5:])
    if name == "table_scan":                    # per2 = 2 on the RE pass, per = 2 on the other
        assert case["rows"][0][:2] == (1, 1025)
    outs = sh.out_targets()
    vals, st = data.generate_witness(pws, outs)
    assert st == [0, 0, 0]
    assert vals == [sh.want_values(w) for w in range(3)]
    E.gpu_proofs_hold(gpu, orc, data, pws, oracle=True)


@pytest.mark.parametrize("name", E.VANISHING_CASES)
def test_gpu_vanishing_identity_on_the_lookup_openings(gpu, name):
    """The lookup view of k_vfy_vanishing alone (p2_gpu_vanishing_flags: no transcript, so a changed opening reaches the
    identity, where in a whole proof the proof-of-work check answers first): Python's verdict on valid opening sets and on
    every perturbation of the lookup openings and the selectors, the host evaluator asked too."""
    import vanishing_cases as VC
    data, _, _, _ = E.lookup_case(gpu, name)
    info, circ, cases, want = E.vanishing_lookup_sweep(data)
    flags = VC.gpu_flags(gpu, data, info, cases)
    for c, f, w in zip(cases, flags, want):
        assert VC.flags_verdict(f) == w, c.label
        assert VC.host(gpu, info, data.blob, c)[0] == w, c.label


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("which,message", [("seventh", "too many lookup tables"), ("unused", "LUT is unused")])
def test_refused_at_build(gpu, which, message):
    b = E.build_refusal(gpu, which)
    with pytest.raises(gpu.P2Error, match=message):
        b.build()


@pytest.mark.parametrize("value", E.MISS_VALUES)
def test_a_lookup_input_outside_the_table_faults_as_on_the_host(gpu, orc, value):
    """The miss in the middle slot of a batch of three: statuses from generate_witness, prove_batch and explain equal the host
    twin's, the fault names the value with the twin's fields, the honest neighbours' proofs are the oracle's and the failed
    slot of the proof buffer is zeroed."""
    data, pws, sh = E.miss_circuit(gpu, value)
    outs = sh.out_targets()
    twin = [gpu.host_witness(data.blob, pw, outs) for pw in pws]
    assert [t[1] for t in twin] == [0, 1, 0]
    vals, st = data.generate_witness(pws, outs)
    assert st == [t[1] for t in twin] and vals == [t[0] for t in twin]
    assert vals[0] == sh.want_values(0) and vals[2] == sh.want_values(2) and vals[1] == [gpu.VALUE_UNSET]
    for pw, t in zip(pws, twin):
        fault = data.explain(pw)
        assert fault == t[2], (fault, t[2])
    fault = data.explain(pws[1])
    assert (fault.status, fault.kind, fault.op_kind, fault.found) == (1, "LOOKUP_MISS", "LOOKUP", value)
    # the proof buffer itself, filled beforehand so that "zeroed" is the library's doing
    pb = data.proof_bytes
    asg, keep = data._assignments(pws)
    buf = C.create_string_buffer(b"\xff" * (3 * pb), 3 * pb)
    status = (C.c_int * 3)(-1, -1, -1)
    assert gpu.lib().p2_prove_batch(data.gpu(), 3, asg, buf, status) == 0, gpu.lib().p2_last_error()
    assert list(status) == [0, 1, 0]
    raw = buf.raw
    assert raw[pb:2 * pb] == bytes(pb)
    oc = orc.OracleCircuit(data.blob)
    assert data.verifier_data() == oc.verifier_data()
    for w in (0, 2):
        assert oc.prove(pws[w].map) == (0, raw[w * pb:(w + 1) * pb])
        data.verify(raw[w * pb:(w + 1) * pb])
    assert oc.prove(pws[1].map) == (1, None)
    assert data.verify_batch(raw) == [gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_OK]
