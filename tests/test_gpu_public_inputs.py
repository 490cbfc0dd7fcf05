"""Public inputs on the MI355X: the prover's trailer and public-input hash (k_pi_hash), the transcript and the PublicInputGate
constraint that use it, and both verifiers on honest and tampered proofs -- the GPU verdict always the host verifier's."""
import ctypes as C
import struct

import pytest

import pi_circuits

pytestmark = pytest.mark.gpu

P = pi_circuits.P


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def _circuit(pkg, name):
    if name.startswith("small"):
        data, pws, vals, _ = pi_circuits.small(pkg, int(name[5:]))
    elif name == "aes_gcm_1k":
        data, pws, vals = pi_circuits.aes_gcm(pkg, 1024, 3)
    else:
        data, pws, vals = pi_circuits.zk(pkg)
        data.set_zk_seed(7)
    return data, pws, vals


CASES = ["small1", "small7", "small8", "small9", "small17", "aes_gcm_1k", "zk"]
_cache = {}


@pytest.fixture(scope="module", params=CASES)
def proven(gpu, request):
    """(data, pws, values, proofs) per circuit: one batch through p2_prove_batch."""
    pkg = gpu
    if request.param not in _cache:
        data, pws, vals = _circuit(pkg, request.param)
        proofs, st = data.prove_batch(pws)
        assert st == [0] * len(pws), st
        _cache[request.param] = (request.param, data, pws, vals, proofs)
    return _cache[request.param]


def host_code(pkg, data, proof, vd=None):
    vd = data.verifier_data() if vd is None else vd
    L = pkg.lib()
    rc = L.p2_verify(data.blob, len(data.blob), (C.c_uint64 * len(vd))(*vd), len(vd), bytes(proof), len(proof))
    if rc == 0:
        return pkg.VERIFY_OK
    assert rc == 4, L.p2_last_error().decode()
    return pkg.VERIFY_REASONS[L.p2_last_error().decode()]


def test_both_verifiers_accept_honest_proofs(gpu, proven):
    name, data, pws, vals, proofs = proven
    for p in proofs:
        data.verify(p)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * len(proofs)


def test_trailer_holds_the_witness_values(gpu, proven):
    name, data, pws, vals, proofs = proven
    k = data.num_public_inputs
    assert k == len(vals[0])
    L = gpu.lib()
    assert L.p2_circuit_num_public_inputs(data.gpu()) == k
    out, n = (C.c_uint64 * k)(), C.c_size_t()
    for p, want in zip(proofs, vals):
        assert data.public_inputs(p) == want
        assert struct.unpack_from("<Q", p, len(p) - 8 * (k + 1))[0] == k
        assert L.p2_circuit_public_inputs(data.gpu(), p, len(p), out, k, C.byref(n)) == 0  # the handle form
        assert n.value == k and list(out) == want
    if name == "aes_gcm_1k":
        assert all(v < 256 for v in vals[0]) and len(vals[0]) == 1024 + 16  # the real ciphertext and tag bytes


def test_public_inputs_hash_matches_oracle_and_gate_wires(gpu, orc, proven):
    """debug_read("public_inputs_hash") of every proof of the last batch = the oracle's hash_no_pad of the values = the
    PublicInputGate row's wires 0..3 of the device witness; the whole wire matrix and wires_cap equal the oracle's."""
    name, data, pws, vals, proofs = proven
    pkg = gpu
    proofs2, st = data.prove_batch(pws)  # make this circuit's batch the handle's last one
    assert st == [0] * len(pws)
    if name != "zk":
        assert proofs2 == proofs  # non-zk proofs are deterministic
    oc = orc.OracleCircuit(data.blob)
    n = 1 << data.info["degree_bits"]
    row = pi_circuits.pi_gate_row(oc, n)
    for i, (pw, want) in enumerate(zip(pws, vals)):
        h = (C.c_uint64 * 4)()
        orc.lib().orc_hash_no_pad((C.c_uint64 * len(want))(*want), len(want), h)
        got = data.debug_read("public_inputs_hash", i)
        assert got == list(h)
        assert got == pkg.poseidon_native.hash_n_to_m_no_pad(want, 4)
        wires = data.debug_read("wires", i)
        assert [wires[c * n + row] for c in range(4)] == got
        if name == "zk" or i > 0:
            continue  # zk: blinding rows come from the handle's key; the oracle's witness is compared on the other circuits
        st_o, ow = oc.generate_witness(pw.map, data.info["num_wires"] * n)
        assert st_o == 0 and ow == wires
        st_p, _ = oc.prove(pw.map, trace=True)
        assert oc.trace("wires_cap") == data.debug_read("wires_cap", i)


def _hip():
    """The HIP runtime the library itself uses (found in this process's mappings)."""
    h = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    vp = C.c_void_p
    h.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    h.hipFree.argtypes = [vp]
    h.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    return h


def test_device_path_bytes_equal_host_path(gpu, proven):
    name, data, pws, vals, proofs = proven
    if name == "zk":
        pytest.skip("zk proofs draw fresh blinding per proof")
    H, H2D, D2H = _hip(), 1, 2
    targets = list(pws[0].map)
    B, pb = len(pws), data.proof_bytes
    hv = (C.c_uint64 * (B * len(targets)))(*[pw.map[t] for pw in pws for t in targets])
    bufs = {k: C.c_void_p() for k in ("vals", "proofs", "st")}
    sizes = {"vals": C.sizeof(hv), "proofs": B * pb, "st": 4 * B}
    for k, b in bufs.items():
        assert H.hipMalloc(C.byref(b), sizes[k]) == 0
    try:
        assert H.hipMemcpy(bufs["vals"], hv, sizes["vals"], H2D) == 0
        data.prove_batch_device(targets, bufs["vals"].value, bufs["proofs"].value, bufs["st"].value, B)
        data.synchronize()
        assert H.hipDeviceSynchronize() == 0
        out, st = C.create_string_buffer(B * pb), (C.c_int * B)()
        assert H.hipMemcpy(out, bufs["proofs"], B * pb, D2H) == 0 and H.hipMemcpy(st, bufs["st"], 4 * B, D2H) == 0
        assert list(st) == [0] * B
        assert out.raw == b"".join(proofs)
    finally:
        for b in bufs.values():
            H.hipFree(b)


def test_failed_slot_is_zeroed_with_its_trailer(gpu):
    pkg = gpu
    data, pws, vals, pis = pi_circuits.small(pkg, 9)
    bad = pkg.PartialWitness()
    bad.map = dict(pws[0].map)
    bad.map.pop(next(iter(bad.map)))  # an input target left unset: witness generation fails
    pb = data.proof_bytes
    buf = C.create_string_buffer(2 * pb)
    asg = (pkg.api._Assignment * 2)()
    keep = []
    for i, pw in enumerate([pws[0], bad]):
        ts, vs = pkg.api._arr(list(pw.map)), pkg.api._arr(list(pw.map.values()))
        keep.append((ts, vs))
        asg[i].targets, asg[i].values, asg[i].count = ts, vs, len(pw.map)
    status = (C.c_int * 2)()
    assert pkg.lib().p2_prove_batch(data.gpu(), 2, asg, buf, status) == 0
    assert status[0] == 0 and status[1] != 0
    assert buf.raw[pb:2 * pb] == bytes(pb)
    assert data.public_inputs(buf.raw[:pb]) == vals[0]


def _tampered(name, data, proofs):
    k, pb = data.num_public_inputs, data.proof_bytes
    t0 = pb - 8 * (k + 1)
    out = {}
    p = bytearray(proofs[0])
    v = struct.unpack_from("<Q", p, t0 + 8)[0]
    struct.pack_into("<Q", p, t0 + 8, (v + 1) % P)
    out["value changed"] = bytes(p)
    p = bytearray(proofs[0])
    struct.pack_into("<Q", p, pb - 8, P)
    out["value = p"] = bytes(p)
    p = bytearray(proofs[0])
    struct.pack_into("<Q", p, t0, k + 1)
    out["count word"] = bytes(p)
    p = bytearray(proofs[0])
    p[t0:] = proofs[1][t0:]
    out["trailers swapped"] = bytes(p)
    return out


def test_tampered_proofs_rejected_by_both_verifiers(gpu, proven):
    name, data, pws, vals, proofs = proven
    pkg = gpu
    cases = _tampered(name, data, proofs)
    expect = {"value changed": None, "value = p": pkg.VERIFY_NON_CANONICAL, "count word": pkg.VERIFY_SHAPE, "trailers swapped": None}
    if vals[0] == vals[1]:
        del cases["trailers swapped"]
    codes = data.verify_batch(list(cases.values()))
    for (case, proof), code in zip(cases.items(), codes):
        host = host_code(pkg, data, proof)
        assert host != pkg.VERIFY_OK, case
        assert code == host, (case, code, host)
        if expect[case] is not None:
            assert host == expect[case], (case, host)


def test_zero_pi_twin_verifier_data_rejects(gpu):
    """A proof of the circuit with public inputs, checked against the verifier data of the same circuit without them."""
    pkg = gpu
    data, pws, vals, _ = pi_circuits.small(pkg, 9)
    twin, _, _, _ = pi_circuits.small(pkg, 9, register=False)
    proofs, st = data.prove_batch(pws)
    assert st == [0, 0]
    vd = twin.verifier_data()
    assert vd != data.verifier_data()
    codes = data.verify_batch(proofs, verifier_data=vd)
    for p, code in zip(proofs, codes):
        host = host_code(pkg, data, p, vd)
        assert host != pkg.VERIFY_OK and code == host
