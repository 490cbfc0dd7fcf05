"""Witness outputs, dry runs and fault diagnosis on the GPU: p2_witness_batch(_device), p2_prove_batch_outputs(_device) and
p2_witness_explain against the host twin (p2_host_witness, itself checked against the CPU oracle and against independent values
in tests/test_witness_host.py), against the same independent values directly, and against the prover they must not disturb.

Shapes: poseidon-cipher L = 3 (n = 2^4), random circuits, AES-GCM L = 13 with tag and L = 17 without (n = 2^13), ElGamal
(n = 2^14) once.  Out-lists of 1, 64, 65, 256 and 257 targets (the gather's wave and block edges; wires, virtual targets and
duplicates), batches of 1, 3 and 5 under witness_chunk = 2 (chunks of 2 + 2 + 1).  Everything compared is a field element, a
byte or a status code: exact."""
import ctypes as C
import threading

import pytest

import circuits
import pi_circuits
import test_witness_host as hw

pytestmark = pytest.mark.gpu

P = hw.P
OUT_LENGTHS = (1, 64, 65, 256, 257)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def out_list(data, extra):
    """257 out-targets: routed wires spread over the circuit, the given virtual targets, and duplicates of both."""
    wires, _, _ = hw.wired_targets(data.blob)
    step = max(len(wires) // 150, 1)
    base = list(extra) + wires[::step][:150]
    outs = [base[(7 * i) % len(base)] for i in range(257)]   # 7 is coprime to no particular length: duplicates appear early
    outs[0], outs[1] = base[0], base[0]
    return outs


def broken(pw_map):
    """(wrong last entry -> conflict or lookup miss, first entry missing)"""
    last, first = list(pw_map)[-1], list(pw_map)[0]
    wrong = dict(pw_map)
    wrong[last] = (wrong[last] + 1) % 256 if wrong[last] < 256 else (wrong[last] + 1) % P
    missing = dict(pw_map)
    del missing[first]
    return wrong, missing


def twin_check(pkg, data, maps, outs, batches, lengths):
    """generate_witness == host_witness, value for value and status for status, for each batch size and out-list length."""
    data.set_option("witness_chunk", 2)
    twin = [pkg.host_witness(data.blob, m, outs, explain=False)[:2] for m in maps]
    for B in batches:
        for n_out in lengths:
            vals, st = data.generate_witness(maps[:B], outs[:n_out])
            assert st == [t[1] for t in twin[:B]], (B, n_out)
            assert vals == [t[0][:n_out] for t in twin[:B]], (B, n_out)
    return [t[1] for t in twin]


@pytest.fixture(scope="module")
def gcm13(gpu):
    data, t = hw.gcm_circuit(gpu, 4, 13, True)
    key, iv, pt = (bytes.fromhex(hw.KAT13[k]) for k in ("key", "iv", "pt"))
    honest = hw.gcm_inputs(t, key, iv, pt, False)
    honest.update(zip(t.ct + t.tag, bytes.fromhex(hw.KAT13["ct"]) + bytes.fromhex(hw.KAT13["tag"])))
    return data, t, honest


# ------------------------------------------------------------------ device against the host twin
def test_poseidon_cipher_equals_the_host_twin(gpu):
    data, pws, t, _ = circuits.poseidon_encrypt(gpu, 3, [1, 2, 3])
    wrong, missing = broken(pws[0].map)
    maps = [pws[0].map, wrong, pws[1].map, missing, pws[2].map]   # the failing ones between honest ones, in different chunks
    assert twin_check(gpu, data, maps, out_list(data, t.ct[:8]), (1, 3, 5), OUT_LENGTHS) == [0, 1, 0, 2, 0]


@pytest.mark.parametrize("seed", range(3))
def test_random_circuits_equal_the_host_twin(gpu, orc, seed):
    data, pws = circuits.random_circuit(gpu, orc, seed, n_witnesses=3)
    wrong, missing = broken(pws[0].map)
    maps = [pws[0].map, wrong, pws[1].map, missing, pws[2].map]
    st = twin_check(gpu, data, maps, out_list(data, list(pws[0].map)), (1, 3, 5), (1, 65, 257))
    assert st[0] == st[2] == st[4] == 0   # (what the two changed witnesses do depends on the circuit drawn; the twin decides)


def test_aes_gcm_with_tag_equals_the_host_twin(gpu, gcm13):
    data, t, honest = gcm13
    wrong, missing = broken(honest)
    other = dict(honest)
    del other[t.ct[0]]   # still honest: a computed target left out
    maps = [honest, wrong, other, missing, honest]
    assert twin_check(gpu, data, maps, out_list(data, t.ct + t.tag), (1, 3, 5), (64, 256, 257)) == [0, 1, 0, 2, 0]


def test_aes_gcm_without_tag_equals_the_host_twin(gpu):
    v = hw.GOLD["derived_by_pinned_oracle"][1]
    data, t = hw.gcm_circuit(gpu, 4, 17, False)
    key, iv, pt = (bytes.fromhex(v[k]) for k in ("key", "iv", "pt"))
    no_tag = dict(zip(t.key + t.nonce + t.pt, key + iv + pt))       # the trap: status 2, the ciphertext is there all the same
    zero_tag = hw.gcm_inputs(t, key, iv, pt, True)
    maps = [zero_tag, no_tag, zero_tag]
    assert twin_check(gpu, data, maps, out_list(data, t.ct), (3,), (1, 65)) == [0, 2, 0]
    vals, st = data.generate_witness(maps, t.ct)
    assert st == [0, 2, 0] and [bytes(x).hex() for x in vals] == [v["ct"]] * 3


@pytest.fixture(scope="module")
def elgamal(gpu):
    return circuits.ecgfp5_elgamal(gpu, [7, 8])


def test_elgamal_equals_the_host_twin_and_the_natives(gpu, elgamal):
    data, pws, (pk_t, nonce_t, msg_t, ct_t), cases = elgamal
    wrong, _ = broken(pws[0].map)
    inputs_only = []
    for _, pk, msg, nonce, _ in cases:
        inputs_only.append(dict(zip(pk_t + msg_t + nonce_t, hw.flat(pk) + hw.flat(msg) + [(nonce >> i) & 1 for i in range(320)])))
    maps = [inputs_only[0], wrong, inputs_only[1]]
    outs = ct_t[0] + ct_t[1] + out_list(data, [])[:237]
    assert twin_check(gpu, data, maps, outs, (3,), (257,)) == [0, 1, 0]
    vals, st = data.generate_witness(inputs_only, ct_t[0] + ct_t[1])
    assert st == [0, 0]
    for v, (_, pk, msg, nonce, ct) in zip(vals, cases):
        assert v == hw.flat(ct[0]) + hw.flat(ct[1])


# ------------------------------------------------------------------ device against independent values
@pytest.mark.parametrize("seed", range(3))
def test_every_node_of_a_random_circuit_reads_back_as_its_python_value(gpu, seed):
    data, inputs, nodes = hw.node_circuit(gpu, seed)
    vals, st = data.generate_witness([inputs], [t for t, _ in nodes])
    assert st == [0] and vals[0] == [v for _, v in nodes]


def test_aes_gcm_known_answer_is_computed_from_the_inputs_alone(gpu, gcm13):
    data, t, honest = gcm13
    inputs = {k: honest[k] for k in t.key + t.nonce + t.pt}
    vals, st = data.generate_witness([inputs], t.ct + t.tag)
    assert st == [0] and bytes(vals[0]).hex() == hw.KAT13["ct"] + hw.KAT13["tag"]


# ------------------------------------------------------------------ proving with outputs
def test_prove_batch_with_outputs_changes_no_proof(gpu, gcm13):
    data, t, honest = gcm13
    wrong, missing = broken(honest)
    inputs = {k: honest[k] for k in t.key + t.nonce + t.pt}
    pws = [honest, wrong, inputs, missing, honest]
    outs = out_list(data, t.ct + t.tag)
    plain, st_plain = data.prove_batch(pws)
    proofs, st, vals = data.prove_batch(pws, outs)
    assert st == st_plain == [0, 1, 0, 2, 0]
    assert proofs == plain                      # non-zk proofs are deterministic: byte for byte
    assert proofs[0] == proofs[2] == proofs[4]  # the proof made from the inputs alone is the asserted one
    assert (vals, st) == data.generate_witness(pws, outs)
    assert data.prove_batch(pws, []) == (plain, st_plain, [[]] * 5)
    data.verify(proofs[2])
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_OK]


def test_outputs_are_the_public_inputs_of_the_proof(gpu):
    data, pws, want, pis = pi_circuits.small(gpu, 7)
    proofs, st, vals = data.prove_batch(pws, pis)
    assert st == [0] * len(pws)
    assert vals == want == [data.public_inputs(p) for p in proofs]
    assert data.prove_batch(pws)[0] == proofs


# ------------------------------------------------------------------ status parity with the prover
def test_statuses_are_the_provers(gpu, gcm13):
    data, t, honest = gcm13
    cases = [honest]
    for change in ({t.key[3]: 256}, {t.pt[3]: None}, {t.nonce[0]: P + 1}, {t.tag[2]: 2**64 - 1}):
        m = dict(honest)
        for k, v in change.items():
            if v is None:
                del m[k]
            else:
                m[k] = v
        cases.append(m)
    want = data.prove_batch(cases)[1]
    assert want == [0, 1, 2, 1, 1]
    assert data.generate_witness(cases, t.ct)[1] == want
    for m, s in zip(cases, want):   # and one at a time: the shared-target-list path
        assert data.generate_witness([m], [])[1] == [s] == data.prove_batch([m])[1]
    b = gpu.CircuitBuilder()
    x, y = b.add_virtual_target(), b.add_virtual_target()
    b.connect(x, y)
    out = b.mul(x, y)
    small = b.build()
    cases = [{x: 3, y: 3}, {x: 3, y: 4}, {x: 3}]
    want = small.prove_batch(cases)[1]
    assert want == [0, 1, 0]
    vals, st = small.generate_witness(cases, [out])
    assert st == want and vals[0] == vals[2] == [9]


# ------------------------------------------------------------------ one stream, no host synchronisation
def _hip():
    """The HIP runtime the library itself uses (device buffers and a stream without a second runtime in the process)."""
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    h = C.CDLL(path)
    vp = C.c_void_p
    h.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    h.hipFree.argtypes = [vp]
    h.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    h.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    h.hipStreamCreate.argtypes = [C.POINTER(vp)]
    h.hipStreamSynchronize.argtypes = [vp]
    h.hipStreamDestroy.argtypes = [vp]
    return h


def test_witness_then_prove_then_verify_on_one_stream(gpu, gcm13):
    """The circuit computes ciphertext and tag on the device; they go into the prover's value matrix by a device-to-device copy
    on the same stream; the proofs are the ones made from host-asserted witnesses."""
    data, t, honest = gcm13
    H = _hip()
    H2D, D2H, D2D = 1, 2, 3
    B, pb = 3, data.proof_bytes
    in_t, all_t = t.key + t.nonce + t.pt, list(honest)
    keys = [bytes([i + 1] * 16) for i in range(B)]
    witnesses = []
    for key in keys:
        ct, tag = gpu.native.gcm_encrypt(key, bytes(12), bytes(range(13)))
        m = dict(zip(t.key + t.nonce + t.pt + t.ct + t.tag, key + bytes(12) + bytes(range(13)) + ct + tag))
        witnesses.append({k: m[k] for k in all_t})
    want, st = data.prove_batch(witnesses)
    assert st == [0] * B
    data.set_option("witness_chunk", 2)
    vals = (C.c_uint64 * (B * len(in_t)))(*[m[k] for m in witnesses for k in in_t])
    sizes = {"in": C.sizeof(vals), "out": 8 * B * len(all_t), "vals": 8 * B * len(all_t), "wst": 4 * B, "proofs": B * pb, "pst": 4 * B, "vst": 4 * B}
    bufs = {k: C.c_void_p() for k in sizes}
    for k, b in bufs.items():
        assert H.hipMalloc(C.byref(b), sizes[k]) == 0
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        assert H.hipMemcpyAsync(bufs["in"], vals, sizes["in"], H2D, s) == 0
        data.witness_batch_device(in_t, bufs["in"].value, all_t, bufs["out"].value, bufs["wst"].value, B, stream=s)
        assert H.hipMemcpyAsync(bufs["vals"], bufs["out"], sizes["out"], D2D, s) == 0
        data.prove_batch_device(all_t, bufs["vals"].value, bufs["proofs"].value, bufs["pst"].value, B, stream=s)
        data.verify_batch_device(bufs["proofs"].value, bufs["vst"].value, B, stream=s)
        assert H.hipStreamSynchronize(s) == 0
        wst, pst, vst = (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for o, k in ((wst, "wst"), (pst, "pst"), (vst, "vst")):
            assert H.hipMemcpy(o, bufs[k], 4 * B, D2H) == 0
        assert list(wst) == list(pst) == [0] * B and list(vst) == [gpu.VERIFY_OK] * B
        host = C.create_string_buffer(B * pb)
        assert H.hipMemcpy(host, bufs["proofs"], B * pb, D2H) == 0
        assert [host.raw[i * pb:(i + 1) * pb] for i in range(B)] == want
    finally:
        H.hipStreamSynchronize(s)
        H.hipStreamDestroy(s)
        for b in bufs.values():
            H.hipFree(b)


# ------------------------------------------------------------------ explain
def test_explain_equals_the_host_twin(gpu, gcm13):
    data, t, honest = gcm13
    cases = [honest]
    for change in ({t.nonce[4]: P + 3}, {t.key[7]: 256}, {t.ct[5]: honest[t.ct[5]] ^ 0x40}, {t.pt[3]: None}, {t.ct[5]: honest[t.ct[5]] ^ 1, t.pt[3]: None},
                   {t.key[9]: 300, t.ct[5]: honest[t.ct[5]] ^ 1}, {t.tag[15]: 2**64 - 1}):
        m = dict(honest)
        for k, v in change.items():
            if v is None:
                del m[k]
            else:
                m[k] = v
        cases.append(m)
    got = [data.explain(m) for m in cases]
    assert got == [gpu.host_witness(data.blob, m)[2] for m in cases]
    assert [f.kind for f in got] == ["NONE", "INPUT_NOT_CANONICAL", "LOOKUP_MISS", "GENERATOR_CONFLICT", "NOT_SET", "GENERATOR_CONFLICT", "LOOKUP_MISS",
                                     "INPUT_NOT_CANONICAL"]
    assert all(hw.kind_matches_status(f) for f in got)
    assert got[3].target == t.ct[5] and got[3].computed == honest[t.ct[5]] and got[4].target == t.pt[3]
    b = gpu.CircuitBuilder()
    x, y, z = (b.add_virtual_target() for _ in range(3))
    b.connect(x, y)
    b.add(b.mul(x, y), z)
    small = b.build()
    for m in ({z: 1, x: 5, y: 6}, {z: 1, x: 5, y: 5}, {x: 5, y: 5}):
        f = small.explain(m)
        assert f == gpu.host_witness(small.blob, m)[2] and hw.kind_matches_status(f)
    assert small.explain({z: 1, x: 5, y: 6}).kind == "INPUT_CONFLICT"
    data2, pws, tt, _ = circuits.poseidon_encrypt(gpu, 3, [5])   # a conflict inside a PoseidonGate row
    wrong, missing = broken(pws[0].map)
    for m in (pws[0].map, wrong, missing):
        f = data2.explain(m)
        assert f == gpu.host_witness(data2.blob, m)[2] and hw.kind_matches_status(f)
    assert data2.explain(wrong).op_kind == "POSEIDON"


# ------------------------------------------------------------------ threads, zk
def test_proving_and_witness_generation_share_a_handle(gpu, gcm13):
    data, t, honest = gcm13
    inputs = {k: honest[k] for k in t.key + t.nonce + t.pt}
    want_proofs, want_st = data.prove_batch([honest] * 4)
    want_vals = data.generate_witness([inputs] * 5, t.ct + t.tag)
    res = {}

    def prove():
        res["p"] = [data.prove_batch([honest] * 4) for _ in range(2)]

    def witness():
        res["w"] = [data.generate_witness([inputs] * 5, t.ct + t.tag) for _ in range(4)]

    th = [threading.Thread(target=prove), threading.Thread(target=witness)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert res["p"] == [(want_proofs, want_st)] * 2
    assert res["w"] == [want_vals] * 4


def test_zk_outputs_ignore_blinding_and_witness_calls_leave_the_counter(gpu):
    data, pws = circuits.zk_gf_2_8_add(gpu, [(1, 2), (0x57, 0x13)])
    xy = list(pws[0].map)[2]
    inputs = [{k: pw.map[k] for k in list(pw.map)[:2]} for pw in pws]
    key = [11, 22, 33, 44]
    data.set_zk_key(key)
    first = data.prove_batch(pws)
    again = type(data)(data.blob)
    again.set_zk_key(key)
    for _ in range(3):
        assert again.generate_witness(inputs, [xy]) == ([[3], [0x57 ^ 0x13]], [0, 0])
    assert again.explain(inputs[0]).kind == "NONE"
    proofs, st, vals = again.prove_batch(pws, [xy])
    assert (proofs, st) == first and vals == [[3], [0x57 ^ 0x13]]
