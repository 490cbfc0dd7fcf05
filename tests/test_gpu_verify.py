"""Batched GPU verification (p2_verify_batch / p2_verify_batch_device) against the host verifier, verdict for verdict.

The host verifier (csrc/verifier.h, p2_verify) is the independent check: for every proof -- honest, tampered, or made by the
CPU oracle from a witness that violates one constraint family -- the GPU's P2_VERIFY_* code must be the code of the reason
string the host returns for the same bytes."""
import ctypes as C
import threading

import pytest

import circuits
import verify_layout

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def host_code(pkg, data, proof, vd=None):
    """Verdict code of the host verifier (p2_verify) for these bytes."""
    vd = data.verifier_data() if vd is None else vd
    L = pkg.lib()
    rc = L.p2_verify(data.blob, len(data.blob), (C.c_uint64 * len(vd))(*vd), len(vd), proof, len(proof))
    if rc == 0:
        return pkg.VERIFY_OK
    assert rc == 4, L.p2_last_error().decode()  # P2_ERR_VERIFY
    return pkg.VERIFY_REASONS[L.p2_last_error().decode()]


def proved(pkg, data, pws):
    proofs, st = data.prove_batch(pws)
    assert st == [0] * len(pws), st
    return proofs


@pytest.mark.parametrize("name", ["aes_gcm_1k", "elgamal", "poseidon_cipher", "zk", "arithmetic_only"])
def test_accepts_gpu_proofs(gpu, name):
    pkg = gpu
    if name == "aes_gcm_1k":
        keys = [(bytes([i] * 16), bytes([i + 1] * 12), bytes([(7 * i) & 255] * 1024)) for i in range(16)]
        data, pws, _ = circuits.encrypt(pkg, 4, 1024, False, keys)
    elif name == "elgamal":
        data, pws, _, _ = circuits.ecgfp5_elgamal(pkg, [1, 2, 3])
    elif name == "poseidon_cipher":
        data, pws, _, _ = circuits.poseidon_encrypt(pkg, 3, [1, 2, 3, 4])
    elif name == "zk":
        data, pws = circuits.zk_gf_2_8_add(pkg, [(1, 2), (0x57, 0x13), (255, 0)])
    else:
        data, pws = circuits.arithmetic_only(pkg, [(3, 5, 7, 15 + 49), (2, 9, 4, 1), (P - 1, 2, 3, 0)])
    proofs = proved(pkg, data, pws)
    assert data.verify_batch(proofs) == [pkg.VERIFY_OK] * len(proofs)
    assert data.verify_batch(b"".join(proofs)) == [pkg.VERIFY_OK] * len(proofs)
    for p in proofs[:2]:
        assert host_code(pkg, data, p) == pkg.VERIFY_OK


def test_accepts_aes_gcm_64k(gpu):
    pkg = gpu
    keys = [(bytes([i + 3] * 16), bytes([i] * 12), bytes([i * 5 + 1] * 65536)) for i in range(2)]
    data, pws, _ = circuits.encrypt(pkg, 4, 65536, False, keys)
    assert data.info["degree_bits"] == 19
    proofs = proved(pkg, data, pws)
    assert data.verify_batch(proofs) == [pkg.VERIFY_OK] * 2
    assert host_code(pkg, data, proofs[0]) == pkg.VERIFY_OK


def _tampered(info, proof):
    """(label, bytes) for single-byte flips and non-canonical word writes in every section of the layout."""
    sec = verify_layout.sections(info)
    last = 27
    names = ["wires_cap", "zs_cap", "quotient_cap"] + [n for n in sec if n.startswith("open_") and sec[n][1]]
    names += [n for n in sec if n.startswith("fri_cap")] + ["final_poly", "pow_witness"]
    for q in (0, last):
        names += [n for n in sec if n.startswith("q%d_" % q)]
    out = []
    off0 = sec["q0_round0_evals"][0] if "q0_round0_evals" in sec else 0
    for e in range(16 if off0 else 0):   # one of the sixteen is the element the round-0 fold check compares
        b = bytearray(proof)
        b[off0 + 16 * e + 2] ^= 0x04
        out.append(("q0_round0_evals element %d flip" % e, bytes(b)))
    for n in names:
        off, ln, kind = sec[n]
        if kind == "count":
            b = bytearray(proof)
            b[off] ^= 1
            out.append((n + " flip", bytes(b)))
            continue
        for at in sorted({off, off + ln - 8}):
            b = bytearray(proof)
            b[at + 3] ^= 0x10
            out.append(("%s flip @%d" % (n, at - off), bytes(b)))
        for v in (P, (1 << 64) - 1):
            b = bytearray(proof)
            b[off:off + 8] = v.to_bytes(8, "little")
            out.append(("%s = %#x" % (n, v), bytes(b)))
    return out


@pytest.mark.parametrize("which", ["mix_columns", "zk"])
def test_tampered_proofs_get_the_host_verdict(gpu, which):
    pkg = gpu
    if which == "mix_columns":
        data, pws = circuits.mix_columns(pkg, circuits.random_states(3, 2))
    else:
        data, pws = circuits.zk_gf_2_8_add(pkg, [(9, 200), (1, 1)])
    proofs = proved(pkg, data, pws)
    cases = _tampered(data.info, proofs[0])
    batch, labels = [], []
    for label, b in cases:   # untouched copies interleaved
        batch += [b, proofs[1]]
        labels += [label, "untouched"]
    got = data.verify_batch(batch)
    want = [host_code(pkg, data, b) if lab != "untouched" else pkg.VERIFY_OK for lab, b in zip(labels, batch)]
    bad = [(lab, g, w) for lab, g, w in zip(labels, got, want) if g != w]
    assert not bad, bad[:20]
    # the tampering reaches every check class it can reach from single bytes
    seen = set(want)
    for code in (pkg.VERIFY_SHAPE, pkg.VERIFY_NON_CANONICAL, pkg.VERIFY_MERKLE_INITIAL, pkg.VERIFY_FRI_FOLD, pkg.VERIFY_MERKLE_FRI):
        assert code in seen, (code, sorted(seen))


def test_every_constraint_family_reaches_the_vanishing_check(gpu, orc):
    """The oracle's fault injection (test_soundness_every_constraint_family_bites): honest PoW and Merkle data, one violated
    constraint family.  The GPU gives the host's verdict, and that verdict is the zeta identity."""
    pkg = gpu
    G_LUT, G_PI, G_ARITH, G_POS = 1, 4, 5, 6
    OP_ARITH, OP_CONST, OP_LOOKUP = 0, 1, 2
    batch, datas = [], []

    def faulty(data, oc, pw_map):
        st, proof = oc.prove(pw_map)
        oc.set_fault(0)
        assert st == 0
        return proof

    data, pws = circuits.mix_columns(pkg, circuits.random_states(7, 1))
    oc = orc.OracleCircuit(data.blob)
    n = 1 << data.info["degree_bits"]
    kinds = [oc.row_gate_kind(r) for r in range(n)]
    ops = oc.ops()
    inputs_only = {k: pws[0].map[k] for k in list(pws[0].map)[:16]}
    proofs = []
    for kind in (OP_ARITH, OP_LOOKUP, OP_CONST):
        oc.set_fault(1, next(o for k, o in ops if k == kind), 0, 1)
        proofs.append(faulty(data, oc, inputs_only))
    for col, row, delta in ((2, kinds.index(G_LUT), 1), (1, kinds.index(G_LUT), 1), (0, kinds.index(G_ARITH), 5), (0, kinds.index(G_PI), 1)):
        oc.set_fault(2, col, row, delta)
        proofs.append(faulty(data, oc, pws[0].map))
    batch.append((data, proofs))
    data, pws, _, _ = circuits.poseidon_encrypt(pkg, 3, [1])
    oc = orc.OracleCircuit(data.blob)
    n = 1 << data.info["degree_bits"]
    row = [oc.row_gate_kind(r) for r in range(n)].index(G_POS)
    proofs = []
    for col in (100, 66, 24):
        oc.set_fault(2, col, row, 1)
        proofs.append(faulty(data, oc, pws[0].map))
    batch.append((data, proofs))
    for data, proofs in batch:
        want = [host_code(pkg, data, p) for p in proofs]
        assert want == [pkg.VERIFY_VANISHING] * len(proofs), want
        assert data.verify_batch(proofs) == want


def test_verifier_data_mismatches(gpu):
    pkg = gpu
    data, pws = circuits.mix_columns(pkg, circuits.random_states(5, 2))
    other, _ = circuits.arithmetic_only(pkg, [(1, 2, 3, 4)])
    proofs = proved(pkg, data, pws)
    vd = data.verifier_data()
    wrong_cap = list(vd)
    for k in range(16):   # every cap entry: whichever entries the queries reach, the initial-tree check fails
        wrong_cap[4 * k] = (wrong_cap[4 * k] + 1) % P
    wrong_digest = list(vd)
    wrong_digest[-1] = (wrong_digest[-1] + 1) % P
    for v in (wrong_cap, wrong_digest, other.verifier_data(), vd):
        want = [host_code(pkg, data, p, v) for p in proofs]
        assert data.verify_batch(proofs, v) == want
    assert host_code(pkg, data, proofs[0], wrong_cap) == pkg.VERIFY_MERKLE_INITIAL
    with pytest.raises(pkg.P2Error):
        data.verify_batch(proofs, vd[:-1])      # wrong vd_len


def _hip():
    """The HIP runtime the library itself uses (device buffers and a stream without a second runtime in the process)."""
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)   # already loaded by the library
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


def test_device_path_on_one_stream(gpu):
    pkg = gpu
    L, H = pkg.lib(), _hip()
    H2D, D2H = 1, 2
    data, pws = circuits.mix_columns(pkg, circuits.random_states(11, 6))
    B, pb = len(pws), data.proof_bytes
    h = data.gpu()
    targets = list(pws[0].map.keys())
    vals = (C.c_uint64 * (B * len(targets)))(*[pw.map[t] for pw in pws for t in targets])
    bufs = {k: C.c_void_p() for k in ("vals", "proofs", "pst", "vst")}
    sizes = {"vals": C.sizeof(vals), "proofs": B * pb, "pst": 4 * B, "vst": 4 * B}
    for k, b in bufs.items():
        assert H.hipMalloc(C.byref(b), sizes[k]) == 0
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        assert H.hipMemcpy(bufs["vals"], vals, sizes["vals"], H2D) == 0
        tarr = (C.c_uint64 * len(targets))(*targets)
        assert L.p2_prove_batch_device(h, B, tarr, len(targets), bufs["vals"], bufs["proofs"], bufs["pst"], s) == 0
        data.verify_batch_device(bufs["proofs"].value, bufs["vst"].value, B, stream=s)   # no host synchronisation in between
        assert H.hipStreamSynchronize(s) == 0
        pst, vst = (C.c_int * B)(), (C.c_int * B)()
        assert H.hipMemcpy(pst, bufs["pst"], 4 * B, D2H) == 0 and H.hipMemcpy(vst, bufs["vst"], 4 * B, D2H) == 0
        assert list(pst) == [0] * B
        assert list(vst) == [pkg.VERIFY_OK] * B
        # flip one byte of proof 2 in device memory, on the same stream, and verify again
        host = C.create_string_buffer(B * pb)
        assert H.hipMemcpy(host, bufs["proofs"], B * pb, D2H) == 0
        one = C.create_string_buffer(bytes([host.raw[2 * pb + 777] ^ 1]), 1)
        assert H.hipMemcpyAsync(C.c_void_p(bufs["proofs"].value + 2 * pb + 777), one, 1, H2D, s) == 0
        data.verify_batch_device(bufs["proofs"].value, bufs["vst"].value, B, stream=s)
        assert H.hipStreamSynchronize(s) == 0
        assert H.hipMemcpy(vst, bufs["vst"], 4 * B, D2H) == 0
        assert H.hipMemcpy(host, bufs["proofs"], B * pb, D2H) == 0
        raw = host.raw
        want = [host_code(pkg, data, raw[i * pb:(i + 1) * pb]) for i in range(B)]
        assert want[2] != pkg.VERIFY_OK and want[:2] + want[3:] == [pkg.VERIFY_OK] * (B - 1)
        assert list(vst) == want
    finally:
        H.hipStreamSynchronize(s)
        H.hipStreamDestroy(s)
        for b in bufs.values():
            H.hipFree(b)


def test_concurrency_chunks_and_zeroed_slots(gpu):
    pkg = gpu
    data, pws = circuits.mix_columns(pkg, circuits.random_states(13, 9))
    proofs = proved(pkg, data, pws)
    bad = bytearray(proofs[4])
    bad[-3] ^= 0x40   # inside the PoW witness
    batch = proofs[:4] + [bytes(bad), None] + proofs[5:]
    want = [host_code(pkg, data, bytes(data.proof_bytes) if p is None else p) for p in batch]
    assert want[5] == pkg.VERIFY_SHAPE and want[4] != pkg.VERIFY_OK
    serial_v = data.verify_batch(batch)
    serial_p = proved(pkg, data, pws)
    assert serial_v == want
    results = {}

    def prover():
        results["p"] = [data.prove_batch(pws) for _ in range(3)]

    def verifier():
        results["v"] = [data.verify_batch(batch) for _ in range(6)]

    ts = [threading.Thread(target=prover), threading.Thread(target=verifier)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert all(v == want for v in results["v"])
    assert all(st == [0] * len(pws) and ps == serial_p for ps, st in results["p"])
    data.set_option("verify_chunk", 3)     # batch of 10 -> chunks 3 + 3 + 3 + 1
    assert data.verify_batch(batch) == want
    assert data.verify_batch([]) == []
