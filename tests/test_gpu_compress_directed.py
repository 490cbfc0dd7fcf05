"""GPU tests (pytest -m gpu): the compressed-proof kernels of csrc/kernels_compress.h on directed input.

The query indices a compressed proof writes decide every byte offset that k_cmp_plan, k_cmp_scatter, k_cmp_infer, k_cmp_merkle /
k_kcc_merkle and k_cmp_pack use.  Here the kernels get the malformed proofs of tests/compress_cases.py -- lengths, index
tables, re-laid-out index sets, every count byte, non-canonical words at the ends of every kind of block, canonical flips with
the class each must get, two faults at once -- and the index sets of an index sweep that reach the branches of the layout code
(twins, shared cosets, blocks with no and with all siblings).  The reference is the host decoder of csrc/compress.h, which
tests/test_compress_cases_host.py holds to the cases' construction and to the independent Python compressor; every comparison
is exact.  Circuits: the arithmetic chains at 2, 7 and 11 bits (no FRI round and one-sibling paths; one round with a round
tree two levels deep; two rounds), nine public inputs, the zk circuit, and the Keccak chains at 2 and 7 bits.  Proofs come
from prove_batch; no oracle is used."""
import ctypes as C

import pytest

import compress_cases as CC
import test_compress_cases_host as HC
import test_compress_host as H
import test_gpu_verify as TV
from test_gpu_merkle import D2H, H2D, Device

pytestmark = pytest.mark.gpu

CIRCUITS = ["chain_2", "chain_7", "chain_11", "public_inputs", "zk", "chain_2-keccak", "chain_7-keccak"]
WITNESSES = 16


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return pkg


class Proven:
    """One circuit: 16 proofs of prove_batch, the chosen sweep proofs made from the first, the malformed cases of the first
    and the host's verdicts on them -- each computed once and shared by the tests."""

    def __init__(self, pkg, key):
        name, _, hasher = key.partition("-")
        self.pkg, self.key, self.name = pkg, key, name
        self.data, pws = HC.build(pkg, name, WITNESSES, hasher=hasher or "poseidon")
        assert self.data.info.get("hasher", "poseidon") == (hasher or "poseidon")
        self.proofs, st = self.data.prove_batch(pws)
        assert st == [0] * WITNESSES, st
        assert len(set(self.proofs)) == WITNESSES
        self.vd = self.data.verifier_data()
        self.info = dict(self.data.info)
        self._cases = self._sweep = None

    def compress(self, proof):
        return H.compress(self.pkg, self.data, self.vd, proof)

    def indices(self, proof):
        return CC.written_indices(self.info, self.compress(proof))

    def vc_reason(self, b):
        return HC.vc_reason(self.pkg, self.data, self.vd, b)

    def cases(self):
        """[(label, bytes, want, host verify_compressed reason, host decompress reason)]"""
        if self._cases is None:
            p = self.proofs[0]
            raw = CC.malformed(self.info, p, self.indices(p), pow_fails=lambda b: self.vc_reason(b) == CC.POW)
            self._cases = [(lbl, b, want) + HC.host_verdicts(self.pkg, self.data, self.vd, b) for lbl, b, want in raw]
        return self._cases

    def sweep(self):
        """(chosen sweep proofs, predicates they and the honest proofs show)"""
        if self._sweep is None:
            chosen, shown = HC.chosen_sweep(self.name, self.info, self.proofs[0], self.indices)
            for p in self.proofs:
                shown |= {k for k, hit in CC.index_predicates(self.indices(p), self.info).items() if hit}
            self._sweep = chosen, shown
        return self._sweep


@pytest.fixture(scope="module")
def store(gpu):
    """the circuits proved so far, released with the module (before the library goes away)"""
    made = {}
    yield made
    made.clear()


def _proven(gpu, store, key):
    if key not in store:
        store[key] = Proven(gpu, key)
    return store[key]


@pytest.fixture(scope="module", params=CIRCUITS)
def proven(gpu, store, request):
    return _proven(gpu, store, request.param)


# ------------------------------------------------------------------------------------------------ raw batch calls on (buffer, length)
def _slots(data, items):
    pb = data.proof_bytes
    parts = [CC.case_bytes(b) for b in items]
    assert all(len(buf) <= pb for buf, _ in parts)
    buf = C.create_string_buffer(len(parts) * pb)
    for i, (b, _) in enumerate(parts):
        C.memmove(C.addressof(buf) + i * pb, b, len(b))
    return buf, (C.c_uint32 * len(parts))(*[n for _, n in parts])


def gpu_verify(pkg, data, items):
    buf, lengths = _slots(data, items)
    status = (C.c_int * len(items))()
    assert pkg.lib().p2_verify_compressed_batch(data.gpu(), len(items), buf, lengths, None, 0, status) == 0, pkg.lib().p2_last_error()
    return list(status)


def gpu_decompress(pkg, data, items):
    """(the output slots as the C call left them, statuses); the output buffer is not zero beforehand"""
    buf, lengths = _slots(data, items)
    pb, B = data.proof_bytes, len(items)
    out = C.create_string_buffer(b"\xaa" * (B * pb), B * pb)
    status = (C.c_int * B)()
    assert pkg.lib().p2_decompress_batch(data.gpu(), B, buf, lengths, None, 0, out, status) == 0, pkg.lib().p2_last_error()
    return [C.string_at(C.addressof(out) + i * pb, pb) for i in range(B)], list(status)     # (out.raw would copy the buffer per slot)


def _interleaved(pr, cases):
    """the cases at the even places, untouched honest compressed proofs (of proofs 1, 2, ..) at the odd ones"""
    honest = [pr.compress(p) for p in pr.proofs[1:]]
    batch = []
    for i, c in enumerate(cases):
        batch += [c[1], honest[i % len(honest)]]
    return batch


def _mismatches(labels, got, want):
    return [(lbl, g, w) for lbl, g, w in zip(labels, got, want) if g != w][:12]


# ------------------------------------------------------------------------------------------------ malformed cases
def test_malformed_cases_get_the_host_verdict(gpu, proven):
    pr, R = proven, gpu.VERIFY_REASONS
    cases = pr.cases()
    outside = [(lbl, r, sorted(want)) for lbl, _, want, r, _ in cases if r not in want]
    assert not outside, outside[:12]
    batch = _interleaved(pr, cases)
    got = gpu_verify(gpu, pr.data, batch)
    want = [R[c[3]] for c in cases]
    assert not _mismatches([c[0] for c in cases], got[0::2], want)
    assert got[1::2] == [gpu.VERIFY_OK] * len(cases)
    classes = {gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_NON_CANONICAL, gpu.VERIFY_POW, gpu.VERIFY_MERKLE_INITIAL}
    if pr.info["num_fri_rounds"]:
        classes.add(gpu.VERIFY_MERKLE_FRI)
    assert classes <= set(got[0::2]), classes - set(got)


def test_malformed_cases_decompress_as_on_the_host(gpu, proven):
    pr, R = proven, gpu.VERIFY_REASONS
    cases = pr.cases()
    batch = _interleaved(pr, cases)
    slots, st = gpu_decompress(gpu, pr.data, batch)
    assert not _mismatches([c[0] for c in cases], st[0::2], [R[c[4]] for c in cases])
    assert st[1::2] == [gpu.VERIFY_OK] * len(cases)
    zero, accepted = bytes(pr.data.proof_bytes), 0
    for (lbl, b, _, _, err), slot in zip(cases, slots[0::2]):
        if err:
            assert slot == zero, lbl
        else:
            assert slot == HC.decompress(gpu, pr.data, pr.vd, b)[0], lbl
            accepted += 1
    assert accepted >= 5        # the canonical flips of leaves, siblings and evaluations decompress, and the 0xFF-filled slot
    for p, slot in zip(pr.proofs[1:], slots[1::2]):
        assert slot == p
    # the Python wrapper on the same batch: None for every rejected slot
    full, st2 = pr.data.decompress_batch([CC.case_bytes(b)[0][:CC.case_bytes(b)[1]] for b in batch])
    assert st2 == st
    assert [f is None for f in full] == [s != gpu.VERIFY_OK for s in st]


# ------------------------------------------------------------------------------------------------ index sets
def test_index_sets_compress_and_decompress_as_on_the_host(gpu, proven):
    pr = proven
    chosen, shown = pr.sweep()
    required = set(HC.CIRCUITS[pr.name][1])
    if "keccak" not in pr.key:      # (the Poseidon proofs are the oracle's, for which the sweep lengths were found)
        assert required <= shown, sorted(required - shown)
    full = pr.proofs + chosen
    host_c = [pr.compress(p) for p in full]
    got, st = pr.data.compress_batch(full)
    assert st == [gpu.VERIFY_OK] * len(full)
    assert got == host_c
    for p, c in zip(full, got):
        assert c == CC.py_compress(pr.info, p, CC.written_indices(pr.info, c))[0]
    back, st = pr.data.decompress_batch(got)
    assert st == [gpu.VERIFY_OK] * len(full)
    want = [HC.decompress(gpu, pr.data, pr.vd, c)[0] for c in host_c]
    assert all(w is not None for w in want) and back == want
    assert back[:WITNESSES] == pr.proofs
    codes = pr.data.verify_compressed_batch(got)
    assert codes[:WITNESSES] == [gpu.VERIFY_OK] * WITNESSES
    assert codes[WITNESSES:] == [gpu.VERIFY_REASONS[pr.vc_reason(c)] for c in host_c[WITNESSES:]]
    assert gpu.VERIFY_OK not in codes[WITNESSES:]


@pytest.mark.parametrize("key", [k for k in CIRCUITS if "keccak" not in k])   # (test_gpu_keccak does this for Keccak)
def test_malformed_full_proofs_compress_as_on_the_host(gpu, store, key):
    pr = _proven(gpu, store, key)
    L, R = gpu.lib(), gpu.VERIFY_REASONS
    cases = TV._tampered(CC._body_info(pr.info), pr.proofs[0])
    host = [H._call(gpu, L.p2_proof_compress, pr.data, pr.vd, b) for _, b in cases]
    got, st = pr.data.compress_batch([b for _, b in cases])
    labels = [lbl for lbl, _ in cases]
    assert not _mismatches(labels, st, [gpu.VERIFY_OK if rc == 0 else R[r] for rc, r in host])
    assert not _mismatches(labels, got, [r if rc == 0 else None for rc, r in host])
    assert {gpu.VERIFY_OK, gpu.VERIFY_SHAPE, gpu.VERIFY_NON_CANONICAL} <= set(st)
    packed = [(lbl, c) for lbl, c in zip(labels, got) if c is not None]
    codes = pr.data.verify_compressed_batch([c for _, c in packed])
    assert not _mismatches([lbl for lbl, _ in packed], codes, [R[pr.vc_reason(c)] for _, c in packed])
    assert {gpu.VERIFY_POW, gpu.VERIFY_MERKLE_INITIAL} <= set(codes)     # a cap word moves the transcript; query 0 stores its leaves


# ------------------------------------------------------------------------------------------------ batch mechanics
def test_chunks_and_order_do_not_change_the_verdicts(gpu, store):
    pr = _proven(gpu, store, "chain_7")
    cases = pr.cases()
    batch = _interleaved(pr, cases)
    want, want_d = [], []
    for c in cases:
        want += [gpu.VERIFY_REASONS[c[3]], gpu.VERIFY_OK]
        want_d += [gpu.VERIFY_REASONS[c[4]], gpu.VERIFY_OK]
    assert gpu_verify(gpu, pr.data, batch[::-1]) == want[::-1]
    pr.data.set_option("verify_chunk", 7)
    try:
        assert gpu_verify(gpu, pr.data, batch) == want
        assert gpu_verify(gpu, pr.data, batch[::-1]) == want[::-1]
        assert gpu_decompress(gpu, pr.data, batch)[1] == want_d
    finally:
        pr.data.set_option("verify_chunk", 512)


# ------------------------------------------------------------------------------------------------ device forms
@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


@pytest.mark.parametrize("key", ["chain_7", "chain_7-keccak"])
def test_device_forms_judge_the_lengths(gpu, store, dev, key):
    """Lengths [honest, stride + 1, 0xFFFFFFFF, 0, honest] on one stream: a length above the stride is SHAPE in the device
    forms, the bytes of a slot past its length are ignored, and a rejected slot of decompress is zeroed."""
    pr = _proven(gpu, store, key)
    data, pb, B = pr.data, pr.data.proof_bytes, 5
    cps = [pr.compress(p) for p in pr.proofs[:B]]
    lengths = [len(cps[0]), pb + 1, 0xFFFFFFFF, 0, len(cps[4])]
    inp = b"".join(c + b"\xff" * (pb - len(c)) for c in cps)      # the slack past every proof is 0xFF
    d_in, d_out, d_len, d_vst, d_dst = dev.alloc(B * pb), dev.alloc(B * pb), dev.alloc(4 * B), dev.alloc(4 * B), dev.alloc(4 * B)
    Hh = dev.H
    assert Hh.hipMemcpy(d_in, inp, B * pb, H2D) == 0
    assert Hh.hipMemcpy(d_out, b"\xaa" * (B * pb), B * pb, H2D) == 0
    assert Hh.hipMemcpy(d_len, (C.c_uint32 * B)(*lengths), 4 * B, H2D) == 0
    s = C.c_void_p()
    assert Hh.hipStreamCreate(C.byref(s)) == 0
    try:
        data.verify_compressed_batch_device(d_in.value, d_len.value, d_vst.value, B, stream=s)
        data.decompress_batch_device(d_in.value, d_len.value, d_out.value, d_dst.value, B, stream=s)
        assert Hh.hipStreamSynchronize(s) == 0
    finally:
        Hh.hipStreamSynchronize(s)
        Hh.hipStreamDestroy(s)
    want = [gpu.VERIFY_OK] + [gpu.VERIFY_SHAPE] * 3 + [gpu.VERIFY_OK]
    assert dev.get(d_vst, B, C.c_int) == want
    assert dev.get(d_dst, B, C.c_int) == want
    out = C.create_string_buffer(B * pb)
    assert Hh.hipMemcpy(out, d_out, B * pb, D2H) == 0
    slots = [C.string_at(C.addressof(out) + i * pb, pb) for i in range(B)]
    for i in (0, 4):
        assert slots[i] == HC.decompress(gpu, data, pr.vd, cps[i])[0] == pr.proofs[i]
    for i in (1, 2, 3):
        assert slots[i] == bytes(pb), i
