"""MerkleMap on the device (p2_merkle_map_*; kernels_merkle_map.h) against tests/merkle_map_ref.py, a Python map over the CPU
oracle's Poseidon: cap, len, the number of hashes (every non-empty node above the leaves once) and lookups of present and absent
keys, at the smallest shapes at which each kernel can go wrong -- no entry, no level, one workgroup and one lane into the next,
sixteen workgroups shrinking to one, single-child chains with the empty digest on alternating sides.  Then the round trip
through verify_batch, the pointer forms, refusals, stream ordering, and a nullifier set end to end: four chained spends with the
siblings written by the map straight into the prover's value matrix.  Everything compared is exact."""
import ctypes as C
import gc
import random

import numpy as np
import pytest

import merkle_map_cases as mc
import merkle_map_ref as ref
import proof_ref as R
from test_gpu_merkle import D2H, Device

pytestmark = pytest.mark.gpu

P = ref.P
FILL = 0xF00D000000000000


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture
def dev(gpu):
    d = Device()
    yield d
    d.free()


def space(D):
    return min(1 << D, P)


def random_keys(D, n, seed):
    r, keys = random.Random(seed), set()
    while len(keys) < n:
        keys.add(r.randrange(space(D)))
    return tuple(sorted(keys, key=lambda k: (k * 0x9E3779B97F4A7C15) & 0xFFFF))       # not in key order


def clustered():
    """256 keys inside one 2^8-leaf subtree and one key with the top bit set: chains of single children up to level 63"""
    base = 0x0123456789ABCD00
    return tuple([base + i for i in range(255, -1, -1)] + [(1 << 63) + 5])


# (name, key_bits, cap_height, value_len, keys)
CASES = [("D1 h0 empty", 1, 0, 0, ()), ("D1 h0 one", 1, 0, 3, (1,)), ("D1 h1 both", 1, 1, 4, (1, 0)), ("D1 h1 empty", 1, 1, 8, ()),
         ("D8 h0 empty", 8, 0, 4, ()), ("D8 h0 one", 8, 0, 0, (200,)), ("D8 h4 two", 8, 4, 3, (77, 76)), ("D8 h0 255", 8, 0, 8, random_keys(8, 255, 1)),
         ("D8 h4 dense", 8, 4, 4, random_keys(8, 256, 2)), ("D8 h0 dense set", 8, 0, 0, random_keys(8, 256, 3)),
         ("D13 h0 257", 13, 0, 3, random_keys(13, 257, 4)), ("D13 h0 4096", 13, 0, 4, random_keys(13, 4096, 5)), ("D13 h3 256 set", 13, 3, 0, random_keys(13, 256, 6)),
         ("D64 h0 empty", 64, 0, 0, ()), ("D64 h0 one", 64, 0, 0, (P - 1,)), ("D64 h4 two", 64, 4, 8, (5, 1 << 63)), ("D64 h0 255", 64, 0, 4, random_keys(64, 255, 7)),
         ("D64 h4 257 set", 64, 4, 0, random_keys(64, 257, 8)), ("D64 h0 4096", 64, 0, 3, random_keys(64, 4096, 9)), ("D64 h4 4096", 64, 4, 4, random_keys(64, 4096, 10)),
         ("D64 h0 clustered set", 64, 0, 0, clustered()), ("D64 h4 clustered", 64, 4, 4, clustered()),
         ("D64 h0 edge keys", 64, 0, 4, tuple(mc.KEYS_64)), ("D64 h4 edge keys", 64, 4, 3, tuple(mc.KEYS_64))]
BY_NAME = {c[0]: c for c in CASES}


def queries(D, keys, seed=0):
    """present: every key (N <= 257) or both sides of every 256-boundary of the sorted order; absent: the neighbours +-1 of
    present keys, keys that share all but the low four bits with one, random ones"""
    s, r = sorted(keys), random.Random(100 + seed)
    present = s if len(s) <= 257 else [s[i] for b in range(256, len(s), 256) for i in (b - 1, b)] + [s[0], s[-1]]
    near = [k + d for k in present[:40] for d in (-1, 1)] + [k ^ r.randrange(1, 16) for k in present[:40]]
    absent = [k for k in near + [r.randrange(space(D)) for _ in range(16)] + [0, space(D) - 1] if 0 <= k < space(D) and k not in set(keys)]
    return present + absent


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_map_equals_the_reference(gpu, name):
    _, D, h, V, keys = BY_NAME[name]
    m = mc.model(keys, D, h, V)
    mm = gpu.MerkleMap(list(keys), [m.entries[k] for k in keys], D, h, value_len=V)
    q = queries(D, keys)
    mc.check_map(mm, m, q)
    assert mm.hashes == m.hashes
    proofs = mm.get_batch(q)
    assert gpu.merkle_map.verify_batch(q, D, proofs, mm.cap) == [0] * len(q)
    assert [p[0] for p in proofs] == [int(k in m.entries) for k in q]


def test_a_dense_map_is_the_dense_tree(gpu):
    _, D, h, V, keys = BY_NAME["D8 h4 dense"]
    m = mc.model(keys, D, h, V)
    mm = gpu.MerkleMap(list(keys), [m.entries[k] for k in keys], D, h)
    tree = gpu.MerkleTree([m.entries[k] + [1] for k in range(256)], h)
    assert mm.cap == tree.cap and [p[2] for p in mm.get_batch(range(256))] == tree.prove_batch(range(256))
    assert mm.hashes == 256 - 16


@pytest.mark.parametrize("name", ("D8 h4 two", "D64 h4 two", "D64 h4 clustered", "D64 h4 edge keys"))
def test_tampered_proofs_get_the_host_twins_statuses(gpu, name):
    _, D, h, V, keys = BY_NAME[name]
    m = mc.model(keys, D, h, V)
    some = sorted(keys)[len(keys) // 2]
    absent = next(k for k in (some ^ 2, some ^ (1 << 20)) if k not in m.entries)
    cases = mc.tampered(m, some) + mc.tampered(m, absent)[1:]
    for cap in {tuple(map(tuple, c[3])) for c in cases}:          # one batch per cap
        batch = [c for c in cases if tuple(map(tuple, c[3])) == cap]
        got = gpu.merkle_map.verify_batch([c[1] for c in batch], D, [c[2] for c in batch], batch[0][3])
        twin = gpu.merkle_map.verify_batch([c[1] for c in batch], D, [c[2] for c in batch], batch[0][3], device=None)
        assert got == twin == [c[4] for c in batch], [c[0] for c in batch]


class Rows:
    """a [n][stride] matrix on the device, filled with a pattern, that get_batch_device writes into"""

    def __init__(self, dev, n, stride):
        self.dev, self.n, self.stride = dev, n, stride
        self.fill = [FILL + i for i in range(max(n * stride, 1))]
        self.d = dev.put(self.fill)
        self.d_st = dev.put([0x7777777777777777] * ((n + 1) // 2))

    def read(self):
        return self.dev.get(self.d, len(self.fill)), self.dev.get(self.d_st, self.n, C.c_int)


@pytest.mark.parametrize("name", ("D1 h1 both", "D8 h0 255", "D13 h0 4096", "D64 h4 257 set", "D64 h4 clustered", "D64 h0 empty"))
def test_device_pointer_forms(gpu, dev, name):
    """from_device builds what the host form builds; a strided get_batch_device writes its three fields and nothing else; a key
    out of range is status 2 and its row stays; verify_batch_device accepts what came out"""
    _, D, h, V, keys = BY_NAME[name]
    m = mc.model(keys, D, h, V)
    d_keys, d_vals = dev.put(list(keys)), dev.put([w for k in keys for w in m.entries[k]])
    mm = gpu.MerkleMap.from_device(d_keys.value, d_vals.value, len(keys), V, D, h)
    q = queries(D, keys, 1)
    out_of_range = ((1 << 64) - 1, P) if D == 64 else (1 << D, (1 << 63) + 1)
    q = q[:1] + [out_of_range[0]] + q[1:] + [out_of_range[1]]
    bad = {1, len(q) - 1}
    depth = D - h
    stride, p_off, v_off, s_off = 4 * depth + V + 9, 2, 4, V + 7
    rows = Rows(dev, len(q), stride)
    d_q = dev.put(q)
    mm.get_batch_device(d_q.value, len(q), rows.d.value, stride, p_off, v_off, s_off, rows.d_st.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    mat, st = rows.read()
    want = list(rows.fill)
    for j, k in enumerate(q):
        if j in bad:
            continue
        present, value, sibs = m.proof(k)
        want[j * stride + p_off] = present
        want[j * stride + v_off:j * stride + v_off + V] = value
        want[j * stride + s_off:j * stride + s_off + 4 * depth] = [w for s in sibs for w in s]
    assert st == [2 if j in bad else 0 for j in range(len(q))]
    assert mat == want
    assert mm.cap == m.cap and len(mm) == len(keys) and mm.hashes == m.hashes
    # verify on the device what the device gave: gather the fields into dense arrays on the host, the bad rows as they are
    flags = [mat[j * stride + p_off] for j in range(len(q))]
    vals = [w for j in range(len(q)) for w in mat[j * stride + v_off:j * stride + v_off + V]]
    sibs = [w for j in range(len(q)) for w in mat[j * stride + s_off:j * stride + s_off + 4 * depth]]
    d_f, d_v, d_s, d_c, d_out = dev.put(flags), dev.put(vals), dev.put(sibs), dev.put([w for e in m.cap for w in e]), dev.alloc(4 * len(q))
    gpu.merkle_map.verify_batch_device(d_q.value, D, d_f.value, d_v.value, V, d_s.value, d_c.value, h, len(q), d_out.value)
    assert dev.H.hipStreamSynchronize(None) == 0
    assert dev.get(d_out, len(q), C.c_int) == [2 if j in bad else 0 for j in range(len(q))]
    for args in ((stride, stride, v_off, s_off), (stride, p_off, stride - V + 1, s_off), (stride, p_off, v_off, stride - 4 * depth + 1), (0, 0, 0, 0)):
        with pytest.raises(gpu.P2Error):
            mm.get_batch_device(d_q.value, len(q), rows.d.value, *args, rows.d_st.value)
    with pytest.raises(gpu.P2Error, match="entry 1"):
        mm.get_batch(q)


def test_the_device_constructor_refuses_bad_entries(gpu, dev):
    keys = list(random_keys(64, 600, 20))
    vals = [mc.value_of(k, 2) for k in keys]
    flat = lambda vs: [w for v in vs for w in v]            # noqa: E731

    def build(ks, vs, D=64):
        d_k, d_v = dev.put(ks), dev.put(flat(vs))
        return gpu.MerkleMap.from_device(d_k.value, d_v.value, len(ks), 2, D, 0)

    gc.collect()
    live = gpu.lib().p2_debug_live_resources()
    dup = list(keys)
    dup[599] = keys[300]                                     # in another workgroup than its twin
    word = [list(v) for v in vals]
    word[511][1] = P
    both = list(dup)
    both[100] = P                                            # the lowest bad entry is named, whatever its kind
    for ks, vs, D, message in ((dup, vals, 64, "entry 599 is a duplicate"), (keys, word, 64, "value word of entry 511"), (both, word, 64, "key of entry 100"),
                               ([1, 2, 1 << 13], vals[:3], 13, "key of entry 2")):
        with pytest.raises(gpu.P2Error, match=message):
            build(ks, vs, D)
        with pytest.raises(gpu.P2Error, match=message):
            gpu.MerkleMap(ks, vs, D, 0)
    for args in (([1], [[1]], 0, 0), ([1], [[1]], 65, 0), ([1], [[1]], 8, 9), ([1], [[1]], 20, 17), ([1], [[1] * 135], 8, 0)):
        with pytest.raises(gpu.P2Error):
            gpu.MerkleMap(*args)
    assert gpu.lib().p2_debug_live_resources() == live       # a refused build leaves no handle and no memory
    mm = build(keys, vals)
    assert len(mm) == 600 and mm.cap == mc.model(tuple(keys), 64, 0, 2).cap


def test_build_and_lookups_on_two_streams_are_ordered_by_the_handle(gpu, dev):
    """the lookups go on another non-blocking stream than the build: nothing but the handle's event orders them"""
    _, D, h, V, keys = BY_NAME["D64 h4 4096"]
    m = mc.model(keys, D, h, V)
    d_keys, d_vals = dev.put(list(keys)), dev.put([w for k in keys for w in m.entries[k]])
    q = queries(D, keys, 2)
    depth = D - h
    stride = 1 + V + 4 * depth
    rows, d_q = Rows(dev, len(q), stride), dev.put(q)
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert dev.H.hipStreamCreateWithFlags(C.byref(s), C.c_uint(1)) == 0        # hipStreamNonBlocking
    try:
        mm = gpu.MerkleMap.from_device(d_keys.value, d_vals.value, len(keys), V, D, h, stream=streams[0])
        mm.get_batch_device(d_q.value, len(q), rows.d.value, stride, 0, 1, 1 + V, rows.d_st.value, stream=streams[1])
        assert dev.H.hipStreamSynchronize(streams[1]) == 0
        mat, st = rows.read()
        assert st == [0] * len(q)
        assert [mat[j * stride:(j + 1) * stride] for j in range(len(q))] == [[p[0]] + p[1] + [w for s in p[2] for w in s] for p in map(m.proof, q)]
        assert mm.cap == m.cap
    finally:
        for s in streams:
            dev.H.hipStreamSynchronize(s)
            dev.H.hipStreamDestroy(s)


# ------------------------------------------------------------------ end to end: a nullifier set
class Spend:
    """nf = hash(secret | note)[0] is not in the set with root old_root, and new_root is the set with it; both roots public.
    `spent` takes the presence word the map's lookup writes and is tied to zero."""

    def __init__(self, pkg, public=True, split=True):
        b = pkg.CircuitBuilder()
        self.secret, self.note = b.add_virtual_target(), b.add_virtual_target()
        nf = b.hash_n_to_m_no_pad([self.secret, self.note], 1)[0]
        # split = False: the key bits are inputs.  The CPU oracle does not know split_le's LIMB op, so the
        # circuit it proves for the byte-for-byte comparison is the hash and the insert walk without the decomposition between them
        self.bits = None if split else b.add_virtual_target_arr(64)
        bits = b.split_le(nf, 64) if split else self.bits
        self.old_root = b.add_virtual_hash()
        self.sibs = [b.add_virtual_hash() for _ in range(64)]
        self.spent = b.add_virtual_target()
        b.connect(self.spent, b.zero())
        self.new_root = b.merkle_map_insert(bits, [], self.old_root, self.sibs)
        if public:
            b.register_public_inputs(self.old_root + self.new_root)
        self.data = b.build()
        self.sib_t = [t for s in self.sibs for t in s]
        self.targets = [self.secret, self.note] + self.old_root + [self.spent] + self.sib_t

    def witness(self, pkg, secret, note, old_root, siblings):
        pw = pkg.PartialWitness()
        if self.bits is not None:
            pw.set_target_arr(self.bits, [(nullifier(secret, note) >> i) & 1 for i in range(64)])
        pw.set_target_arr([self.secret, self.note, self.spent], [secret, note, 0])
        pw.set_hash_target(self.old_root, old_root)
        for t, s in zip(self.sibs, siblings):
            pw.set_hash_target(t, s)
        return pw.map


def nullifier(secret, note):
    return int(R.poseidon_hasher()[0](np.array([secret, note], dtype=np.uint64))[0])


def test_a_chain_of_four_spends_with_siblings_from_the_device(gpu, orc, dev):
    B = 4
    c = Spend(gpu)
    data = c.data
    assert data.info["degree_bits"] == 8 and data.num_public_inputs == 8
    r = random.Random(31)
    notes = [(r.randrange(P), r.randrange(P)) for _ in range(B)]
    nfs = [nullifier(*n) for n in notes]
    models = [ref.Map({k: [] for k in nfs[:j]}, 64, 0, 0) for j in range(B + 1)]
    maps = [gpu.MerkleMap(nfs[:j], [[]] * j, 64, 0, value_len=0) for j in range(B + 1)]
    assert [m.cap for m in maps] == [m.cap for m in models]
    n_t, col = len(c.targets), len(c.targets) - len(c.sib_t)
    rows = []
    for j in range(B):
        rows += list(notes[j]) + models[j].cap[0] + [gpu.VALUE_UNSET] * (1 + len(c.sib_t))
    # row B: nullifier 1 once more, against the set that already holds it
    rows += list(notes[1]) + models[B].cap[0] + [gpu.VALUE_UNSET] * (1 + len(c.sib_t))
    pb = data.proof_bytes
    d_vals, d_q, d_mst, d_proofs, d_pst = dev.put(rows), dev.put(nfs + [nfs[1]]), dev.alloc(4 * (B + 1)), dev.alloc((B + 1) * pb), dev.alloc(4 * (B + 1))
    s = C.c_void_p()
    assert dev.H.hipStreamCreate(C.byref(s)) == 0
    try:
        for j in range(B + 1):
            maps[j].get_batch_device(d_q.value + 8 * j, 1, d_vals.value + 8 * j * n_t, n_t, col - 1, col, col, d_mst.value + 4 * j, stream=s)
        data.prove_batch_device(c.targets, d_vals.value, d_proofs.value, d_pst.value, B + 1, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    finally:
        dev.H.hipStreamSynchronize(s)
        dev.H.hipStreamDestroy(s)
    assert dev.get(d_mst, B + 1, C.c_int) == [0] * (B + 1) and dev.get(d_pst, B + 1, C.c_int) == [0] * B + [1]
    mat = dev.get(d_vals, (B + 1) * n_t)
    for j in range(B):
        assert mat[j * n_t + col - 1:(j + 1) * n_t] == [0] + [w for h in models[j].proof(nfs[j])[2] for w in h]
    assert mat[B * n_t + col - 1] == 1
    host = C.create_string_buffer((B + 1) * pb)
    assert dev.H.hipMemcpy(host, d_proofs, (B + 1) * pb, D2H) == 0
    proofs = [host.raw[j * pb:(j + 1) * pb] for j in range(B)]
    for j, p in enumerate(proofs):
        data.verify(p)
        assert data.public_inputs(p) == models[j].cap[0] + models[j + 1].cap[0] == maps[j].cap[0] + maps[j + 1].cap[0]
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * B
    cproofs, st = data.compress_batch(proofs)
    assert st == [gpu.VERIFY_OK] * B and all(len(cp) < pb for cp in cproofs)
    assert data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * B
    hasher, vd = R.memoised(R.poseidon_hasher()), data.verifier_data()
    for p in proofs:
        assert R.replay(data.info, vd, p, hasher) is None
    # without public inputs and without split_le (the oracle proves no others; see Spend): byte for byte the oracle's proofs
    plain = Spend(gpu, public=False, split=False)
    ws = [plain.witness(gpu, notes[j][0], notes[j][1], models[j].cap[0], models[j].proof(nfs[j])[2]) for j in range(B)]
    got, st = plain.data.prove_batch(ws + [plain.witness(gpu, notes[1][0], notes[1][1], models[B].cap[0], models[B].proof(nfs[1])[2])])
    assert st == [0] * B + [1]
    oc = orc.OracleCircuit(plain.data.blob)
    assert plain.data.verifier_data() == oc.verifier_data()
    for j in (0, B - 1):
        st_o, want = oc.prove(ws[j])
        assert st_o == 0 and got[j] == want, "proof %d differs from the oracle's" % j
