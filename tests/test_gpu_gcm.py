"""AES-GCM in GPU batches, and additional authenticated data inside the circuit, on the GPU.

Kernels: k_gcm_setup, k_gcm_ctr (both instantiations), k_gcm_ghash<1> and <64>, k_aes_encrypt_blocks, k_bytes_to_words.  The block
cipher and GHASH alone are held to the host's p2_native_aes_encrypt_block and p2_native_ghash (GHASH at both lane counts at the
block counts where the lane striding and the owed powers of H change); the batch calls to tests/gcm_ref.py (plain Python,
nothing of the library) on 12 items per shape and to the host twins at counts 1, 63, 64, 65 and 257 with two rejected items, and
on 65 537-byte messages, which take the wide GHASH through the public call.  The device forms run on buffers with guard words
behind every output, on the aligned and the byte-access path, on a stream of the caller's.  Circuit: four items encrypted under a
13-byte aad, the aad circuit proven from a host assignment and from device memory through bytes_to_words_device, both verifiers,
compression, the replay of tests/proof_ref.py and the CPU oracle's proof bytes.  Everything compared is exact."""
import ctypes as C
import random

import pytest

import gcm_circuits as K
import gcm_ref
import proof_ref as R
from test_gpu_merkle import D2H, H2D, Device
from test_gpu_schnorr import Stream

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257)
GUARD = 0x5A
P2_ERR_INVALID = 1


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


def rnd(r, n):
    return bytes(r.randrange(256) for _ in range(n))


def items(seed, n, nk, l, al):
    r = random.Random(seed)
    return [rnd(r, 4 * nk) for _ in range(n)], [rnd(r, 12) for _ in range(n)], [rnd(r, l) for _ in range(n)], [rnd(r, al) for _ in range(n)]


def flip(b, byte, bit=0):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def put_bytes(dev, data, offset=0):
    """device copy of `data`, `offset` bytes into an allocation (offset 0: 256-byte aligned, as hipMalloc gives it)"""
    base = dev.alloc(len(data) + offset + 16)
    p = C.c_void_p(base.value + offset)
    if data:
        assert dev.H.hipMemcpy(p, bytes(data), len(data), H2D) == 0
    return p


def get_bytes(dev, p, n):
    out = C.create_string_buffer(max(n, 1))
    if n:
        assert dev.H.hipMemcpy(out, p, n, D2H) == 0
    return out.raw[:n]


# ------------------------------------------------------------------ the block cipher and GHASH alone
@pytest.mark.parametrize("nk", (4, 6, 8))
def test_block_cipher_equals_the_host(gpu, nk):
    r = random.Random(nk)
    fips = (bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"), bytes.fromhex("3243f6a8885a308d313198a2e0370734"), bytes.fromhex("3925841d02dc09fbdc118597196a0b32"))
    for count in (1, 64, 65):
        keys, blocks = [rnd(r, 4 * nk) for _ in range(count)], [rnd(r, 16) for _ in range(count)]
        if nk == 4:
            keys[count - 1], blocks[count - 1] = fips[:2]
        out = C.create_string_buffer(16 * count)
        assert gpu.lib().p2_gpu_aes_encrypt_blocks(b"".join(keys), nk, b"".join(blocks), count, out, 0) == 0, gpu.lib().p2_last_error()
        want = [gpu.native.encrypt_block(k, b) for k, b in zip(keys, blocks)]
        assert [out.raw[16 * i:16 * i + 16] for i in range(count)] == want
        if nk == 4:
            assert want[count - 1] == fips[2]                                # FIPS-197 appendix B
    assert gpu.lib().p2_gpu_aes_encrypt_blocks(bytes(20), 5, bytes(16), 1, out, 0) == P2_ERR_INVALID


@pytest.mark.parametrize("lanes", (1, 64))
@pytest.mark.parametrize("blocks", (1, 2, 63, 64, 65, 127, 128, 129))
def test_ghash_kernels_equal_the_host(gpu, lanes, blocks):
    r = random.Random(blocks)
    hs = [bytes(16), b"\x80" + bytes(15), rnd(r, 16)]                        # h = 0, h = 1 || 0^127 (the field's one), a random h
    xs = [b"\xff" * (16 * blocks), rnd(r, 16 * blocks), rnd(r, 16 * blocks)]
    for rot in range(3):                                                     # every h meets every kind of input
        h3, x3 = hs, xs[rot:] + xs[:rot]
        out = C.create_string_buffer(48)
        assert gpu.lib().p2_gpu_gcm_ghash(b"".join(h3), b"".join(x3), blocks, 3, lanes, out, 0) == 0, gpu.lib().p2_last_error()
        assert [out.raw[16 * i:16 * i + 16] for i in range(3)] == [gpu.native.ghash(h, x) for h, x in zip(h3, x3)]
    assert gpu.lib().p2_gpu_gcm_ghash(bytes(16), bytes(16), 1, 1, 2, out, 0) == P2_ERR_INVALID


# ------------------------------------------------------------------ against the reference and the twins
@pytest.fixture(scope="module")
def reference():
    """(nk, len, aad_len) -> (keys, nonces, pts, aads, [(ct, tag)]) of tests/gcm_ref.py, computed once"""
    out = {}
    for nk in (4, 8):
        for l in (0, 1, 15, 16, 17, 33):
            for al in (0, 13, 17):
                it = items(1000 * nk + 50 * l + al, 12, nk, l, al)
                out[nk, l, al] = it + ([gcm_ref.encrypt(*a) for a in zip(*it)],)
    return out


@pytest.mark.parametrize("nk", (4, 8))
@pytest.mark.parametrize("l", (0, 1, 15, 16, 17, 33))
def test_both_directions_equal_the_reference(gpu, reference, nk, l):
    for al in (0, 13, 17):
        keys, ivs, pts, aads, want = reference[nk, l, al]
        cts, tags = [w[0] for w in want], [w[1] for w in want]
        assert gpu.native.gcm_encrypt_batch(keys, ivs, pts, aads) == (cts, tags, [0] * 12), (l, al)
        assert gpu.native.gcm_decrypt_batch(keys, ivs, cts, tags, aads) == (pts, [0] * 12), (l, al)
        if al == 0:
            assert gpu.native.gcm_encrypt_batch(keys, ivs, pts) == (cts, tags, [0] * 12)      # aads=None is no aad


@pytest.mark.parametrize("l", (13, 16, 48))
def test_counts_against_the_host_twins(gpu, l):
    keys, ivs, pts, aads = items(l, 257, 6, l, 5)
    want = gpu.native.gcm_encrypt_batch(keys, ivs, pts, aads, device=None)
    tags, bad_aads = list(want[1]), list(aads)
    tags[62] = flip(tags[62], 15, 7)                                         # a wrong tag beside a block's last lane
    bad_aads[64] = flip(aads[64], 4, 2)                                      # a flipped aad bit at a block's first lane
    back = gpu.native.gcm_decrypt_batch(keys, ivs, want[0], tags, bad_aads, device=None)
    assert back[1] == [1 if i in (62, 64) else 0 for i in range(257)]
    assert back[0][62] == back[0][64] == bytes(l) and back[0][63] == pts[63] and back[0][65] == pts[65]
    for count in COUNTS:
        assert gpu.native.gcm_encrypt_batch(keys[:count], ivs[:count], pts[:count], aads[:count]) == tuple(w[:count] for w in want), count
        assert gpu.native.gcm_decrypt_batch(keys[:count], ivs[:count], want[0][:count], tags[:count], bad_aads[:count]) == (back[0][:count], back[1][:count]), count


def test_long_messages_take_the_wide_ghash(gpu):
    l = 65537                                                                # 4097 blocks, the last of one byte
    keys, ivs, pts, aads = items(7, 3, 4, l, 13)
    want = gpu.native.gcm_encrypt_batch(keys, ivs, pts, aads, device=None)
    assert gpu.native.gcm_encrypt_batch(keys, ivs, pts, aads) == want
    tags = [want[1][0], flip(want[1][1], 0), want[1][2]]
    assert gpu.native.gcm_decrypt_batch(keys, ivs, want[0], tags, aads) == ([pts[0], bytes(l), pts[2]], [0, 1, 0])


# ------------------------------------------------------------------ the device forms
@pytest.mark.parametrize("l,stride,offset", [(13, 13, 0), (13, 16, 0), (48, 48, 0), (48, 48, 4), (33, 48, 0), (33, 40, 0)])
def test_device_forms_with_guards_on_a_stream(gpu, dev, l, stride, offset):
    """(13, 13): the byte-access path of a contiguous row; stride 16 * ceil(l / 16) on an aligned base: the 128-bit path;
    offset 4: a misaligned base; stride 40: a stride that is no multiple of 16"""
    n, nk, al = 65, 4, 13
    keys, ivs, pts, aads = items(l + stride + offset, n, nk, l, al)
    cts, tags, _ = gpu.native.gcm_encrypt_batch(keys, ivs, pts, aads, device=None)
    bad_tags = list(tags)
    bad_tags[64] = flip(tags[64], 8)
    rows = lambda data: b"".join(d + bytes([GUARD]) * (stride - l) for d in data)        # noqa: E731
    guard = bytes([GUARD]) * (stride - l)
    d_key, d_iv, d_aad = put_bytes(dev, b"".join(keys)), put_bytes(dev, b"".join(ivs)), put_bytes(dev, b"".join(aads))
    d_pt = put_bytes(dev, rows(pts), offset)
    d_ct, d_back = put_bytes(dev, bytes([GUARD]) * (stride * n + 64), offset), put_bytes(dev, bytes([GUARD]) * (stride * n + 64), offset)
    d_tag, d_bad = put_bytes(dev, bytes([GUARD]) * (16 * n + 64)), put_bytes(dev, b"".join(bad_tags))
    d_st = [put_bytes(dev, bytes([GUARD]) * (4 * n + 64)) for _ in range(2)]
    ws = gpu.native.gcm_batch_workspace(nk, l, al, n)
    d_work = put_bytes(dev, bytes([GUARD]) * (ws + 64))
    with Stream(dev) as s:
        gpu.native.gcm_encrypt_batch_device(d_key.value, nk, d_iv.value, d_aad.value, al, d_pt.value, l, stride, n, d_ct.value, d_tag.value, d_st[0].value, d_work.value, stream=s)
        gpu.native.gcm_decrypt_batch_device(d_key.value, nk, d_iv.value, d_aad.value, al, d_ct.value, d_bad.value, l, stride, n, d_back.value, d_st[1].value, d_work.value, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    tail = bytes([GUARD]) * 64
    assert get_bytes(dev, d_ct, stride * n + 64) == b"".join(c + guard for c in cts) + tail          # the bytes between rows untouched
    assert get_bytes(dev, d_tag, 16 * n + 64) == b"".join(tags) + tail
    assert get_bytes(dev, d_back, stride * n + 64) == b"".join((p if i != 64 else bytes(l)) + guard for i, p in enumerate(pts)) + tail
    assert get_bytes(dev, d_work, ws + 64)[ws:] == tail
    for k, want in enumerate(([0] * n, [0] * 64 + [1])):
        raw = get_bytes(dev, d_st[k], 4 * n + 64)
        assert [int.from_bytes(raw[4 * i:4 * i + 4], "little") for i in range(n)] == want and raw[4 * n:] == tail


@pytest.mark.parametrize("row_bytes,byte_stride,stride_words", [(13, 13, 13), (13, 16, 77), (16, 16, 20)])
def test_bytes_to_words_device(gpu, dev, row_bytes, byte_stride, stride_words):
    n = 65
    data = rnd(random.Random(row_bytes), byte_stride * n)
    d_b, d_out = put_bytes(dev, data), dev.put([7] * (n * stride_words + 4))
    with Stream(dev) as s:
        gpu.native.bytes_to_words_device(d_b.value, row_bytes, byte_stride, n, d_out.value, stride_words, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    want = [v for i in range(n) for v in list(data[byte_stride * i:byte_stride * i + row_bytes]) + [7] * (stride_words - row_bytes)]
    assert dev.get(d_out, n * stride_words + 4) == want + [7] * 4
    with pytest.raises(gpu.P2Error, match="stride_words"):
        gpu.native.bytes_to_words_device(d_b.value, row_bytes, byte_stride, n, d_out.value, row_bytes - 1)
    gpu.native.bytes_to_words_device(d_b.value, row_bytes, byte_stride, 0, d_out.value, stride_words)


def test_shape_errors_come_before_any_launch(gpu, dev):
    lib = gpu.lib()
    d = dev.alloc(4096).value
    st = (C.c_int * 1)()
    buf = C.create_string_buffer(64)
    for nk, al, l, stride, message in ((5, 0, 16, 16, "nk is 4, 6 or 8"), (4, 0, (1 << 24) + 1, 1 << 25, "len is at most 2^24 bytes"),
                                       (4, (1 << 16) + 1, 16, 16, "aad_len is at most 2^16 bytes"), (4, 0, 16, 15, "row_stride is at least len")):
        for fn in (lib.p2_aes_gcm_encrypt_batch_device, lib.p2_aes_gcm_decrypt_batch_device):
            # every pointer but d_work is NULL: a launch, or the null check that follows the shape check, would say so
            args = [None, nk, None, None, al, None] + ([l, stride, 1, None, None, None] if fn is lib.p2_aes_gcm_encrypt_batch_device else [None, l, stride, 1, None, None])
            assert fn(*args, d, 0, None) == P2_ERR_INVALID and lib.p2_last_error().decode() == message
    assert lib.p2_aes_gcm_encrypt_batch(buf, 5, buf, buf, 0, buf, 16, 1, buf, buf, st, 0) == P2_ERR_INVALID
    assert lib.p2_aes_gcm_decrypt_batch(buf, 4, buf, buf, (1 << 16) + 1, buf, buf, 16, 1, buf, st, 0) == P2_ERR_INVALID
    assert lib.p2_aes_gcm_encrypt_batch_device(d, 4, d, d, 0, d, 16, 16, 1, d, d, d, d + 4, 0, None) == P2_ERR_INVALID     # d_work not 16-byte aligned
    assert lib.p2_aes_gcm_encrypt_batch_device(d, 4, d, d, 0, d, 16, 16, 1, d, d, d, None, 0, None) == P2_ERR_INVALID      # no d_work
    assert lib.p2_aes_gcm_encrypt_batch(None, 4, None, None, 0, None, 16, 0, None, None, None, 0) == 0                      # count = 0
    assert gpu.native.gcm_encrypt_batch([], [], []) == ([], [], []) and gpu.native.gcm_decrypt_batch([], [], [], []) == ([], [])


# ------------------------------------------------------------------ the circuit with an aad
B, L, AL = 4, 13, 13


@pytest.fixture(scope="module")
def encrypted(gpu):
    keys, ivs, pts, aads = items(99, B, 4, L, AL)
    cts, tags, st = gpu.native.gcm_encrypt_batch(keys, ivs, pts, aads)
    assert st == [0] * B and list(zip(cts, tags)) == [gcm_ref.encrypt(*a) for a in zip(keys, ivs, pts, aads)]
    return keys, ivs, pts, aads, cts, tags


@pytest.fixture(scope="module")
def proven(gpu, encrypted):
    keys, ivs, pts, aads, cts, tags = encrypted
    data, t = K.gcm_aad(gpu, 4, L, AL)
    maps = [K.inputs(t, k, n, p, a) for k, n, p, a in zip(keys, ivs, pts, aads)]
    maps.append(K.inputs(t, keys[0], ivs[0], pts[0], aads[0], flip(tags[0], 3)))          # a tampered tag
    maps.append(K.inputs(t, keys[1], ivs[1], pts[1], flip(aads[1], 12), tags[1]))        # a tampered aad byte under the right tag
    proofs, st, vals = data.prove_batch(maps, outputs=t.ct + t.tag)
    return data, t, maps, proofs, st, vals


def test_aad_circuit_proves_what_the_batch_encrypted(gpu, encrypted, proven):
    keys, ivs, pts, aads, cts, tags = encrypted
    data, t, maps, proofs, st, vals = proven
    assert data.info["degree_bits"] == 14
    assert st == [0] * B + [1, 1]
    assert [bytes(v) for v in vals[:B]] == [c + g for c, g in zip(cts, tags)]             # the witness computes the kernels' ct and tag
    good = proofs[:B]
    for p in good:
        data.verify(p)
    assert data.verify_batch(good) == [gpu.VERIFY_OK] * B
    cproofs, cst = data.compress_batch(good)
    assert cst == [gpu.VERIFY_OK] * B and all(len(x) < data.proof_bytes for x in cproofs)
    assert data.verify_compressed_batch(cproofs) == [gpu.VERIFY_OK] * B
    back, bst = data.decompress_batch(cproofs)
    assert bst == [gpu.VERIFY_OK] * B and back == good
    for m in maps[B:]:
        f = data.explain(m)
        assert f.kind.endswith("CONFLICT") and f == gpu.host_witness(data.blob, m)[2]


def test_one_aad_proof_replays_and_equals_the_oracles(gpu, orc, proven):
    data, t, maps, proofs = proven[:4]
    assert R.replay(data.info, data.verifier_data(), proofs[0], R.memoised(R.poseidon_hasher()), blob=data.blob) is None
    oc = orc.OracleCircuit(data.blob)
    st, ref = oc.prove(maps[0])
    assert st == 0 and ref == proofs[0]


def test_aad_circuit_from_device_memory(gpu, dev, encrypted, proven):
    """encrypt, bytes_to_words and prove on one stream: key, nonce, plaintext, aad and the computed ciphertext and tag reach the
    prover's value matrix without a host round trip, and the proofs are the host assignment's"""
    keys, ivs, pts, aads, cts, tags = encrypted
    data, t, _, proofs = proven[:4]
    targets = t.key + t.nonce + t.pt + t.aad + t.ct + t.tag
    n_t, pb = len(targets), data.proof_bytes
    assert n_t == 16 + 12 + L + AL + L + 16
    d_key, d_iv, d_aad, d_pt = (put_bytes(dev, b"".join(x)) for x in (keys, ivs, aads, pts))
    d_ct, d_tag, d_st = dev.alloc(L * B), dev.alloc(16 * B), dev.alloc(4 * B)
    d_work = dev.alloc(gpu.native.gcm_batch_workspace(4, L, AL, B))
    d_vals, d_proofs, d_pst = dev.put([gpu.VALUE_UNSET] * (B * n_t)), dev.alloc(B * pb), dev.alloc(4 * B)
    with Stream(dev) as s:
        gpu.native.gcm_encrypt_batch_device(d_key.value, 4, d_iv.value, d_aad.value, AL, d_pt.value, L, L, B, d_ct.value, d_tag.value, d_st.value, d_work.value, stream=s)
        col = 0
        for d_b, w in ((d_key, 16), (d_iv, 12), (d_pt, L), (d_aad, AL), (d_ct, L), (d_tag, 16)):
            gpu.native.bytes_to_words_device(d_b.value, w, w, B, d_vals.value + 8 * col, n_t, stream=s)
            col += w
        data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=s)
        assert dev.H.hipStreamSynchronize(s) == 0
    assert dev.get(d_st, B, C.c_int) == [0] * B and dev.get(d_pst, B, C.c_int) == [0] * B
    assert dev.get(d_vals, B * n_t) == [v for i in range(B) for v in keys[i] + ivs[i] + pts[i] + aads[i] + cts[i] + tags[i]]
    got = get_bytes(dev, d_proofs, B * pb)
    assert [got[k * pb:(k + 1) * pb] for k in range(B)] == proofs[:B]
