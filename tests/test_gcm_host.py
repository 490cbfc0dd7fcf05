"""AES-GCM with additional authenticated data on the CPU: tests/gcm_ref.py (plain Python, nothing of the library) pinned on
published vectors -- the four CAVP vectors of tests/golden/aes_kat.json and McGrew-Viega's test cases 4 and 16 in
tests/golden/gcm_aad_kat.json -- then the host twins native.gcm_encrypt(aad=) and native.gcm_decrypt against it at the edge
lengths, the rejections of authenticated decryption, and the device=None batch forms."""
import itertools
import json
import os
import random

import pytest

import gcm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "aes_kat.json")))["cavp_gcm128"]
AAD_GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "gcm_aad_kat.json")))["vectors"]
LENS = (0, 1, 13, 15, 16, 17, 31, 32, 33)
AAD_LENS = (0, 1, 5, 13, 16, 17, 20)


def rnd(r, n):
    return bytes(r.randrange(256) for _ in range(n))


def shapes():
    """every len and every aad_len with every nk: the two axes walked together, the shorter one cycling"""
    for nk in (4, 6, 8):
        for k in range(max(len(LENS), len(AAD_LENS))):
            yield nk, LENS[k % len(LENS)], AAD_LENS[(k + nk) % len(AAD_LENS)]


def test_shapes_cover_every_value_with_every_key_size():
    for nk in (4, 6, 8):
        assert {l for n, l, a in shapes() if n == nk} == set(LENS) and {a for n, l, a in shapes() if n == nk} == set(AAD_LENS)


# ------------------------------------------------------------------------------------------ the reference on published vectors
def test_reference_on_the_no_aad_vectors():
    assert len(GOLD) == 4
    for v in GOLD:
        key, iv, pt, ct, tag = (bytes.fromhex(v[k]) for k in ("key", "iv", "pt", "ct", "tag"))
        assert gcm_ref.encrypt(key, iv, pt) == (ct, tag)
        assert gcm_ref.decrypt(key, iv, ct, tag) == pt


def test_reference_on_the_aad_vectors():
    assert [len(bytes.fromhex(v["key"])) for v in AAD_GOLD] == [16, 32]
    for v in AAD_GOLD:
        key, iv, aad, pt, ct, tag = (bytes.fromhex(v[k]) for k in ("key", "iv", "aad", "pt", "ct", "tag"))
        assert len(pt) == 60 and len(aad) == 20
        assert gcm_ref.encrypt(key, iv, pt, aad) == (ct, tag)
        assert gcm_ref.decrypt(key, iv, ct, tag, aad) == pt
        assert gcm_ref.decrypt(key, iv, ct, tag, aad[:-1] + b"\x00") is None


def test_reference_sbox_is_fips197():
    assert gcm_ref.SBOX[0x00] == 0x63 and gcm_ref.SBOX[0x53] == 0xED and sorted(gcm_ref.SBOX) == list(range(256))


# ------------------------------------------------------------------------------------------ the host twins
def test_host_twins_on_the_published_vectors(pkg):
    for v in GOLD:
        key, iv, pt, ct, tag = (bytes.fromhex(v[k]) for k in ("key", "iv", "pt", "ct", "tag"))
        assert pkg.native.gcm_encrypt(key, iv, pt) == (ct, tag)            # without aad: the old output
        assert pkg.native.gcm_encrypt(key, iv, pt, aad=b"") == (ct, tag)
        assert pkg.native.gcm_decrypt(key, iv, ct, tag) == pt
    for v in AAD_GOLD:
        key, iv, aad, pt, ct, tag = (bytes.fromhex(v[k]) for k in ("key", "iv", "aad", "pt", "ct", "tag"))
        assert pkg.native.gcm_encrypt(key, iv, pt, aad) == (ct, tag)
        assert pkg.native.gcm_decrypt(key, iv, ct, tag, aad) == pt


def test_aad_len_zero_entry_equals_the_old_entry(pkg):
    import ctypes as C
    r = random.Random(11)
    for nk, l in itertools.product((4, 6, 8), LENS):
        key, iv, pt = rnd(r, 4 * nk), rnd(r, 12), rnd(r, l)
        old = (C.create_string_buffer(max(l, 1)), C.create_string_buffer(16))
        new = (C.create_string_buffer(max(l, 1)), C.create_string_buffer(16))
        pkg.lib().p2_native_aes_gcm_encrypt(key, nk, nk + 6, iv, pt, l, *old)
        pkg.lib().p2_native_aes_gcm_encrypt_aad(key, nk, nk + 6, iv, None, 0, pt, l, *new)
        assert old[0].raw == new[0].raw and old[1].raw == new[1].raw


@pytest.mark.parametrize("nk,l,al", list(shapes()))
def test_host_twins_equal_the_reference(pkg, nk, l, al):
    r = random.Random(1000 * nk + 37 * l + al)
    key, iv, pt, aad = rnd(r, 4 * nk), rnd(r, 12), rnd(r, l), rnd(r, al)
    ct, tag = gcm_ref.encrypt(key, iv, pt, aad)
    assert pkg.native.gcm_encrypt(key, iv, pt, aad) == (ct, tag)
    assert pkg.native.gcm_decrypt(key, iv, ct, tag, aad) == pt              # decrypt inverts encrypt


def flip(b, byte, bit=0):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("nk", (4, 6, 8))
def test_decrypt_rejects_one_flipped_bit_anywhere(pkg, nk):
    r = random.Random(nk)
    key, iv, pt, aad = rnd(r, 4 * nk), rnd(r, 12), rnd(r, 33), rnd(r, 13)
    ct, tag = pkg.native.gcm_encrypt(key, iv, pt, aad)
    assert pkg.native.gcm_decrypt(key, iv, ct, tag, aad) == pt
    tampered = [(key, iv, flip(ct, 32, 7), tag, aad), (key, iv, ct, flip(tag, 0), aad), (key, iv, ct, tag, flip(aad, 12, 3)),
                (key, flip(iv, 11), ct, tag, aad), (flip(key, 4 * nk - 1, 5), iv, ct, tag, aad),
                (key, iv, ct, flip(tag, 15, 7), aad),                      # the only wrong byte is the last one
                (key, iv, ct, tag, aad + b"\x00"), (key, iv, ct, tag, b"")]
    for k, n, c, t, a in tampered:
        assert gcm_ref.decrypt(k, n, c, t, a) is None
        with pytest.raises(pkg.P2Error, match="authentication failed"):
            pkg.native.gcm_decrypt(k, n, c, t, a)


def test_rejected_plaintext_is_zeroed(pkg):
    import ctypes as C
    key, iv, pt = bytes(range(16)), bytes(12), bytes(range(40))
    ct, tag = pkg.native.gcm_encrypt(key, iv, pt, b"hdr")
    out = C.create_string_buffer(b"\xaa" * 40, 40)
    assert pkg.lib().p2_native_aes_gcm_decrypt(key, 4, 10, iv, b"hdr", 3, ct, 40, flip(tag, 7), out) == 1
    assert out.raw == bytes(40)
    assert pkg.lib().p2_native_aes_gcm_decrypt(key, 4, 10, iv, b"hdr", 3, ct, 40, tag, out) == 0 and out.raw == pt


def test_empty_message_authenticates_the_aad_alone(pkg):
    key, iv = bytes(range(32)), bytes(range(12))
    ct, tag = pkg.native.gcm_encrypt(key, iv, b"", b"header only")
    assert ct == b"" and (ct, tag) == gcm_ref.encrypt(key, iv, b"", b"header only")
    assert tag != pkg.native.gcm_encrypt(key, iv, b"")[1]
    assert pkg.native.gcm_decrypt(key, iv, b"", tag, b"header only") == b""
    with pytest.raises(pkg.P2Error):
        pkg.native.gcm_decrypt(key, iv, b"", tag, b"header 0nly")


# ------------------------------------------------------------------------------------------ device=None batches
def batch(r, n, nk, l, al):
    return [rnd(r, 4 * nk) for _ in range(n)], [rnd(r, 12) for _ in range(n)], [rnd(r, l) for _ in range(n)], [rnd(r, al) for _ in range(n)]


@pytest.mark.parametrize("nk,l,al", [(4, 13, 13), (6, 0, 5), (8, 33, 0)])
def test_host_batches(pkg, nk, l, al):
    keys, ivs, pts, aads = batch(random.Random(l), 5, nk, l, al)
    cts, tags, st = pkg.native.gcm_encrypt_batch(keys, ivs, pts, aads if al else None, device=None)
    assert st == [0] * 5
    assert list(zip(cts, tags)) == [gcm_ref.encrypt(*a) for a in zip(keys, ivs, pts, aads)]
    bad_tags = list(tags)
    bad_tags[1] = flip(tags[1], 15)
    bad_aads = list(aads)
    if al:
        bad_aads[3] = flip(aads[3], 0)
    got, st = pkg.native.gcm_decrypt_batch(keys, ivs, cts, bad_tags, bad_aads if al else None, device=None)
    want_st = [0, 1, 0, 1 if al else 0, 0]
    assert st == want_st
    assert got == [bytes(l) if s else p for s, p in zip(want_st, pts)]       # rejected rows are zero, the others the plaintexts


def test_empty_batches(pkg):
    assert pkg.native.gcm_encrypt_batch([], [], [], device=None) == ([], [], [])
    assert pkg.native.gcm_decrypt_batch([], [], [], [], device=None) == ([], [])


def test_batch_shape_errors(pkg):
    keys, ivs, pts, aads = batch(random.Random(3), 3, 4, 16, 5)
    cts, tags, _ = pkg.native.gcm_encrypt_batch(keys, ivs, pts, aads, device=None)
    for dev in (None, 0):                                                    # raised before any library call, so no GPU is needed
        with pytest.raises(pkg.P2Error, match="one entry per item"):
            pkg.native.gcm_encrypt_batch(keys, ivs[:2], pts, aads, device=dev)
        with pytest.raises(pkg.P2Error, match="one entry per item"):
            pkg.native.gcm_decrypt_batch(keys, ivs, cts, tags[:2], aads, device=dev)
        with pytest.raises(pkg.P2Error, match="one entry per item"):
            pkg.native.gcm_encrypt_batch(keys, ivs, pts, aads[:1], device=dev)
        with pytest.raises(pkg.P2Error, match="one length"):
            pkg.native.gcm_encrypt_batch(keys, ivs, [pts[0], pts[1], pts[2][:15]], aads, device=dev)
        with pytest.raises(pkg.P2Error, match="one length"):
            pkg.native.gcm_encrypt_batch([keys[0], keys[1], keys[2] + bytes(8)], ivs, pts, aads, device=dev)
        with pytest.raises(pkg.P2Error, match="nk is 4, 6 or 8"):
            pkg.native.gcm_encrypt_batch([k[:12] for k in keys], ivs, pts, aads, device=dev)
        with pytest.raises(pkg.P2Error, match="12 bytes"):
            pkg.native.gcm_encrypt_batch(keys, [n + b"\x00" for n in ivs], pts, aads, device=dev)
        with pytest.raises(pkg.P2Error, match="12 bytes"):
            pkg.native.gcm_decrypt_batch(keys, ivs, cts, [t[:15] for t in tags], aads, device=dev)
    with pytest.raises(pkg.P2Error, match="nk is 4, 6 or 8"):
        pkg.native.gcm_batch_workspace(5, 16, 0, 1)
    assert pkg.native.gcm_batch_workspace(4, 16, 0, 0) == 0 and pkg.native.gcm_batch_workspace(8, 1 << 20, 13, 3) % 16 == 0
    assert pkg.lib().p2_aes_gcm_batch_workspace(5, 16, 0, 1) == 0


# ------------------------------------------------------------------------------------------ the C entries' argument contract
NEW_ENTRIES = ("p2_native_aes_gcm_encrypt_aad", "p2_native_aes_gcm_decrypt", "p2_aes_gcm_build_aad", "p2_aes_gcm_batch_workspace", "p2_aes_gcm_encrypt_batch",
               "p2_aes_gcm_decrypt_batch", "p2_aes_gcm_encrypt_batch_device", "p2_aes_gcm_decrypt_batch_device", "p2_bytes_to_words_device", "p2_gpu_gcm_ghash",
               "p2_gpu_aes_encrypt_blocks", "p2_gpu_gcm_kernel_times")
DEVICE_ERRORS = ((2, "no HIP device available"), (1, "device index out of range"))       # P2_ERR_NO_DEVICE, P2_ERR_INVALID


def test_entry_points_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "p2aes.h")).read()
    for f in NEW_ENTRIES:
        assert f in pkg.lib()._p2_signatures and hasattr(pkg.lib(), f) and f + "(" in header, f


def test_batch_argument_contract_without_a_device(pkg):
    """every call names device -1: the shape error comes first, then an empty batch is accepted with NULL pointers, then a NULL
    pointer is "null argument", and only then is the device looked at -- nothing is launched"""
    import ctypes as C
    L = pkg.lib()
    b, st = C.create_string_buffer(4096), (C.c_int * 4)()
    w = C.cast(b, C.c_void_p)

    def enc(nk=4, al=5, l=16, n=1, key=b, work_dev=w, stride=16):
        host = (L.p2_aes_gcm_encrypt_batch(key, nk, b, b, al, b, l, n, b, b, st, -1), L.p2_last_error().decode())
        d = C.cast(key, C.c_void_p) if key is not None else None
        dev = (L.p2_aes_gcm_encrypt_batch_device(d, nk, w, w, al, w, l, stride, n, w, w, w, work_dev, -1, None), L.p2_last_error().decode())
        return host, dev

    def dec(nk=4, al=5, l=16, n=1, tag=b, stride=16):
        host = (L.p2_aes_gcm_decrypt_batch(b, nk, b, b, al, b, tag, l, n, b, st, -1), L.p2_last_error().decode())
        d = C.cast(tag, C.c_void_p) if tag is not None else None
        dev = (L.p2_aes_gcm_decrypt_batch_device(w, nk, w, w, al, w, d, l, stride, n, w, w, w, -1, None), L.p2_last_error().decode())
        return host, dev

    for call in (enc, dec):
        for kw, message in (({"nk": 5}, "nk is 4, 6 or 8"), ({"nk": 0}, "nk is 4, 6 or 8"), ({"l": (1 << 24) + 1, "stride": 1 << 25}, "len is at most 2^24 bytes"),
                            ({"al": (1 << 16) + 1}, "aad_len is at most 2^16 bytes")):
            for n in (0, 1):                                                  # the shape check comes before the empty return
                assert call(n=n, **kw) == ((1, message),) * 2, (kw, n)
        assert call(stride=15)[1] == (1, "row_stride is at least len")
        assert [r[0] for r in call(n=0)] == [0, 0]
        assert all(r in DEVICE_ERRORS for r in call()) and all(r in DEVICE_ERRORS for r in call(l=0, al=0, stride=0))
        assert all(r in DEVICE_ERRORS for r in call(l=1 << 24, stride=1 << 24, al=1 << 16, nk=8))      # the limits themselves pass
    assert enc(key=None) == ((1, "null argument"),) * 2 and dec(tag=None) == ((1, "null argument"),) * 2
    assert enc(work_dev=None)[1] == (1, "null argument")                       # the host form sizes its own workspace, the device form is given one
    assert enc(work_dev=C.c_void_p(w.value + 4))[1] == (1, "d_work is 16-byte aligned")
    assert L.p2_aes_gcm_encrypt_batch(None, 4, None, None, 0, None, 16, 0, None, None, None, -1) == 0
    assert (L.p2_bytes_to_words_device(w, 13, 13, 1, w, 12, -1, None), L.p2_last_error().decode()) == (1, "stride_words is at least row_bytes")
    assert L.p2_bytes_to_words_device(None, 13, 13, 0, None, 13, -1, None) == 0 and L.p2_bytes_to_words_device(w, 0, 0, 5, w, 0, -1, None) == 0
    assert (L.p2_bytes_to_words_device(None, 13, 13, 1, w, 13, -1, None), L.p2_last_error().decode()) == (1, "null argument")
    assert (L.p2_bytes_to_words_device(w, 13, 13, 1, w, 13, -1, None), L.p2_last_error().decode()) in DEVICE_ERRORS
    assert (L.p2_gpu_gcm_ghash(b, b, 1, 1, 2, b, -1), L.p2_last_error().decode()) == (1, "lanes is 1 or 64")
    assert (L.p2_gpu_gcm_ghash(b, b, 1, 1, 64, b, -1), L.p2_last_error().decode()) in DEVICE_ERRORS
    assert (L.p2_gpu_aes_encrypt_blocks(b, 7, b, 1, b, -1), L.p2_last_error().decode()) == (1, "nk is 4, 6 or 8")
    assert (L.p2_gpu_aes_encrypt_blocks(b, 8, b, 1, b, -1), L.p2_last_error().decode()) in DEVICE_ERRORS
