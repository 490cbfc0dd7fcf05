"""An independent AES-GCM with additional authenticated data in plain Python: FIPS-197 for the block cipher, SP 800-38D for the
mode, GF(2^128) on Python integers.  Nothing of the library is used; tests/test_gcm_host.py pins it on published vectors.
96-bit nonces and 16-byte tags only, as the library."""


def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = _xtime(a), b >> 1
    return r


def _make_sbox():
    # FIPS-197 5.1.1: the multiplicative inverse in GF(2^8) (0 -> 0), then the affine map
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    box = []
    for a in range(256):
        x = inv[a]
        y = x
        for s in range(1, 5):
            y ^= ((x << s) | (x >> (8 - s))) & 0xFF
        box.append(y ^ 0x63)
    return box


SBOX = _make_sbox()


def key_expansion(key):
    nk = len(key) // 4
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return w


def encrypt_block(w, block):
    nr = len(w) // 4 - 1
    s = [[block[r + 4 * c] for c in range(4)] for r in range(4)]  # s[row][col]

    def add_round_key(rnd):
        for r in range(4):
            for c in range(4):
                s[r][c] ^= w[4 * rnd + c][r]

    add_round_key(0)
    for rnd in range(1, nr + 1):
        s = [[SBOX[s[r][(c + r) % 4]] for c in range(4)] for r in range(4)]  # SubBytes and ShiftRows
        if rnd < nr:
            for c in range(4):
                a = [s[r][c] for r in range(4)]
                for r in range(4):
                    s[r][c] = _gmul(a[r], 2) ^ _gmul(a[(r + 1) % 4], 3) ^ a[(r + 2) % 4] ^ a[(r + 3) % 4]
        add_round_key(rnd)
    return bytes(s[r][c] for c in range(4) for r in range(4))


_R = 0xE1 << 120


def gf128_mul(x, y):
    """SP 800-38D algorithm 1 on integers whose most significant bit is the first bit of the block"""
    z, v = 0, y
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


def ghash(h, data):
    assert len(data) % 16 == 0
    hi, y = int.from_bytes(h, "big"), 0
    for i in range(0, len(data), 16):
        y = gf128_mul(y ^ int.from_bytes(data[i:i + 16], "big"), hi)
    return y.to_bytes(16, "big")


def _gctr(w, icb, data):
    out, ctr = bytearray(), int.from_bytes(icb[12:], "big")
    for i in range(0, len(data), 16):
        ks = encrypt_block(w, icb[:12] + ctr.to_bytes(4, "big"))
        out += bytes(a ^ b for a, b in zip(data[i:i + 16], ks))
        ctr = (ctr + 1) & 0xFFFFFFFF
    return bytes(out)


def _pad(data):
    return data + bytes(-len(data) % 16)


def _tag(w, nonce, aad, ct):
    h = encrypt_block(w, bytes(16))
    s = ghash(h, _pad(aad) + _pad(ct) + (8 * len(aad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big"))
    return _gctr(w, nonce + b"\x00\x00\x00\x01", s)


def encrypt(key, nonce, pt, aad=b""):
    """-> (ct, tag)"""
    key, nonce, pt, aad = bytes(key), bytes(nonce), bytes(pt), bytes(aad)
    assert len(key) in (16, 24, 32) and len(nonce) == 12
    w = key_expansion(key)
    ct = _gctr(w, nonce + b"\x00\x00\x00\x02", pt)
    return ct, _tag(w, nonce, aad, ct)


def decrypt(key, nonce, ct, tag, aad=b""):
    """-> the plaintext, or None when the tag does not match"""
    key, nonce, ct, aad = bytes(key), bytes(nonce), bytes(ct), bytes(aad)
    w = key_expansion(key)
    if _tag(w, nonce, aad, ct) != bytes(tag):
        return None
    return _gctr(w, nonce + b"\x00\x00\x00\x02", ct)
