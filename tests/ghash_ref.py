"""GHASH from carry-less multiply tables, restated in plain Python: the two byte tables, the bit-serial multiplication of
NIST SP 800-38D (the algorithm the reference's circuit spells out), the table multiplication with its 32-byte accumulator and
its fold, and GHASH with lanes.  Test-side only; csrc/aes_gadgets.h derives the same things a second time.

GCM's bit order: bit i of a block is bit 7 - i % 8 of byte i / 8 and the coefficient of x^i, so a byte B stands for the
polynomial whose plain-integer form is rev8(B)."""


def rev8(b):
    return int("{:08b}".format(b)[::-1], 2)


def clmul(a, b):
    r = 0
    for i in range(8):
        if (b >> i) & 1:
            r ^= a << i
    return r


def tables():
    lo, hi = [0] * 65536, [0] * 65536
    for a in range(256):
        ra = rev8(a)
        for b in range(256):
            c = clmul(ra, rev8(b))
            lo[a << 8 | b] = rev8(c & 255)
            hi[a << 8 | b] = rev8(c >> 8)
    return lo, hi


LO, HI = tables()


def gf_mul_bit_serial(x, y):
    """SP 800-38D algorithm 1 on 16-byte strings: Z <- Z ^ V where bit i of x is set, V <- V >> 1, ^ R where a bit fell out."""
    z, v = 0, int.from_bytes(bytes(y), "big")
    xi = int.from_bytes(bytes(x), "big")
    for i in range(128):
        if (xi >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xE1 << 120 if v & 1 else 0)
    return z.to_bytes(16, "big")


def accumulate(d, x, y):
    """d[0..31] ^= x * y, unreduced: the low byte of x[p] * y[q] at position p + q, the high byte at p + q + 1"""
    for p in range(16):
        for q in range(16):
            i = x[p] << 8 | y[q]
            d[p + q] ^= LO[i]
            d[p + q + 1] ^= HI[i]


def fold(d):
    """x^128 = 1 + x + x^2 + x^7, the byte 0xE1: k = 15 writes d[16], which k = 0 reads, so k = 0 goes last"""
    d = list(d)
    for k in list(range(15, 0, -1)) + [0]:
        i = d[16 + k] << 8 | 0xE1
        d[k] ^= LO[i]
        d[k + 1] ^= HI[i]
    return bytes(d[:16])


def gf_mul_tables(x, y):
    d = [0] * 32
    accumulate(d, x, y)
    return fold(d)


def ghash_bit_serial(h, x):
    y = bytes(16)
    for i in range(0, len(x), 16):
        y = gf_mul_bit_serial(bytes(a ^ b for a, b in zip(y, x[i:i + 16])), h)
    return y


def ghash_lanes(h, x, lanes):
    """y <- (y ^ x_1) h^k ^ x_2 h^(k-1) ^ .. ^ x_k h per group of k = lanes blocks (a last group of r < k: h^r .. h), all
    products of a group in one accumulator with one fold."""
    assert len(x) % 16 == 0 and 1 <= lanes <= 16
    blocks = [bytes(x[i:i + 16]) for i in range(0, len(x), 16)]
    pw = [None, bytes(h)]
    for i in range(2, min(lanes, len(blocks)) + 1):
        pw.append(gf_mul_tables(pw[(i + 1) // 2], pw[i // 2]))
    y = bytes(16)
    for g in range(0, len(blocks), lanes):
        group = blocks[g:g + lanes]
        r = len(group)
        d = [0] * 32
        for j, xj in enumerate(group):
            if j == 0:
                xj = bytes(a ^ b for a, b in zip(y, xj))
            accumulate(d, xj, pw[r - j])
        y = fold(d)
    return y
