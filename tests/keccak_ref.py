"""Keccak-256 (original padding) and the Keccak Merkle trees of hasher="keccak", restated in Python over numpy uint64 arrays:
one array lane per leaf or node, so a tree of 2^17 leaves takes seconds.  Shares no code with csrc/; pinned by the published
vectors Keccak-256("") and Keccak-256("abc") (tests/test_keccak_host.py).

A 25-byte digest is four words holding bytes 0-6, 7-13, 14-20 and 21-24, little-endian."""
import numpy as np

U = np.uint64
RATE = 17  # words


def _round_constants():
    rc, lfsr = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if lfsr & 1:
                c ^= 1 << ((1 << j) - 1)
            lfsr = ((lfsr << 1) ^ 0x171) & 0xFF if lfsr & 0x80 else lfsr << 1
        rc.append(c)
    return rc


RC = _round_constants()


def _rotations():
    rot, x, y = [[0] * 5 for _ in range(5)], 1, 0
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


ROT = _rotations()


def _rotl(v, r):
    return v if r == 0 else (v << U(r)) | (v >> U(64 - r))


def keccak_f(a):
    """a[x][y]: numpy uint64 arrays of one shape; returns the permuted state."""
    for rnd in range(24):
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[None] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rotl(a[x][y], ROT[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] = a[0][0] ^ U(RC[rnd])
    return a


def sponge_words(words):
    """words: uint64 array [..., n] whose last axis is the message as little-endian 8-byte words (n * 8 bytes exactly);
    returns the first four state lanes [..., 4] after absorbing the padded message."""
    words = np.asarray(words, dtype=U)
    n = words.shape[-1]
    blocks = n // RATE + 1
    padded = np.zeros(words.shape[:-1] + (blocks * RATE,), dtype=U)
    padded[..., :n] = words
    padded[..., n] ^= U(0x01)
    padded[..., -1] ^= U(0x80 << 56)
    zero = np.zeros(words.shape[:-1], dtype=U)
    a = [[zero.copy() for _ in range(5)] for _ in range(5)]
    for b in range(blocks):
        for k in range(RATE):
            a[k % 5][k // 5] = a[k % 5][k // 5] ^ padded[..., b * RATE + k]
        a = keccak_f(a)
    return np.stack([a[0][0], a[1][0], a[2][0], a[3][0]], axis=-1)


def keccak256(data):
    """Keccak-256 of a bytes object (any length), as bytes: the byte-level definition, for the published vectors."""
    msg = bytearray(data) + b"\x01"
    msg += b"\0" * (-len(msg) % 136)
    msg[-1] |= 0x80
    a = [[np.zeros((), dtype=U) for _ in range(5)] for _ in range(5)]
    for off in range(0, len(msg), 136):
        for k in range(RATE):
            a[k % 5][k // 5] = a[k % 5][k // 5] ^ U(int.from_bytes(msg[off + 8 * k:off + 8 * k + 8], "little"))
        a = keccak_f(a)
    return b"".join(int(a[x][0]).to_bytes(8, "little") for x in range(4))


M56 = U((1 << 56) - 1)


def pack(lanes):
    """first 25 bytes of the state lanes [..., 4] -> four words of 7, 7, 7, 4 bytes"""
    s0, s1, s2, s3 = (lanes[..., i] for i in range(4))
    return np.stack([s0 & M56, ((s0 >> U(56)) | (s1 << U(8))) & M56, ((s1 >> U(48)) | (s2 << U(16))) & M56,
                     ((s2 >> U(40)) | (s3 << U(24))) & U(0xFFFFFFFF)], axis=-1)


def digest_bytes(h):
    """the 25 bytes of one digest in the four-word form"""
    return b"".join(int(w).to_bytes(8, "little")[:k] for w, k in zip(h, (7, 7, 7, 4)))


def hash_no_pad(words):
    """[..., n] words -> [..., 4] digests"""
    return pack(sponge_words(words))


def two_to_one(l, r):
    """[..., 4] x [..., 4] digests (words in range) -> [..., 4]: Keccak-256 over the 50 bytes, which are not a whole number of
    words: laid out as 6.25 words with the padding byte right behind them."""
    l, r = np.asarray(l, dtype=U), np.asarray(r, dtype=U)
    by = []  # 50 byte planes
    for h in (l, r):
        for i, k in enumerate((7, 7, 7, 4)):
            by += [(h[..., i] >> U(8 * j)) & U(0xFF) for j in range(k)]
    by.append(np.full(l.shape[:-1], 0x01, dtype=U))
    zero = np.zeros(l.shape[:-1], dtype=U)
    by += [zero] * (136 - len(by))
    by[135] = by[135] | U(0x80)
    a = [[zero.copy() for _ in range(5)] for _ in range(5)]
    for k in range(RATE):
        w = zero.copy()
        for j in range(8):
            w = w | (by[8 * k + j] << U(8 * j))
        a[k % 5][k // 5] = w
    a = keccak_f(a)
    return pack(np.stack([a[0][0], a[1][0], a[2][0], a[3][0]], axis=-1))


def merkle_cap(leaves, cap_height):
    """leaves: [num_leaves, width] rows -> cap [2^cap_height, 4]"""
    level = hash_no_pad(leaves)
    while level.shape[0] > (1 << cap_height):
        level = two_to_one(level[0::2], level[1::2])
    return level


def merkle_cap_columns(cols_major, num_leaves, width, cap_height):
    """column-major data [cols held][num_leaves], flat; the leaf is `width` words wide and the columns not held are zeros"""
    held = np.asarray(cols_major, dtype=U).reshape(-1, num_leaves)
    rows = np.zeros((num_leaves, width), dtype=U)
    rows[:, :held.shape[0]] = held.T
    return merkle_cap(rows, cap_height)
