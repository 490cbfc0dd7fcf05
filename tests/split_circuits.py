"""Circuits of the bit and byte decomposition gadgets (split_le, range_check, split_bytes_le, is_less_than), shared by
tests/test_split_host.py (host twin) and tests/test_gpu_split.py (device).  Every expected value is Python's own integer
arithmetic; nothing here reads a result of the code under test."""
P = 0xFFFFFFFF00000001
WIDTHS = (1, 8, 32, 63, 64)
BYTE_COUNTS = (1, 7, 8)
LT_WIDTHS = (1, 8, 32, 62)
WIDE_INPUTS, WIDE_BITS = 40, 63   # 2520 bit hints in one level: more than one trip of k_witness's 4 x 512 single-op loop


def bits_of(v, n):
    return [(v >> i) & 1 for i in range(n)]


def values_for(width_bits):
    """0, 1, 2^k - 1, 2^32 - 1, 2^32, 0xFFFFFFFF00000000, p - 1: those that fit the width and are field elements"""
    cand = [0, 1, (1 << width_bits) - 1, (1 << 32) - 1, 1 << 32, 0xFFFFFFFF00000000, P - 1]
    out = []
    for v in cand:
        if v < (1 << width_bits) and v < P and v not in out:
            out.append(v)
    return out


def split_le(pkg, zero_knowledge=False, hasher="poseidon", widths=WIDTHS):
    """One input per width, each split into its bits.  Returns (data, xs, bits, maps, want): maps[j] sets every x to the j-th
    value of its width (cycling), want[j] the bits of all widths in order."""
    b = pkg.CircuitBuilder(zero_knowledge=zero_knowledge, hasher=hasher)
    xs = [b.add_virtual_target() for _ in widths]
    bits = [b.split_le(x, k) for x, k in zip(xs, widths)]
    data = b.build()
    vals = [values_for(k) for k in widths]
    maps, want = [], []
    for j in range(max(len(v) for v in vals)):
        chosen = [v[j % len(v)] for v in vals]
        maps.append(dict(zip(xs, chosen)))
        want.append([bit for v, k in zip(chosen, widths) for bit in bits_of(v, k)])
    return data, xs, bits, maps, want


def split_bytes_le(pkg, counts=BYTE_COUNTS):
    b = pkg.CircuitBuilder()
    lut = b.sbox_lut()
    xs = [b.add_virtual_target() for _ in counts]
    parts = [b.split_bytes_le(x, k, lut) for x, k in zip(xs, counts)]
    data = b.build()
    vals = [values_for(8 * k) for k in counts]
    maps, want = [], []
    for j in range(max(len(v) for v in vals)):
        chosen = [v[j % len(v)] for v in vals]
        maps.append(dict(zip(xs, chosen)))
        want.append([byte for v, k in zip(chosen, counts) for byte in v.to_bytes(k, "little")])
    return data, xs, parts, maps, want


def is_less_than(pkg, num_bits):
    b = pkg.CircuitBuilder()
    x, y = b.add_virtual_target(), b.add_virtual_target()
    lt = b.is_less_than(x, y, num_bits)
    return b.build(), x, y, lt


def lt_pairs(n):
    top = (1 << n) - 1
    return [(0, 0), (0, 1), (1, 0), (top, top), (top, max(top - 1, 0))]


_wide = {}


def wide(pkg):
    """WIDE_INPUTS distinct inputs, each split into WIDE_BITS bits.  (data, xs, flat list of all bit targets)"""
    if "c" not in _wide:
        b = pkg.CircuitBuilder()
        xs = [b.add_virtual_target() for _ in range(WIDE_INPUTS)]
        bits = [t for x in xs for t in b.split_le(x, WIDE_BITS)]
        _wide["c"] = (b.build(), xs, bits)
    return _wide["c"]


def wide_values(seed):
    """distinct 63-bit values with both edges: 0, 2^63 - 1, then a fixed multiplicative walk"""
    vals, v = [0, (1 << WIDE_BITS) - 1], 0x9E3779B97F4A7C15 * (seed + 1)
    while len(vals) < WIDE_INPUTS:
        v = (v * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        vals.append(v >> 1)
    return vals


_bridge = {}


def bridge(pkg):
    """The circuit the gadgets exist for: an AES-128 key derived in the circuit from a Poseidon hash.  secret[4] ->
    hash_n_to_m_no_pad(secret, 2) -> split_bytes_le(h_i, 8) -> 16 key bytes -> key_expansion -> encrypt_block of one block.
    Returns (data, secret targets, block targets, ciphertext targets) with block and ciphertext in byte order."""
    if "c" not in _bridge:
        b = pkg.CircuitBuilder()
        xl, ml, sl = b.byte_xor_lut(), b.gf_2_8_mul_lut(), b.sbox_lut()
        secret = [b.add_virtual_target() for _ in range(4)]
        h = b.hash_n_to_m_no_pad(secret, 2)
        key = [t for w in h for t in b.split_bytes_le(w, 8, sl)]
        ek = b.key_expansion(4, 10, xl, sl, key)
        ist = b.add_virtual_state_target(sl)
        out = b.encrypt_block(10, xl, ml, sl, ist, ek)
        order = [4 * (k % 4) + k // 4 for k in range(16)]   # byte k of a block is state[k % 4][k // 4] (tests/circuits.py encrypt_block)
        _bridge["c"] = (b.build(), secret, [ist[i] for i in order], [out[i] for i in order])
    return _bridge["c"]


def bridge_key(pkg, secret):
    h = pkg.poseidon_native.hash_n_to_m_no_pad(list(secret), 2)
    return h[0].to_bytes(8, "little") + h[1].to_bytes(8, "little")


def bridge_cases(pkg, count=3):
    """(maps setting only the secret and the block, expected ciphertexts)"""
    data, secret, block, ct = bridge(pkg)
    maps, want = [], []
    for i in range(count):
        sec = [(0x0123456789ABCDEF * (i + 1) + 977 * j) % P for j in range(4)]
        blk = bytes((17 * i + 31 * j + 5) & 0xFF for j in range(16))
        maps.append(dict(zip(secret + block, sec + list(blk))))
        want.append(pkg.native.encrypt_block(bridge_key(pkg, sec), blk))
    return maps, want
