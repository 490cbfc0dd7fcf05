"""Circuits of the table-driven GHASH gadgets (csrc/aes_gadgets.h gf_2_128_mul_tables_target, ghash_tables_target and
AesGcmTarget under CircuitBuilder(ghash_tables=lanes)), shared by tests/test_ghash_tables_host.py and
tests/test_gpu_ghash_tables.py.  Inputs are range-checked byte targets, as the gadget demands."""
import random

_cache = {}


def edge_pairs(seed=7, count=2):
    """(x, y) pairs: zero, all 0xff, then `count` random ones"""
    r = random.Random(seed)
    rnd = lambda: bytes(r.randrange(256) for _ in range(16))  # noqa: E731
    return [(bytes(16), bytes(16)), (b"\xff" * 16, b"\xff" * 16)] + [(rnd(), rnd()) for _ in range(count)]


def single_bit_blocks():
    """the 128 blocks with one bit set, in GCM's bit order: bit i is bit 7 - i % 8 of byte i / 8"""
    return [bytes((0x80 >> (i % 8)) if j == i // 8 else 0 for j in range(16)) for i in range(128)]


def mul(pkg):
    """One multiplication z = x * y: (data, x, y, z, (lo_lut, hi_lut)).  2^13 rows."""
    if "mul" not in _cache:
        b = pkg.CircuitBuilder()
        sb, xl, lo, hi = b.sbox_lut(), b.byte_xor_lut(), b.clmul_lo_lut(), b.clmul_hi_lut()
        x = [b.add_virtual_byte_target(sb) for _ in range(16)]
        y = [b.add_virtual_byte_target(sb) for _ in range(16)]
        z = b.gf_2_128_mul_tables(xl, lo, hi, x, y)
        _cache["mul"] = (b.build(), x, y, z, (lo, hi))
    return _cache["mul"]


def mul_inputs(x_t, y_t, x, y):
    return dict(zip(x_t + y_t, bytes(x) + bytes(y)))


def ghash(pkg, lanes, block_counts):
    """GHASH_h of one input per entry of block_counts, all in one circuit over one h: (data, h, [x targets], [out targets])"""
    key = ("ghash", lanes, tuple(block_counts))
    if key not in _cache:
        b = pkg.CircuitBuilder()
        sb, xl, lo, hi = b.sbox_lut(), b.byte_xor_lut(), b.clmul_lo_lut(), b.clmul_hi_lut()
        h = [b.add_virtual_byte_target(sb) for _ in range(16)]
        xs = [[b.add_virtual_byte_target(sb) for _ in range(16 * n)] for n in block_counts]
        outs = [b.ghash_tables(xl, lo, hi, h, x, lanes) for x in xs]
        _cache[key] = (b.build(), h, xs, outs)
    return _cache[key]


def gcm(pkg, nk, L, lanes, tag=True, public=False, **kw):
    """AesGcmTarget<nk, 4, nk + 6, L, tag> from a builder with ghash_tables = lanes: (data, target); public registers the
    ciphertext bytes and then the 16 tag bytes as public inputs"""
    key = ("gcm", nk, L, lanes, tag, public, tuple(sorted(kw.items())))
    if key not in _cache:
        b = pkg.CircuitBuilder(ghash_tables=lanes, **kw)
        t = pkg.AesGcmTarget.build(b, nk, nk + 6, L, tag)
        if public:
            b.register_public_inputs(t.ct + t.tag)
        _cache[key] = (b.build(), t)
    return _cache[key]


def gcm_inputs(t, key, iv, pt, tag=None):
    """key, nonce and plaintext, and the tag if given (the tag targets are tied to the computed tag: a wrong one is a conflict)"""
    m = dict(zip(t.key + t.nonce + t.pt, bytes(key) + bytes(iv) + bytes(pt)))
    if tag is not None:
        m.update(zip(t.tag, bytes(tag)))
    return m
