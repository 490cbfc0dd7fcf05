"""Circuits with public inputs (CircuitBuilder.register_public_input) for the public-input tests, with the values every
public input takes under each witness, computed here on the host."""
import struct

P = 0xFFFFFFFF00000001
PI_TAG = 0x49425550  # csrc/circuit.h BLOB_PI_TAG
G_PUBLIC_INPUT = 4


def small(pkg, k, witnesses=((3, 5, 7, 11), (P - 1, 2, 1 << 40, 9)), zero_knowledge=False, register=True):
    """Four inputs x0..x3, two computed targets and a constant; k public inputs cycling through
    [x0*x1, x2, 12345, x3 + x0, x0 (a duplicate of an earlier entry from the 5th on), x1, ...].
    Returns (data, pws, values per witness)."""
    b = pkg.CircuitBuilder(zero_knowledge=zero_knowledge)
    xs = [b.add_virtual_target() for _ in range(4)]
    prod, total, c = b.mul(xs[0], xs[1]), b.add(xs[3], xs[0]), b.constant(12345)
    cycle = [prod, xs[2], c, total, xs[0], xs[1]]
    pis = [cycle[i % len(cycle)] for i in range(k)]
    if register:
        b.register_public_inputs(pis)
    data = b.build()
    pws, vals = [], []
    for w in witnesses:
        pw = pkg.PartialWitness()
        pw.set_target_arr(xs, w)
        pws.append(pw)
        v = {prod: w[0] * w[1] % P, xs[2]: w[2], c: 12345, total: (w[3] + w[0]) % P, xs[0]: w[0], xs[1]: w[1]}
        vals.append([v[t] for t in pis])
    return data, pws, vals, pis


def aes_gcm(pkg, L=1024, n=2, public=True):
    """AES-GCM-128 over L bytes with the tag; ciphertext and tag registered public (ct bytes, then the 16 tag bytes)."""
    b = pkg.CircuitBuilder()
    t = pkg.AesGcmTarget.build(b, 4, 10, L, True)
    if public:
        b.register_public_inputs(t.ct + t.tag)
    data = b.build()
    pws, vals = [], []
    for i in range(n):
        key, nonce, pt = bytes([i + 1] * 16), bytes([i + 2] * 12), bytes([(5 * i + j) & 255 for j in range(L)])
        ct, tag = pkg.native.gcm_encrypt(key, nonce, pt)
        pw = pkg.PartialWitness()
        t.set_targets(pw, key, nonce, pt, ct, tag)
        pws.append(pw)
        vals.append(list(ct) + list(tag))
    return data, pws, vals


def zk(pkg, pairs=((1, 2), (0x57, 0x13))):
    """test_gf_2_8_add's circuit in the zk config, with x and x ^ y public."""
    b = pkg.CircuitBuilder(zero_knowledge=True)
    lut = b.byte_xor_lut()
    x, y = b.add_virtual_byte_target_unsafe(), b.add_virtual_byte_target_unsafe()
    xy = b.gf_2_8_add(lut, x, y)
    b.register_public_input(x)
    b.register_public_input(xy)
    data = b.build()
    pws, vals = [], []
    for a, c in pairs:
        pw = pkg.PartialWitness()
        pw.set_byte_target(x, a)
        pw.set_byte_target(y, c)
        pw.set_byte_target(xy, a ^ c)
        pws.append(pw)
        vals.append([a, a ^ c])
    return data, pws, vals


def pi_section(blob, k):
    """(offset of the section, pi_slots) from the tail of a blob with k public inputs."""
    off = len(blob) - (12 + 4 * k)
    tag, cnt = struct.unpack_from("<IQ", blob, off)
    assert tag == PI_TAG and cnt == k
    return off, list(struct.unpack_from("<%dI" % k, blob, off + 12))


def pi_gate_row(orc_circuit, n):
    """The PublicInputGate row (the oracle reads each row's gate kind from the selector columns)."""
    rows = [r for r in range(n) if orc_circuit.row_gate_kind(r) == G_PUBLIC_INPUT]
    assert len(rows) == 1, rows
    return rows[0]


def target_value(wires, n, t):
    """Value of a routed-wire target (bit 63 set: row << 8 | column) in a column-major [wires][n] witness."""
    assert t >> 63
    row, col = (t & ~(1 << 63)) >> 8, t & 0xFF
    return wires[col * n + row]
