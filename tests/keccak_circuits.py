"""The circuits of tests/circuits.py and tests/pi_circuits.py built with hasher="keccak": a view of the package whose
CircuitBuilder defaults to the Keccak configuration, so the circuit definitions are the ones the Poseidon tests use."""
import circuits
import pi_circuits


class KeccakPkg:
    def __init__(self, pkg):
        self._pkg = pkg

    def __getattr__(self, name):
        return getattr(self._pkg, name)

    def CircuitBuilder(self, zero_knowledge=False):
        return self._pkg.CircuitBuilder(zero_knowledge=zero_knowledge, hasher="keccak")


def build(pkg, name, n=4):
    """(data, pws) of a named circuit with `n` witnesses (where the circuit takes a count), under whatever hasher `pkg` builds with."""
    if name == "aes_block":
        return circuits.encrypt_block(pkg, bytes(range(16)), bytes(range(16, 32)))
    if name == "aes_gcm_13":
        return circuits.encrypt(pkg, 4, 13, False)[:2]
    if name == "aes_gcm_13_tag":
        return circuits.encrypt(pkg, 4, 13, True)[:2]
    if name == "aes_gcm_1k":
        keys = [(bytes([i, 1] * 8), bytes([i + 1] * 12), bytes([(7 * i + j) & 255 for j in range(1024)])) for i in range(n)]
        return circuits.encrypt(pkg, 4, 1024, False, keys)[:2]
    if name == "poseidon_cipher":
        return circuits.poseidon_encrypt(pkg, 3, list(range(1, n + 1)))[:2]
    if name == "elgamal":
        return circuits.ecgfp5_elgamal(pkg, list(range(1, n + 1)))[:2]
    if name == "zk":
        return circuits.zk_gf_2_8_add(pkg, [(1, 2), (0x57, 0x13), (255, 0), (9, 9)][:n])
    if name == "public_inputs":
        return pi_circuits.aes_gcm(pkg, L=64, n=n)[:2]
    if name == "gf_mul":
        return circuits.gf_2_8_mul(pkg, [(0x57, 0x13, 0xFE)] * n)
    raise KeyError(name)
