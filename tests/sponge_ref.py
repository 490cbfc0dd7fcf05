"""The textbook overwrite-mode Poseidon sponge (plonky2's hash_n_to_hash_no_pad, two_to_one and hash_or_noop) over the CPU
oracle's permutation, for the tests of the hash kernels' sponge steps; and the ctypes signatures of the entry points they use."""
import ctypes as C

P = 0xFFFFFFFF00000001
u64p = C.POINTER(C.c_uint64)
EXTREMES = [0, 1, P - 1, P - 2, 0xFFFFFFFF, 1 << 32, P - (1 << 32), (1 << 63) % P, 0xFFFFFFFE00000002 % P]


def bind(lib):
    sz = C.c_size_t
    lib.p2_host_poseidon_known.restype, lib.p2_host_poseidon_known.argtypes = C.c_int, [u64p, sz, C.c_int, C.c_uint32, C.c_int]
    lib.p2_host_hash_leaves.restype, lib.p2_host_hash_leaves.argtypes = C.c_int, [u64p, sz, sz, sz, u64p]
    lib.p2_gpu_hash_leaves.restype, lib.p2_gpu_hash_leaves.argtypes = C.c_int, [u64p, sz, sz, sz, sz, u64p, C.c_int]
    lib.p2_gpu_merkle_level.restype, lib.p2_gpu_merkle_level.argtypes = C.c_int, [u64p, sz, sz, u64p, C.c_int]
    lib.p2_gpu_hash_fri_leaves.restype, lib.p2_gpu_hash_fri_leaves.argtypes = C.c_int, [u64p, sz, C.c_int, sz, u64p, C.c_int]
    return lib


def permute(orc, state):
    s = (C.c_uint64 * 12)(*state)
    orc.lib().orc_poseidon(s)
    return list(s)


def hash_no_pad(orc, words):
    """Every chunk of eight words overwrites the front of the rate, then one permutation; the digest is words 0..3."""
    st = [0] * 12
    for c0 in range(0, len(words), 8):
        chunk = words[c0:c0 + 8]
        st[:len(chunk)] = chunk
        st = permute(orc, st)
    return st[:4]


def hash_or_noop(orc, words):
    return (list(words) + [0] * 4)[:4] if len(words) <= 4 else hash_no_pad(orc, words)


def two_to_one(orc, a, b):
    return permute(orc, list(a) + list(b) + [0] * 4)[:4]
