"""CPU checks of the argument contract of the per-item batch calls (include/p2aes.h), host and _device forms: the shape check
comes first, then an empty batch is accepted with NULL pointers, then a required pointer that is NULL is "null argument", and
only then is the device looked at.  Every call here names device -1, so "all argument checks passed" reads as the device
error -- "no HIP device available" without a GPU, "device index out of range" with one -- and nothing is ever launched."""
import ctypes as C

import pytest

import sponge_ref

P2_OK, P2_ERR_INVALID, P2_ERR_NO_DEVICE = 0, 1, 2
# an argument of a row: P a required pointer, O a pointer that may be NULL at the row's scalars, N the count, DEV the device
# index, STREAM the stream; an int is a scalar at a valid value
P, O, N, DEV, STREAM = "P", "O", "N", "DEV", "STREAM"
MSG_LEN = (1025, "msg_len is at most 1024 words")
ATTEMPTS = (0, "attempts is between 1 and 256")
PCIPHER_L = (3073, "l is at most 3072 elements")
STRIDE = (319, "stride is at least 320 words")
LEAF_LEN = (0, "leaf_len >= 1, cap_height 0 to 16, siblings + cap_height at most 32")


def _pair(name, args, bad=None):
    """the host form and the _device form of one call: the same arguments, the device form with a stream behind the device"""
    return [(name, args, bad), (name + "_device", args + [STREAM], bad)]


# (entry point, its arguments in C order, (index of the shape argument, a value it refuses, the message) or None)
ROWS = (
    _pair("p2_ecgfp5_mul_batch", [P, P, N, P, P, DEV])
    + _pair("p2_schnorr_sign_batch", [P, P, O, 0, N, P, O, P, DEV], (3,) + MSG_LEN)      # msg at msg_len 0 and pk may be NULL
    + _pair("p2_schnorr_sign_batch", [P, P, P, 3, N, P, O, P, DEV], (3,) + MSG_LEN)
    + _pair("p2_schnorr_verify_batch", [P, O, 0, P, N, P, DEV], (2,) + MSG_LEN)
    + _pair("p2_schnorr_verify_batch", [P, P, 1024, P, N, P, DEV], (2,) + MSG_LEN)
    + _pair("p2_ecgfp5_decompress_batch", [P, N, P, P, DEV])
    + _pair("p2_ecgfp5_encode_binary_batch", [P, P, 1, N, P, P, P, DEV], (2,) + ATTEMPTS)
    + _pair("p2_ecgfp5_encode_binary_batch", [P, P, 256, N, P, P, P, DEV], (2, 257, ATTEMPTS[1]))
    + _pair("p2_elgamal_encrypt_batch", [P, P, P, N, P, P, P, DEV])
    + _pair("p2_elgamal_decrypt_batch", [P, P, P, N, P, P, DEV])
    + _pair("p2_hashed_elgamal_encrypt_batch", [P, P, P, N, P, P, P, DEV])
    + _pair("p2_hashed_elgamal_decrypt_batch", [P, P, P, N, P, P, DEV])
    + _pair("p2_poseidon_encrypt_batch", [P, P, O, 0, N, P, P, DEV], (3,) + PCIPHER_L)   # no message words at l = 0
    + _pair("p2_poseidon_encrypt_batch", [P, P, P, 4, N, P, P, DEV], (3,) + PCIPHER_L)
    + _pair("p2_poseidon_decrypt_batch", [P, P, P, 0, N, O, P, DEV], (3,) + PCIPHER_L)
    + _pair("p2_poseidon_decrypt_batch", [P, P, P, 3072, N, P, P, DEV], (3,) + PCIPHER_L)
    + [("p2_ecgfp5_scalar_bits_device", [P, N, P, 320, DEV, STREAM], (3,) + STRIDE)]
    + _pair("p2_merkle_verify_batch", [P, 1, P, O, 0, P, 0, N, P, DEV], (1,) + LEAF_LEN)  # no siblings at depth 0
    + _pair("p2_merkle_verify_batch", [P, 7, P, P, 16, P, 16, N, P, DEV], (4, 17, LEAF_LEN[1]))
    + [("p2_gpu_ecgfp5_scalar_muladd", [P, P, P, N, P, DEV], None)]
)
DEVICE_ERRORS = ((P2_ERR_NO_DEVICE, "no HIP device available"), (P2_ERR_INVALID, "device index out of range"))


def _call(L, name, args, count, null=(), override=None):
    """call `name`: the pointers whose index is in `null` as NULL, the others to a host array of zeros; -> (rc, message)"""
    fn = getattr(L, name)
    dummy = (C.c_uint64 * 512)()
    vals = []
    for i, (a, t) in enumerate(zip(args, fn.argtypes)):
        if override and i == override[0]:
            vals.append(override[1])
        elif a in (P, O):
            vals.append(None if i in null else C.cast(dummy, t))
        elif a == N:
            vals.append(count)
        elif a == DEV:
            vals.append(-1)
        elif a == STREAM:
            vals.append(None)
        else:
            vals.append(a)
    assert len(vals) == len(fn.argtypes), name
    rc = fn(*vals)
    return rc, L.p2_last_error().decode() if rc else ""


def _pointers(args, kinds=(P, O)):
    return [i for i, a in enumerate(args) if a in kinds]


@pytest.mark.parametrize("name,args,bad", ROWS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(ROWS)])
def test_argument_contract(pkg, name, args, bad):
    L = pkg.lib()
    if bad:  # (a) the shape check comes before the empty return
        assert _call(L, name, args, 0, override=bad[:2]) == (P2_ERR_INVALID, bad[2])
        assert _call(L, name, args, 0, null=_pointers(args), override=bad[:2]) == (P2_ERR_INVALID, bad[2])
    # (b) an empty batch is accepted with every pointer NULL
    assert _call(L, name, args, 0, null=_pointers(args)) == (P2_OK, "")
    # (c) each required pointer in turn
    for i in _pointers(args, (P,)):
        assert _call(L, name, args, 1, null=[i]) == (P2_ERR_INVALID, "null argument"), (name, i)
    # (d) with every pointer that may be NULL as NULL the argument checks pass: the device is looked at next
    assert _call(L, name, args, 1, null=_pointers(args, (O,))) in DEVICE_ERRORS
    assert _call(L, name, args, 1) in DEVICE_ERRORS


def test_a_null_required_pointer_is_reported_before_the_device(pkg):
    """the cases of the contract spelled out once, apart from the table"""
    L = pkg.lib()
    buf = (C.c_uint64 * 64)()
    st = (C.c_int * 1)()
    u64p = C.POINTER(C.c_uint64)
    p = C.cast(buf, u64p)
    assert L.p2_schnorr_verify_batch(p, None, 0, p, 1, st, -1) in (P2_ERR_NO_DEVICE, P2_ERR_INVALID)
    assert L.p2_last_error().decode() in [m for _, m in DEVICE_ERRORS]
    assert L.p2_schnorr_verify_batch(None, None, 1025, None, 0, None, -1) == P2_ERR_INVALID
    assert L.p2_last_error().decode() == MSG_LEN[1]
    assert L.p2_schnorr_verify_batch(None, None, 0, None, 0, None, -1) == P2_OK
    assert L.p2_schnorr_verify_batch(None, p, 1, p, 1, st, -1) == P2_ERR_INVALID
    assert L.p2_last_error().decode() == "null argument"
    assert L.p2_elgamal_encrypt_batch(p, p, p, 1, p, None, st, -1) == P2_ERR_INVALID
    assert L.p2_last_error().decode() == "null argument"


# The single-launch test primitives: their range checks and messages, and a valid call reaching the device.
PRIMITIVES = [
    # (entry point, arguments with device -1, the message or None for "reaches the device")
    ("p2_gpu_poseidon", lambda p: (p, 1, -1), None),
    ("p2_gpu_partial_rounds", lambda p: (p, 1, -1), None),
    ("p2_gpu_partial_rounds", lambda p: (p, 0, -1), "count out of range"),
    ("p2_gpu_partial_rounds", lambda p: (p, (1 << 24) + 1, -1), "count out of range"),
    ("p2_gpu_merged_middle", lambda p: (p, 1, -1), None),
    ("p2_gpu_merged_middle", lambda p: (p, 0, -1), "count out of range"),
    ("p2_gpu_merged_middle", lambda p: (p, (1 << 24) + 1, -1), "count out of range"),
    ("p2_gpu_ecstep_constraints", lambda p: (p, 1, p, -1), None),
    ("p2_gpu_ecstep_constraints", lambda p: (p, 0, p, -1), "count out of range"),
    ("p2_gpu_ecstep_constraints", lambda p: (p, (1 << 20) + 1, p, -1), "count out of range"),
    ("p2_gpu_ecstep_constraints", lambda p: (None, 1, p, -1), "count out of range"),
    ("p2_gpu_ecstep_constraints", lambda p: (p, 1, None, -1), "count out of range"),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 8, 4, 1, p, -1), None),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 8, 0, 1, p, -1), "shape out of range"),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 8, 65, 1, p, -1), "shape out of range"),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 0, 4, 1, p, -1), "shape out of range"),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 9, 4, 1, p, -1), "shape out of range"),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 8, 4, 0, p, -1), "shape out of range"),
    ("p2_gpu_hash_fri_leaves", lambda p: (p, 8, 4, 65536, p, -1), "shape out of range"),
]


@pytest.mark.parametrize("name,make,message", PRIMITIVES, ids=["%s-%d" % (r[0], i) for i, r in enumerate(PRIMITIVES)])
def test_primitive_range_checks(pkg, name, make, message):
    L = sponge_ref.bind(pkg.lib())  # (the signature of p2_gpu_hash_fri_leaves)
    buf = (C.c_uint64 * 512)()
    rc = getattr(L, name)(*make(C.cast(buf, C.POINTER(C.c_uint64))))
    got = (rc, L.p2_last_error().decode())
    if message is None:
        assert got in DEVICE_ERRORS
    else:
        assert got == (P2_ERR_INVALID, message)


def test_ecstep_constraints_refuses_a_non_canonical_wire(pkg):
    L = pkg.lib()
    wires, out = (C.c_uint64 * 80)(), (C.c_uint64 * 40)()
    wires[79] = 0xFFFFFFFF00000001
    assert L.p2_gpu_ecstep_constraints(wires, 1, out, -1) == P2_ERR_INVALID
    assert L.p2_last_error().decode() == "p2_gpu_ecstep_constraints: non-canonical wire"
