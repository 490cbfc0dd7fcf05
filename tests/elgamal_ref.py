"""The ecgfp5 crate's native side in Python, for the ElGamal tests: curve, decompress and the plain cipher from
oracle/oracle_ecgfp5.py (textbook affine arithmetic), the five-word hash of the hashed cipher from sponge_ref.permute over the CPU
oracle's Poseidon.  It calls nothing of the library under test.  One g_mul costs about 0.14 s, one decompress about 0.05 s: the
tests hold the library to this file on a dozen items and the device to the host twin on the rest."""
import functools
import os
import sys

import oracle_lib
import sponge_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_ecgfp5 as ec  # noqa: E402

P, N = ec.P, ec.GROUP_ORDER
M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def g_mul(k, p):
    """k p, remembered: keys, nonces and points recur across tests"""
    return ec.g_mul(k, p)


def g_mul_gen(k):
    return g_mul(k, ec.generator())


def hash5(words):
    """hash_n_to_m_no_pad(words, 5): overwrite mode, one permutation per chunk of eight, the first five state words"""
    st = [0] * 12
    for c0 in range(0, len(words), 8):
        chunk = [int(w) for w in words[c0:c0 + 8]]
        st[:len(chunk)] = chunk
        st = sponge_ref.permute(oracle_lib, st)
    return tuple(st[:5])


@functools.lru_cache(maxsize=None)
def decompress(w):
    return ec.decompress(tuple(w))


@functools.lru_cache(maxsize=None)
def decodes(w):
    """Whether w is the encoding of a group element, at the cost of one square test: x^2 + (a - 1/u^2) x + b has roots iff its
    discriminant is a square, they multiply to b, which is not a square, so exactly one of them is not a square -- in the group.
    (decompress says the same; tests/test_elgamal_host.py holds the two together.)"""
    w = tuple(w)
    if w == ec.ZERO:
        return True
    bc = ec.f_sub(ec.A, ec.f_inv(ec.f_mul(w, w)))
    return ec.f_is_square(ec.f_sub(ec.f_mul(bc, bc), ec.f_small(ec.B, 4)))


def attempt_word(limbs, row):
    return tuple(lo + (hi << 32) for lo, hi in zip(limbs, row))


def first_attempt(limbs, pads):
    """the number of the first attempt of encode_binary that decodes (a word not below p is skipped); len(pads) when none does"""
    for a, row in enumerate(pads):
        w = attempt_word(limbs, row)
        if all(v < P for v in w) and decodes(w):
            return a
    return len(pads)


def encode_padded(limbs, pads):
    """(point, attempt) of encode_binary (lib.rs:48) with the high halves given; (None, len(pads)) when no attempt decodes"""
    for a, row in enumerate(pads):
        w = attempt_word(limbs, row)
        if any(v >= P for v in w):
            continue
        g = decompress(w)
        if g is not None:
            return g, a
    return None, len(pads)


def decode(p):
    return tuple(v & M32 for v in p[1])


def limbs_of(x):
    return tuple((x >> (32 * i)) & M32 for i in range(5))


def int_of(limbs):
    return sum(v << (32 * i) for i, v in enumerate(limbs))


def elgamal_encrypt(pk, nonce, msg):
    return g_mul_gen(nonce), ec.g_add(msg, g_mul(nonce, pk))


def elgamal_decrypt(sk, c0, c1):
    return ec.g_add(c1, ec.g_neg(g_mul(sk, c0)))


def hashed_elgamal_encrypt(pk, nonce, msg):
    h = hash5(ec.as_fields(g_mul(nonce, pk)))
    return g_mul_gen(nonce), tuple((m + x) % P for m, x in zip(msg, h))


def hashed_elgamal_decrypt(sk, c0, ct):
    h = hash5(ec.as_fields(g_mul(sk, c0)))
    return tuple((c - x) % P for c, x in zip(ct, h))
