"""The Schnorr scheme of DESIGN.md section 9g in Python: curve arithmetic from oracle/oracle_ecgfp5.py (textbook affine), scalars
as Python integers, the challenge hash from the CPU oracle's Poseidon (proof_ref.poseidon_hasher: liboracle.so).  It calls
nothing of the library under test.  One g_mul costs about 0.14 s: tests keep the number of calls small (sign takes r_point and pk
so that one k G serves many messages)."""
import functools
import os
import sys

import numpy as np

import proof_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_ecgfp5 as ec  # noqa: E402

P, N = ec.P, ec.GROUP_ORDER
_hash_no_pad, _ = proof_ref.poseidon_hasher()


@functools.lru_cache(maxsize=None)
def g_mul_gen(k):
    """k G, remembered: keys and nonces recur across tests"""
    return ec.g_mul(k, ec.generator())


def challenge(r, pk, msg):
    words = ec.as_fields(r) + ec.as_fields(pk) + [int(w) for w in msg]
    return tuple(int(w) for w in _hash_no_pad(np.array(words, dtype=np.uint64)))


def e_int(e_words):
    return sum(w << (64 * i) for i, w in enumerate(e_words))


def sign(sk, msg, k):
    """(s, e_words); k = 0 gives the signature the verifier accepts although no signer emits it"""
    pk = g_mul_gen(sk)
    e = challenge(g_mul_gen(k), pk, msg)
    return (k + e_int(e) * sk) % N, e


def verify(pk, msg, sig):
    """0 accepted, 1 rejected, 2 malformed (two g_mul)"""
    s, e = sig
    if s >= N or any(w >= P for w in list(e) + list(msg) + ec.as_fields(pk)) or pk == ec.NEUTRAL or not ec.in_group(pk):
        return 2
    r = ec.g_add(g_mul_gen(s), ec.g_mul(e_int(e), ec.g_neg(pk)))
    return 0 if challenge(r, pk, msg) == tuple(e) else 1
