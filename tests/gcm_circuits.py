"""The AES-GCM circuit with additional authenticated data, shared by tests/test_gcm_circuits_host.py and tests/test_gpu_gcm.py
(built once per process)."""
_cache = {}


def gcm_aad(pkg, nk, L, aad_len, lanes=1):
    """AesGcmTarget<nk, 4, nk + 6, L, true> with aad_len aad bytes, from a builder with ghash_tables = lanes: (data, target)"""
    key = (nk, L, aad_len, lanes)
    if key not in _cache:
        b = pkg.CircuitBuilder(ghash_tables=lanes)
        t = pkg.AesGcmTarget.build(b, nk, nk + 6, L, True, aad_len=aad_len)
        _cache[key] = (b.build(), t)
    return _cache[key]


def inputs(t, key, iv, pt, aad, tag=None):
    """key, nonce, plaintext and aad, and the tag if given (the tag targets are tied to the computed tag: a wrong one is a conflict)"""
    m = dict(zip(t.key + t.nonce + t.pt + t.aad, bytes(key) + bytes(iv) + bytes(pt) + bytes(aad)))
    if tag is not None:
        m.update(zip(t.tag, bytes(tag)))
    return m
