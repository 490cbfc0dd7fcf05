"""Additional authenticated data inside the AES-GCM circuit, through the host witness generator: aad_len = 0 is the circuit that
never heard of it, blob for blob; with an aad the circuit computes tests/gcm_ref.py's ciphertext and tag, a wrong tag byte and a
wrong aad byte are conflicts that the fault report names, and an aad without the tag is refused."""
import random

import pytest

import gcm_circuits as K
import gcm_ref

P2_ERR_INVALID = 1                       # include/p2aes.h


def rnd(r, n):
    return bytes(r.randrange(256) for _ in range(n))


@pytest.mark.parametrize("lanes", (0, 1))
def test_aad_len_zero_is_the_same_blob(pkg, lanes):
    def blob(**kw):
        b = pkg.CircuitBuilder(ghash_tables=lanes)
        t = pkg.AesGcmTarget.build(b, 4, 10, 13, True, **kw)
        return b.build().blob, t
    (plain, t0), (zero, t1) = blob(), blob(aad_len=0)
    assert plain == zero and t1.aad == [] and (t0.key, t0.nonce, t0.pt, t0.ct, t0.tag) == (t1.key, t1.nonce, t1.pt, t1.ct, t1.tag)
    assert blob(aad_len=13)[0] != plain


def test_degree_bits_of_the_tls12_shape(pkg):
    data, t = K.gcm_aad(pkg, 4, 13, 13)
    print("AES-GCM-128, L = 13, aad_len = 13, ghash_tables = 1: degree_bits %d, %d ops, %d levels" % (data.info["degree_bits"], data.info["num_ops"], data.info["num_levels"]))
    assert len(t.aad) == 13 and len(set(t.aad)) == 13 and min(t.aad) > max(t.tag)      # created after the tag targets
    assert data.info["degree_bits"] == 14                                               # as the 13-byte circuit without aad


@pytest.mark.parametrize("nk,L,al,lanes", [(4, 13, 13, 1), (4, 13, 5, 0), (8, 33, 17, 2), (6, 16, 16, 1), (4, 0, 20, 1)])
def test_circuit_computes_the_reference(pkg, nk, L, al, lanes):
    r = random.Random(nk + L + al)
    key, iv, pt, aad = rnd(r, 4 * nk), rnd(r, 12), rnd(r, L), rnd(r, al)
    ct, tag = gcm_ref.encrypt(key, iv, pt, aad)
    data, t = K.gcm_aad(pkg, nk, L, al, lanes)
    vals, st, fault = pkg.host_witness(data.blob, K.inputs(t, key, iv, pt, aad), t.ct + t.tag)
    assert st == 0 and fault.kind == "NONE"
    assert bytes(vals[:L]) == ct and bytes(vals[L:]) == tag
    honest = K.inputs(t, key, iv, pt, aad, tag)
    honest.update(zip(t.ct, ct))
    assert pkg.host_witness(data.blob, honest)[1] == 0


def test_set_targets_takes_the_aad(pkg):
    r = random.Random(5)
    key, iv, pt, aad = rnd(r, 16), rnd(r, 12), rnd(r, 13), rnd(r, 13)
    ct, tag = gcm_ref.encrypt(key, iv, pt, aad)
    data, t = K.gcm_aad(pkg, 4, 13, 13)
    pw = pkg.PartialWitness()
    t.set_targets(pw, key, iv, pt, ct, tag, aad=aad)
    assert pkg.host_witness(data.blob, pw)[1] == 0
    with pytest.raises(AssertionError):
        t.set_targets(pkg.PartialWitness(), key, iv, pt, ct, tag)                       # the aad is missing


def test_wrong_tag_and_wrong_aad_are_named_conflicts(pkg):
    r = random.Random(6)
    key, iv, pt, aad = rnd(r, 16), rnd(r, 12), rnd(r, 13), rnd(r, 13)
    ct, tag = gcm_ref.encrypt(key, iv, pt, aad)
    data, t = K.gcm_aad(pkg, 4, 13, 13)
    honest = K.inputs(t, key, iv, pt, aad, tag)
    for target in (t.tag[15], t.tag[0], t.aad[0], t.aad[12]):
        bad = dict(honest)
        bad[target] ^= 0x01
        _, st, fault = pkg.host_witness(data.blob, bad)
        print(fault)
        assert st == 1 and fault.kind.endswith("CONFLICT"), fault
        assert fault.target is not None and fault.computed != fault.found and "holds" in str(fault) or "sets" in str(fault)


def test_aad_without_the_tag_is_refused(pkg):
    b = pkg.CircuitBuilder()
    with pytest.raises(pkg.P2Error, match="aad needs the tag"):
        pkg.AesGcmTarget.build(b, 4, 10, 16, False, aad_len=5)
    import ctypes as C
    u = (C.c_uint64 * 16)
    assert pkg.lib().p2_aes_gcm_build_aad(b._h, 4, 10, 16, 0, 5, u(), u(), u(), u(), u(), u()) == P2_ERR_INVALID
    pkg.AesGcmTarget.build(b, 4, 10, 16, False, aad_len=0)                               # no aad: as before
