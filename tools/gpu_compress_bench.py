#!/usr/bin/env python3
"""Compressed proofs on one GPU: for 256 proofs each of the AES-GCM 1 KiB bench circuit, ElGamal encryption and AES-GCM 64 KiB
(n = 2^19), the compressed sizes (mean, min, max) and the median times of compress_batch, verify_compressed_batch and
verify_batch on the same proofs, one warm-up, then REPEATS runs.  Host-memory forms (`*_ms`, Python buffer handling included)
and device forms on proofs already in HBM (`*_device_ms`, the GPU work alone).  Prints one JSON line per circuit.

The 64 KiB circuit proves COMPRESS_BENCH_DISTINCT_64K distinct witnesses (default 64) and repeats them to fill the batch: its
Python witness maps are large, and the timings do not depend on which proofs repeat."""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import circuits  # noqa: E402

pkg = g.load_package()
B = int(os.environ.get("COMPRESS_BENCH_BATCH", "256"))
REPEATS = int(os.environ.get("COMPRESS_BENCH_REPEATS", "5"))
DISTINCT_64K = int(os.environ.get("COMPRESS_BENCH_DISTINCT_64K", "64"))
WHICH = os.environ.get("COMPRESS_BENCH_CIRCUITS", "aes_gcm_1k,elgamal,aes_gcm_64k").split(",")


def workload(name):
    rnd = random.Random(7)
    if name == "elgamal":
        data, pws, _, _ = circuits.ecgfp5_elgamal(pkg, list(range(1, B + 1)))
        return data, pws, B
    L, n = (1024, B) if name == "aes_gcm_1k" else (65536, min(B, DISTINCT_64K))
    b = pkg.CircuitBuilder()
    t = pkg.AesGcmTarget.build(b, 4, 10, L, False)
    data = b.build()
    pws = []
    for _ in range(n):
        key, nonce, pt = bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(12)), bytes(rnd.randrange(256) for _ in range(L))
        ct, tag = pkg.native.gcm_encrypt(key, nonce, pt)
        pw = pkg.PartialWitness()
        t.set_targets(pw, key, nonce, pt, ct, tag)
        pws.append(pw)
    return data, pws, n


H = None


def hip():
    """The HIP runtime the library uses (found in this process's mappings once the library has run)."""
    global H
    if H is None:
        H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
        H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        H.hipFree.argtypes = [C.c_void_p]
        H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        H.hipDeviceSynchronize.argtypes = []
    return H


def dalloc(nbytes, host=None):
    p = C.c_void_p()
    assert hip().hipMalloc(C.byref(p), nbytes) == 0
    if host is not None:
        assert hip().hipMemcpy(p, host, nbytes, 1) == 0
    return p


def timed(f):
    f()  # warm-up
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


for name in WHICH:
    data, pws, distinct = workload(name)
    proofs = []
    for i in range(0, len(pws), 64):
        ps, st = data.prove_batch(pws[i:i + 64])
        assert st == [0] * len(st), st
        proofs += ps
    proofs = (proofs * (B // len(proofs) + 1))[:B]
    blob = b"".join(proofs)
    cps, st = data.compress_batch(proofs)
    assert st == [0] * B, st
    assert data.verify_compressed_batch(cps) == [0] * B
    assert data.verify_batch(blob) == [0] * B
    sizes = [len(c) for c in cps]
    res = {"circuit": name, "proofs": B, "distinct_witnesses": distinct, "proof_bytes": data.proof_bytes,
           "compressed_mean": round(statistics.mean(sizes), 1), "compressed_min": min(sizes), "compressed_max": max(sizes),
           "compressed_ratio_mean": round(statistics.mean(sizes) / data.proof_bytes, 4)}
    res["compress_batch_ms"] = timed(lambda: data.compress_batch(proofs))
    res["verify_compressed_batch_ms"] = timed(lambda: data.verify_compressed_batch(cps))
    res["verify_batch_ms"] = timed(lambda: data.verify_batch(blob))
    res["verify_compressed_over_verify"] = round(res["verify_compressed_batch_ms"] / res["verify_batch_ms"], 3)
    pb = data.proof_bytes
    cblob = b"".join(c + bytes(pb - len(c)) for c in cps)
    lens = (C.c_uint32 * B)(*sizes)
    d_full, d_c, d_len, d_out, d_lo, d_st = dalloc(B * pb, blob), dalloc(B * pb, cblob), dalloc(4 * B, lens), dalloc(B * pb), dalloc(4 * B), dalloc(4 * B)

    def device(f):
        def run():
            f()
            assert hip().hipDeviceSynchronize() == 0
        return timed(run)

    res["compress_batch_device_ms"] = device(lambda: data.compress_batch_device(d_full.value, d_out.value, d_lo.value, d_st.value, B))
    res["verify_compressed_batch_device_ms"] = device(lambda: data.verify_compressed_batch_device(d_c.value, d_len.value, d_st.value, B))
    res["verify_batch_device_ms"] = device(lambda: data.verify_batch_device(d_full.value, d_st.value, B))
    st = (C.c_int * B)()
    assert hip().hipMemcpy(st, d_st, 4 * B, 2) == 0 and list(st) == [0] * B
    for d in (d_full, d_c, d_len, d_out, d_lo, d_st):
        hip().hipFree(d)
    res["verify_compressed_over_verify_device"] = round(res["verify_compressed_batch_device_ms"] / res["verify_batch_device_ms"], 3)
    for k in list(res):
        if k.endswith("_ms"):
            res[k] = round(res[k], 2)
    res["repeats"] = REPEATS
    print(json.dumps(res), flush=True)
