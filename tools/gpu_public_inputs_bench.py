#!/usr/bin/env python3
"""Cost of public inputs on the flagship workload: proofs/s of AES-GCM-128 over 1 KiB (with the tag) with and without the
ciphertext and tag registered public, in one process on one GPU.  Reports each circuit's degree_bits and proof bytes, the
median wall time of p2_prove_batch over a batch, and the public-input kernel's time per chunk (kernel event timing, one
extra timed batch), and whether the hash rows push the circuit to the next power of two.  Prints one JSON line.

    python3 tools/gpu_public_inputs_bench.py            # PI_BENCH_BATCH=256 PI_BENCH_REPEATS=5"""
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
B = int(os.environ.get("PI_BENCH_BATCH", "256"))
REPEATS = int(os.environ.get("PI_BENCH_REPEATS", "5"))
L = 1024

rnd = random.Random(11)
inputs = [(bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(12)), bytes(rnd.randrange(256) for _ in range(L)))
          for _ in range(B)]


def run(public):
    b = pkg.CircuitBuilder()
    t = pkg.AesGcmTarget.build(b, 4, 10, L, True)
    if public:
        b.register_public_inputs(t.ct + t.tag)
    data = b.build()
    pws = []
    for key, nonce, pt in inputs:
        ct, tag = pkg.native.gcm_encrypt(key, nonce, pt)
        pw = pkg.PartialWitness()
        t.set_targets(pw, key, nonce, pt, ct, tag)
        pws.append(pw)
    proofs, st = data.prove_batch(pws)  # warm-up: load, workspaces
    assert st == [0] * B, st
    assert data.verify_batch(proofs) == [0] * B
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        _, st = data.prove_batch(pws)
        ts.append(time.perf_counter() - t0)
        assert st == [0] * B
    h = data.gpu()
    pkg.lib().p2_circuit_set_timing(h, 1)
    data.prove_batch(pws)
    pkg.lib().p2_circuit_synchronize(h)
    arr = (pkg.api._KernelTime * 128)()
    k = pkg.lib().p2_circuit_get_timing(h, arr, 128)
    pkg.lib().p2_circuit_set_timing(h, 0)
    times = {arr[i].name.decode(): (arr[i].ms, arr[i].count) for i in range(min(k, 128))}
    pi_ms, pi_launches = times.get("pi_hash", (0.0, 0))
    med = statistics.median(ts)
    return {"public_inputs": data.num_public_inputs, "degree_bits": data.info["degree_bits"], "proof_bytes": data.proof_bytes,
            "prove_batch_ms": round(1e3 * med, 2), "proofs_per_s": round(B / med, 1),
            "pi_hash_ms_per_chunk": round(pi_ms / pi_launches, 3) if pi_launches else None, "pi_hash_launches": pi_launches}


res = {"batch": B, "repeats": REPEATS, "plaintext_bytes": L, "private": run(False), "public_ct_tag": run(True)}
res["overhead"] = round(res["private"]["proofs_per_s"] / res["public_ct_tag"]["proofs_per_s"] - 1, 4)
res["pi_rows_raise_degree"] = res["public_ct_tag"]["degree_bits"] > res["private"]["degree_bits"]  # the hash rows cross a power of two
print(json.dumps(res), flush=True)
