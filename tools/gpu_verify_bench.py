#!/usr/bin/env python3
"""Times, in one process on one GPU, the four ways to prove or check a batch of 256 AES-GCM 1 KiB proofs: proving them
(p2_prove_batch), the host verifier in a loop (p2_verify, one proof per call), p2_verify_batch from host memory and
p2_verify_batch_device on proofs already in HBM (default stream).  Every path runs over the whole batch: one warm-up, then
the median of several repeats (three for the host loop, which takes seconds); prints one JSON line."""
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
B = int(os.environ.get("VERIFY_BENCH_BATCH", "256"))
REPEATS = int(os.environ.get("VERIFY_BENCH_REPEATS", "5"))
HOST_REPEATS = int(os.environ.get("VERIFY_BENCH_HOST_REPEATS", "3"))  # the host loop over all B proofs takes seconds

b = pkg.CircuitBuilder()
t = pkg.AesGcmTarget.build(b, 4, 10, 1024, False)
data = b.build()
rnd = random.Random(7)
pws = []
for i in range(B):
    key, nonce, pt = bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(12)), bytes(rnd.randrange(256) for _ in range(1024))
    ct, tag = pkg.native.gcm_encrypt(key, nonce, pt)
    pw = pkg.PartialWitness()
    t.set_targets(pw, key, nonce, pt, ct, tag)
    pws.append(pw)


def timed(f, repeats=REPEATS):
    f()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


res = {}
proofs = []


def prove():
    proofs[:] = data.prove_batch(pws)[0]


res["prove_batch_ms"] = 1e3 * timed(prove, 3)
assert all(p is not None for p in proofs)
blob = b"".join(proofs)
assert data.verify_batch(blob) == [0] * B


def host_loop():
    for p in proofs:
        data.verify(p)


res["host_verify_loop_ms"] = 1e3 * timed(host_loop, HOST_REPEATS)
res["verify_batch_host_ms"] = 1e3 * timed(lambda: data.verify_batch(blob))

import ctypes as C  # noqa: E402

H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))  # the runtime the library uses: proofs placed in HBM once, outside the timed region
H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
H.hipDeviceSynchronize.argtypes = []
d_proofs, d_status = C.c_void_p(), C.c_void_p()
assert H.hipMalloc(C.byref(d_proofs), len(blob)) == 0 and H.hipMalloc(C.byref(d_status), 4 * B) == 0
assert H.hipMemcpy(d_proofs, blob, len(blob), 1) == 0


def dev():
    data.verify_batch_device(d_proofs.value, d_status.value, B, stream=None)
    assert H.hipDeviceSynchronize() == 0


res["verify_batch_device_ms"] = 1e3 * timed(dev)
st = (C.c_int * B)()
assert H.hipMemcpy(st, d_status, 4 * B, 2) == 0 and list(st) == [0] * B
res.update(proofs=B, proof_bytes=data.proof_bytes, repeats=REPEATS, host_repeats=HOST_REPEATS,
           speedup_vs_host=round(res["host_verify_loop_ms"] / res["verify_batch_host_ms"], 1),
           verify_share_of_prove=round(res["verify_batch_host_ms"] / res["prove_batch_ms"], 3))
for k in list(res):
    if k.endswith("_ms"):
        res[k] = round(res[k], 2)
print(json.dumps(res), flush=True)
