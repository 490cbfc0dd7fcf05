#!/usr/bin/env python3
"""AES-GCM-128 with the tag, GHASH built the reference's bit-serial way (ghash_tables = 0) against GHASH from the carry-less
multiply tables (CircuitBuilder(ghash_tables=lanes)), on one GPU.

    python3 tools/gpu_ghash_bench.py                  the 1 KiB circuit built three ways -- off, lanes = 1, lanes = 8 -- in ONE
                                                      process on the same card, their runs alternated: GHASH_BENCH_BATCH (256)
                                                      proofs per call through the device path (p2_prove_batch_device, inputs and
                                                      proofs in HBM, on a caller's stream), one warm-up, then the median of 5 timed calls each
    python3 tools/gpu_ghash_bench.py 65536 LANES      the 64 KiB circuit with one setting (one process per setting: the
                                                      workspaces are tens of GB): GHASH_BENCH_BIG_BATCH (2) proofs per call through
                                                      prove_batch, one warm-up, then the median of 3 calls

Per setting: degree_bits, ops, levels, build seconds, blob bytes, load seconds (upload and the constants | sigmas commitment),
seconds per proof, and the host verifier's verdict on a proof of the timed circuit, whose ciphertext and tag are read back from
the witness run and compared with the native cipher's.  Appends one JSON line per setting to profiles/ghash_bench.jsonl and
prints it."""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("GHASH_BENCH_OUT", os.path.join(ROOT, "profiles", "ghash_bench.jsonl"))
B = int(os.environ.get("GHASH_BENCH_BATCH", "256"))
BIG_B = int(os.environ.get("GHASH_BENCH_BIG_BATCH", "2"))
REPEATS, BIG_REPEATS, DISTINCT = 5, 3, 16


def build(pkg, L, lanes, count):
    """the circuit, `count` witnesses (key, nonce and plaintext only) and what the native cipher makes of them"""
    r = random.Random(L + lanes)
    t0 = time.perf_counter()
    b = pkg.CircuitBuilder(ghash_tables=lanes)
    t = pkg.AesGcmTarget.build(b, 4, 10, L, True)
    data = b.build()
    build_s = time.perf_counter() - t0
    maps, want = [], []
    for _ in range(count):
        key, iv, pt = (bytes(r.randrange(256) for _ in range(n)) for n in (16, 12, L))
        maps.append(dict(zip(t.key + t.nonce + t.pt, key + iv + pt)))
        ct, tag = pkg.native.gcm_encrypt(key, iv, pt)
        want.append(list(ct) + list(tag))
    t0 = time.perf_counter()
    data.gpu()
    load_s = time.perf_counter() - t0
    info = data.info
    rec = {"L": L, "ghash_tables": lanes, "degree_bits": info["degree_bits"], "num_ops": info["num_ops"], "num_levels": info["num_levels"],
           "build_s": round(build_s, 3), "blob_bytes": len(data.blob), "load_s": round(load_s, 3), "proof_bytes": data.proof_bytes}
    return data, t, maps, want, rec


def check(data, t, maps, want, rec):
    """one proof with the ciphertext and tag read back from its witness run, through the host verifier"""
    proofs, st, vals = data.prove_batch(maps[:1], outputs=t.ct + t.tag)
    assert st == [0] and vals[0] == want[0], "the circuit does not compute the native ciphertext and tag"
    try:
        data.verify(proofs[0])
        rec["verified"] = True
    except Exception as e:  # the verdict is part of the record
        rec["verified"] = False
        rec["verify_error"] = str(e)


def emit(rec):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def small(pkg, L):
    distinct = min(DISTINCT, B)
    runs = []
    H = None
    for lanes in (0, 1, 8):
        data, t, maps, want, rec = build(pkg, L, lanes, distinct)
        check(data, t, maps, want, rec)
        if H is None:  # the HIP runtime the library loaded
            H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
            H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            H.hipStreamSynchronize.argtypes = [C.c_void_p]
            caller = C.c_void_p()
            assert H.hipStreamCreate(C.byref(caller)) == 0
        maps = (maps * (B // distinct + 1))[:B]
        targets = list(maps[0])
        vals = (C.c_uint64 * (B * len(targets)))(*[m[x] for m in maps for x in targets])
        d = {}
        for key, nbytes in (("vals", C.sizeof(vals)), ("proofs", B * data.proof_bytes), ("st", 4 * B)):
            p = C.c_void_p()
            assert H.hipMalloc(C.byref(p), nbytes) == 0
            d[key] = p
        assert H.hipMemcpy(d["vals"], vals, C.sizeof(vals), 1) == 0
        runs.append({"data": data, "targets": targets, "d": d, "rec": rec, "s": []})

    def prove(r):
        t0 = time.perf_counter()
        r["data"].prove_batch_device(r["targets"], r["d"]["vals"].value, r["d"]["proofs"].value, r["d"]["st"].value, B, stream=caller)
        r["data"].synchronize()
        assert H.hipStreamSynchronize(caller) == 0
        return time.perf_counter() - t0

    for r in runs:  # warm-up: the workspaces
        prove(r)
        out = (C.c_int * B)()
        assert H.hipMemcpy(out, r["d"]["st"], 4 * B, 2) == 0 and list(out) == [0] * B
    for _ in range(REPEATS):  # alternated: every build sees the same card in the same state
        for r in runs:
            r["s"].append(prove(r))
    for r in runs:
        med = statistics.median(r["s"])
        r["rec"].update({"batch": B, "repeats": REPEATS, "s_per_proof": round(med / B, 6), "proofs_per_s": round(B / med, 2),
                         "proofs_per_s_runs": [round(B / s, 2) for s in r["s"]]})
        emit(r["rec"])


def big(pkg, L, lanes):
    data, t, maps, want, rec = build(pkg, L, lanes, BIG_B)
    print("built: n=2^%d ops=%d levels=%d blob=%dMB in %.1fs, loaded in %.1fs" % (rec["degree_bits"], rec["num_ops"], rec["num_levels"], rec["blob_bytes"] >> 20,
                                                                                 rec["build_s"], rec["load_s"]), flush=True)
    check(data, t, maps, want, rec)   # also the warm-up
    times = []
    for _ in range(BIG_REPEATS):
        t0 = time.perf_counter()
        proofs, st = data.prove_batch(maps)
        times.append(time.perf_counter() - t0)
        assert st == [0] * BIG_B
    med = statistics.median(times)
    rec.update({"batch": BIG_B, "repeats": BIG_REPEATS, "s_per_proof": round(med / BIG_B, 4), "s_per_proof_runs": [round(s / BIG_B, 4) for s in times]})
    emit(rec)


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    pkg = g.load_package()
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    if len(sys.argv) > 2:
        big(pkg, L, int(sys.argv[2]))
    else:
        small(pkg, L)


if __name__ == "__main__":
    main()
