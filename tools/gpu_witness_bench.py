#!/usr/bin/env python3
"""Witness-only runs and witness outputs on one GPU.  For AES-GCM 1 KiB and ElGamal encryption, WITNESS_BENCH_BATCH witnesses
(default 256), one warm-up, then WITNESS_BENCH_REPEATS runs, medians:

  * witnesses/s of p2_witness_batch_device (inputs and outputs in HBM: the GPU work alone), inputs only set, the computed
    targets (ciphertext / ElGamal pair) read back;
  * p2_prove_batch_outputs against p2_prove_batch on the same inputs, alternated in one run;
  * ElGamal only: the host-native path (p2_elgamal_encrypt per witness, then prove the asserted witnesses) against the
    circuit-computed path (prove the inputs alone and read the pair back).

Appends one JSON line per circuit to profiles/witness_bench.jsonl and prints it."""
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
B = int(os.environ.get("WITNESS_BENCH_BATCH", "256"))
REPEATS = int(os.environ.get("WITNESS_BENCH_REPEATS", "5"))
WHICH = os.environ.get("WITNESS_BENCH_CIRCUITS", "aes_gcm_1k,elgamal").split(",")
OUT = os.path.join(ROOT, "profiles", "witness_bench.jsonl")


def flat(point):
    return list(point[0]) + list(point[1])


def workload(name):
    """(data, asserted witnesses, inputs-only witnesses, computed targets, host-native function or None)"""
    if name == "elgamal":
        data, pws, (pk_t, nonce_t, msg_t, ct_t), cases = circuits.ecgfp5_elgamal(pkg, list(range(1, B + 1)))
        ins = [dict(zip(pk_t + msg_t + nonce_t, flat(pk) + flat(msg) + [(nonce >> i) & 1 for i in range(320)])) for _, pk, msg, nonce, _ in cases]

        def natives():
            return [pkg.ecgfp5.elgamal_encrypt(pk, nonce, msg) for _, pk, msg, nonce, _ in cases]
        return data, [pw.map for pw in pws], ins, ct_t[0] + ct_t[1], natives
    rnd = random.Random(7)
    b = pkg.CircuitBuilder()
    t = pkg.AesGcmTarget.build(b, 4, 10, 1024, False)
    data = b.build()
    full, ins = [], []
    for _ in range(B):
        key, nonce, pt = bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(12)), bytes(rnd.randrange(256) for _ in range(1024))
        ct, tag = pkg.native.gcm_encrypt(key, nonce, pt)
        pw = pkg.PartialWitness()
        t.set_targets(pw, key, nonce, pt, ct, tag)
        full.append(pw.map)
        ins.append({k: pw.map[k] for k in t.key + t.nonce + t.pt + t.tag})   # TAG = false: the tag targets are inputs (zero)
    return data, full, ins, t.ct, None


def hip():
    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipDeviceSynchronize.argtypes = []
    return H


def median_ms(f):
    f()  # warm-up
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


for name in WHICH:
    data, full, ins, outs, natives = workload(name)
    want, st = data.generate_witness(ins, outs)
    assert st == [0] * B, st
    assert want == [[m[t] for t in outs] for m in full]   # the circuit computes what the natives assert
    res = {"circuit": name, "witnesses": B, "outputs": len(outs), "repeats": REPEATS, "degree_bits": data.info["degree_bits"]}
    # ---- device form: everything in HBM
    H = hip()
    targets = list(ins[0])
    vals = (C.c_uint64 * (B * len(targets)))(*[m[t] for m in ins for t in targets])
    d_in, d_out, d_st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for p, nbytes in ((d_in, C.sizeof(vals)), (d_out, 8 * B * len(outs)), (d_st, 4 * B)):
        assert H.hipMalloc(C.byref(p), nbytes) == 0
    assert H.hipMemcpy(d_in, vals, C.sizeof(vals), 1) == 0

    def device():
        data.witness_batch_device(targets, d_in.value, outs, d_out.value, d_st.value, B)
        assert H.hipDeviceSynchronize() == 0
    ms = median_ms(device)
    got = (C.c_uint64 * (B * len(outs)))()
    assert H.hipMemcpy(got, d_out, C.sizeof(got), 2) == 0 and list(got) == [v for w in want for v in w]
    for p in (d_in, d_out, d_st):
        H.hipFree(p)
    res["witness_batch_device_ms"] = round(ms, 2)
    res["witnesses_per_s"] = round(B / ms * 1e3, 1)
    res["witness_batch_host_ms"] = round(median_ms(lambda: data.generate_witness(ins, outs)), 2)
    # ---- proving with and without outputs, alternated
    plain, with_out = [], []
    data.prove_batch(full)
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        data.prove_batch(full)
        plain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        data.prove_batch(full, outs)
        with_out.append(time.perf_counter() - t0)
    res["prove_batch_ms"] = round(1e3 * statistics.median(plain), 2)
    res["prove_batch_outputs_ms"] = round(1e3 * statistics.median(with_out), 2)
    res["outputs_over_plain"] = round(res["prove_batch_outputs_ms"] / res["prove_batch_ms"], 4)
    # ---- who computes the answer: the host natives, or the circuit
    if natives is not None:
        def host_native_path():
            natives()
            data.prove_batch(full)
        res["natives_then_prove_ms"] = round(median_ms(host_native_path), 2)
        res["natives_ms"] = round(median_ms(natives), 2)
        res["prove_inputs_read_outputs_ms"] = round(median_ms(lambda: data.prove_batch(ins, outs)), 2)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")
    print(line, flush=True)
