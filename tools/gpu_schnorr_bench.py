#!/usr/bin/env python3
"""Native ecGFp5 batches and the signature circuit on one GPU, everything in ONE process, runs alternated, medians of
SCHNORR_BENCH_REPEATS (5) after a warm-up.

  native   p2_schnorr_verify_batch_device, p2_schnorr_sign_batch_device and p2_ecgfp5_mul_batch_device at 2^10, 2^14 and 2^16 items,
           msg_len 5, buffers in HBM, on a stream of the caller's.  The signatures verified are the ones the signing kernel
           made (all must be accepted); 64 rows of every output are compared with the host twins.
           Baseline: a host loop over p2_schnorr_verify / p2_schnorr_sign / p2_ecgfp5_mul on 64 items, one core, through ctypes
           -- the call overhead of ctypes is in the figure (a few microseconds against milliseconds per item).
  circuit  proofs per second of the ec_gate=True signature circuit (pk and a 5-word message public) at SCHNORR_BENCH_BATCH (256)
           proofs per call through p2_prove_batch_device, beside the ElGamal step-gate circuit of tools/gpu_ecstep_bench.py, the
           two alternated as that tool alternates its circuits.

Appends one JSON line to profiles/schnorr_bench.jsonl and prints it."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("SCHNORR_BENCH_OUT", os.path.join(ROOT, "profiles", "schnorr_bench.jsonl"))
REPEATS = int(os.environ.get("SCHNORR_BENCH_REPEATS", "5"))
SIZES = [1 << int(b) for b in os.environ.get("SCHNORR_BENCH_BITS", "10,14,16").split(",")]
B = int(os.environ.get("SCHNORR_BENCH_BATCH", "256"))
STEPS = int(os.environ.get("SCHNORR_BENCH_STEPS", "3"))
MSG_LEN, N_HOST, DISTINCT = 5, 64, 64
P = 0xFFFFFFFF00000001


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    import ec_circuits

    pkg = g.load_package()
    L = pkg.lib()
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    u64p, vp, ip = C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_int)
    rng = np.random.default_rng(9)
    n_max = max(SIZES)

    def scalars(n):  # below 2^318 < n, and not zero
        k = rng.integers(1, 1 << 62, size=(n, 5), dtype=np.uint64)
        return np.ascontiguousarray(k)

    sk, nonce = scalars(n_max), scalars(n_max)
    msg = np.ascontiguousarray(rng.integers(0, P, size=(n_max, MSG_LEN), dtype=np.uint64))
    # the first call loads the HIP runtime
    sig = np.zeros((n_max, 9), dtype=np.uint64)
    pk = np.zeros((n_max, 10), dtype=np.uint64)
    status = np.full(n_max, -1, dtype=np.int32)
    assert L.p2_schnorr_sign_batch(sk.ctypes.data_as(u64p), nonce.ctypes.data_as(u64p), msg.ctypes.data_as(u64p), MSG_LEN, N_HOST, sig.ctypes.data_as(u64p),
                                   pk.ctypes.data_as(u64p), status.ctypes.data_as(ip), 0) == 0, L.p2_last_error()

    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(vp)]
    H.hipStreamSynchronize.argtypes = [vp]

    def dalloc(nbytes, host=None):
        p = vp()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        if host is not None:
            assert H.hipMemcpy(p, host.ctypes.data_as(vp), nbytes, 1) == 0
        return p

    def read(p, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert H.hipMemcpy(out.ctypes.data_as(vp), p, out.nbytes, 2) == 0
        return out

    s = vp()
    assert H.hipStreamCreate(C.byref(s)) == 0
    d_sk, d_k, d_msg = dalloc(sk.nbytes, sk), dalloc(nonce.nbytes, nonce), dalloc(msg.nbytes, msg)
    d_sig, d_pk, d_out = dalloc(72 * n_max), dalloc(80 * n_max), dalloc(80 * n_max)
    d_st = {k: dalloc(4 * n_max) for k in ("sign", "verify", "mul")}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        assert H.hipStreamSynchronize(s) == 0
        return 1e3 * (time.perf_counter() - t0)

    def forms(n):
        return {"sign": lambda: L.p2_schnorr_sign_batch_device(d_sk, d_k, d_msg, MSG_LEN, n, d_sig, d_pk, d_st["sign"], 0, s),
                "verify": lambda: L.p2_schnorr_verify_batch_device(d_pk, d_msg, MSG_LEN, d_sig, n, d_st["verify"], 0, s),
                "mul": lambda: L.p2_ecgfp5_mul_batch_device(d_k, d_pk, n, d_out, d_st["mul"], 0, s)}

    res = {"msg_len": MSG_LEN, "repeats": REPEATS, "native": {}}
    for n in SIZES:
        runs = {k: [] for k in ("sign", "verify", "mul")}
        for rep in range(REPEATS + 1):            # the first round warms up (and signs what verify reads)
            for name, fn in forms(n).items():     # alternated: every round runs every kernel once
                t0 = time.perf_counter()
                assert fn() == 0, L.p2_last_error()
                assert H.hipStreamSynchronize(s) == 0
                if rep:
                    runs[name].append(1e3 * (time.perf_counter() - t0))
        for name in runs:
            assert not read(d_st[name], n, np.int32).any(), name
        res["native"][str(n)] = {name: {"ms": round(statistics.median(v), 3), "ms_runs": [round(t, 3) for t in v], "per_s": round(n / statistics.median(v) * 1e3)}
                                 for name, v in runs.items()}
    # the device's outputs against the host twins, and the host loops
    g_sig, g_pk, g_out = read(d_sig, (n_max, 9)), read(d_pk, (n_max, 10)), read(d_out, (n_max, 10))
    h_sig, h_pk, h_out = np.zeros((N_HOST, 9), dtype=np.uint64), np.zeros((N_HOST, 10), dtype=np.uint64), np.zeros((N_HOST, 10), dtype=np.uint64)
    st = C.c_int()

    def host_sign():
        for i in range(N_HOST):
            assert L.p2_schnorr_sign(sk[i].ctypes.data_as(u64p), nonce[i].ctypes.data_as(u64p), msg[i].ctypes.data_as(u64p), MSG_LEN, h_sig[i].ctypes.data_as(u64p),
                                     h_pk[i].ctypes.data_as(u64p), C.byref(st)) == 0 and st.value == 0

    def host_verify():
        for i in range(N_HOST):
            assert L.p2_schnorr_verify(h_pk[i].ctypes.data_as(u64p), msg[i].ctypes.data_as(u64p), MSG_LEN, h_sig[i].ctypes.data_as(u64p), C.byref(st)) == 0 and st.value == 0

    def host_mul():
        for i in range(N_HOST):
            L.p2_ecgfp5_mul(nonce[i].ctypes.data_as(u64p), h_pk[i].ctypes.data_as(u64p), h_out[i].ctypes.data_as(u64p))

    host = {}
    for name, fn in (("sign", host_sign), ("verify", host_verify), ("mul", host_mul)):
        t = statistics.median(timed(fn) for _ in range(3))
        host[name] = {"n": N_HOST, "ms": round(t, 3), "per_s": round(N_HOST / t * 1e3, 1)}
    assert (g_sig[:N_HOST] == h_sig).all() and (g_pk[:N_HOST] == h_pk).all() and (g_out[:N_HOST] == h_out).all(), "device and host disagree"
    res["host_loop_one_core_ctypes"] = host

    # ---- the circuits
    b = pkg.CircuitBuilder(ec_gate=True)
    pk_t, msg_t = b.add_virtual_point_target(), b.add_virtual_target_arr(MSG_LEN)
    b.register_public_inputs(pk_t + msg_t)
    sig_t = b.add_virtual_schnorr_signature_target()
    b.verify_schnorr_signature(pk_t, msg_t, sig_t)
    data = b.build()
    distinct = min(DISTINCT, B)
    maps = []
    for i in range(distinct):
        pw = pkg.PartialWitness()
        pw.set_target_arr(pk_t, [int(w) for w in g_pk[i]])
        pw.set_target_arr(msg_t, [int(w) for w in msg[i]])
        pw.set_schnorr_signature_target(sig_t, (sum(int(g_sig[i][j]) << (64 * j) for j in range(5)), [int(w) for w in g_sig[i][5:]]))
        maps.append(pw.map)
    eg_data, eg_pws, _, _ = ec_circuits.elgamal(pkg, list(range(1, distinct + 1)), ec_gate=True)
    callers = [vp(), vp()]
    for c in callers:
        assert H.hipStreamCreate(C.byref(c)) == 0
    runs = {}
    for name, d, ms in (("schnorr_step_gate", data, maps), ("elgamal_step_gate", eg_data, [pw.map for pw in eg_pws])):
        ms = (ms * (B // distinct + 1))[:B]
        targets = list(ms[0])
        first, st1 = d.prove_batch(ms[:1])
        assert st1 == [0]
        d.verify(first[0])
        vals = np.array([m[t] for m in ms for t in targets], dtype=np.uint64)
        runs[name] = {"data": d, "targets": targets, "vals": dalloc(vals.nbytes, vals), "proofs": dalloc(B * d.proof_bytes), "st": dalloc(4 * B), "prove_s": []}

    def prove(r, steps):
        t0 = time.perf_counter()
        for k in range(steps):
            r["data"].prove_batch_device(r["targets"], r["vals"].value, r["proofs"].value, r["st"].value, B, stream=callers[k % 2])
        r["data"].synchronize()
        for c in callers:
            assert H.hipStreamSynchronize(c) == 0
        return time.perf_counter() - t0

    for r in runs.values():   # warm-up: the workspaces
        prove(r, 1)
        assert not read(r["st"], B, np.int32).any()
    for _ in range(REPEATS):  # alternated
        for r in runs.values():
            r["prove_s"].append(prove(r, STEPS))
    res["circuit"] = {"batch": B, "steps": STEPS, "distinct_witnesses": distinct}
    for name, r in runs.items():
        info = r["data"].info
        res["circuit"][name] = {"degree_bits": info["degree_bits"], "proof_bytes": r["data"].proof_bytes,
                                "proofs_per_s": round(B * STEPS / statistics.median(r["prove_s"]), 2), "proofs_per_s_runs": [round(B * STEPS / t, 2) for t in r["prove_s"]]}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
