#!/usr/bin/env python3
"""ElGamal encryption with and without the EcStepGate on one GPU: the arithmetic-gate circuit (2^14 rows, what bench.py
measures) against the step-gate circuit (2^10 rows), both handles in ONE process on the same card, their runs alternated.

Per circuit: proofs per second at ECSTEP_BENCH_BATCH (256) proofs per call through the device path (p2_prove_batch_device,
inputs and proofs in HBM, calls alternating between two caller streams as bench.py issues them), median of 5 timed runs
after one warm-up; and the time of witness generation alone for the same batch through p2_witness_batch (host inputs, the
ciphertext read back), median of 5.  Both circuits prove the same statements: the ciphertexts read back are compared.

Appends one JSON line to profiles/ecstep_bench.jsonl and prints it."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("ECSTEP_BENCH_OUT", os.path.join(ROOT, "profiles", "ecstep_bench.jsonl"))
B = int(os.environ.get("ECSTEP_BENCH_BATCH", "256"))
STEPS = int(os.environ.get("ECSTEP_BENCH_STEPS", "3"))
REPEATS, DISTINCT = 5, 64


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    import ec_circuits

    pkg = g.load_package()
    distinct = min(DISTINCT, B)
    H = None
    runs = {}
    for name, ec_gate in (("arithmetic_gates", False), ("step_gate", True)):
        data, pws, (pk_t, nonce_t, msg_t, ct_t), _ = ec_circuits.elgamal(pkg, list(range(1, distinct + 1)), ec_gate=ec_gate)
        maps = ([pw.map for pw in pws] * (B // distinct + 1))[:B]
        targets = list(maps[0])
        outs = ct_t[0] + ct_t[1]
        first, st = data.prove_batch(maps[:1])  # loads the circuit and the HIP runtime
        assert st == [0]
        data.verify(first[0])
        if H is None:
            H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
            H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            H.hipStreamSynchronize.argtypes = [C.c_void_p]
            callers = [C.c_void_p(), C.c_void_p()]
            for s in callers:
                assert H.hipStreamCreate(C.byref(s)) == 0
        vals = (C.c_uint64 * (B * len(targets)))(*[m[t] for m in maps for t in targets])
        d = {}
        for key, nbytes in (("vals", C.sizeof(vals)), ("proofs", B * data.proof_bytes), ("st", 4 * B)):
            p = C.c_void_p()
            assert H.hipMalloc(C.byref(p), nbytes) == 0
            d[key] = p
        assert H.hipMemcpy(d["vals"], vals, C.sizeof(vals), 1) == 0
        runs[name] = {"data": data, "maps": maps, "targets": targets, "outs": outs, "d": d, "prove_s": [], "witness_s": []}

    def sync(data):
        data.synchronize()
        for s in callers:
            assert H.hipStreamSynchronize(s) == 0

    def prove(r, steps):
        t0 = time.perf_counter()
        for k in range(steps):
            r["data"].prove_batch_device(r["targets"], r["d"]["vals"].value, r["d"]["proofs"].value, r["d"]["st"].value, B, stream=callers[k % 2])
        sync(r["data"])
        return time.perf_counter() - t0

    def witness(r):
        t0 = time.perf_counter()
        vals, st = r["data"].generate_witness(r["maps"], r["outs"])
        dt = time.perf_counter() - t0
        assert st == [0] * B
        return dt, vals

    read_back = {}
    for name, r in runs.items():  # warm-up: the workspaces
        prove(r, 1)
        out = (C.c_int * B)()
        assert H.hipMemcpy(out, r["d"]["st"], 4 * B, 2) == 0 and list(out) == [0] * B
        read_back[name] = witness(r)[1]
    assert read_back["arithmetic_gates"] == read_back["step_gate"], "the two circuits disagree on a ciphertext"
    for _ in range(REPEATS):  # alternated: both circuits see the same card in the same state
        for r in runs.values():
            r["prove_s"].append(prove(r, STEPS))
        for r in runs.values():
            r["witness_s"].append(witness(r)[0])
    res = {"workload": "elgamal", "batch": B, "distinct_witnesses": distinct, "steps": STEPS, "repeats": REPEATS}
    for name, r in runs.items():
        info = r["data"].info
        res[name] = {"degree_bits": info["degree_bits"], "num_ops": info["num_ops"], "num_levels": info["num_levels"], "proof_bytes": r["data"].proof_bytes,
                     "proofs_per_s": round(B * STEPS / statistics.median(r["prove_s"]), 2),
                     "proofs_per_s_runs": [round(B * STEPS / t, 2) for t in r["prove_s"]],
                     "witness_batch_ms": round(1e3 * statistics.median(r["witness_s"]), 3),
                     "witness_batch_ms_runs": [round(1e3 * t, 3) for t in r["witness_s"]]}
    res["step_gate_over_arithmetic_gates"] = round(res["step_gate"]["proofs_per_s"] / res["arithmetic_gates"]["proofs_per_s"], 3)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
