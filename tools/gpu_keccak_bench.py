#!/usr/bin/env python3
"""The Keccak configuration against the Poseidon one on one GPU, both hashers in the same run on the same card.

For AES-GCM 1 KiB, ElGamal encryption and AES-GCM 64 KiB (n = 2^19): proofs per second at KECCAK_BENCH_BATCH (256) proofs per
call through the device path (p2_prove_batch_device, inputs and proofs in HBM, calls alternating between two caller streams
as bench.py issues them), the latency of a single proof, the time of verify_batch_device on the batch, and the per-stage
times of p2_circuit_get_timing for one batch.  Medians of repeated runs after one warm-up.

Without arguments: one child process per (workload, hasher), each under its own time limit, stopping at the first that fails;
every child appends one JSON line to profiles/keccak_bench.jsonl and the parent prints the Keccak / Poseidon ratios.
`--child WORKLOAD HASHER` is one such measurement."""
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("KECCAK_BENCH_OUT", os.path.join(ROOT, "profiles", "keccak_bench.jsonl"))
B = int(os.environ.get("KECCAK_BENCH_BATCH", "256"))
WHICH = os.environ.get("KECCAK_BENCH_CIRCUITS", "aes_gcm_1k,elgamal,aes_gcm_64k").split(",")
# (steps per timed run, timed runs, distinct witnesses, time limit of the child in seconds)
PLAN = {"aes_gcm_1k": (5, 5, 256, 300), "elgamal": (3, 5, 64, 300), "aes_gcm_64k": (1, 3, 8, 900)}


def child(name, hasher):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    import circuits

    pkg = g.load_package()
    steps, repeats, distinct, _ = PLAN[name]
    distinct = min(distinct, B)

    class Pkg:  # the circuits of tests/circuits.py under the chosen hasher
        def __getattr__(self, n):
            return getattr(pkg, n)

        def CircuitBuilder(self, zero_knowledge=False):
            return pkg.CircuitBuilder(zero_knowledge=zero_knowledge, hasher=hasher)

    rnd = random.Random(7)
    if name == "elgamal":
        data, pws, _, _ = circuits.ecgfp5_elgamal(Pkg(), list(range(1, distinct + 1)))
    else:
        L = 1024 if name == "aes_gcm_1k" else 65536
        keys = [(bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(12)), bytes(rnd.randrange(256) for _ in range(L)))
                for _ in range(distinct)]
        data, pws, _ = circuits.encrypt(Pkg(), 4, L, False, keys)
    assert data.info["hasher"] == hasher
    pws = (pws * (B // len(pws) + 1))[:B]
    targets = list(pws[0].map)
    nt, pb = len(targets), data.proof_bytes
    vals = (C.c_uint64 * (B * nt))(*[pw.map[t] for pw in pws for t in targets])
    first, st = data.prove_batch(pws[:1])  # loads the circuit and the HIP runtime
    assert st == [0]
    data.verify(first[0])
    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipStreamSynchronize.argtypes = [C.c_void_p]

    def dalloc(nbytes, host=None):
        p = C.c_void_p()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        if host is not None:
            assert H.hipMemcpy(p, host, nbytes, 1) == 0
        return p

    d_vals, d_proofs, d_st, d_vst = dalloc(C.sizeof(vals), vals), dalloc(B * pb), dalloc(4 * B), dalloc(4 * B)
    callers = [C.c_void_p(), C.c_void_p()]
    for s in callers:
        assert H.hipStreamCreate(C.byref(s)) == 0

    def sync():
        data.synchronize()
        for s in callers:
            assert H.hipStreamSynchronize(s) == 0

    def statuses(d):
        out = (C.c_int * B)()
        assert H.hipMemcpy(out, d, 4 * B, 2) == 0
        return list(out)

    def run(batch, n_steps):
        t0 = time.perf_counter()
        for k in range(n_steps):
            data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_st.value, batch, stream=callers[k % 2])
        sync()
        return time.perf_counter() - t0

    run(B, 1)  # warm-up: the workspaces
    assert statuses(d_st) == [0] * B
    ts = [run(B, steps) for _ in range(repeats)]
    res = {"circuit": name, "hasher": hasher, "batch": B, "distinct_witnesses": distinct, "degree_bits": data.info["degree_bits"], "proof_bytes": pb,
           "steps": steps, "repeats": repeats, "proofs_per_s": round(B * steps / statistics.median(ts), 2),
           "proofs_per_s_runs": [round(B * steps / t, 2) for t in ts]}
    # verification of the batch just proven, in HBM
    def verify():
        t0 = time.perf_counter()
        data.verify_batch_device(d_proofs.value, d_vst.value, B, stream=callers[0])
        sync()
        return time.perf_counter() - t0

    verify()
    assert statuses(d_vst) == [0] * B
    res["verify_batch_device_ms"] = round(1e3 * statistics.median(verify() for _ in range(max(repeats, 3))), 3)
    # per-stage times of one batch
    h = data.gpu()
    pkg.lib().p2_circuit_set_timing(h, 1)
    run(B, 1)
    arr = (pkg.api._KernelTime * 128)()
    k = pkg.lib().p2_circuit_get_timing(h, arr, 128)
    pkg.lib().p2_circuit_set_timing(h, 0)
    res["stage_ms"] = {arr[i].name.decode(): round(arr[i].ms, 3) for i in range(min(k, 128))}
    res["stage_launches"] = {arr[i].name.decode(): arr[i].count for i in range(min(k, 128))}
    # one proof at a time (the workspaces stay those of the batch)
    run(1, 1)
    res["single_proof_ms"] = round(1e3 * statistics.median(run(1, 1) for _ in range(9)), 3)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


def main():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    done = {}
    for name in WHICH:
        for hasher in ("poseidon", "keccak"):
            limit = PLAN[name][3]
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", name, hasher], capture_output=True, text=True)
            if r.returncode != 0:  # nothing more on the GPU after a failure
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("%s / %s failed with exit status %d" % (name, hasher, r.returncode))
            done[(name, hasher)] = json.loads(r.stdout.strip().splitlines()[-1])
        p, k = done[(name, "poseidon")], done[(name, "keccak")]
        print(json.dumps({"circuit": name, "poseidon_proofs_per_s": p["proofs_per_s"], "keccak_proofs_per_s": k["proofs_per_s"],
                          "keccak_over_poseidon": round(k["proofs_per_s"] / p["proofs_per_s"], 3),
                          "single_proof_ms": [p["single_proof_ms"], k["single_proof_ms"]],
                          "verify_batch_device_ms": [p["verify_batch_device_ms"], k["verify_batch_device_ms"]]}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
