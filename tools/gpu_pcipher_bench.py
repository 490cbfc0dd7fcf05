#!/usr/bin/env python3
"""The Poseidon cipher in GPU batches on one GPU, everything in ONE process, runs alternated, medians of PCIPHER_BENCH_REPEATS
(5) after a warm-up, lowest and highest beside each median.

  native    the _device forms of encrypt and decrypt at l in 3, 129, 1023 and 2^10, 2^14, 2^16 messages, buffers in HBM, on a
            stream of the caller's; permutations/s counts the five permutations of every hash_state (the closing one runs four).
  yardstick in the same rounds p2_gpu_poseidon, the plain batch permutation, on count * 5 (pad3(l) / 3 + 1) states, capped at
            PCIPHER_BENCH_YARD_STATES (2^21) -- that entry point takes host pointers, so its time includes both copies over PCIe
            and it is a lower bound of the kernel's rate, not the kernel's rate.
  host      a loop over p2_native_poseidon_encrypt / _decrypt on 64 items, one core, through ctypes.
  sealed    seal_batch and open_batch (Python lists in and out, two resp. one ecgfp5.mul_batch and the cipher) at 2^16, l = 3.

Appends one JSON line to profiles/pcipher_bench.jsonl and prints it."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("PCIPHER_BENCH_OUT", os.path.join(ROOT, "profiles", "pcipher_bench.jsonl"))
REPEATS = int(os.environ.get("PCIPHER_BENCH_REPEATS", "5"))
SIZES = [1 << int(b) for b in os.environ.get("PCIPHER_BENCH_BITS", "10,14,16").split(",")]
LENGTHS = [int(x) for x in os.environ.get("PCIPHER_BENCH_LENGTHS", "3,129,1023").split(",")]
YARD = int(os.environ.get("PCIPHER_BENCH_YARD_STATES", str(1 << 21)))
SEALED = 1 << int(os.environ.get("PCIPHER_BENCH_SEALED_BITS", "16"))
N_HOST = 64
P = 0xFFFFFFFF00000001


def stats(times, per_call):
    med = statistics.median(times)
    return {"ms": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "per_s": round(per_call / med * 1e3)}


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    pkg = g.load_package()
    L = pkg.lib()
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    u64p, vp = C.POINTER(C.c_uint64), C.c_void_p
    rng = np.random.default_rng(11)
    n_max, l_max = max(SIZES), max(LENGTHS)
    pad3 = lambda l: (l + 2) // 3 * 3  # noqa: E731
    warm = np.zeros((1, 12), dtype=np.uint64)
    assert L.p2_gpu_poseidon(warm.ctypes.data_as(u64p), 1, 0) == 0, L.p2_last_error()   # the first call loads the HIP runtime

    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(vp)]
    H.hipStreamSynchronize.argtypes = [vp]

    def dalloc(nbytes, host=None):
        p = vp()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        if host is not None:
            assert H.hipMemcpy(p, host.ctypes.data_as(vp), host.nbytes, 1) == 0
        return p

    def read(p, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert H.hipMemcpy(out.ctypes.data_as(vp), p, out.nbytes, 2) == 0
        return out

    s = vp()
    assert H.hipStreamCreate(C.byref(s)) == 0
    ks = np.ascontiguousarray(rng.integers(0, P, size=(n_max, 10), dtype=np.uint64))
    nonce = np.ascontiguousarray(rng.integers(0, P, size=(n_max, 2), dtype=np.uint64))
    # message words: 2^12 random rows of the longest length, repeated -- what the words are does not change the work
    block = np.ascontiguousarray(rng.integers(0, P, size=(min(n_max, 1 << 12) * 5 * l_max,), dtype=np.uint64))
    d_ks, d_nonce = dalloc(ks.nbytes, ks), dalloc(nonce.nbytes, nonce)
    d_msg = dalloc(8 * 5 * l_max * n_max)
    for off in range(0, 8 * 5 * l_max * n_max, block.nbytes):
        assert H.hipMemcpy(vp(d_msg.value + off), block.ctypes.data_as(vp), min(block.nbytes, 8 * 5 * l_max * n_max - off), 1) == 0
    d_ct, d_back = dalloc(8 * 5 * (pad3(l_max) + 1) * n_max), dalloc(8 * 5 * l_max * n_max)
    d_st = [dalloc(4 * n_max), dalloc(4 * n_max)]
    yard = np.ascontiguousarray(rng.integers(0, P, size=(YARD, 12), dtype=np.uint64))

    res = {"repeats": REPEATS, "native": {}, "yardstick_states_cap": YARD}
    for l in LENGTHS:
        hashes = pad3(l) // 3 + 1
        for n in SIZES:
            states = min(n * 5 * hashes, YARD)
            forms = {"encrypt": lambda: L.p2_poseidon_encrypt_batch_device(d_ks, d_nonce, d_msg, l, n, d_ct, d_st[0], 0, s),
                     "decrypt": lambda: L.p2_poseidon_decrypt_batch_device(d_ks, d_nonce, d_ct, l, n, d_back, d_st[1], 0, s),
                     "plain_poseidon_host_pointers": lambda: L.p2_gpu_poseidon(yard.ctypes.data_as(u64p), states, 0)}
            runs = {k: [] for k in forms}
            for rep in range(REPEATS + 1):        # the first round warms up, and makes the ciphertexts that decrypt reads
                for name, fn in forms.items():    # alternated: every round runs every form once
                    t0 = time.perf_counter()
                    assert fn() == 0, L.p2_last_error()
                    assert H.hipStreamSynchronize(s) == 0
                    if rep:
                        runs[name].append(1e3 * (time.perf_counter() - t0))
            assert not read(d_st[0], n, np.int32).any() and not read(d_st[1], n, np.int32).any()
            assert (read(d_back, (N_HOST * 5 * l,)) == read(d_msg, (N_HOST * 5 * l,))).all(), "round trip"
            perms = n * (5 * hashes - 1)
            row = {"encrypt": stats(runs["encrypt"], n), "decrypt": stats(runs["decrypt"], n), "plain_poseidon_host_pointers": stats(runs["plain_poseidon_host_pointers"], states)}
            row["plain_poseidon_host_pointers"]["states"] = states
            for k in ("encrypt", "decrypt"):
                row[k]["permutations_per_s"] = round(perms / row[k]["ms"] * 1e3)
                row[k]["elements_per_s"] = round(n * l / row[k]["ms"] * 1e3)
            res["native"]["l=%d,n=%d" % (l, n)] = row

    # the host twins on 64 items, and the device's rows against them
    host = {}
    for l in LENGTHS:
        nct = pad3(l) + 1
        assert L.p2_poseidon_encrypt_batch_device(d_ks, d_nonce, d_msg, l, N_HOST, d_ct, d_st[0], 0, s) == 0 and H.hipStreamSynchronize(s) == 0
        g_msg, g_ct = read(d_msg, (N_HOST, 5 * l)), read(d_ct, (N_HOST, 5 * nct))
        h_ct, h_back = np.zeros_like(g_ct), np.zeros_like(g_msg)
        p64 = lambda a, i: a[i].ctypes.data_as(u64p)  # noqa: E731

        def host_encrypt():
            for i in range(N_HOST):
                L.p2_native_poseidon_encrypt(p64(ks, i), p64(g_msg, i), l, p64(nonce, i), p64(h_ct, i))

        def host_decrypt():
            for i in range(N_HOST):
                assert L.p2_native_poseidon_decrypt(p64(ks, i), p64(g_ct, i), nct, p64(nonce, i), l, p64(h_back, i)) == 0

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return 1e3 * (time.perf_counter() - t0)

        host["l=%d" % l] = {name: stats([timed(fn) for _ in range(3)], N_HOST) for name, fn in (("encrypt", host_encrypt), ("decrypt", host_decrypt))}
        assert (h_ct == g_ct).all() and (h_back == g_msg).all(), "device and host disagree at l = %d" % l
    res["host_loop_one_core_ctypes"] = host

    # seal_batch / open_batch: the whole Python call, lists in and out
    PN, E = pkg.poseidon_native, pkg.ecgfp5
    n = SEALED
    pyr = np.random.default_rng(12)
    sks = [int(x) for x in pyr.integers(1, 1 << 62, size=n)]
    rs = [int(x) for x in pyr.integers(1, 1 << 62, size=n)]
    nonces = [tuple(int(v) for v in row) for row in nonce[:n]]
    msgs = [[tuple(int(v) for v in row[5 * j:5 * j + 5]) for j in range(3)] for row in pyr.integers(0, P, size=(n, 15), dtype=np.uint64)]
    pks, st = E.mul_batch(sks, [E.generator()] * n)
    assert not any(st)
    t_seal, t_open = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        Rs, cts, st = PN.seal_batch(pks, rs, nonces, msgs)
        t1 = time.perf_counter()
        back, st2 = PN.open_batch(sks, Rs, nonces, cts, 3)
        t2 = time.perf_counter()
        assert not any(st) and not any(st2) and back == msgs
        if rep:
            t_seal.append(1e3 * (t1 - t0))
            t_open.append(1e3 * (t2 - t1))
    res["sealed_python_lists"] = {"n": n, "l": 3, "seal_batch": stats(t_seal, n), "open_batch": stats(t_open, n)}

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
