#!/usr/bin/env python3
"""ElGamal on ecGFp5 in GPU batches and the circuit they feed, on one GPU, everything in ONE process, runs alternated, medians
of ELGAMAL_BENCH_REPEATS (5) after a warm-up.

  native   the _device forms of decompress, encode_binary (16 attempts), elgamal and hashed-elgamal encrypt and decrypt and
           scalar_bits at 2^10, 2^14 and 2^16 items, buffers in HBM, on a stream of the caller's; in the same rounds
           p2_schnorr_sign_batch_device (msg_len 5) as a yardstick -- it is also two ladders per item.  64 rows of every output
           are compared with the host twins.
           Baseline: a host loop over the single-item entry points on 64 items, one core, through ctypes -- the call overhead of
           ctypes is in the figure (a few microseconds against milliseconds per item).
  circuit  the ec_gate=True ElGamal circuit (tests/ec_circuits.py) at ELGAMAL_BENCH_BATCH (256) proofs per call through
           p2_prove_batch_device, once with the inputs prepared on the device (encode_binary, scalar_bits and the value matrix
           assembled by device-to-device copies, all on the proving stream) and once with the inputs prepared by the host loop
           (p2_ecgfp5_encode_binary_padded per item, the bits spelled on the host, one upload); the two alternated.

Appends one JSON line to profiles/elgamal_bench.jsonl and prints it."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("ELGAMAL_BENCH_OUT", os.path.join(ROOT, "profiles", "elgamal_bench.jsonl"))
REPEATS = int(os.environ.get("ELGAMAL_BENCH_REPEATS", "5"))
SIZES = [1 << int(b) for b in os.environ.get("ELGAMAL_BENCH_BITS", "10,14,16").split(",")]
B = int(os.environ.get("ELGAMAL_BENCH_BATCH", "256"))
STEPS = int(os.environ.get("ELGAMAL_BENCH_STEPS", "3"))
ATTEMPTS, MSG_LEN, N_HOST = 16, 5, 64
P = 0xFFFFFFFF00000001


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    import ec_circuits

    pkg = g.load_package()
    L = pkg.lib()
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    u64p, u32p, vp, ip = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_int)
    rng = np.random.default_rng(10)
    n_max = max(SIZES + [B])

    def scalars(n):  # below 2^318 < n, and not zero
        return np.ascontiguousarray(rng.integers(1, 1 << 62, size=(n, 5), dtype=np.uint64))

    sk, nonce = scalars(n_max), scalars(n_max)
    limbs = np.ascontiguousarray(rng.integers(0, 1 << 32, size=(n_max, 5), dtype=np.uint32))
    pad = np.ascontiguousarray(rng.integers(0, 1 << 32, size=(n_max, ATTEMPTS, 5), dtype=np.uint32))
    m5 = np.ascontiguousarray(rng.integers(0, P, size=(n_max, MSG_LEN), dtype=np.uint64))
    # the first call loads the HIP runtime
    warm = np.zeros((N_HOST, 10), dtype=np.uint64)
    wst = np.full(N_HOST, -1, dtype=np.int32)
    assert L.p2_ecgfp5_decompress_batch(m5.ctypes.data_as(u64p), N_HOST, warm.ctypes.data_as(u64p), wst.ctypes.data_as(ip), 0) == 0, L.p2_last_error()

    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    H.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    H.hipMemcpy2DAsync.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, vp]
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
    d_sk, d_k, d_limbs, d_pad, d_m5 = dalloc(sk.nbytes, sk), dalloc(nonce.nbytes, nonce), dalloc(limbs.nbytes, limbs), dalloc(pad.nbytes, pad), dalloc(m5.nbytes, m5)
    d_pk, d_msg, d_used, d_c0, d_c1, d_back = dalloc(80 * n_max), dalloc(80 * n_max), dalloc(4 * n_max), dalloc(80 * n_max), dalloc(80 * n_max), dalloc(80 * n_max)
    d_h0, d_ct, d_hback, d_dec, d_bits, d_sig, d_spk = (dalloc(80 * n_max), dalloc(40 * n_max), dalloc(40 * n_max), dalloc(80 * n_max), dalloc(8 * 320 * n_max), dalloc(72 * n_max),
                                                        dalloc(80 * n_max))
    names = ("encode", "decompress", "encrypt", "decrypt", "hashed_encrypt", "hashed_decrypt", "scalar_bits", "schnorr_sign")
    d_st = {k: dalloc(4 * n_max) for k in names + ("mul",)}
    # public keys once: pk = sk G
    gen = np.zeros(10, dtype=np.uint64)
    L.p2_ecgfp5_generator(gen.ctypes.data_as(u64p))
    d_gen = dalloc(80 * n_max, np.ascontiguousarray(np.tile(gen, (n_max, 1))))
    assert L.p2_ecgfp5_mul_batch_device(d_sk, d_gen, n_max, d_pk, d_st["mul"], 0, s) == 0 and H.hipStreamSynchronize(s) == 0
    assert not read(d_st["mul"], n_max, np.int32).any()
    d_w = dalloc(40 * n_max)  # compressed points: the u halves of what encode makes

    def forms(n):
        return {"encode": lambda: L.p2_ecgfp5_encode_binary_batch_device(d_limbs, d_pad, ATTEMPTS, n, d_msg, d_used, d_st["encode"], 0, s),
                "decompress": lambda: L.p2_ecgfp5_decompress_batch_device(d_w, n, d_dec, d_st["decompress"], 0, s),
                "encrypt": lambda: L.p2_elgamal_encrypt_batch_device(d_pk, d_k, d_msg, n, d_c0, d_c1, d_st["encrypt"], 0, s),
                "decrypt": lambda: L.p2_elgamal_decrypt_batch_device(d_sk, d_c0, d_c1, n, d_back, d_st["decrypt"], 0, s),
                "hashed_encrypt": lambda: L.p2_hashed_elgamal_encrypt_batch_device(d_pk, d_k, d_m5, n, d_h0, d_ct, d_st["hashed_encrypt"], 0, s),
                "hashed_decrypt": lambda: L.p2_hashed_elgamal_decrypt_batch_device(d_sk, d_h0, d_ct, n, d_hback, d_st["hashed_decrypt"], 0, s),
                "scalar_bits": lambda: L.p2_ecgfp5_scalar_bits_device(d_k, n, d_bits, 320, 0, s),
                "schnorr_sign": lambda: L.p2_schnorr_sign_batch_device(d_sk, d_k, d_m5, MSG_LEN, n, d_sig, d_spk, d_st["schnorr_sign"], 0, s)}

    res = {"attempts": ATTEMPTS, "repeats": REPEATS, "native": {}}
    for n in SIZES:
        runs = {k: [] for k in names}
        for rep in range(REPEATS + 1):            # the first round warms up (and makes what the later kernels of a round read)
            for name, fn in forms(n).items():     # alternated: every round runs every kernel once
                t0 = time.perf_counter()
                assert fn() == 0, L.p2_last_error()
                assert H.hipStreamSynchronize(s) == 0
                if rep:
                    runs[name].append(1e3 * (time.perf_counter() - t0))
                if name == "encode" and rep == 0:  # decompress reads the compressed forms of what encode made
                    u = np.ascontiguousarray(read(d_msg, (n, 10))[:, 5:])
                    assert H.hipMemcpy(d_w, u.ctypes.data_as(vp), u.nbytes, 1) == 0
        undecoded = int(read(d_st["encode"], n, np.int32).sum())
        for name in names[1:-2] + names[-1:]:
            assert not read(d_st[name], n, np.int32).any(), name
        res["native"][str(n)] = {name: {"ms": round(statistics.median(v), 3), "ms_runs": [round(t, 3) for t in v], "per_s": round(n / statistics.median(v) * 1e3)}
                                 for name, v in runs.items()}
        res["native"][str(n)]["encode_items_without_a_point"] = undecoded
        assert (read(d_back, (n, 10)) == read(d_msg, (n, 10))).all() and (read(d_hback, (n, 5)) == m5[:n]).all(), "round trips"
        assert (read(d_dec, (n, 10)) == read(d_msg, (n, 10))).all(), "decompress of compress"

    # the device's outputs against the host twins, and the host loops
    g_pk, g_msg, g_used, g_c0, g_c1, g_back = (read(d_pk, (N_HOST, 10)), read(d_msg, (N_HOST, 10)), read(d_used, N_HOST, np.uint32), read(d_c0, (N_HOST, 10)),
                                               read(d_c1, (N_HOST, 10)), read(d_back, (N_HOST, 10)))
    g_h0, g_ct, g_hback = read(d_h0, (N_HOST, 10)), read(d_ct, (N_HOST, 5)), read(d_hback, (N_HOST, 5))
    h = {k: np.zeros((N_HOST, w), dtype=np.uint64) for k, w in (("msg", 10), ("dec", 10), ("c0", 10), ("c1", 10), ("back", 10), ("h0", 10), ("ct", 5), ("hback", 5))}
    h_used = np.zeros(N_HOST, dtype=np.uint32)
    p64 = lambda a, i: a[i].ctypes.data_as(u64p)  # noqa: E731

    def host_encode():
        for i in range(N_HOST):
            L.p2_ecgfp5_encode_binary_padded(limbs[i].ctypes.data_as(u32p), pad[i].ctypes.data_as(u32p), ATTEMPTS, p64(h["msg"], i), h_used[i:].ctypes.data_as(u32p))

    def host_decompress():
        for i in range(N_HOST):
            L.p2_ecgfp5_decompress(g_msg[i][5:].ctypes.data_as(u64p), p64(h["dec"], i))

    def host_encrypt():
        for i in range(N_HOST):
            assert L.p2_elgamal_encrypt(p64(g_pk, i), p64(nonce, i), p64(g_msg, i), p64(h["c0"], i), p64(h["c1"], i)) == 0

    def host_decrypt():
        for i in range(N_HOST):
            assert L.p2_elgamal_decrypt(p64(sk, i), p64(g_c0, i), p64(g_c1, i), p64(h["back"], i)) == 0

    def host_hashed_encrypt():
        for i in range(N_HOST):
            assert L.p2_hashed_elgamal_encrypt(p64(g_pk, i), p64(nonce, i), p64(m5, i), p64(h["h0"], i), p64(h["ct"], i)) == 0

    def host_hashed_decrypt():
        for i in range(N_HOST):
            assert L.p2_hashed_elgamal_decrypt(p64(sk, i), p64(g_h0, i), p64(g_ct, i), p64(h["hback"], i)) == 0

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    host = {}
    for name, fn in (("encode", host_encode), ("decompress", host_decompress), ("encrypt", host_encrypt), ("decrypt", host_decrypt), ("hashed_encrypt", host_hashed_encrypt),
                     ("hashed_decrypt", host_hashed_decrypt)):
        t = statistics.median(timed(fn) for _ in range(3))
        host[name] = {"n": N_HOST, "ms": round(t, 3), "per_s": round(N_HOST / t * 1e3, 1)}
    for k, dev in (("msg", g_msg), ("dec", g_msg), ("c0", g_c0), ("c1", g_c1), ("back", g_back), ("h0", g_h0), ("ct", g_ct), ("hback", g_hback)):
        assert (h[k] == dev).all(), "device and host disagree on " + k
    assert (h_used == g_used).all()
    res["host_loop_one_core_ctypes"] = host

    # ---- the circuit: B proofs per call, inputs prepared on the device against inputs prepared by the host loop
    data, _, (pk_t, nonce_t, msg_t, ct_t), _ = ec_circuits.elgamal(pkg, [], ec_gate=True)
    targets = pk_t + msg_t + nonce_t
    n_t, pb = len(targets), data.proof_bytes
    d_vals, d_proofs, d_pst = dalloc(8 * n_t * B), dalloc(B * pb), dalloc(4 * B)
    callers = [vp(), vp()]
    for c in callers:
        assert H.hipStreamCreate(C.byref(c)) == 0
    h_pk = read(d_pk, (B, 10))

    def prepare_device(c):
        assert L.p2_ecgfp5_encode_binary_batch_device(d_limbs, d_pad, ATTEMPTS, B, d_msg, d_used, d_st["encode"], 0, c) == 0
        assert L.p2_ecgfp5_scalar_bits_device(d_k, B, vp(d_vals.value + 8 * 20), n_t, 0, c) == 0
        assert H.hipMemcpy2DAsync(d_vals, 8 * n_t, d_pk, 80, 80, B, 3, c) == 0
        assert H.hipMemcpy2DAsync(vp(d_vals.value + 80), 8 * n_t, d_msg, 80, 80, B, 3, c) == 0

    def prepare_host(c):
        vals = np.zeros((B, n_t), dtype=np.uint64)
        vals[:, :10] = h_pk
        used = C.c_uint32()
        for i in range(B):
            assert L.p2_ecgfp5_encode_binary_padded(limbs[i].ctypes.data_as(u32p), pad[i].ctypes.data_as(u32p), ATTEMPTS, vals[i, 10:20].ctypes.data_as(u64p), C.byref(used)) == 0
        vals[:, 20:] = (nonce[:B, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]).reshape(B, 320) & np.uint64(1)
        assert H.hipMemcpyAsync(d_vals, vals.ctypes.data_as(vp), vals.nbytes, 1, c) == 0
        assert H.hipStreamSynchronize(c) == 0      # `vals` goes out of scope

    def prove(prepare, steps):
        t0 = time.perf_counter()
        for k in range(steps):
            prepare(callers[0])                    # one value matrix: the calls of a run share a stream
            data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=callers[0])
        data.synchronize()
        for c in callers:
            assert H.hipStreamSynchronize(c) == 0
        return time.perf_counter() - t0

    runs = {"inputs_on_device": (prepare_device, []), "inputs_by_host_loop": (prepare_host, [])}
    proofs = {}
    for name, (prep, _) in runs.items():           # warm-up: the workspace; and both ways must make the same proofs
        prove(prep, 1)
        assert not read(d_pst, B, np.int32).any(), name
        proofs[name] = read(d_proofs, B * pb, np.uint8)
    assert (proofs["inputs_on_device"] == proofs["inputs_by_host_loop"]).all(), "the two ways of preparing inputs give different proofs"
    data.verify(bytes(proofs["inputs_on_device"][:pb]))
    for _ in range(REPEATS):                       # alternated
        for prep, times in runs.values():
            times.append(prove(prep, STEPS))
    res["circuit"] = {"batch": B, "steps": STEPS, "degree_bits": data.info["degree_bits"], "proof_bytes": pb}
    for name, (_, times) in runs.items():
        res["circuit"][name] = {"proofs_per_s": round(B * STEPS / statistics.median(times), 2), "proofs_per_s_runs": [round(B * STEPS / t, 2) for t in times]}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
