#!/usr/bin/env python3
"""AES-GCM in GPU batches on one GPU, everything in ONE process, runs alternated, medians of GCM_BENCH_REPEATS (5) after a
warm-up, lowest and highest beside each median.

  (a) batch      2^16 items of 1 KiB, AES-128, 13-byte aad: encryptions/s and decryptions/s through the _device forms (buffers in
                 HBM, a stream of the caller's) and through the host-pointer forms (both copies over PCIe inside the call); the
                 host loop on one core over the twins on 64 items; the time of each kernel of an encryption
                 (p2_gpu_gcm_kernel_times: events between the launches) and the bytes a call has to move over the 8 TB/s of HBM.
  (b) long       256 items of 64 KiB with the GHASH kernel forced to LANES = 1 and to LANES = 64.
  (c) crossover  the GHASH kernel alone at 2, 8, 32, 128, 512 and 4096 blocks per item, both lane counts, count x blocks = 2^22:
                 `threshold` is the smallest block count from which LANES = 64 is faster by more than the spread of the runs
                 (the larger of the two ranges) at that and every larger size -- the constant GCM_WIDE_MIN_BLOCKS of
                 csrc/prover_gpu.hip.
  (d) proofs     256 proofs of the AES-GCM 1 KiB circuit with a 13-byte aad (ghash_tables = 1): inputs prepared on the device
                 (gcm_encrypt_batch_device, bytes_to_words_device, prove_batch_device on one stream) against the same proofs
                 from the host loop (gcm_encrypt per item, one assignment per proof, prove_batch).

Appends one JSON line to profiles/gcm_bench.jsonl and prints it."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("GCM_BENCH_OUT", os.path.join(ROOT, "profiles", "gcm_bench.jsonl"))
REPEATS = int(os.environ.get("GCM_BENCH_REPEATS", "5"))
N_BATCH = 1 << int(os.environ.get("GCM_BENCH_BITS", "16"))
N_PROOFS = int(os.environ.get("GCM_BENCH_PROOFS", "256"))
FILL = 1 << int(os.environ.get("GCM_BENCH_FILL_BITS", "22"))
BLOCKS = (2, 8, 32, 128, 512, 4096)
N_HOST = 64
HBM_PEAK = 8e12


def stats(times, per_call):
    med = statistics.median(times)
    return {"ms": round(med, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "per_s": round(per_call / med * 1e3)}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g

    pkg = g.load_package()
    L, N = pkg.lib(), pkg.native
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    vp = C.c_void_p
    warm = (C.c_uint64 * 3)()
    assert L.p2_gpu_gcm_kernel_times(4, 16, 0, 1, 0, 1, warm, 0) == 0, L.p2_last_error()   # the first call loads the HIP runtime

    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(vp)]
    H.hipStreamSynchronize.argtypes = [vp]

    def dalloc(nbytes, host=None):
        p = vp()
        assert H.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        if host is not None:
            assert H.hipMemcpy(p, host.ctypes.data_as(vp), host.nbytes, 1) == 0
        return p

    def read(p, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        assert H.hipMemcpy(out.ctypes.data_as(vp), p, nbytes, 2) == 0
        return out

    s = vp()
    assert H.hipStreamCreate(C.byref(s)) == 0
    rng = np.random.default_rng(11)
    res = {"repeats": REPEATS}

    def kernel_times(nk, length, aad_len, count, lanes):
        ns = (C.c_uint64 * (3 * REPEATS))()
        assert L.p2_gpu_gcm_kernel_times(nk, length, aad_len, count, lanes, REPEATS, ns, 0) == 0, L.p2_last_error()
        return [[ns[3 * r + k] / 1e6 for r in range(REPEATS)] for k in range(3)]

    # ---- (a)
    n, l, al, nk = N_BATCH, 1024, 13, 4
    key, iv, aad, pt = (np.ascontiguousarray(rng.integers(0, 256, size=(n, w), dtype=np.uint8)) for w in (16, 12, al, l))
    d_key, d_iv, d_aad, d_pt = dalloc(key.nbytes, key), dalloc(iv.nbytes, iv), dalloc(aad.nbytes, aad), dalloc(pt.nbytes, pt)
    d_ct, d_back, d_tag = dalloc(n * l), dalloc(n * l), dalloc(16 * n)
    d_st = [dalloc(4 * n), dalloc(4 * n)]
    d_work = dalloc(N.gcm_batch_workspace(nk, l, al, n))
    h_ct, h_back, h_tag = np.zeros((n, l), np.uint8), np.zeros((n, l), np.uint8), np.zeros((n, 16), np.uint8)
    h_st = (C.c_int * n)()
    u8 = lambda a: a.ctypes.data_as(C.c_char_p)  # noqa: E731
    forms = {
        "encrypt_device": lambda: L.p2_aes_gcm_encrypt_batch_device(d_key, nk, d_iv, d_aad, al, d_pt, l, l, n, d_ct, d_tag, d_st[0], d_work, 0, s),
        "decrypt_device": lambda: L.p2_aes_gcm_decrypt_batch_device(d_key, nk, d_iv, d_aad, al, d_ct, d_tag, l, l, n, d_back, d_st[1], d_work, 0, s),
        "encrypt_host_pointers": lambda: L.p2_aes_gcm_encrypt_batch(u8(key), nk, u8(iv), u8(aad), al, u8(pt), l, n, u8(h_ct), u8(h_tag), h_st, 0),
        "decrypt_host_pointers": lambda: L.p2_aes_gcm_decrypt_batch(u8(key), nk, u8(iv), u8(aad), al, u8(h_ct), u8(h_tag), l, n, u8(h_back), h_st, 0),
    }
    runs = {k: [] for k in forms}
    for rep in range(REPEATS + 1):            # the first round warms up, and makes the ciphertexts that the decryptions read
        for name, fn in forms.items():        # alternated: every round runs every form once
            t0 = time.perf_counter()
            assert fn() == 0, L.p2_last_error()
            assert H.hipStreamSynchronize(s) == 0
            if rep:
                runs[name].append(1e3 * (time.perf_counter() - t0))
    assert not read(d_st[0], 4 * n).any() and not read(d_st[1], 4 * n).any() and not any(h_st)
    assert (read(d_back, n * l).reshape(n, l) == pt).all() and (h_back == pt).all(), "round trip"
    assert (read(d_ct, n * l).reshape(n, l) == h_ct).all() and (read(d_tag, 16 * n).reshape(n, 16) == h_tag).all()
    a = {"items": n, "len": l, "aad_len": al, "nk": nk}
    a.update({k: stats(v, n) for k, v in runs.items()})
    moved = n * (2 * l + al + 4 * nk + 12 + 16 + 4)   # every input read once, every output written once
    a["bytes_moved_per_call"] = moved
    a["ms_at_hbm_peak"] = round(moved / HBM_PEAK * 1e3, 4)
    for k in ("encrypt_device", "decrypt_device"):
        a[k]["share_of_hbm_peak"] = round(moved / HBM_PEAK * 1e3 / a[k]["ms"], 4)
    kt = kernel_times(nk, l, al, n, 0)
    a["kernels_of_an_encryption"] = {name: stats(t, n) for name, t in zip(("k_gcm_setup", "k_gcm_ctr", "k_gcm_ghash"), kt)}
    total = sum(v["ms"] for v in a["kernels_of_an_encryption"].values())
    for v in a["kernels_of_an_encryption"].values():
        v["share"] = round(v["ms"] / total, 3)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    rows = [(bytes(key[i]), bytes(iv[i]), bytes(pt[i]), bytes(aad[i])) for i in range(N_HOST)]
    sealed = []

    def host_encrypt():
        sealed[:] = [N.gcm_encrypt(*r) for r in rows]

    def host_decrypt():
        for (k, nn, p, ad), (ct, tag) in zip(rows, sealed):
            assert N.gcm_decrypt(k, nn, ct, tag, ad) == p
    a["host_loop_one_core_ctypes"] = {"items": N_HOST, "encrypt": stats([timed(host_encrypt) for _ in range(3)], N_HOST),
                                      "decrypt": stats([timed(host_decrypt) for _ in range(3)], N_HOST)}
    assert all(bytes(h_ct[i]) == sealed[i][0] and bytes(h_tag[i]) == sealed[i][1] for i in range(N_HOST)), "device and host disagree"
    res["batch"] = a

    # ---- (b) and (c): p2_gpu_gcm_kernel_times with the lane count forced; the two lane counts alternate
    def lanes_pair(length, count):
        t = {1: [[], [], []], 64: [[], [], []]}
        for _ in range(2):                    # two calls of REPEATS runs per lane count, alternated; the first pair is dropped
            for lanes in (1, 64):
                t[lanes] = kernel_times(4, length, 0, count, lanes)
        return t

    t = lanes_pair(65536, 256)
    res["long"] = {"items": 256, "len": 65536,
                   "lanes_1": {"k_gcm_ctr": stats(t[1][1], 256), "k_gcm_ghash": stats(t[1][2], 256)},
                   "lanes_64": {"k_gcm_ctr": stats(t[64][1], 256), "k_gcm_ghash": stats(t[64][2], 256)}}
    cross, wins = {}, []
    for blocks in BLOCKS:
        count = FILL // blocks
        t = lanes_pair(16 * (blocks - 1), count)          # the length block is the last of `blocks`
        one, wide = stats(t[1][2], count), stats(t[64][2], count)
        spread = max(one["ms_max"] - one["ms_min"], wide["ms_max"] - wide["ms_min"])
        cross["blocks=%d" % blocks] = {"items": count, "lanes_1": one, "lanes_64": wide, "spread_ms": round(spread, 4)}
        wins.append(one["ms"] - wide["ms"] > spread)
    threshold = None
    for i in range(len(BLOCKS) - 1, -1, -1):
        if not wins[i]:
            break
        threshold = BLOCKS[i]
    res["crossover"] = {"fill_blocks": FILL, "ghash_kernel": cross, "threshold": threshold}

    # ---- (d)
    import gcm_circuits as K
    B, l = N_PROOFS, 1024
    data, t = K.gcm_aad(pkg, 4, l, al)
    targets = t.key + t.nonce + t.pt + t.aad + t.ct + t.tag
    n_t, pb = len(targets), data.proof_bytes
    unset = np.full(B * n_t, pkg.VALUE_UNSET, dtype=np.uint64)
    d_vals, d_proofs, d_pst = dalloc(unset.nbytes, unset), dalloc(B * pb), dalloc(4 * B)

    def device_path():
        assert L.p2_aes_gcm_encrypt_batch_device(d_key, 4, d_iv, d_aad, al, d_pt, l, l, B, d_ct, d_tag, d_st[0], d_work, 0, s) == 0
        col = 0
        for d_b, w in ((d_key, 16), (d_iv, 12), (d_pt, l), (d_aad, al), (d_ct, l), (d_tag, 16)):
            N.bytes_to_words_device(d_b, w, w, B, vp(d_vals.value + 8 * col), n_t, stream=s)
            col += w
        data.prove_batch_device(targets, d_vals.value, d_proofs.value, d_pst.value, B, stream=s)
        assert H.hipStreamSynchronize(s) == 0

    host_proofs = []

    def host_path():
        maps = []
        for i in range(B):
            k, nn, p, ad = bytes(key[i]), bytes(iv[i]), bytes(pt[i]), bytes(aad[i])
            ct, tag = N.gcm_encrypt(k, nn, p, ad)
            maps.append(dict(zip(targets, k + nn + p + ad + ct + tag)))
        proofs, st = data.prove_batch(maps)
        assert not any(st)
        host_proofs[:] = proofs

    runs = {"device_inputs": [], "host_loop_inputs": []}
    for rep in range(REPEATS + 1):
        for name, fn in (("device_inputs", device_path), ("host_loop_inputs", host_path)):
            ms = timed(fn)
            if rep:
                runs[name].append(ms)
    assert not read(d_pst, 4 * B).any()
    got = read(d_proofs, B * pb).tobytes()
    assert [got[k * pb:(k + 1) * pb] for k in range(B)] == host_proofs, "the two paths prove different bytes"
    data.verify(host_proofs[0])
    res["proofs"] = {"proofs": B, "len": l, "aad_len": al, "ghash_tables": 1, "degree_bits": data.info["degree_bits"],
                     "device_inputs": stats(runs["device_inputs"], B), "host_loop_inputs": stats(runs["host_loop_inputs"], B)}

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
