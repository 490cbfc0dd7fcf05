"""Compressed proofs in GPU batches (p2_compress_batch / p2_decompress_batch / p2_verify_compressed_batch and their device forms)
against the host path of csrc/compress.h, byte for byte and verdict for verdict."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import circuits
import pi_circuits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky2-aes_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = 0xFFFFFFFF00000001
KERNELS = ["k_cmp_plan", "k_cmp_scatter", "k_cmp_reductions", "k_cmp_infer", "k_cmp_merkle", "k_cmp_pack", "k_cmp_emit", "k_cmp_finish"]


def test_compress_kernels_have_no_scratch(tmp_path):
    """The compiler's resource remarks for the new kernels (gfx950 cross-compile): no scratch memory."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "p.s"), os.path.join(CSRC, "prover_gpu.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    info, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = info.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    for k in KERNELS:
        names = [n for n in info if k in n]
        assert names, k
        for n in names:
            assert info[n]["ScratchSize"] == 0, (n, info[n])
            assert info[n]["VGPRs"] <= 128, (n, info[n])


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def _build(pkg, name):
    if name == "aes_gcm_1k":
        keys = [(bytes([i, 1] * 8), bytes([i + 1] * 12), bytes([(7 * i + j) & 255 for j in range(1024)])) for i in range(64)]
        data, pws, _ = circuits.encrypt(pkg, 4, 1024, False, keys)
    elif name == "elgamal":
        data, pws, _, _ = circuits.ecgfp5_elgamal(pkg, [1, 2, 3, 4])
    elif name == "zk":
        data, pws = circuits.zk_gf_2_8_add(pkg, [(1, 2), (0x57, 0x13), (255, 0), (9, 9)])
    elif name == "public_inputs":
        data, pws, _ = pi_circuits.aes_gcm(pkg, L=64, n=4)
    elif name == "aes_gcm_64k":
        keys = [(bytes([i + 3] * 16), bytes([i] * 12), bytes([i * 5 + 1] * 65536)) for i in range(2)]
        data, pws, _ = circuits.encrypt(pkg, 4, 65536, False, keys)
    return data, pws


_cache = {}


def _proven(pkg, name):
    if name not in _cache:
        data, pws = _build(pkg, name)
        proofs, st = data.prove_batch(pws)
        assert st == [0] * len(pws), st
        _cache[name] = (data, proofs)
    return (name,) + _cache[name]


@pytest.fixture(scope="module", params=["aes_gcm_1k", "elgamal", "zk", "public_inputs", "aes_gcm_64k"])
def proven(gpu, request):
    return _proven(gpu, request.param)


def host_reason(pkg, data, cproof):
    try:
        data.verify_compressed(cproof)
        return ""
    except pkg.P2Error as e:
        return str(e).split("verify_compressed failed: ", 1)[1]


@pytest.mark.gpu
def test_compress_batch_equals_host(gpu, proven):
    name, data, proofs = proven
    want = [data.compress(p) for p in proofs]
    got, st = data.compress_batch(proofs)
    assert st == [gpu.VERIFY_OK] * len(proofs)
    assert got == want
    assert all(len(c) < data.proof_bytes for c in got)


@pytest.mark.gpu
def test_decompress_batch_returns_the_proofs(gpu, proven):
    name, data, proofs = proven
    cps = [data.compress(p) for p in proofs]
    full, st = data.decompress_batch(cps)
    assert st == [gpu.VERIFY_OK] * len(proofs)
    assert full == proofs
    assert data.verify_compressed_batch(cps) == [gpu.VERIFY_OK] * len(proofs)


def _tampered(data, c, rnd):
    """Honest and tampered compressed proofs: a flipped bit anywhere, a non-canonical word, a wrong index, truncation."""
    b = bytearray(c)
    kind = rnd.randrange(5)
    if kind == 0:
        b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
    elif kind == 1:
        p = rnd.randrange(len(b) - 8)
        b[p:p + 8] = struct.pack("<Q", P + 1)
    elif kind == 2:
        return bytes(b[:-1])
    elif kind == 3:
        b += b"\0"
    else:
        p = rnd.randrange(len(b) // 2, len(b) - 8)
        b[p:p + 8] = struct.pack("<Q", struct.unpack_from("<Q", b, p)[0] ^ 2)
    return bytes(b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aes_gcm_1k", "elgamal", "zk", "public_inputs"])  # (host verdicts of 2^19-row proofs take seconds each)
def test_verdicts_equal_host(gpu, name):
    name, data, proofs = _proven(gpu, name)
    rnd = random.Random(5)
    cps = [data.compress(p) for p in proofs]
    batch = []
    for i, c in enumerate(cps[:16]):
        batch.append(c)
        batch.append(_tampered(data, c, rnd))
    got = data.verify_compressed_batch(batch)
    want = [gpu.VERIFY_REASONS[host_reason(gpu, data, c)] for c in batch]
    assert got == want
    assert got[0::2] == [gpu.VERIFY_OK] * len(cps[:16])


@pytest.mark.gpu
def test_edge_cases(gpu):
    _, data, proofs = _proven(gpu, "aes_gcm_1k")
    cps = [data.compress(p) for p in proofs]
    # a batch larger than one chunk, with zeroed slots and zero lengths
    data.set_option("verify_chunk", 7)
    try:
        batch = cps[:20] + [bytes(len(cps[0])), None]
        assert data.verify_compressed_batch(batch) == [gpu.VERIFY_OK] * 20 + [gpu.VERIFY_SHAPE] * 2
        got, st = data.compress_batch(proofs[:20] + [bytes(data.proof_bytes)])
        assert got[:20] == cps[:20] and st == [0] * 20 + [gpu.VERIFY_SHAPE] and got[20] is None
        full, st = data.decompress_batch(cps[:20] + [None])
        assert full[:20] == proofs[:20] and st == [0] * 20 + [gpu.VERIFY_SHAPE]
    finally:
        data.set_option("verify_chunk", 512)
    # a length above the stride is an error of the call
    with pytest.raises(gpu.P2Error, match="exceeds the stride"):
        data.verify_compressed_batch(cps[:2], lengths=[len(cps[0]), data.proof_bytes + 1])


def _hip():
    h = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    vp = C.c_void_p
    h.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    h.hipFree.argtypes = [vp]
    h.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    h.hipStreamCreate.argtypes = [C.POINTER(vp)]
    h.hipStreamSynchronize.argtypes = [vp]
    h.hipStreamDestroy.argtypes = [vp]
    return h


@pytest.mark.gpu
def test_device_chain_on_one_stream(gpu):
    """prove_batch_device -> compress_batch_device -> verify_compressed_batch_device -> decompress_batch_device on one stream,
    with no host synchronisation in between."""
    pkg = gpu
    H, H2D, D2H = _hip(), 1, 2
    data, pws = circuits.mix_columns(pkg, circuits.random_states(11, 6))
    B, pb = len(pws), data.proof_bytes
    targets = list(pws[0].map)
    vals = (C.c_uint64 * (B * len(targets)))(*[pw.map[t] for pw in pws for t in targets])
    sizes = {"vals": C.sizeof(vals), "proofs": B * pb, "cproofs": B * pb, "full": B * pb, "len": 4 * B, "pst": 4 * B, "cst": 4 * B,
             "vst": 4 * B, "dst": 4 * B}
    bufs = {k: C.c_void_p() for k in sizes}
    for k, b in bufs.items():
        assert H.hipMalloc(C.byref(b), sizes[k]) == 0
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        assert H.hipMemcpy(bufs["vals"], vals, sizes["vals"], H2D) == 0
        d = {k: b.value for k, b in bufs.items()}
        data.prove_batch_device(targets, d["vals"], d["proofs"], d["pst"], B, stream=s)
        data.compress_batch_device(d["proofs"], d["cproofs"], d["len"], d["cst"], B, stream=s)
        data.verify_compressed_batch_device(d["cproofs"], d["len"], d["vst"], B, stream=s)
        data.decompress_batch_device(d["cproofs"], d["len"], d["full"], d["dst"], B, stream=s)
        assert H.hipStreamSynchronize(s) == 0
        out = {k: (C.c_int * B)() for k in ("pst", "cst", "vst", "dst")}
        for k, o in out.items():
            assert H.hipMemcpy(o, bufs[k], 4 * B, D2H) == 0
            assert list(o) == [0] * B, k
        lens = (C.c_uint32 * B)()
        assert H.hipMemcpy(lens, bufs["len"], 4 * B, D2H) == 0
        proofs, full, cps = (C.create_string_buffer(B * pb) for _ in range(3))
        for buf, k in ((proofs, "proofs"), (full, "full"), (cps, "cproofs")):
            assert H.hipMemcpy(buf, bufs[k], B * pb, D2H) == 0
        assert full.raw == proofs.raw
        for i in range(B):
            p = proofs.raw[i * pb:(i + 1) * pb]
            assert cps.raw[i * pb:i * pb + lens[i]] == data.compress(p)
            assert cps.raw[i * pb + lens[i]:(i + 1) * pb] == bytes(pb - lens[i])
    finally:
        H.hipStreamDestroy(s)
        for b in bufs.values():
            H.hipFree(b)
