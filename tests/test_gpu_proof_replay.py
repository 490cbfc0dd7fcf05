"""Keccak and public-input proofs held to the independent proof replay of tests/proof_ref.py.  The CPU oracle hashes with
Poseidon and hard-codes the public-inputs hash 0^4, so it cannot follow these proofs past the wires commitment; the replay
(pinned on the oracle's own proofs by tests/test_proof_ref_host.py) can: transcript, caps, Merkle paths, opened leaves,
openings and FRI of the last proof of a batch of three are compared with it exactly, and the vanishing identity at zeta holds
as tests/vanishing_ref.py restates it."""
import ctypes as C

import numpy as np
import pytest

import circuits
import keccak_circuits
import oracle_lib
import proof_ref as R
import vanishing_ref

pytestmark = pytest.mark.gpu

# the smallest circuits that reach every shape: lookup columns, salted leaves (zk), a non-zero public-inputs hash under both
# hashers, and no FRI round at all (poseidon_cipher, 2^4 rows, which also has no lookups and uses all 135 wires)
CASES = [("keccak", "aes_gcm_13"), ("keccak", "aes_gcm_13_tag"), ("keccak", "zk"), ("keccak", "public_inputs"),
         ("keccak", "poseidon_cipher"), ("poseidon", "public_inputs")]
PI_CASES = [c for c in CASES if c[1] == "public_inputs"]
ALL_COLUMNS_MAX_BITS = 13  # above: first, last and six evenly spaced columns of every opening section
_cache = {}


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.fixture(scope="module")
def kpkg(gpu):
    return keccak_circuits.KeccakPkg(gpu)


def _build(pkg_view, name):
    """keccak_circuits.build(pkg_view, name, 3); the AES-GCM L = 13 circuits, which it builds with the one witness of the
    reference's test, get three witnesses here so that the proof looked at is not the first of its batch."""
    if name in ("aes_gcm_13", "aes_gcm_13_tag"):
        keys = [(bytes([i + 1, 42] * 8), bytes([111 + i] * 12), bytes([(42 + 3 * i + j) & 255 for j in range(13)])) for i in range(3)]
        return circuits.encrypt(pkg_view, 4, 13, name.endswith("_tag"), keys)[:2]
    return keccak_circuits.build(pkg_view, name, 3)


class Proven:
    """The last proof of a batch of three, its replayed transcript and what the device held for it (read once, right after
    proving, so that nothing a later test runs on the handle can stand between the proof and its buffers)."""

    def __init__(self, gpu, pkg_view, hasher, name):
        self.data, pws = _build(pkg_view, name)
        data = self.data
        self.info = info = dict(data.info)
        assert info["hasher"] == hasher and info["degree_bits"] <= 14
        if info["zero_knowledge"]:
            data.set_zk_seed(5)
        proofs, st = data.prove_batch(pws)
        assert st == [0, 0, 0] and len(set(proofs)) == 3
        self.last = last = 2
        self.proof, self.vd = proofs[last], data.verifier_data()
        self.hasher = R.keccak_hasher() if hasher == "keccak" else R.poseidon_hasher()
        self.other_hasher = R.poseidon_hasher() if hasher == "keccak" else R.keccak_hasher()
        self.S = R.sections(info)
        self.pi_hash = R.hash_public_inputs(R.trailer_values(info, self.proof))
        self.t = R.replay_transcript(info, self.vd, self.proof, self.pi_hash)
        n, N, W = 1 << info["degree_bits"], 8 << info["degree_bits"], info["num_wires"]
        salt = 4 if info["zero_knowledge"] else 0

        def read(name, index, cap):
            return np.frombuffer(data.debug_read_bytes(name, index, cap=cap), dtype=np.uint64)

        self.challenges = [int(w) for w in read("challenges", last, 128)]
        self.dev_pi_hash = [int(w) for w in read("public_inputs_hash", last, 4)]
        self.zs_cap = [int(w) for w in read("zs_cap", last, 64)]
        self.quotient_cap = [int(w) for w in read("quotient_cap", last, 64)]
        lde = read("wires_lde", last, (W + salt) * N).reshape(-1, N)
        self.lde_rows = lde[:, self.t["query_indices"]].T.copy()  # [query][materialised wires | salt]
        del lde
        self.wires_coeffs = read("wires_coeffs", last, W * n).reshape(-1, n)
        self.quotient_coeffs = read("quotient_coeffs", last, info["num_quotient_cols"] * n).reshape(-1, n)
        self.pre_coeffs = read("pre_coeffs", 0, (info["num_constants_cols"] + R.ROUTED) * n).reshape(-1, n)
        self.zs = read("zs", last, info["num_zs_cols"] * n).reshape(-1, n)
        self.fri_in = read("fri_final_poly_in", last, 2 * n).reshape(2, n)


def _proven(gpu, kpkg, case):
    if case not in _cache:
        _cache[case] = Proven(gpu, kpkg if case[0] == "keccak" else gpu, *case)
    return _cache[case]


@pytest.fixture(params=CASES, ids=["-".join(c) for c in CASES])
def proven(request, gpu, kpkg):
    return _proven(gpu, kpkg, request.param)


def host_reason(pkg, data, proof):
    try:
        data.verify(proof)
        return ""
    except pkg.P2Error as e:
        return str(e).split("verify failed: ", 1)[1]


# ---------------------------------------------------------------------------------------------- transcript
def test_transcript(proven):
    """k_pi_hash, k_challenger, k_pow / k_pow_finish: every challenge word, the PoW witness and the 28 indices."""
    p, t, ch = proven, proven.t, proven.challenges
    nr = p.info["num_fri_rounds"]
    assert p.dev_pi_hash == p.pi_hash
    assert (p.pi_hash != [0, 0, 0, 0]) == bool(p.info["num_public_inputs"])
    stages = [("betas|gammas", ch[0:4], t["betas"] + t["gammas"]),
              ("deltas", ch[4:12] if t["deltas"] else [], t["deltas"]),
              ("alphas", ch[12:14], t["alphas"]),
              ("zeta", ch[14:16], t["zeta"]),
              ("fri_alpha", ch[16:18], t["fri_alpha"]),
              ("fri_betas", ch[18:18 + 2 * nr], t["fri_betas"]),
              ("pow_witness", ch[34:35], t["pow_witness"]),
              ("query_indices", ch[36:36 + 28], t["query_indices"])]
    for name, got, want in stages:
        assert got == want, "stage %s differs from the replay (first divergence in transcript order)" % name
    assert len(t["fri_betas"]) == 2 * nr and bool(t["deltas"]) == R.shape(p.info)["lookups"]
    assert t["pow_ok"], "the PoW witness %#x does not satisfy the replayed response %#x" % (t["pow_witness"][0], t["pow_response"])


# ---------------------------------------------------------------------------------------------- caps and paths
def test_caps_and_merkle_paths(proven):
    """k_kc_leaves / k_kc_fri_leaves / k_kc_level (k_hash_fri_leaves, k_merkle_level, k_merkle_top* under Poseidon) and
    k_write_queries: all 28 queries, four initial trees and every FRI round, against the caps."""
    p = proven
    assert p.zs_cap == R.words(p.proof, p.S, "zs_cap")
    assert p.quotient_cap == R.words(p.proof, p.S, "quotient_cap")
    idx = p.t["query_indices"]
    assert R.check_merkle(p.info, p.vd, p.proof, idx, p.hasher) is None
    # the check tells the two hashers apart
    wrong = R.check_merkle(p.info, p.vd, p.proof, idx, p.other_hasher)
    assert wrong is not None and ("Merkle path" in wrong or "out of range" in wrong), wrong


# ---------------------------------------------------------------------------------------------- leaves
def test_wires_leaves(proven):
    """The wires leaf of query x is row x of the LDE the device holds, salt columns included.  Row order, from the oracle's
    commit_from_coeffs: leaf x holds every column's value at g w^rev(x), the transform's bit-reversed storage order; columns
    the device does not materialise (routed-only circuits) are identically zero."""
    p, info = proven, proven.info
    W, salt = info["num_wires"], 4 if info["zero_knowledge"] else 0
    act = p.lde_rows.shape[1] - salt
    assert act in (R.ROUTED, W) and p.wires_coeffs.shape[0] == act
    lde_bits = info["degree_bits"] + R.RATE_BITS
    w = R.root_of_unity(lde_bits)
    first, last = p.wires_coeffs[0].tolist(), p.wires_coeffs[act - 1].tolist()
    for q, x in enumerate(p.t["query_indices"]):
        leaf = R.words(p.proof, p.S, "q%d_init1_leaf" % q)
        row = [int(v) for v in p.lde_rows[q]]
        assert len(leaf) == W + salt
        assert leaf[:act] == row[:act], "query %d" % q
        assert leaf[act:W] == [0] * (W - act), "query %d" % q
        assert leaf[W:] == row[act:], "query %d (salt)" % q
        point = R.GENERATOR * pow(w, R.rev_bits(x, lde_bits), R.P) % R.P
        for col, coeffs in ((0, first), (act - 1, last)):
            acc = 0
            for c in reversed(coeffs):
                acc = (acc * point + c) % R.P
            assert leaf[col] == acc, "query %d column %d is not the polynomial's value at g w^rev(x)" % (q, col)
    if salt:
        assert any(any(R.words(p.proof, p.S, "q%d_init1_leaf" % q)[W:]) for q in range(28))


# ---------------------------------------------------------------------------------------------- openings
def _pick(k, all_columns):
    if all_columns or k <= 8:
        return list(range(k))
    return sorted({0, k - 1} | {round((i + 1) * (k - 1) / 7) for i in range(6)})


def test_openings(proven):
    """k_eval_polys_refs: each open_* section from the coefficient columns the device holds (the Z columns' coefficients from
    their values by the oracle's inverse FFT), at the replayed zeta, and at g zeta for zs_next and lookup_zs_next.  Every
    column for n <= 2^13; for n = 2^14 the first, the last and six evenly spaced columns of each section."""
    p, info = proven, proven.info
    bits = info["degree_bits"]
    n, sh = 1 << bits, R.shape(info)
    all_columns = bits <= ALL_COLUMNS_MAX_BITS
    ncc, nzpp, zc = info["num_constants_cols"], sh["nzpp"], sh["zc"]
    zeta = tuple(p.t["zeta"])
    g_zeta = R.xmul(zeta, (R.root_of_unity(bits), 0))
    zcoef = np.ascontiguousarray(p.zs).copy()
    for col in zcoef:
        oracle_lib.lib().orc_fft(col.ctypes.data_as(C.POINTER(C.c_uint64)), bits, 1)
    act = p.wires_coeffs.shape[0]
    wires = np.zeros((info["num_wires"], n), dtype=np.uint64)
    wires[:act] = p.wires_coeffs
    groups = [("constants", p.pre_coeffs[:ncc], zeta), ("sigmas", p.pre_coeffs[ncc:], zeta), ("wires", wires, zeta),
              ("zs", zcoef[:R.NUM_CHALLENGES], zeta), ("zs_next", zcoef[:R.NUM_CHALLENGES], g_zeta),
              ("lookup_zs", zcoef[nzpp:zc], zeta), ("lookup_zs_next", zcoef[nzpp:zc], g_zeta),
              ("partial_products", zcoef[R.NUM_CHALLENGES:nzpp], zeta), ("quotient", p.quotient_coeffs, zeta)]
    assert p.pre_coeffs.shape[0] == ncc + R.ROUTED and zcoef.shape[0] == zc
    for name, cols, point in groups:
        want = R.ext_words(p.proof, p.S, "open_" + name)
        assert len(want) == cols.shape[0], name
        pick = _pick(len(want), all_columns)
        if pick:
            assert R.eval_openings(cols[pick], n, point) == [want[i] for i in pick], "open_" + name


# ---------------------------------------------------------------------------------------------- FRI
def test_fri(proven):
    """k_fri_compose / k_fri_divide / k_fri_fold and the FRI leaves: the composition value of all 28 queries, every fold, the
    final polynomial; and final_poly is the device's FRI input folded at the replayed betas (the input itself without a round)."""
    p = proven
    assert R.check_fri(p.info, p.proof, p.t, p.t["query_indices"]) is None
    betas = list(zip(p.t["fri_betas"][0::2], p.t["fri_betas"][1::2]))
    coeffs = list(zip(p.fri_in[0].tolist(), p.fri_in[1].tolist()))
    assert R.fold_coefficients(coeffs, betas) == R.ext_words(p.proof, p.S, "final_poly")
    if not betas:
        assert R.words(p.proof, p.S, "final_poly") == [int(w) for w in p.fri_in.T.reshape(-1)]


# ---------------------------------------------------------------------------------------------- vanishing identity
def test_vanishing_identity(proven):
    """k_quotient (k_ecstep_post) and the openings: the quotient the device committed to satisfies the identity as
    tests/vanishing_ref.py restates it, under the replayed challenges -- not only as the product's verifiers evaluate it."""
    p = proven
    assert vanishing_ref.check_vanishing(p.info, p.data.blob, p.proof, p.t) is None


# ---------------------------------------------------------------------------------------------- both verifiers
def test_tampers_replay_host_and_gpu(gpu, kpkg):
    """The teeth list of the host tests on one Keccak proof (n = 2^13), one batch through verify_batch and one host call per
    case: the GPU verdict equals the host's, and neither accepts what the replay rejects."""
    p = _proven(gpu, kpkg, ("keccak", "aes_gcm_13"))
    hasher = R.memoised(p.hasher)
    assert R.replay(p.info, p.vd, p.proof, hasher, blob=p.data.blob) is None
    cases = R.tamper_cases(p.info, p.proof)
    assert len(cases) == 3 + 9 + 2 + 2 + 3 * (12 + 3 * 2)
    got = p.data.verify_batch([c[1] for c in cases] + [p.proof])
    assert got[-1] == gpu.VERIFY_OK
    for (label, bad), code in zip(cases, got):
        verdict = R.replay(p.info, p.vd, bad, hasher)
        host_code = gpu.VERIFY_REASONS[host_reason(gpu, p.data, bad)]
        assert verdict is not None, label
        assert code != gpu.VERIFY_OK, (label, verdict)
        assert code == host_code, (label, verdict, code, host_code)


@pytest.mark.parametrize("case", PI_CASES, ids=["-".join(c) for c in PI_CASES])
def test_public_input_values_are_bound(gpu, kpkg, case):
    """One bit of a public-input value in the trailer: the hash the transcript observes moves, so the replay rejects, and so do
    both verifiers."""
    p = _proven(gpu, kpkg, case)
    bad = dict(R.tamper_cases(p.info, p.proof))["pi_values"]
    assert R.hash_public_inputs(R.trailer_values(p.info, bad)) != p.pi_hash
    t = R.replay_transcript(p.info, p.vd, bad, R.hash_public_inputs(R.trailer_values(p.info, bad)))
    assert t["betas"] != p.t["betas"]
    assert R.replay(p.info, p.vd, bad, R.memoised(p.hasher)) is not None
    code = p.data.verify_batch([bad, p.proof])
    assert code[0] == gpu.VERIFY_REASONS[host_reason(gpu, p.data, bad)] != gpu.VERIFY_OK and code[1] == gpu.VERIFY_OK
