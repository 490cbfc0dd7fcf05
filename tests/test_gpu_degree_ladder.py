"""GPU tests (pytest -m gpu): whole proofs at the row counts between and beyond the ones the workloads produce.

Oracle rungs (byte for byte against the CPU oracle, then edge_circuits.gpu_proofs_hold's verifiers, replay and compressor):
degree_bits 2..5 have no FRI round (the final polynomial is the whole polynomial); at 2 the LDE has 32 leaves under 16 cap
entries, so every Merkle path is one sibling long.  Three circuit families: the routed-only arithmetic chain, one 26-entry
lookup table whose lookups set the rows, and PoseidonGate rows (135 wire columns, the two-walk quotient).

Validity rungs (degree_bits 16, 17, 18: 4, 8 and 16 linked segments in k_perm_seg_products / k_perm_scan and k_fri_seg_sums /
k_fri_divide) leave the oracle out on cost alone: a wrong link between two segments gives an invalid proof, not a slightly
different one, so the host verifier, the GPU verifier and the Python replay decide.

The sizes (n_ops, lookups, permutations) were found once on the CPU; every rung asserts the degree_bits and FRI rounds it
was chosen for."""
import pytest

import edge_circuits as E
import proof_ref
import verify_layout

pytestmark = pytest.mark.gpu

ROUNDS = {2: 0, 3: 0, 4: 0, 5: 0, 7: 1, 9: 1, 11: 2, 12: 2, 16: 3, 17: 3, 18: 4, 21: 4}
CHAIN_OPS = {2: 1, 3: 10, 4: 20, 5: 40, 7: 200, 9: 800, 11: 3000, 12: 6000, 16: 90000, 17: 180000, 18: 360000, 21: 3000000}
TABLE_LOOKUPS = {3: 40, 4: 240, 5: 800, 7: 4000, 9: 16000, 12: 120000}
HASH_PERMS = {2: 1, 5: 20, 7: 100, 9: 400, 12: 3000}
TABLE_16 = (400000, 50000)      # lookups (10 000 LookupGate rows: ten rows per thread of k_lookup_scan) and n_ops in front of them


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return pkg


def _seeds(bits, base):
    return [base + i for i in range(3 if bits <= 10 else 2)]


def _assert_rung(data, bits, luts):
    assert data.info["degree_bits"] == bits, data.info
    assert data.info["num_fri_rounds"] == ROUNDS[bits], data.info
    assert data.info["num_luts"] == luts
    S = verify_layout.sections(data.info)
    assert S["q0_init0_siblings"][1] == 32 * (bits + 3 - 4)        # bits = 2: one sibling
    assert S["final_poly"][1] == 16 * ((1 << bits) >> (4 * ROUNDS[bits]))
    if ROUNDS[bits] == 0:
        assert "fri_cap0" not in S


def _one_table(gpu, lookups, seeds, n_ops=0):
    table = E.spread_table(26, 7)
    picks = [E.random_picks([table], [lookups], s) for s in seeds]
    data, pws, sh = E.table_circuit(gpu, [table], picks, n_ops, seed=seeds[0])
    E.assert_table_shape(data, sh, [table], [lookups])
    return data, pws


# ---------------------------------------------------------------------------------------------- oracle rungs
@pytest.mark.parametrize("bits", [2, 3, 4, 5, 7, 9, 11, 12])
def test_chain_against_the_oracle(gpu, orc, bits):
    data, pws = E.chain(gpu, CHAIN_OPS[bits], _seeds(bits, 10 * bits))
    _assert_rung(data, bits, 0)
    E.gpu_proofs_hold(gpu, orc, data, pws, oracle=True)


@pytest.mark.parametrize("bits", [3, 4, 5, 7, 9, 12])
def test_one_table_against_the_oracle(gpu, orc, bits):
    data, pws = _one_table(gpu, TABLE_LOOKUPS[bits], _seeds(bits, 20 * bits))
    _assert_rung(data, bits, 1)
    E.gpu_proofs_hold(gpu, orc, data, pws, oracle=True)


@pytest.mark.parametrize("bits", [2, 5, 7, 9, 12])
def test_poseidon_rows_against_the_oracle(gpu, orc, bits):
    data, pws, gates = E.hash_rows(gpu, HASH_PERMS[bits], _seeds(bits, 30 * bits))
    assert gates == HASH_PERMS[bits] and data.info["num_wires"] == 135
    _assert_rung(data, bits, 0)
    E.gpu_proofs_hold(gpu, orc, data, pws, oracle=True)


# ---------------------------------------------------------------------------------------------- Keccak rungs
@pytest.mark.parametrize("bits", [2, 3, 5])
def test_keccak_chain_without_a_fri_round(gpu, bits):
    """The oracle has no Keccak: both verifiers and the replay under the Keccak tree hasher."""
    data, pws = E.chain(gpu, CHAIN_OPS[bits], _seeds(bits, 40 * bits), hasher="keccak")
    assert data.info["hasher"] == "keccak"
    _assert_rung(data, bits, 0)
    E.gpu_proofs_hold(gpu, None, data, pws, oracle=False, hasher=proof_ref.keccak_hasher())


# ---------------------------------------------------------------------------------------------- validity rungs
def _timed(gpu, data):
    assert gpu.lib().p2_circuit_set_timing(data.gpu(), 1) == 0


def _launch_counts(gpu, data):
    data.synchronize()
    arr = (gpu.api._KernelTime * 128)()
    k = gpu.lib().p2_circuit_get_timing(data.gpu(), arr, 128)
    assert 0 < k <= 128
    return {arr[i].name.decode(): arr[i].count for i in range(k)}


def _assert_segmented(gpu, data):
    """perm_scan and fri_divide each ran their two-launch form (segment products / sums, then the linked scan) once per chunk"""
    count = _launch_counts(gpu, data)
    chunks = count["quotient"]
    assert chunks >= 1
    assert count["perm_scan"] == 2 * chunks and count["fri_divide"] == 2 * chunks, count


@pytest.mark.parametrize("bits", [16, 17, 18])
def test_chain_in_linked_segments(gpu, bits):
    data, pws = E.chain(gpu, CHAIN_OPS[bits], [50 * bits, 50 * bits + 1])
    _assert_rung(data, bits, 0)
    assert (1 << bits) >> 14 == {16: 4, 17: 8, 18: 16}[bits]
    _timed(gpu, data)
    E.gpu_proofs_hold(gpu, None, data, pws, oracle=False)
    _assert_segmented(gpu, data)


def test_one_table_in_linked_segments(gpu):
    lookups, n_ops = TABLE_16
    data, pws = _one_table(gpu, lookups, [61, 62], n_ops)
    _assert_rung(data, 16, 1)
    _timed(gpu, data)
    E.gpu_proofs_hold(gpu, None, data, pws, oracle=False)
    _assert_segmented(gpu, data)


# ---------------------------------------------------------------------------------------------- the capped rung
def test_chain_with_capped_segments_2_21_rows(gpu):
    """n = 2^21 is the smallest size at which PERM_MAX_SEGS = FRI_MAX_SEGS = 64 caps the segment count: a segment is 2^15 rows,
    two sweeps of the 2^14 that every smaller size has.  One proof of the arithmetic chain, held to both verifiers and the
    replay.  The one ladder test that takes longer than a few seconds: most of it is the builder's work on 3 M operations and
    a 2 GiB circuit blob.  Measured on an MI355X host, one pytest process: 19.4 s, next to 23.6 s of
    test_gpu_parity.py::test_ghash_chain_2_20_rows in the same run (kept while it stays within three times that)."""
    data, pws = E.chain(gpu, CHAIN_OPS[21], [77])
    _assert_rung(data, 21, 0)
    assert min((1 << 21) >> 14, 64) == 64 and (1 << 21) // 64 == 1 << 15
    _timed(gpu, data)
    E.gpu_proofs_hold(gpu, None, data, pws, oracle=False)
    _assert_segmented(gpu, data)
