"""The transform launch shapes that only whole proofs used to reach, through hooks that run the prover's own code on the tables of
the loader's own builder: the LDEs of the FRI rounds (strided twiddle tables, no folded table, shift g^(16^r), round tables and
their pass-1 tables above 2^14, batches with padded strides) and the quotient inverse (bit-reversed input and output, the post
table, coset blocks, the block permutation of the two-pass form, k_quotient_chunks_rev)."""
import ctypes as C

import numpy as np
import pytest

import ntt_ref as R

pytestmark = pytest.mark.gpu
P = R.P
u64p = C.POINTER(C.c_uint64)
PAD = 3  # words between the proofs of a batch
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return pkg


def ptr(a):
    return a.ctypes.data_as(u64p)


def schedule(degree_bits):
    """The project's FRI schedule: 4 bits per round while more than 5 bits remain."""
    ar, left = [], degree_bits
    while left > 5:
        ar.append(4)
        left -= 4
    return ar


def lde_round(gpu, orc, degree_bits, rnd, cols=2, batch=2):
    ar = schedule(degree_bits)
    bits_r = degree_bits - sum(ar[:rnd])
    n_r, rng = 1 << bits_r, np.random.default_rng(degree_bits * 16 + rnd)
    in_stride, out_stride = cols * n_r + PAD, 8 * cols * n_r + PAD
    coeffs = np.full(batch * in_stride, SENTINEL, dtype=np.uint64)
    out = np.full(batch * out_stride, SENTINEL, dtype=np.uint64)
    for b in range(batch):
        coeffs[b * in_stride:b * in_stride + cols * n_r] = R.random_field_np(rng, cols * n_r)
    coeffs[:4] = [0, P - 1, 1, P - 2]
    arr = (C.c_uint32 * max(len(ar), 1))(*ar)
    rc = gpu.lib().p2_gpu_lde_round(ptr(coeffs), cols, degree_bits, arr, len(ar), rnd, batch, in_stride, ptr(out), out_stride, 0)
    assert rc == 0, gpu.lib().p2_last_error()
    # the round's coset is g^(16^r) <w>: f(g^(16^r) x) = sum (c_i t^i) (g x)^i with t = g^(16^r - 1), which the oracle's LDE (shift g)
    # evaluates from the coefficients c_i t^i
    tpow = R.powers_np(pow(R.MULT_GEN, 16 ** rnd - 1, P), n_r)
    ref = np.zeros(8 * n_r, dtype=np.uint64)
    for b in range(batch):
        for c in range(cols):
            col = np.ascontiguousarray(R.gl_mul(coeffs[b * in_stride + c * n_r:b * in_stride + (c + 1) * n_r], tpow))
            orc.lib().orc_lde(ptr(col), bits_r, 3, ptr(ref))
            got = out[b * out_stride + c * 8 * n_r:b * out_stride + (c + 1) * 8 * n_r]
            bad = np.nonzero(ref != got)[0]
            assert len(bad) == 0, "proof %d column %d: %d words differ, first at %s" % (b, c, len(bad), bad[:4])
        assert (out[b * out_stride + 8 * cols * n_r:(b + 1) * out_stride] == SENTINEL).all(), "wrote between the proofs"


ROUND_CASES = [(d, r) for d in range(5, 23) for r in range(1, len(schedule(d)))]


def test_round_cases_cover_the_strided_half_column_shapes():
    assert {(17, 1), (18, 1), (21, 2), (22, 2)} <= set(ROUND_CASES) and len(ROUND_CASES) == 28
    assert schedule(22) == [4] * 5 and schedule(5) == [] and schedule(6) == [4]


@pytest.mark.parametrize("degree_bits,rnd", ROUND_CASES)
def test_lde_of_a_fri_round(gpu, orc, degree_bits, rnd):
    """Every round >= 1 of every degree_bits 5..22 (5..9 have none): 2 columns, 2 proofs, both strides 3 words wider than tight."""
    lde_round(gpu, orc, degree_bits, rnd)


@pytest.mark.parametrize("degree_bits", [13, 14])
def test_main_lde_through_the_folded_table(gpu, orc, degree_bits):
    """round 0 at the two sizes of the half-column kernel: the shared builder gives the hooks the folded shift-twiddle table."""
    lde_round(gpu, orc, degree_bits, 0)


@pytest.mark.parametrize("degree_bits", list(range(2, 19)) + [19, 20])
def test_quotient_inverse_round_trip(gpu, orc, degree_bits):
    """Random polynomials of degree < 8 n, evaluated on the LDE coset by the oracle (its bit-reversed-output transform of c_i g^i
    at degree_bits + 3), come back from the GPU as their coefficients, chunk by chunk."""
    chunks, batch = (2, 2) if degree_bits <= 18 else (1, 1)
    N, rng = 8 << degree_bits, np.random.default_rng(300 + degree_bits)
    coef = R.random_field_np(rng, batch * chunks * N)
    coef[:8] = [0, P - 1, 1, P - 2, P - 1, 0, P - 2, 1]
    gpow = R.powers_np(R.MULT_GEN, N)
    vals = np.zeros_like(coef)
    for k in range(batch * chunks):
        v = np.ascontiguousarray(R.gl_mul(coef[k * N:(k + 1) * N], gpow))
        orc.lib().orc_fft_bitrev_out(ptr(v), degree_bits + 3)
        vals[k * N:(k + 1) * N] = v
    out = np.zeros_like(coef)
    assert gpu.lib().p2_gpu_quotient_chunks(ptr(vals), chunks, degree_bits, batch, ptr(out), 0) == 0, gpu.lib().p2_last_error()
    n = 1 << degree_bits
    for k in range(batch * chunks):
        for c in range(8):
            lo = k * N + c * n
            assert (out[lo:lo + n] == coef[lo:lo + n]).all(), "proof/column %d chunk %d" % (k, c)
