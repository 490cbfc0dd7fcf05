"""The NTT kernels' own arithmetic on the device, and transforms whose inputs are aimed at the reduction's borrow case.

Every product of the transforms goes through gl::mul_nb, the only user of the branch-free two-sided correction.  Its borrow-only
half is reached by random operands once in about 2^32 products, so random columns never test it.  The forward twiddle tables hold
exact powers of two (w_64 = 8, so w_n^(k n / 64) = 2^(3k); k = 11..21 gives 2^33 .. 2^63 below index n/2), and
2^j * (m 2^(96 - j)) = m 2^96 borrows with certainty.  A column whose state before a chosen stage has the difference m 2^(96 - j) at
every butterfly with such a twiddle therefore drives the kernels through that path; ntt_ref.py builds it by running the earlier
stages backwards and dividing by the coset shift's powers, and the condition is asserted from the reference's stage states alone
before anything runs on the GPU."""
import ctypes as C

import numpy as np
import pytest

import ntt_ref as R

pytestmark = pytest.mark.gpu
P = R.P
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return pkg


def ptr(a):
    return a.ctypes.data_as(u64p)


def test_device_selftest_of_the_transform_arithmetic(gpu):
    """gl::mul_nb on unreduced extremes and on borrow pairs next to random lanes, the butterfly, and the four register stages of a
    radix-16 step in both forms against the textbook operations: 2^20 threads x 16 rounds, one planted violation."""
    assert gpu.lib().p2_selftest_ntt_device(0x2E77, 1 << 20, 0) == 0


# 6, 7: k_ntt_lds without and with the leading radix-2 stage; 8, 11: k_ntt_r16<false> with rem = 4 and 3; 13, 14: the half-column
# kernel; 15, 16: pass 1 (3 and 4 stages down the rows) + pass 2 -- the smallest sizes of each family
@pytest.mark.parametrize("bits", [6, 7, 8, 11, 13, 14, 15, 16])
def test_transforms_aimed_at_the_borrow_case(gpu, orc, bits):
    n, rng = 1 << bits, np.random.default_rng(1000 + bits)
    stages = list(range(bits - 1))  # half-size h = n >> (s + 1) >= 2
    cols = len(stages)
    coeffs = np.zeros((cols, n), dtype=np.uint64)
    for c, s in enumerate(stages):
        y, planted = R.borrow_column(rng, bits, s)
        assert planted >= (11 if (n >> s) >= 64 else 1)
        coeffs[c] = R.coset_unscale_np(R.dif_backward_np(y, bits, s), R.MULT_GEN)
    # the condition, from the reference alone: coset 0 of the LDE scales by g^i and transforms; before stage s of column s every
    # butterfly with a power-of-two twiddle 2^j, j = 33, 36, .., 63, has a difference that borrows against it
    for c, s in enumerate(stages):
        state = R.dif_stages_np(R.coset_scale_np(coeffs[c], R.MULT_GEN), bits, upto=s)[-1]
        h, hits = n >> (s + 1), 0
        for pos in range(h):
            tw = R.stage_twiddle(bits, s, pos)
            if tw & (tw - 1) or tw.bit_length() - 1 not in R.BORROW_EXPONENTS:
                continue
            for blk in range(0, n, 2 * h):
                assert R.borrows((int(state[blk + pos]) - int(state[blk + pos + h])) % P, tw), (s, blk, pos)
                hits += 1
        assert hits >= (11 if 2 * h >= 64 else 1), (s, hits)
    lde = np.zeros((cols, 8 * n), dtype=np.uint64)
    assert gpu.lib().p2_gpu_lde(ptr(coeffs), cols, bits, 3, ptr(lde), 0) == 0, gpu.lib().p2_last_error()
    out = np.zeros((cols, n), dtype=np.uint64)
    assert gpu.lib().p2_gpu_intt(ptr(coeffs), cols, bits, ptr(out), 0) == 0, gpu.lib().p2_last_error()
    for c in range(cols):
        ref = np.zeros(8 * n, dtype=np.uint64)
        orc.lib().orc_lde(ptr(coeffs[c]), bits, 3, ptr(ref))
        bad = np.nonzero(ref != lde[c])[0]
        assert len(bad) == 0, "LDE of the column aimed at stage %d: %d words differ, first at %s" % (stages[c], len(bad), bad[:4])
        inv = coeffs[c].copy()
        orc.lib().orc_fft(ptr(inv), bits, 1)
        assert (inv == out[c]).all(), "iNTT of the column aimed at stage %d" % stages[c]
