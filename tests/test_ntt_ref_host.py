"""The transform reference of the GPU NTT tests (ntt_ref.py) against the CPU oracle, and its model of the device reduction's
borrow case.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

import ntt_ref as R

P = R.P
u64p = C.POINTER(C.c_uint64)


def _column(r, n):
    return [r.choice([0, 1, P - 1, P - 2, 0xFFFFFFFF, 1 << 32]) if r.random() < 0.2 else r.randrange(P) for _ in range(n)]


@pytest.mark.parametrize("bits", range(1, 13))
def test_reference_transform_is_the_oracles(orc, bits):
    """Both forms of the reference (Python integers, numpy limbs) equal orc_fft_bitrev_out; every recorded stage state of the
    two forms agrees; running stages backwards from any state gives the input back."""
    r, n = random.Random(bits), 1 << bits
    x = _column(r, n)
    a = (C.c_uint64 * n)(*x)
    orc.lib().orc_fft_bitrev_out(a, bits)
    states = R.dif_stages(x, bits)
    states_np = R.dif_stages_np(np.array(x, dtype=np.uint64), bits)
    assert states[-1] == list(a)
    assert len(states) == len(states_np) == bits + 1
    for s in range(bits + 1):
        assert states_np[s].tolist() == states[s], s
    for s in {0, 1, bits // 2, bits - 1, bits}:
        assert R.dif_backward(states[s], bits, s) == x, s
        assert R.dif_backward_np(states_np[s], bits, s).tolist() == x, s
    assert R.dif_stages_np(np.array(x, dtype=np.uint64), bits, upto=bits // 2)[-1].tolist() == states[bits // 2]


@pytest.mark.parametrize("bits", range(1, 13))
def test_reference_lde_is_the_oracles(orc, bits):
    """The coset pre-scale followed by the transform, coset by coset as the kernels run it, equals orc_lde; and so does the one
    transform of 8 n points on the zero-padded scaled coefficients.  The pre-scale and its inverse undo each other."""
    r, n = random.Random(100 + bits), 1 << bits
    c = _column(r, n)
    out = (C.c_uint64 * (8 * n))()
    orc.lib().orc_lde((C.c_uint64 * n)(*c), bits, 3, out)
    assert R.lde(c, bits) == list(out)
    padded = np.array(R.coset_scale(c, R.MULT_GEN) + [0] * (7 * n), dtype=np.uint64)
    assert R.dif_stages_np(padded, bits + 3)[-1].tolist() == list(out)
    assert R.coset_unscale(R.coset_scale(c, R.MULT_GEN), R.MULT_GEN) == c
    cn = np.array(c, dtype=np.uint64)
    assert R.coset_scale_np(cn, R.MULT_GEN).tolist() == R.coset_scale(c, R.MULT_GEN)
    assert R.coset_unscale_np(R.coset_scale_np(cn, R.MULT_GEN), R.MULT_GEN).tolist() == c


def test_limb_multiply_equals_integer_arithmetic():
    r = random.Random(5)
    edge = [0, 1, 0xFFFFFFFF, 1 << 32, P - 1, P - 2, (1 << 32) + 1, 0xFFFFFFFF << 32]
    edge += [1 << j for j in range(33, 64)]                                 # zero low limb
    edge += [((r.randrange(1 << 16) | 1) << 48) for _ in range(16)]         # zero low limbs
    edge += [r.randrange(1 << 32) << 32 for _ in range(16)]
    edge += [r.randrange(1 << 32) for _ in range(16)]                       # zero high limb
    vals = edge + [r.randrange(P) for _ in range(400)]
    a = np.array([x for x in vals for _ in vals], dtype=np.uint64)
    b = np.array([y for _ in vals for y in vals], dtype=np.uint64)
    assert R.gl_mul(a, b).tolist() == [x * y % P for x in vals for y in vals]
    assert R.gl_add(a, b).tolist() == [(x + y) % P for x in vals for y in vals]
    assert R.gl_sub(a, b).tolist() == [(x - y) % P for x in vals for y in vals]
    assert R.powers_np(R.MULT_GEN, 1000).tolist() == [pow(R.MULT_GEN, i, P) for i in range(1000)]


def test_borrow_model():
    """borrows() is true for every 2^j * (m 2^(96 - j)), j = 33, 36, .., 63, 1 <= m < 2^(j - 32), in both operand orders, and
    false on 10^5 random pairs; the powers of two are the 64th root's: w_64 = 8."""
    assert R.root_of_unity(6) == 8
    assert [pow(8, k, P) for k in range(11, 22)] == [1 << j for j in R.BORROW_EXPONENTS]
    r = random.Random(9)
    for j in R.BORROW_EXPONENTS:
        span = 1 << (j - 32)
        ms = {1, span - 1} | {r.randrange(1, span) if span > 2 else 1 for _ in range(200)}
        for m in ms:
            q = m << (96 - j)
            assert q < P
            assert R.borrows(1 << j, q) and R.borrows(q, 1 << j), (j, m)
    assert not any(R.borrows(r.randrange(P), r.randrange(P)) for _ in range(100000))
    # neighbours that do not borrow: a set low limb, or a carry next to the borrow
    assert not R.borrows(1 << 48, (5 << 48) | 1 << 20 | 1 << 40)
    assert not R.borrows(3, 5)


def test_borrow_column_aims_every_power_of_two_butterfly():
    """What the directed GPU test builds: per block of the stage, one butterfly per power-of-two twiddle (eleven where the
    stage's blocks hold 64 points or more), each with a borrowing difference, found again from the stage state alone."""
    rng = np.random.default_rng(3)
    for bits, s, per_block in [(6, 0, 11), (7, 1, 11), (8, 0, 11), (8, 3, 5), (8, 4, 3), (8, 5, 1), (8, 6, 1), (8, 7, 0)]:
        y, count = R.borrow_column(rng, bits, s)
        assert count == per_block << s
        h = (1 << bits) >> (s + 1)
        hits = sum(R.borrows((int(y[i]) - int(y[i + h])) % P, R.stage_twiddle(bits, s, i & (h - 1)))
                   for i in range(1 << bits) if not i & h)
        assert hits == count
