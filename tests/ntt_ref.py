"""A plain reference for the transforms of the NTT kernels, which shows its stages.  Test infrastructure only.

The transform is the textbook decimation in frequency over Goldilocks (p = 2^64 - 2^32 + 1): natural order in, bit-reversed
order out, log n stages; stage s has half-size h = n >> (s + 1) and turns every pair (x[i], x[i + h]), i mod 2h < h, into
(x[i] + x[i + h], (x[i] - x[i + h]) w^((i mod h) n / 2h)) with w the primitive n-th root of unity.  It is written twice: on Python
integers (`dif_stages`, the definition) and on numpy uint64 arrays (`dif_stages_np`, for the sizes where integers are too slow;
its field operations are `gl_add`, `gl_sub`, `gl_mul`, built from 32-bit limbs).  Both return the state before every stage, and
`dif_backward*` runs stages 0..s-1 backwards, so that a test can choose what a given stage is to see.

`borrows(a, b)` is a model of the device multiply's reduction (the comment above mulr_add_dev in csrc/gl.h): whether the product
a * b ends in the borrow-only correction, the case that random operands reach once in about 2^32 products."""
import numpy as np

P = 0xFFFFFFFF00000001
MULT_GEN = 14293326489335486720   # the coset shift g
POW2_GEN = 7277203076849721926    # of order 2^32
M32 = 0xFFFFFFFF
INV2 = (P + 1) // 2
# the exponents j of the forward twiddles that are powers of two with a set high limb only: w_64 = 8, w_64^k = 2^(3k), k = 11..21
BORROW_EXPONENTS = tuple(range(33, 64, 3))


def root_of_unity(bits):
    return pow(POW2_GEN, 1 << (32 - bits), P)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


_TW = {}


def twiddles(bits):
    """[w^k for k < n/2] as Python integers, w the primitive 2^bits-th root."""
    if bits not in _TW:
        w, t, x = root_of_unity(bits), [], 1
        for _ in range(max(1 << bits >> 1, 1)):
            t.append(x)
            x = x * w % P
        _TW[bits] = t
    return _TW[bits]


def stage_twiddle(bits, s, pos):
    """The twiddle of the butterfly at position pos (< h) of a block of stage s."""
    return twiddles(bits)[pos << s]


# ---------------------------------------------------------------------------------------------- Python integers
def dif_stages(x, bits):
    """[state before stage 0, .., state before stage bits-1, output]; the output is in bit-reversed order."""
    n, tw = 1 << bits, twiddles(bits)
    assert len(x) == n
    states = [list(x)]
    for s in range(bits):
        h, cur = n >> (s + 1), list(states[-1])
        for i in range(n):
            if i & h:
                continue
            u, v = cur[i], cur[i + h]
            cur[i] = (u + v) % P
            cur[i + h] = (u - v) * tw[(i & (h - 1)) << s] % P
        states.append(cur)
    return states


def dif(x, bits):
    return dif_stages(x, bits)[-1]


def dif_backward(y, bits, s):
    """The transform input whose state before stage s is y (stages s-1, .., 0 undone)."""
    n, tw, cur = 1 << bits, twiddles(bits), list(y)
    for st in range(s - 1, -1, -1):
        h = n >> (st + 1)
        for i in range(n):
            if i & h:
                continue
            a, d = cur[i], cur[i + h] * pow(tw[(i & (h - 1)) << st], P - 2, P) % P
            cur[i] = (a + d) * INV2 % P
            cur[i + h] = (a - d) * INV2 % P
    return cur


def coset_scale(x, shift):
    """x[i] * shift^i: the coefficients of f(shift X)."""
    out, c = [], 1
    for v in x:
        out.append(v * c % P)
        c = c * shift % P
    return out


def coset_unscale(x, shift):
    return coset_scale(x, pow(shift, P - 2, P))


def lde(coeffs, bits, rate_bits=3):
    """Values of the polynomial on g <w_{8n}>, bit-reversed order, coset by coset as the kernels do it: coset j is scaled by
    (g w_{8n}^j)^i and transformed at size n, and lands in block rev(j) of the output."""
    n, wl, out = 1 << bits, root_of_unity(bits + rate_bits), [0] * (len(coeffs) << rate_bits)
    for j in range(1 << rate_bits):
        blk = bitrev(j, rate_bits)
        out[blk * n:(blk + 1) * n] = dif(coset_scale(coeffs, MULT_GEN * pow(wl, j, P) % P), bits)
    return out


def borrows(a, b):
    """Whether the device product a * b takes the borrow-only correction.  The steps of mulr_add_dev on 32-bit limbs:
    P = a0 b0; Y = a0 b1 + P.hi; Y = a1 b0 + Y (carry k); H = a1 b1 + Y.hi; R = (Y.lo, P.lo) + H.lo (2^32 - 1) (carry C);
    R = R - H.hi - k (borrow B); the correction is (C - B)(2^32 - 1)."""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p = a0 * b0
    y = a0 * b1 + (p >> 32)
    y = a1 * b0 + y
    k, y = y >> 64, y & (2**64 - 1)
    h = a1 * b1 + (y >> 32)
    lo = ((y & M32) << 32) | (p & M32)
    r = lo + (h & M32) * M32
    c, r = r >> 64, r & (2**64 - 1)
    bb = r < (h >> 32) + k
    return bool(bb and not c)


# ---------------------------------------------------------------------------------------------- numpy uint64
_P, _EPS, _S32 = np.uint64(P), np.uint64(M32), np.uint64(32)


def gl_add(a, b):
    s = a + b
    return np.where((s < a) | (s >= _P), s - _P, s)


def gl_sub(a, b):
    return np.where(a >= b, a - b, a + (_P - b))


def gl_mul(a, b):
    """a * b mod p elementwise for canonical uint64 arrays (wrapping uint64 arithmetic on 32-bit limbs)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    a0, a1, b0, b1 = a & _EPS, a >> _S32, b & _EPS, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = p01 + (p00 >> _S32)            # < 2^64: (2^32-1)^2 + 2^32 - 1
    mid2 = p10 + (mid & _EPS)            # likewise
    lo = (mid2 << _S32) | (p00 & _EPS)
    hi = p11 + (mid >> _S32) + (mid2 >> _S32)
    # hi 2^64 + lo with 2^64 = 2^32 - 1 and 2^96 = -1
    hh, hl = hi >> _S32, hi & _EPS
    t0 = lo - hh
    t0 = np.where(lo < hh, t0 - _EPS, t0)
    t1 = hl * _EPS
    r = t0 + t1
    r = np.where(r < t1, r + _EPS, r)
    return np.where(r >= _P, r - _P, r)


def powers_np(base, n):
    """[base^i for i < n] by doubling."""
    out = np.ones(1, dtype=np.uint64)
    while len(out) < n:
        out = np.concatenate([out, gl_mul(out, np.uint64(pow(base, len(out), P)))])
    return out[:n]


_TWNP = {}


def _tables_np(bits):
    if bits not in _TWNP:
        tw = np.array(twiddles(bits), dtype=np.uint64)
        inv = tw.copy()                  # w^-k = -w^(n/2 - k)
        if len(tw) > 1:
            inv[1:] = _P - tw[:0:-1]
        _TWNP[bits] = (tw, inv)
    return _TWNP[bits]


def _stage_np(cur, bits, s, tw):
    h = (1 << bits) >> (s + 1)
    v = cur.reshape(-1, 2, h)
    u, w = v[:, 0, :], v[:, 1, :]
    return np.stack([gl_add(u, w), gl_mul(gl_sub(u, w), tw[::1 << s][None, :h])], axis=1).reshape(-1)


def dif_stages_np(x, bits, upto=None):
    """The states before stages 0..upto (default: all of them and the output) for a uint64 array."""
    tw = _tables_np(bits)[0]
    states = [np.asarray(x, dtype=np.uint64)]
    for s in range(bits if upto is None else upto):
        states.append(_stage_np(states[-1], bits, s, tw))
    return states


def dif_backward_np(y, bits, s):
    inv, cur, half = _tables_np(bits)[1], np.asarray(y, dtype=np.uint64), np.uint64(INV2)
    for st in range(s - 1, -1, -1):
        h = (1 << bits) >> (st + 1)
        v = cur.reshape(-1, 2, h)
        a, d = v[:, 0, :], gl_mul(v[:, 1, :], inv[::1 << st][None, :h])
        cur = np.stack([gl_mul(gl_add(a, d), half), gl_mul(gl_sub(a, d), half)], axis=1).reshape(-1)
    return cur


def coset_scale_np(x, shift):
    return gl_mul(x, powers_np(shift, len(x)))


def coset_unscale_np(x, shift):
    return gl_mul(x, powers_np(pow(shift, P - 2, P), len(x)))


def random_field_np(rng, size):
    """Uniform canonical field elements (rejection of the 2^32 - 1 values at or above p)."""
    v = rng.integers(0, 1 << 64, size=size, dtype=np.uint64)
    while True:
        bad = v >= _P
        if not bad.any():
            return v
        v[bad] = rng.integers(0, 1 << 64, size=int(bad.sum()), dtype=np.uint64)


def borrow_column(rng, bits, s):
    """The wanted state before stage s of one directed column, and how many butterflies it aims at the borrow case: in every
    block of the stage, every butterfly whose twiddle is 2^j, j in BORROW_EXPONENTS, gets the difference m 2^(96 - j)
    (y[i] = m 2^(96 - j), 1 <= m < 2^(j - 32), y[i + h] = 0); every other point is random."""
    n, h = 1 << bits, (1 << bits) >> (s + 1)
    y = random_field_np(rng, n)
    count = 0
    for pos in range(h):
        tw = stage_twiddle(bits, s, pos)
        if tw & (tw - 1) or tw.bit_length() - 1 not in BORROW_EXPONENTS:
            continue
        j = tw.bit_length() - 1
        for blk in range(0, n, 2 * h):
            m = int(rng.integers(1, 1 << (j - 32))) if j > 33 else 1
            y[blk + pos] = m << (96 - j)
            y[blk + pos + h] = 0
            count += 1
    return y, count
