#!/usr/bin/env python3
"""Derive the constants of two rewritten forms of Poseidon's 22 partial rounds and check both against the naive permutation.

1. The sparse-matrix form (fewest multiplications; every constant a full field element).  It serves poseidon_coop, the
   one-word-per-lane Fiat-Shamir chain, where a multiplication costs the same whatever its constant.

Naive partial round i:   s += c_i ; s0 = s0^7 ; s = M s        (M = 12x12 MDS)
Rewritten (exactly equivalent):
    s[1..] = D0 s[1..]                       dense 11x11, once
    for i in 0..22:  s0 = (s0 + a_i)^7
                     (s0, s[1..]) = (25 s0 + what_i . s[1..],  s[1..] + v_i s0)
    s += L                                   folded into the next full round's constants
Derivation: (A) the non-S-box parts of each round constant commute with the S-box and are pushed forward through M;
(B) M = [[m00, w],[v, Mh]] factors as [[m00, w Mh^-1],[v, I]] . diag(1, Mh); diag(1, Mh) commutes with the partial S-box
and is merged into the previous round's matrix, recursively, from the last round backwards.

2. The block form (derive_blocks): blocks of up to three rounds evaluated on 32-bit halves with small integer coefficients,
   for the thread-per-sponge kernels, where a term with a 64-bit constant costs 8 issue slots (12 with its reduction) and a
   term with a small coefficient 2.  With M the MDS matrix, Z = diag(0, 1, .., 1) and a state x that carries round r's
   constants, let y = (x_0^7, x_1, .., x_11).  Then, over the integers apart from the constants K_i,
       x(1) = M y + K_1
       x(2) = MZM y + (M e0) t_1 + K_2                      t_i = (x(i)_0)^7
       x(3) = MZMZM y + (MZM e0) t_1 + (M e0) t_2 + K_3     K_i = MZ K_(i-1) + c_(r+i) mod p,  K_0 = 0
   Only row 0 of the depths inside a block is needed (it feeds the next S-box); all twelve rows are evaluated once, at the
   block's end.  The matrices are the same for every block, only the K_i differ, and the last block's K carries round 26's
   constants.  Every coefficient is a small non-negative integer: a row's two half-accumulators stay far below 2^64 for
   arbitrary u64 state words (block_bounds proves it, and the bound of the fold that follows, for every row emitted).
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_poseidon_constants import MDS_CIRC, MDS_DIAG, P, constants, permute  # noqa: E402

W = 12


def matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) % P for j in range(len(B[0]))] for i in range(len(A))]


def matvec(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) % P for i in range(len(A))]


def inverse(A):
    n = len(A)
    a = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], P - 2, P)
        a[c] = [x * inv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def derive():
    rc = constants()
    M = [[(MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0)) % P for c in range(W)] for r in range(W)]
    # (A) scalar constants
    e = [0] * W
    a = []
    for i in range(22):
        t = [(rc[12 * (4 + i) + k] + e[k]) % P for k in range(W)]
        a.append(t[0])
        rest = [0] + t[1:]
        e = matvec(M, rest)
    L = e
    # (B) sparse factors, backwards
    Q = M
    what, v = [None] * 22, [None] * 22
    for i in reversed(range(22)):
        Qh = [row[1:] for row in Q[1:]]
        Qhi = inverse(Qh)
        w = [Q[0][1:]]
        what[i] = matmul(w, Qhi)[0]
        v[i] = [Q[r][0] for r in range(1, W)]
        assert Q[0][0] == 25
        D = [[1] + [0] * 11] + [[0] + Qh[r] for r in range(11)]
        Q = matmul(D, M)
    D0 = [row[1:] for row in D[1:]]
    # E = D0 . M[1.., :]: the dense layer merged into the linear layer of the fourth full round (rows 1..11 of its output)
    E = matmul(D0, [M[r] for r in range(1, W)])
    return rc, a, what, v, D0, L, E


def first_round_addends(rc, known):
    """Addends of the first full round's MDS rows when the state words in `known` enter the permutation as 0: such a word
    leaves the S-box as the constant rc[k]^7, and its MDS terms join the row's own constant (the second round's rc[12 + r]):
        addend[r] = rc[12 + r] + sum_{k in known} M[r][k] * rc[k]^7      (canonical)."""
    M = [[(MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0)) % P for c in range(W)] for r in range(W)]
    z = {k: pow(rc[k], 7, P) for k in known}
    return [(rc[12 + r] + sum(M[r][k] * z[k] for k in known)) % P for r in range(W)]


def permute_fast(state, rc, a, what, v, D0, L, E=None):
    s = list(state)

    def full(s, r, extra=None):
        s = [(s[i] + rc[12 * r + i] + (extra[i] if extra else 0)) % P for i in range(W)]
        s = [pow(x, 7, P) for x in s]
        return [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k]) % P for k in range(W)]

    for r in range(3):
        s = full(s, r)
    if E is None:
        s = full(s, 3)
        s = [s[0]] + matvec(D0, s[1:])
    else:   # fourth full round with the dense layer merged in: row 0 by the MDS, rows 1.. by E
        z = [pow((s[i] + rc[12 * 3 + i]) % P, 7, P) for i in range(W)]
        s0 = (sum(z[i % W] * MDS_CIRC[i] for i in range(W)) + z[0] * MDS_DIAG[0]) % P
        s = [s0] + matvec(E, z)
    for i in range(22):
        s0 = pow((s[0] + a[i]) % P, 7, P)
        n0 = (25 * s0 + sum(x * y for x, y in zip(what[i], s[1:]))) % P
        s = [n0] + [(s[j + 1] + v[i][j] * s0) % P for j in range(11)]
    s = full(s, 26, extra=L)
    for r in range(27, 30):
        s = full(s, r)
    return s


# ---- block form
BLOCKS = [3, 3, 3, 3, 3, 3, 3, 1]   # what poseidon_fast.h evaluates: one loop body of three rounds, whose last trip runs one
MASK32 = (1 << 32) - 1


def mds_int():
    return [[MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0) for c in range(W)] for r in range(W)]


def imatmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(W)) for j in range(W)] for i in range(W)]


def depth_matrices(depth):
    """[M, MZM, MZMZM, ..] over the integers."""
    M = mds_int()
    MZ = [[0 if c == 0 else M[r][c] for c in range(W)] for r in range(W)]
    out = [M]
    for _ in range(depth - 1):
        out.append(imatmul(MZ, out[-1]))
    return out


def block_rows(size):
    """size -> the coefficient rows the block evaluates: ('row0', depth d) for d < size and ('end', r) for the twelve rows
    at depth `size`; each row is (coefficients of y_0..y_11, coefficients of t_1..t_(d-1))."""
    A = depth_matrices(size)
    rows = {}
    for d in range(1, size + 1):
        for r in (range(W) if d == size else [0]):
            tcols = [A[d - 1 - i][r][0] for i in range(1, d)]   # t_i enters through M e0 and then d - 1 - i more rounds
            rows[("end", r) if d == size else ("row0", d)] = (A[d - 1][r], tcols)
    return rows


def block_bounds(size):
    """Worst case of a row's half-accumulators on arbitrary 32-bit halves, with a 32-bit half of K on top, and of the fold
    that follows (poseidon_fast.h, fold_al_ah): ah' = ah + (al >> 32) must fit 64 bits, and with x2 = ah' >> 32 the sum
    base + x2 (2^32 - 1) may wrap once; the wrapped sum is below x2 (2^32 - 1), so adding 2^32 - 1 again must not wrap."""
    worst = 0
    for key, (coef, tcols) in block_rows(size).items():
        acc = (sum(coef) + sum(tcols)) * MASK32 + MASK32
        assert acc < 1 << 64, (size, key)
        ah2 = acc + (acc >> 32)
        assert ah2 < 1 << 64, (size, key)
        x2 = ah2 >> 32
        assert x2 * MASK32 + MASK32 < 1 << 64, (size, key)
        worst = max(worst, acc)
    return worst


def block_constants(rc, sizes):
    """Per block: [K of row 0 at depth 1, .., size - 1] and the twelve K of the block's end, canonical."""
    assert sum(sizes) == 22
    M = mds_int()
    out, r = [], 4
    for size in sizes:
        K, row0 = [0] * W, []
        for i in range(1, size + 1):
            K = [(sum(M[a][c] * K[c] for c in range(1, W)) + rc[12 * (r + i) + a]) % P for a in range(W)]
            if i < size:
                row0.append(K[0])
        out.append((row0, K))
        r += size
    assert r == 26
    return out


def fold_halves(al, ah):
    """The fold as the kernels run it: 64-bit registers, one conditional second step."""
    assert al < 1 << 64 and ah < 1 << 64
    ah2 = ah + (al >> 32)
    assert ah2 < 1 << 64
    x2, base = ah2 >> 32, ((ah2 & MASK32) << 32) | (al & MASK32)
    t = base + x2 * MASK32
    if t >> 64:
        t = (t & ((1 << 64) - 1)) + MASK32
        assert t < 1 << 64
    return t


def partial_rounds_blocks(x, rc, sizes):
    """The 22 partial rounds in block form on halves, as poseidon_fast.h evaluates them.  x: twelve arbitrary u64 carrying
    round 4's constants; out: twelve u64 carrying round 26's."""
    def sbox(v):
        return pow(v % P, 7, P)

    def row(coef, tcols, y, t, k):
        al, ah = k & MASK32, k >> 32
        for c, v in list(zip(coef, y)) + list(zip(tcols, t)):
            al += c * (v & MASK32)
            ah += c * (v >> 32)
        return fold_halves(al, ah)

    x = list(x)
    for size, (k_row0, k_end) in zip(sizes, block_constants(rc, sizes)):
        rows = block_rows(size)
        y, t = [sbox(x[0])] + x[1:], []
        for d in range(1, size):
            t.append(sbox(row(*rows[("row0", d)], y, t, k_row0[d - 1])))
        x = [row(*rows[("end", r)], y, t, k_end[r]) for r in range(W)]
    return x


def partial_rounds_naive(x, rc):
    M = mds_int()
    x = [v % P for v in x]
    for r in range(4, 26):
        y = [pow(x[0], 7, P)] + x[1:]
        x = [(sum(M[a][c] * y[c] for c in range(W)) + rc[12 * (r + 1) + a]) % P for a in range(W)]
    return x


def check_blocks(rc, rnd):
    for size in (1, 2, 3):
        assert block_bounds(size) < 1 << 57
    for sizes in (BLOCKS, [3] * 6 + [2, 2], [2] * 11, [1] * 22):
        assert all(n <= 3 for n in sizes)   # a larger block needs block_bounds(n) first
        for t in range(12):
            st = [[0] * 12, [P - 1] * 12, [(1 << 64) - 1] * 12][t] if t < 3 else \
                [rnd.randrange(1 << 64) if (t + k) % 3 else rnd.randrange(P) for k in range(12)]
            got = partial_rounds_blocks(st, rc, sizes)
            assert [v % P for v in got] == partial_rounds_naive(st, rc), (sizes, t)
    # and inside the whole permutation
    for t in range(4):
        st = [rnd.randrange(P) for _ in range(12)]
        s = st
        for r in range(4):
            s = [pow((s[i] + rc[12 * r + i]) % P, 7, P) for i in range(W)]
            s = [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k]) % P for k in range(W)]
        s = [(s[i] + rc[48 + i]) % P for i in range(W)]
        s = [v % P for v in partial_rounds_blocks(s, rc, BLOCKS)]
        for r in range(26, 30):
            s = [pow(v, 7, P) for v in s]
            s = [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k] + (rc[12 * (r + 1) + k] if r < 29 else 0)) % P
                 for k in range(W)]
        assert s == permute(st, rc)


def block_tables(rc):
    """The tables poseidon_fast.h reads for BLOCKS (sizes 3 and 1 only: one loop body).
      PB_ROW0_D2[12]     row 0 of MZM: the y-coefficients of the third S-box's input (its t_1 coefficient, M[0][0], and the
                         whole of depth 1's row 0 are MDS entries, which the kernels hold as inline constants)
      PB_END[2][12][13]  per block size (3, then 1) and output row: the t_1 coefficient, then the twelve y-coefficients; the
                         t_2 coefficient of a block of three is M[r][0], an inline constant again.  A block of one has t = 0.
      PB_K[8][14]        per block: K of row 0 at depths 1 and 2 (0 for the block of one), then the twelve K of its end."""
    assert BLOCKS == [3] * 7 + [1]
    r3, r1 = block_rows(3), block_rows(1)
    M = mds_int()
    assert r3[("row0", 1)] == (M[0], []) and r3[("row0", 2)][1] == [M[0][0]]
    assert all(r3[("end", r)][1][1] == M[r][0] for r in range(W))
    end = [[r3[("end", r)][1][0]] + r3[("end", r)][0] for r in range(W)] + [[0] + r1[("end", r)][0] for r in range(W)]
    assert all(0 <= c <= MASK32 for row in end for c in row)
    K = [(k0 + [0, 0])[:2] + kend for k0, kend in block_constants(rc, BLOCKS)]
    return r3[("row0", 2)][0], end, K


if __name__ == "__main__":
    rc, a, what, v, D0, L, E = derive()
    rnd = random.Random(1)
    for t in range(20):
        st = [0] * 12 if t == 0 else [rnd.randrange(P) for _ in range(12)]
        assert permute(st, rc) == permute_fast(st, rc, a, what, v, D0, L)
        assert permute(st, rc) == permute_fast(st, rc, a, what, v, D0, L, E)
    print("sparse partial rounds == naive permutation on 20 states")
    zcap, zrate = first_round_addends(rc, range(8, 12)), first_round_addends(rc, range(0, 8))
    for t in range(20):   # the two addend tables against a plain first round on states with the known words at 0
        for known, tab in ((range(8, 12), zcap), (range(0, 8), zrate)):
            st = [0 if k in known else rnd.randrange(P) for k in range(12)]
            z = [pow((st[k] + rc[k]) % P, 7, P) for k in range(12)]
            plain = [(sum(z[(i + r) % W] * MDS_CIRC[i] for i in range(W)) + z[r] * MDS_DIAG[r] + rc[12 + r]) % P for r in range(W)]
            live = [(tab[r] + sum((MDS_CIRC[(k - r) % W] + (MDS_DIAG[r] if k == r else 0)) * z[k] for k in range(W) if k not in known)) % P
                    for r in range(W)]
            assert plain == live
    print("first-round addends for known-zero capacity / rate == plain first round on 20 states each")
    check_blocks(rc, rnd)
    print("block form of the partial rounds == naive rounds, accumulator and fold bounds hold for blocks of 1, 2, 3 rounds")
    row0_d2, end, K = block_tables(rc)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("// Generated by tools/gen_poseidon_fast.py; equivalence with the naive permutation checked at generation time.\n")

            def arr(name, vals, dims):
                f.write("P2F_DECL const unsigned long long %s%s = {\n" % (name, dims))
                for i in range(0, len(vals), 4):
                    f.write("    " + ", ".join("0x%016xULL" % x for x in vals[i:i + 4]) + ",\n")
                f.write("};\n")
            arr("PF_A", a, "[22]")
            arr("PF_WHAT", [x for row in what for x in row], "[22 * 11]")
            arr("PF_V", [x for row in v for x in row], "[22 * 11]")
            arr("PF_E", [x for row in E for x in row], "[11 * 12]")
            arr("PF_RC26", [(rc[12 * 26 + k] + L[k]) % P for k in range(12)], "[12]")
            arr("RC1_ZCAP", zcap, "[12]")
            arr("RC1_ZRATE", zrate, "[12]")

            def arr32(name, vals, dims, per_line):
                f.write("P2F_DECL const unsigned int %s%s = {\n" % (name, dims))
                for i in range(0, len(vals), per_line):
                    f.write("    " + ", ".join("%uu" % x for x in vals[i:i + per_line]) + ",\n")
                f.write("};\n")
            arr32("PB_ROW0_D2", row0_d2, "[12]", 12)
            arr32("PB_END", [x for row in end for x in row], "[2 * 12 * 13]", 13)
            arr("PB_K", [x for row in K for x in row], "[8 * 14]")
        print("wrote", sys.argv[1])
