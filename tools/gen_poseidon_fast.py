#!/usr/bin/env python3
"""Derive the constants of the sparse-matrix form of Poseidon's 22 partial rounds and check it against the naive
permutation (same function, fewer multiplications).

Naive partial round i:   s += c_i ; s0 = s0^7 ; s = M s        (M = 12x12 MDS)
Rewritten (exactly equivalent):
    s[1..] = D0 s[1..]                       dense 11x11, once
    for i in 0..22:  s0 = (s0 + a_i)^7
                     (s0, s[1..]) = (25 s0 + what_i . s[1..],  s[1..] + v_i s0)
    s += L                                   folded into the next full round's constants
Derivation: (A) the non-S-box parts of each round constant commute with the S-box and are pushed forward through M;
(B) M = [[m00, w],[v, Mh]] factors as [[m00, w Mh^-1],[v, I]] . diag(1, Mh); diag(1, Mh) commutes with the partial S-box
and is merged into the previous round's matrix, recursively, from the last round backwards.
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
            arr("PF_D0", [x for row in D0 for x in row], "[11 * 11]")
            arr("PF_E", [x for row in E for x in row], "[11 * 12]")
            arr("PF_RC26", [(rc[12 * 26 + k] + L[k]) % P for k in range(12)], "[12]")
            arr("RC1_ZCAP", zcap, "[12]")
            arr("RC1_ZRATE", zrate, "[12]")
        print("wrote", sys.argv[1])
