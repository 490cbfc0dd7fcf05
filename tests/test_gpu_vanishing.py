"""k_vfy_vanishing / k_vfy_ecvanishing on opening sets that tests/vanishing_ref.py alone makes valid, and on every
single-coordinate perturbation of them (p2_gpu_vanishing_flags: the caller's openings, challenges and public-inputs hash, the
kernel verify_batch launches, its ZETA and VANISH flags).  The expected verdict of every case is Python's; the host hook
(p2_vanishing_terms) is asked too, so that the three agree case for case.  Flags and verdicts only: every comparison is exact."""
import pytest

import proof_ref
import vanishing_cases as VC
import vanishing_ref as V

pytestmark = pytest.mark.gpu
P = proof_ref.P
UNTOUCHED_EVERY = 8


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


@pytest.mark.parametrize("name", VC.NAMES)
def test_solved_sets_and_the_sweep_in_one_batch(gpu, name):
    """Solved sets (random, all p - 1, all 0 but the quotient's), then the sweep of the host test -- the first coordinate of
    every element of every open_* section, the second of every seventh -- with an untouched solved set after every eighth
    perturbed one, so that a kernel reading one buffer for the whole batch cannot pass."""
    info, blob, circ, data = VC.build(gpu, name)
    base = VC.solved(name, circ, "random", 100)
    cases = [VC.solved(name, circ, fill, 7) for fill in ("random", P - 1, 0)]
    for k, c in enumerate(VC.sweep(circ, base)):
        cases.append(c)
        if k % UNTOUCHED_EVERY == UNTOUCHED_EVERY - 1:
            cases.append(base)
    want = [VC.python_verdict(circ, c) for c in cases]
    assert want[:3] == [V.HOLDS] * 3 and V.FAILS in want
    flags = VC.gpu_flags(gpu, data, info, cases)
    for c, f, w in zip(cases, flags, want):
        assert VC.flags_verdict(f) == w, c.label
        assert VC.host(gpu, info, blob, c)[0] == w, c.label


@pytest.mark.parametrize("name", ["mix_columns", "ec_steps"])
def test_batch_sizes_around_the_chunk(gpu, name):
    """1, 2 and verify_chunk + 1 buffers (verify_chunk = 3 on a handle of its own): the second chunk's flags land at its offset"""
    info, blob, circ, _ = VC.build(gpu, name)
    data = gpu.CircuitData(blob)
    data.set_option("verify_chunk", 3)
    good = VC.solved(name, circ, "random", 3)
    bad = good.copy("zs[1].1 + 1")
    bad.o["zs"][1] = (bad.o["zs"][1][0], (bad.o["zs"][1][1] + 1) % P)
    assert VC.python_verdict(circ, good) == V.HOLDS and VC.python_verdict(circ, bad) == V.FAILS
    for batch in ([good], [bad], [bad, good], [good, bad], [good, good, good, bad], [bad, bad, bad, good], [good, bad, good, good, bad, bad, good]):
        want = [0 if c is good else 16 for c in batch]
        assert VC.gpu_flags(gpu, data, info, batch) == want


@pytest.mark.parametrize("name", ["arithmetic", "mix_columns", "hashed_elgamal"])
def test_zeta_in_the_subgroup(gpu, name):
    """zeta = 1, the n-th root of unity and its inverse: L_0's denominator is zero or not, the kernel's Fermat inverse of zero is
    zero (gl::inv, a loop over the exponent's 64 bits), and it goes on past the flag where the host returns"""
    info, blob, circ, data = VC.build(gpu, name)
    w = proof_ref.root_of_unity(circ.degree_bits)
    good = VC.solved(name, circ, "random", 5)
    cases = [good]
    for zeta in ([1, 0], [w, 0], [pow(w, circ.n - 1, P), 0], [w, 1]):
        c = good.copy("zeta = %s" % zeta)
        c.ch["zeta"] = zeta
        cases.append(c)
    cases.append(good)
    want = [VC.python_verdict(circ, c) for c in cases]
    assert want == [V.HOLDS] + [V.IN_SUBGROUP] * 3 + [V.FAILS, V.HOLDS]
    assert [VC.flags_verdict(f) for f in VC.gpu_flags(gpu, data, info, cases)] == want
    assert [VC.host(gpu, info, blob, c)[0] for c in cases] == want


def test_each_challenge_alone_and_a_zero_factor(gpu):
    info, blob, circ, data = VC.build(gpu, "mix_columns")
    good = VC.solved("mix_columns", circ, "random", 21)
    alpha1 = good.copy("alphas[1] + 1")
    alpha1.ch["alphas"][1] = (alpha1.ch["alphas"][1] + 1) % P
    zero = VC.solved("mix_columns", circ, "random", 31)
    zero.o["wires"][78] = (zero.o["wires"][78][0], 0)
    zero.o["wires"][79] = (zero.o["wires"][79][0], 0)
    zero.ch["deltas"][6] = (zero.o["wires"][78][0] + zero.ch["deltas"][4] * zero.o["wires"][79][0]) % P     # challenge 1, slot 39
    V.solve_quotient(circ, zero.o, zero.ch, zero.pi_hash)
    cases = [good, alpha1, zero]
    want = [VC.python_verdict(circ, c) for c in cases]
    assert want == [V.HOLDS, V.FAILS, V.HOLDS]
    assert [VC.flags_verdict(f) for f in VC.gpu_flags(gpu, data, info, cases)] == want


def test_the_hook_checks_its_arguments(gpu):
    info, blob, circ, data = VC.build(gpu, "arithmetic")
    case = VC.solved("arithmetic", circ, "random", 5)
    case.ch["zeta"][1] = P
    with pytest.raises(AssertionError, match="non-canonical"):
        VC.gpu_flags(gpu, data, info, [case])
    assert gpu.lib().p2_gpu_vanishing_flags(data.gpu(), 0, None, None, None, None) == 0
