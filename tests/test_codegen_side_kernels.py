"""Code-generation guards for the polynomial-side kernels that run on lazy sums and power tables (CPU: hipcc cross-compiles
gfx950 without a GPU): no scratch, no SGPR hazard, and the instruction counts that the rewrite is about -- a polynomial of the FRI
composition is two exact multiply-accumulates (16 VALU instructions) plus address arithmetic, an element of the power tables one
extension multiply with a uniform factor (four fused products of 17 instructions, two canonicalisations) plus its stores."""
import re

import pytest

import device_build as device
import isa_lint

KERNELS = ["k_fri_compose", "k_zeta_pows", "k_zeta_tabs", "k_eval_polys_refs", "k_perm_chunks", "k_fri_alpha_pows"]


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


def _function(asm, fragment):
    found = {n: b for n, b in isa_lint.parse_functions(asm).items() if fragment in n}
    assert len(found) == 1, (fragment, list(found))
    return next(iter(found.values()))


def _valu(blocks):
    return [mn for b in blocks for _, mn, _ in b[1] if isa_lint._is_valu(mn)]


def _loops(blocks):
    """[(first block, last block)] of every back edge, in layout order."""
    index = {b[0]: i for i, b in enumerate(blocks) if b[0]}
    return [(index[t], i) for i, b in enumerate(blocks) for t in b[2] if t in index and index[t] <= i]


@pytest.mark.parametrize("fragment", KERNELS + ["k_quotient"])
def test_no_scratch(device_build, fragment):
    found = [k for n, k in device_build[0].items() if fragment in n]
    assert found, fragment
    for k in found:
        assert k["ScratchSize"] == 0, k


def test_no_sgpr_hazard(device_build):
    asm = device_build[1]
    for fragment in KERNELS:
        _function(asm, fragment)
    assert isa_lint.sgpr_hazards(asm, only=KERNELS) == []


def _innermost(blocks, loops):
    """The innermost of the loops that multiply.  (A uniform branch inside a loop -- the null-base test of k_fri_compose -- can be
    laid out as a backward branch of its own: such a range holds loads and address arithmetic, but no product.)"""
    loops = [l for l in loops if any(mn.startswith("v_mad_u64_u32") for mn in _valu(blocks[l[0]:l[1] + 1]))]
    return [l for l in loops if not any(m != l and l[0] <= m[0] and m[1] <= l[1] for m in loops)]


def _per_load(blocks, lo, hi):
    """(VALU instructions, global loads) of the blocks lo..hi."""
    loads = sum(1 for b in blocks[lo:hi + 1] for _, mn, _ in b[1] if mn.startswith("global_load"))
    return len(_valu(blocks[lo:hi + 1])), loads


def test_fri_compose_spends_at_most_24_valu_instructions_per_polynomial(device_build):
    """Every innermost loop of the kernel (the four-polynomial trip and the tail loop): VALU instructions per polynomial, a
    polynomial being one global load -- its value; the PolyRef and the power arrive by scalar loads -- and two Acc::fma_k.
    Horner in GF(p^2) stood at 98."""
    blocks = _function(device_build[1], "k_fri_compose")
    seen = []
    for lo, hi in _innermost(blocks, _loops(blocks)):
        valu, loads = _per_load(blocks, lo, hi)
        if loads == 0:  # no polynomial is read here: the rare path of a reduction, laid out behind its branch
            continue
        assert valu <= 24 * loads, (lo, hi, valu, loads)
        assert valu >= 16 * loads, (lo, hi, valu, loads)  # the products are in the loop that was measured
        seen.append(loads)
    assert sorted(seen)[-1] == 4 and len(seen) >= 2, seen


def test_zeta_pows_spends_at_most_400_valu_instructions_per_element(device_build):
    """The main launch has no loop in its source -- a thread is an element; the backward branches of its code are the returns from
    the reductions' rare paths, which sit behind the last block -- so the static count of the whole kernel bounds what a thread
    executes (the square-and-multiply form stood at 3 811 executed per thread)."""
    blocks = _function(device_build[1], "k_zeta_pows")
    valu = _valu(blocks)
    assert 0 < len(valu) <= 400, len(valu)
    assert sum(1 for mn in valu if re.match(r"v_mad_u64_u32", mn)) >= 16  # four products of four mads: the multiply is there


def test_the_loop_scanner_sees_a_planted_loop():
    body = "\tglobal_load_dwordx2 v[2:3], v[6:7], off\n" + "\tv_mad_u64_u32 v[0:1], s[2:3], v2, v3, v[0:1]\n" * 8 + "\tv_add_u32_e32 v4, 1, v4\n" * 17
    asm = ("f:\n\tv_mov_b32_e32 v0, 0\n.LBB0_1:\n\tv_mov_b32_e32 v5, 0\n.LBB0_2:\n" + body + "\ts_cbranch_scc1 .LBB0_2\n\ts_cbranch_vccnz .LBB0_1\n"
           "\ts_endpgm\n.Lfunc_end0:\n")
    blocks = _function(asm, "f")
    assert sorted(_loops(blocks)) == [(1, 3), (2, 2)] and _innermost(blocks, _loops(blocks)) == [(2, 2)]
    assert _per_load(blocks, 2, 2) == (25, 1)  # one more than the bound allows for one polynomial
