"""CPU checks of the batched GPU verifier's interface: the verdict table covers every reason of the host verifier, the C
header and api.py agree, the kernels cross-compile for gfx950 without scratch, and bad arguments are errors, not crashes."""
import ctypes as C
import os
import re

import device_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky2-aes_amd", "csrc")
KERNELS = ["k_vfy_unpack", "k_vfy_transcript", "k_vfy_vanishing", "k_vfy_queries", "k_vfy_finish"]
VGPR_BUDGET = 128  # four waves per SIMD or more; the largest of the five (k_vfy_transcript) takes 96


def test_verify_reasons_cover_the_host_verifier(pkg):
    src = open(os.path.join(CSRC, "verifier.h")).read()
    reasons = set(re.findall(r'return "([^"]*)";', src))
    assert len(reasons) >= 12
    assert reasons <= set(pkg.VERIFY_REASONS), reasons - set(pkg.VERIFY_REASONS)
    assert set(pkg.VERIFY_REASONS) <= reasons, set(pkg.VERIFY_REASONS) - reasons


def test_header_enum_matches_api(pkg):
    hdr = open(os.path.join(ROOT, "include", "p2aes.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"P2_(VERIFY_[A-Z_]+)\s*=\s*(\d+)", hdr)}
    assert len(enum) == 10
    for name, v in enum.items():
        assert getattr(pkg, name) == v, name
    assert len(set(enum.values())) == len(enum)
    assert set(pkg.VERIFY_REASONS.values()) == set(enum.values())


def test_exports(pkg):
    L = pkg.lib()
    assert not L._p2_missing
    for f in ("p2_verify_batch", "p2_verify_batch_device"):
        assert f in L._p2_signatures and hasattr(L, f)


def test_null_handle_and_bad_arguments_are_errors(pkg):
    L = pkg.lib()
    st = (C.c_int * 4)()
    vd = (C.c_uint64 * 68)()
    assert L.p2_verify_batch(None, 4, b"\0" * 64, vd, 68, st) == 1
    assert "null circuit handle" in L.p2_last_error().decode()
    # (a wrong vd_len needs a loaded handle, i.e. a GPU: tests/test_gpu_verify.py::test_verifier_data_mismatches covers it)
    assert L.p2_verify_batch_device(None, 4, None, None, 0, None, None) == 1


def test_verifier_kernels_cross_compile_without_scratch():
    info, _ = device_build.cross_compile()
    for k in KERNELS:
        names = [n for n in info if k in n]
        assert names, k
        for n in names:
            assert info[n]["ScratchSize"] == 0, (n, info[n])
            assert info[n]["VGPRs"] <= VGPR_BUDGET, (n, info[n])
