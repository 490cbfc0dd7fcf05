"""One cross-compile of the product's device code for the code-generation tests (CPU: hipcc targets gfx950 without a GPU):
the compiler's resource remarks per function and the gfx950 assembly, compiled once per process."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@functools.lru_cache(maxsize=None)
def _compile():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "prover.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                            "-o", out, os.path.join(ROOT, "plonky2-aes_amd", "csrc", "prover_gpu.hip")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    info, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = info.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return info, asm


def cross_compile():
    """(resource remarks per function: VGPRs, AGPRs, ScratchSize, Occupancy, LDS Size; assembly text).  Skips without hipcc."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return _compile()
