"""csrc/pool.h -- the one pool and the one lease behind the prover's staging sets, the verification workspaces and the witness
workspaces -- on the host, without HIP: tests/host/pool_check.cpp is a stand-alone program with a counting workspace type.  It
checks reuse of a returned workspace, that workspaces made under an older key are destroyed outside the pool's lock and exactly
once, that a failing make leaves the pool as it was, that a lease drains after a failure and not after a success, and, with four
threads leasing 1000 times each while a fifth changes the key, that every workspace made is destroyed by the time the pool goes.
Built and run once under the address and undefined-behaviour sanitizers and once under the thread sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_pool_and_lease_under_sanitizers(tmp_path, sanitizer):
    exe = str(tmp_path / "pool_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-pthread",
                           "-I", os.path.join(ROOT, "plonky2-aes_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "pool_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("pool ok:") and "Sanitizer" not in run.stderr, run.stdout + run.stderr
