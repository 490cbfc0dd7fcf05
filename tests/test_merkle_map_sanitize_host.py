"""The MerkleMap host twin under the address and undefined-behaviour sanitizers: tests/host/merkle_map_check.cpp is a stand-alone
program (its own main, nothing loaded into Python) that builds maps of 0, 1, 2 and 5 entries over csrc/merkle_host.h for key
spaces of 1 to 64 bits, caps of 1 to 2^16 and values of 0 to 134 words, every buffer a heap allocation of exactly its length,
and checks every proof it takes and the refusals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merkle_map_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "merkle_map_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "plonky2-aes_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "merkle_map_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("merkle map ok: 238 maps") and "Sanitizer" not in run.stderr, run.stdout + run.stderr
