"""The AES-GCM host twins under the address and undefined-behaviour sanitizers: tests/host/gcm_check.cpp is a stand-alone program
(its own main, nothing loaded into Python) that calls gcm_encrypt_aad, gcm_decrypt and gcm_encrypt of csrc/aes_gadgets.h at
len in {0, 1, 13, 15, 16, 17, 31, 32, 33} and aad_len in {0, 1, 5, 13, 16, 17, 20} for the three key sizes, every buffer a heap
allocation of exactly its length."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gcm_twins_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gcm_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "plonky2-aes_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "gcm_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("gcm ok: 189 shapes") and "Sanitizer" not in run.stderr, run.stdout + run.stderr
