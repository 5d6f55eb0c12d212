"""plastid_amd/csrc/canon_host.h -- the host arithmetic of the canonical stream (canonical length and index per strand,
the shift of every (aligned length, strand), the halo test, the buckets a bucket's workgroup looks back) -- is plain
C++: tests/canon_host_test.cpp checks hand-worked rules and a grid of rules, filters and random offset tables against a
brute-force model, compiled with the host compiler (under the address and undefined-behaviour sanitizers where it has
them) and run here.  No GPU needed."""
import os
import shutil
import subprocess

import pytest


def test_canonical_rule_arithmetic(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "canon_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "canon_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"canon_host: ok" in out.stdout
