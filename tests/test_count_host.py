"""plastid_amd/csrc/count_host.h -- the host decisions of pc_count (plan conditions of the canonical stream and the dense
vector, their signatures, the dynamic LDS of k_hist_point, the work-list capacity, the grids, the one-window path, what
is cleared in front of a count, the knobs and their clamps) -- is plain C++: tests/count_host_test.cpp checks them
against literals worked by hand, compiled with the host compiler (under the address and undefined-behaviour sanitizers
where it has them) and run here.  No GPU needed."""
import os
import shutil
import subprocess

import pytest


def test_count_decisions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "count_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "count_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"count_host: ok" in out.stdout
