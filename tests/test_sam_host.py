"""plastid_amd/csrc/sam_host.h -- the SAM line parser that the host reader and the device kernels share, the header parse
and the defect messages -- is plain C++: tests/sam_host_test.cpp checks hand-worked lines for every field rule and every
defect code, the NH look-alikes, long CIGARs, header orders and header defects, and runs the parser on every prefix of
valid lines and on lines of 0xff bytes from buffers that end exactly where the line ends.  Compiled with the host compiler
(under the address and undefined-behaviour sanitizers where it has them) and run here.  No GPU needed."""
import os
import shutil
import subprocess

import pytest


def test_sam_line_parser(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sam_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "sam_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"sam_host: ok" in out.stdout
