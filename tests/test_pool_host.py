"""plastid_amd/csrc/pool_host.h -- the policy of the device-memory plumbing (size classes and rounding of pooled blocks,
the give / take / trim accounting of the per-engine pool and the process-wide reservoir, the growth of the page-locked
buffer, the cut of a transfer into pieces, the choice between the transfer ring, the pinned buffer and a direct copy)
-- is plain C++: tests/pool_host_test.cpp checks it against literals worked by hand, with a fake in place of hipFree,
compiled with the host compiler (under the address and undefined-behaviour sanitizers where it has them) and run here.
No GPU needed."""
import os
import shutil
import subprocess

import pytest


def test_pool_policy(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pool_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "pool_host_test.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "PC_POOL_RESERVOIR_GB"}   # (the literals assume the default limit)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
    assert out.returncode == 0, out.stdout.decode()
    assert b"pool_host: ok" in out.stdout
